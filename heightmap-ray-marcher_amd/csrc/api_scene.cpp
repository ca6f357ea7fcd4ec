// api_scene.cpp -- the C ABI declared in include/hmrm.h, scene lifetime: scene residency in HBM -- create, update, destroy --
// with the environment knobs, the launch state per stream, the pyramids, the window records and the read-backs; and the
// library's per-thread error text.  There is no CPU rendering path in this library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "api_internal.hpp"

namespace hmrm {

thread_local std::string g_error;

int fail(int code, const std::string &msg) {
	g_error = msg;
	return code;
}

// for the other translation units of the library (record.cpp)
int set_error(int code, const char *msg) { return fail(code, msg ? msg : ""); }

} // namespace hmrm

namespace {

Knobs read_knobs() {
	Knobs k;
	// The reference loop has no cap (hmap.cpp:1000).  2^26 steps is > 2800x the longest legitimate
	// march of the largest BASELINE config (8192*sqrt(2)/0.5).  Both kernels count the budget in 32
	// bits, so the cap is at most 2^31-1.
	if (const char *s = getenv("HMRM_STEP_CAP")) {
		const long long v = atoll(s);
		if (v > 0) k.step_cap = v > 0x7fffffffLL ? 0x7fffffffLL : (int64_t)v;
	}
	if (const char *s = getenv("HMRM_KERNEL")) k.kernel = strcmp(s, "simple") == 0 ? 2 : (strcmp(s, "group") == 0 ? 1 : (strcmp(s, "rec") == 0 ? 3 : 0));
	if (const char *s = getenv("HMRM_TILE_ORDER")) {
		k.tile_order = s[0] != '0';
		if (s[0] == '1' || s[0] == '2') k.order_mode = s[0] - '0';
	}
	if (const char *s = getenv("HMRM_DIAG_ITERS")) k.diag_mode = atoi(s);
	if (const char *s = getenv("HMRM_ORDER_VERBOSE")) k.order_verbose = s[0] == '1';
	if (const char *s = getenv("HMRM_TRY_GROUP")) k.try_group = s[0] != '0';
	if (const char *s = getenv("HMRM_TILE_SEGMENTS")) {
		int b = 0, c = 0, used = 0;
		while (k.seg_n < 3 && sscanf(s, "%d:%d%n", &b, &c, &used) == 2 && b >= 0 && c > 0) {
			k.seg_b[k.seg_n] = b;
			k.seg_c[k.seg_n] = c;
			++k.seg_n;
			s += used;
			if (*s != ',') break;
			++s;
		}
	}
	if (const char *s = getenv("HMRM_DEBUG_PLANE_SHIFT")) {
		const int v = atoi(s);
		if (v > 0 && v <= 28) k.min_plane_shift = v; // (8 planes of 2^28 floats: 8 GiB, the layout of the largest legal map)
	}
	if (const char *s = getenv("HMRM_MIN_LEVEL"))
		if (s[0] >= '0' && s[0] < '0' + hmrm::kMipLevels) k.min_level = s[0] - '0';
	if (const char *s = getenv("HMRM_FINEST_PAUSE"))
		if (s[0] >= '0' && s[0] <= '9') k.finest_pause = s[0] - '0';
	return k;
}

void destroy_ctx(StreamCtx *c) {
	if (!c) return;
	for (FrameSlot &sl : c->slots) {
		if (sl.uploaded) (void)hipEventDestroy(sl.uploaded);
		if (sl.measured) (void)hipEventDestroy(sl.measured);
	}
	if (c->d_meas) (void)hipFree(c->d_meas);
	if (c->h_meas) (void)hipHostFree(c->h_meas);
	if (c->d_arena) (void)hipFree(c->d_arena);
	if (c->h_arena) (void)hipHostFree(c->h_arena);
	if (c->d_counters) (void)hipFree(c->d_counters);
	for (ViewStage &v : c->view_stages) {
		if (v.uploaded) (void)hipEventDestroy(v.uploaded);
		if (v.h) (void)hipHostFree(v.h);
	}
	for (RetiredArena &r : c->retired_views) {
		(void)hipEventDestroy(r.after);
		(void)hipFree(r.ptr);
	}
	if (c->d_views) (void)hipFree(c->d_views);
	delete c;
}

// Pyramid layout of a map (DevFrame): windows per level, the common row pitch (level 0's) and the log2 of the
// power-of-two plane pitch (at least min_shift: tests force far-apart planes on small maps).  The kernel forms the
// ELEMENT index (lev << shift) + index in 32 bits -- (kMipLevels + 1) << shift never exceeds 2^31 for a map within
// hmrm_scene_create's 2^29-cell limit -- and the byte offset in 64.  Returns whether 32-bit BYTE offsets would have been
// enough (informational since round 5: every square-ish map; not 16385 x 32766, whose level 0 has 8193 x 16383 windows,
// shift 28 -- round 4 rendered such maps with the literal loop).
bool mip_layout(int32_t map_w, int32_t map_h, int32_t *mip_w, int32_t *mip_h, int32_t *mip_row, int32_t *plane_shift, int32_t min_shift = 0) {
	for (int l = 0; l < hmrm::kMipLevels; ++l) {
		const int stride = 1 << hmrm::mip_stride_shift(l); // windows of win_cells(l) cells every stride cells
		mip_w[l] = (map_w + stride - 1) / stride;
		mip_h[l] = (map_h + stride - 1) / stride;
	}
	*mip_row = mip_w[0];
	*plane_shift = min_shift;
	while (((size_t)1 << *plane_shift) < (size_t)hmrm::mip_index(mip_w[0] - 1, mip_h[0] - 1, *mip_row) + 1) ++*plane_shift;
	return ((uint64_t)(hmrm::kMipLevels + 1) << *plane_shift) <= ((uint64_t)1 << 30);
}

// UpdateHeightmap + pyramid on the scene's stream.  Streams other than the scene's own must not
// have launches in flight while the heights change (as in the reference, where UpdateHeightmap runs
// between frames, hmap.cpp:517-519).
int run_update_heights(hmrm_scene *s) {
	const int64_t n = (int64_t)s->map_w * s->map_h;
	// The ticketed entry points launch on the scene's lanes, not on s->stream: frames still in flight there (and ring
	// frames the copy stream has not delivered yet) read the tables about to be rewritten.  Drain every stream the
	// scene owns first; s->stream itself is ordered by the stream.  (Callers' own streams: their business, hmrm.h.)
	if (const int rc = hmrm::drain_scene_streams(s, false)) return rc;
	HIP_TRY(hipMemsetAsync(s->d_maxkey, 0, sizeof(unsigned long long), s->stream));
	HIP_TRY(hmrm::launch_prepare_heights(s->d_rgb, s->d_thr, n, s->params.lum_r, s->params.lum_g,
	                                     s->params.lum_b, s->params.min_height, s->params.max_height,
	                                     false, s->d_maxkey, s->stream));
	HIP_TRY(hmrm::launch_thr_to_float(s->d_thr, s->d_thr32, n, s->stream)); // (float)thr, round to nearest
	// window-maximum pyramid for the exact-leap traversal (march.hpp)
	HIP_TRY(hmrm::launch_build_mip0(s->d_thr, s->map_w, s->map_h, s->plane(s->d_mipbuf, 0), s->mip_w[0], s->mip_h[0],
	                                s->mip_row, s->stream));
	for (int l = 1; l < hmrm::kMipLevels; ++l)
		HIP_TRY(hmrm::launch_build_mip_up(s->plane(s->d_mipbuf, l - 1), s->mip_w[l - 1], s->mip_h[l - 1],
		                                  s->plane(s->d_mipbuf, l), s->mip_w[l], s->mip_h[l], s->mip_row, l - 1, s->stream));
	s->bil_valid = false; // rebuilt by the next bilinear frame
	s->records_valid = false; // ... and the window records by the next launch of the record kernel
	for (StreamCtx *c : s->ctxs)
		for (FrameSlot &sl : c->slots) sl.valid = false;
	s->settled.clear();
	s->choice.reset(); // (new heights: new content)
	++s->probe_epoch;
	unsigned long long key = 0;
	HIP_TRY(hipMemcpyAsync(&key, s->d_maxkey, sizeof key, hipMemcpyDeviceToHost, s->stream));
	HIP_TRY(hipStreamSynchronize(s->stream));
	s->thr_max = key ? hmrm::max_key_to_double(key) : -__builtin_huge_val();
	// the top plane's one element: the whole-map bound, rounded like the windows
	const float top = hmrm::round_up_to_float_host(s->thr_max);
	HIP_TRY(hipMemcpyAsync(s->plane(s->d_mipbuf, hmrm::kMipLevels), &top, sizeof top, hipMemcpyHostToDevice, s->stream));
	HIP_TRY(hipStreamSynchronize(s->stream));
	return HMRM_OK;
}

} // namespace

namespace hmrm {

// Every stream the scene owns but its own -- the launch lanes of the ticketed entry points -- and the copy stream of the ring are
// drained: what is in flight there has finished with the tables (run_update_heights) or the light plane (hmrm_scene_set_light and
// its siblings) about to change.  `own_too`: s->stream as well, for a change that is not ordered by it.
int drain_scene_streams(hmrm_scene *s, bool own_too) {
	for (StreamCtx *c : s->ctxs)
		if (c->scene_owned && (own_too || c->stream != s->stream)) HIP_TRY(hipStreamSynchronize(c->stream));
	if (s->copy_stream) HIP_TRY(hipStreamSynchronize(s->copy_stream));
	return HMRM_OK;
}

// The scene's light plane: allocated once, map_w x map_h words; dropped by hmrm_scene_clear_light, a HIP failure half-way through
// a change, and hmrm_scene_destroy.
int ensure_light_plane(hmrm_scene *s) {
	if (!s->d_baked) HIP_TRY(hipMalloc((void **)&s->d_baked, (size_t)s->map_w * (size_t)s->map_h * sizeof(uint16_t)));
	return HMRM_OK;
}
void drop_light_plane(hmrm_scene *s) {
	if (s->d_baked) (void)hipFree(s->d_baked);
	s->d_baked = nullptr;
	s->baked_scale = 0;
}

// The launch state of `stream` (created on first use; the least recently used one is dropped, after
// the device has drained, when a scene is driven from more than kMaxStreamCtx streams).
int ctx_for(hmrm_scene *s, hipStream_t stream, StreamCtx **out) {
	for (StreamCtx *c : s->ctxs)
		if (c->stream == stream) {
			c->stamp = ++s->clock;
			*out = c;
			return HMRM_OK;
		}
	if ((int)s->ctxs.size() >= kMaxStreamCtx) {
		size_t victim = 0; // (never the scene's own stream -- entry 0 -- or one of its launch lanes)
		for (size_t i = 1; i < s->ctxs.size(); ++i)
			if (!s->ctxs[i]->scene_owned && (victim == 0 || s->ctxs[i]->stamp < s->ctxs[victim]->stamp)) victim = i;
		if (victim == 0) return fail(HMRM_E_ARG, "too many streams");
		// its kernels may still read the tables / counters about to be freed.  The stream belongs to the caller and
		// may have been destroyed since (no call may name it any more), and nothing is recorded behind a frame for
		// this rare path to wait on: wait for the device (the hipFrees of destroy_ctx would anyway)
		(void)hipDeviceSynchronize();
		if (s->probe_ctx == s->ctxs[victim]) s->probe_ctx = nullptr;
		if (s->measure_fence_ctx == s->ctxs[victim]) s->measure_fence_ctx = nullptr;
		destroy_ctx(s->ctxs[victim]);
		s->ctxs.erase(s->ctxs.begin() + (long)victim);
	}
	StreamCtx *c = new (std::nothrow) StreamCtx();
	if (!c) return fail(HMRM_E_ARG, "out of memory");
	c->stream = stream;
	c->scene_owned = stream == s->stream;
	for (hipStream_t lane : s->lanes) c->scene_owned = c->scene_owned || (lane && stream == lane);
	c->stamp = ++s->clock;
	hipError_t e = hipMalloc((void **)&c->d_counters, 16 * sizeof(unsigned long long));
	// (zeroed on the scene's stream and waited for: the caller's stream may be anything)
	if (e == hipSuccess) e = hipMemsetAsync(c->d_counters, 0, 16 * sizeof(unsigned long long), s->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
	if (e != hipSuccess) {
		destroy_ctx(c);
		return fail(HMRM_E_DEVICE, std::string("stream context: ") + hipGetErrorString(e));
	}
	s->ctxs.push_back(c);
	*out = c;
	return HMRM_OK;
}

// The window records (frame.hpp), built the first time the record kernel is about to run after a height update -- by the
// scene's probe, a verdict for it, or HMRM_KERNEL=rec -- so that a caller who changes the heights every frame, and is never
// probed, does not pay for a table nobody reads (0.26-0.48 ms at 4096 x 4096).  Nothing reads the table while it is
// written: a height update drains the scene's streams, and no record kernel has been launched since.
int ensure_records(hmrm_scene *s) {
	if (s->records_valid) return HMRM_OK;
	if (!s->d_records) return fail(HMRM_E_ARG, "this scene has no window records");
	HIP_TRY(hmrm::launch_build_records(s->d_thr, s->map_w, s->map_h, s->d_records, s->stream));
	HIP_TRY(hipStreamSynchronize(s->stream));
	s->records_valid = true;
	return HMRM_OK;
}

// Bilinear quality mode only: the second pyramid, over the 3x3-dilated (and margin-padded)
// table, built the first time a bilinear frame is asked for after a height update.
int ensure_bilinear_pyramid(hmrm_scene *s) {
	if (s->bil_valid) return HMRM_OK;
	const int64_t n = (int64_t)s->map_w * s->map_h;
	if (!s->d_mipbuf_bil) HIP_TRY(hipMalloc((void **)&s->d_mipbuf_bil, s->mip_floats() * sizeof(float)));
	double *tmp = nullptr;
	HIP_TRY(hipMalloc((void **)&tmp, (size_t)n * sizeof(double)));
	hipError_t e = hmrm::launch_dilate3x3(s->d_thr, s->map_w, s->map_h, tmp, s->stream);
	if (e == hipSuccess)
		e = hmrm::launch_build_mip0(tmp, s->map_w, s->map_h, s->plane(s->d_mipbuf_bil, 0), s->mip_w[0], s->mip_h[0],
		                            s->mip_row, s->stream);
	for (int l = 1; l < hmrm::kMipLevels && e == hipSuccess; ++l)
		e = hmrm::launch_build_mip_up(s->plane(s->d_mipbuf_bil, l - 1), s->mip_w[l - 1], s->mip_h[l - 1],
		                              s->plane(s->d_mipbuf_bil, l), s->mip_w[l], s->mip_h[l], s->mip_row, l - 1, s->stream);
	// whole-map bound = max over the coarsest level (its windows cover every cell)
	const int top = hmrm::kMipLevels - 1;
	const size_t top_span = (size_t)hmrm::mip_index(s->mip_w[top] - 1, s->mip_h[top] - 1, s->mip_row) + 1;
	std::vector<float> coarse(top_span);
	if (e == hipSuccess)
		e = hipMemcpyAsync(coarse.data(), s->plane(s->d_mipbuf_bil, top), top_span * sizeof(float), hipMemcpyDeviceToHost, s->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
	(void)hipFree(tmp);
	if (e != hipSuccess) return fail(HMRM_E_DEVICE, std::string("bilinear pyramid: ") + hipGetErrorString(e));
	float m = -__builtin_huge_valf();
	for (int iy = 0; iy < s->mip_h[top]; ++iy)
		for (int ix = 0; ix < s->mip_w[top]; ++ix) {
			const float v = coarse[hmrm::mip_index(ix, iy, s->mip_row)];
			if (v > m) m = v;
		}
	// (pageable source: the copy is staged before the call returns)
	e = hipMemcpyAsync(s->plane(s->d_mipbuf_bil, hmrm::kMipLevels), &m, sizeof m, hipMemcpyHostToDevice, s->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
	if (e != hipSuccess) return fail(HMRM_E_DEVICE, std::string("bilinear pyramid: ") + hipGetErrorString(e));
	s->thr_max_bil = (double)m;
	s->bil_valid = true;
	return HMRM_OK;
}

} // namespace hmrm

extern "C" {

int hmrm_abi_version(void) { return HMRM_ABI_VERSION; }
const char *hmrm_last_error(void) { return g_error.c_str(); }

int hmrm_device_count(void) {
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess) return fail(HMRM_E_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
	return n;
}

int hmrm_set_device(int device) {
	HIP_TRY(hipSetDevice(device));
	return HMRM_OK;
}

int hmrm_scene_create(const uint8_t *height_rgb, const uint8_t *color_rgba, int32_t map_w,
                      int32_t map_h, const hmrm_scene_params *params, hmrm_scene **out) {
	if (!height_rgb || !color_rgba || !params || !out) return fail(HMRM_E_ARG, "NULL argument");
	if (map_w <= 0 || map_h <= 0) return fail(HMRM_E_ARG, "map dimensions must be positive");
	// the reference indexes (gridx + gridy*W)*4 with int (hmap.cpp:1018)
	if ((int64_t)map_w * map_h > ((int64_t)1 << 31) / 4)
		return fail(HMRM_E_ARG, "map too large (the reference indexes the colormap with int)");
	*out = nullptr;
	hmrm_scene *s = new (std::nothrow) hmrm_scene();
	if (!s) return fail(HMRM_E_ARG, "out of memory");
	const size_t n = (size_t)map_w * (size_t)map_h;
	s->map_w = map_w;
	s->map_h = map_h;
	s->params = *params;
	s->knobs = read_knobs();
	int rc = HMRM_OK;
	auto body = [&]() -> int {
		HIP_TRY(hipGetDevice(&s->device));
		HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
		HIP_TRY(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
		HIP_TRY(hipEventCreate(&s->ev0));
		HIP_TRY(hipEventCreate(&s->ev1));
		HIP_TRY(hipMalloc((void **)&s->d_rgb, n * 3));
		HIP_TRY(hipMalloc((void **)&s->d_cmap, n * 4));
		HIP_TRY(hipMalloc((void **)&s->d_thr, n * (sizeof(double) + sizeof(float)))); // the table, then its float copy
		s->d_thr32 = reinterpret_cast<float *>(s->d_thr + n);
		// every plane has level 0's row pitch and a power-of-two plane pitch (DevFrame); the pyramid of the
		// bilinear mode is allocated by its first frame
		(void)mip_layout(map_w, map_h, s->mip_w, s->mip_h, &s->mip_row, &s->mip_plane_shift, s->knobs.min_plane_shift);
		HIP_TRY(hipMalloc((void **)&s->d_mipbuf, s->mip_floats() * sizeof(float)));
		if ((map_h + 3) / 4 <= 65535 * 16)
			HIP_TRY(hipMalloc((void **)&s->d_records, (size_t)hmrm::rec_row(map_w) * (size_t)((map_h + 3) / 4) * sizeof(hmrm::WindowRecord)));
		HIP_TRY(hipMalloc((void **)&s->d_maxkey, sizeof(unsigned long long)));
		HIP_TRY(hipMemcpyAsync(s->d_rgb, height_rgb, n * 3, hipMemcpyHostToDevice, s->stream));
		HIP_TRY(hipMemcpyAsync(s->d_cmap, color_rgba, n * 4, hipMemcpyHostToDevice, s->stream));
		StreamCtx *own = nullptr;
		const int rc2 = ctx_for(s, s->stream, &own); // entry 0: the scene's own stream
		if (rc2) return rc2;
		return run_update_heights(s);
	};
	rc = body();
	if (rc != HMRM_OK) {
		std::string keep = g_error;
		hmrm_scene_destroy(s);
		g_error = keep;
		return rc;
	}
	*out = s;
	return HMRM_OK;
}

int hmrm_scene_update(hmrm_scene *s, const hmrm_scene_params *params) {
	if (!s || !params) return fail(HMRM_E_ARG, "NULL argument");
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	s->params = *params;
	return run_update_heights(s);
}

void hmrm_scene_destroy(hmrm_scene *s) {
	if (!s) return;
	(void)hipSetDevice(s->device);
	for (StreamCtx *c : s->ctxs) {
		// (a caller's stream may already be gone: only the scene's own streams are drained)
		if (c->scene_owned && c->stream) (void)hipStreamSynchronize(c->stream);
		destroy_ctx(c);
	}
	s->ctxs.clear();
	if (s->copy_stream) (void)hipStreamSynchronize(s->copy_stream);
	for (RingFrame *r : s->ring) {
		r->teardown();
		delete r;
	}
	s->ring.clear();
	for (DevTicket *t : s->dev_tickets) {
		t->teardown();
		delete t;
	}
	s->dev_tickets.clear();
	for (hipStream_t &lane : s->lanes)
		if (lane) {
			(void)hipStreamDestroy(lane);
			lane = nullptr;
		}
	if (s->copy_stream) (void)hipStreamDestroy(s->copy_stream);
	if (s->d_rgb) (void)hipFree(s->d_rgb);
	if (s->d_cmap) (void)hipFree(s->d_cmap);
	if (s->d_thr) (void)hipFree(s->d_thr);
	if (s->d_mipbuf) (void)hipFree(s->d_mipbuf);
	if (s->d_records) (void)hipFree(s->d_records);
	if (s->d_mipbuf_bil) (void)hipFree(s->d_mipbuf_bil);
	if (s->d_maxkey) (void)hipFree(s->d_maxkey);
	hmrm::drop_light_plane(s);
	for (DeviceScratch *b : {&s->d_frame, &s->d_steps, &s->d_entry, &s->d_rays, &s->d_hits, &s->d_limits, &s->d_cells, &s->d_targets,
	                         &s->d_geom, &s->d_light})
		b->release();
	s->h_stage.release();
	if (s->h_probe) (void)hipHostFree(s->h_probe);
	if (s->probe_done) (void)hipEventDestroy(s->probe_done);
	if (s->measure_fence) (void)hipEventDestroy(s->measure_fence);
	if (s->ev0) (void)hipEventDestroy(s->ev0);
	if (s->ev1) (void)hipEventDestroy(s->ev1);
	if (s->stream) (void)hipStreamDestroy(s->stream);
	delete s;
}

// ---- the scene's light plane (hmrm_render_baked reads it) ----
// hmrm_scene_set_light and its device form.  The refusals in the header's order; then the scene's streams are drained -- tickets in
// flight finish with the old plane -- and the plane is filled: 16-bit words by a strided copy, bytes widened on the host (host
// form) or by a small kernel on the caller's stream (device form).  A HIP failure from there on leaves the scene without a plane.
static int set_light_common(hmrm_scene *s, const void *plane, size_t stride_bytes, int32_t format, uint32_t full_scale, bool device,
                            hipStream_t stream) {
	if (!s) return fail(HMRM_E_ARG, "light plane: NULL scene");
	if (!plane) return fail(HMRM_E_ARG, "light plane: NULL plane");
	if (format != HMRM_LIGHT_U8 && format != HMRM_LIGHT_U16) return fail(HMRM_E_ARG, "light plane: format must be HMRM_LIGHT_U8 or HMRM_LIGHT_U16");
	if (full_scale < 1u || full_scale > 65535u) return fail(HMRM_E_ARG, "light plane: full_scale must be 1 .. 65535");
	const size_t W = (size_t)s->map_w, H = (size_t)s->map_h, elem = format == HMRM_LIGHT_U16 ? 2 : 1;
	if (stride_bytes < elem * W) return fail(HMRM_E_ARG, "light plane: stride_bytes is below a row of the map");
	if (elem == 2 && (stride_bytes & 1u)) return fail(HMRM_E_ARG, "light plane: stride_bytes must be even for HMRM_LIGHT_U16");
	if (device && elem == 2 && ((uintptr_t)plane & 1u)) return fail(HMRM_E_ARG, "light plane: d_plane must be 2-byte aligned for HMRM_LIGHT_U16");
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	int rc = drain_scene_streams(s, true);
	if (rc) return rc;
	auto body = [&]() -> int {
		if (const int rc_p = ensure_light_plane(s)) return rc_p;
		if (!device) stream = s->stream;
		std::vector<uint16_t> wide; // (host bytes: widened here, one packed copy)
		if (elem == 2) {
			HIP_TRY(hipMemcpy2DAsync(s->d_baked, W * 2, plane, stride_bytes, W * 2, H, device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
		} else if (device) {
			HIP_TRY(hmrm::launch_widen_light(static_cast<const uint8_t *>(plane), stride_bytes, s->map_w, s->map_h, s->d_baked, stream));
		} else {
			wide.resize(W * H);
			for (size_t y = 0; y < H; ++y) {
				const uint8_t *row = static_cast<const uint8_t *>(plane) + y * stride_bytes;
				for (size_t x = 0; x < W; ++x) wide[y * W + x] = row[x];
			}
			HIP_TRY(hipMemcpyAsync(s->d_baked, wide.data(), W * H * 2, hipMemcpyHostToDevice, stream));
		}
		HIP_TRY(hipStreamSynchronize(stream));
		return HMRM_OK;
	};
	if ((rc = body())) {
		drop_light_plane(s);
		return rc;
	}
	s->baked_scale = full_scale;
	return HMRM_OK;
}

int hmrm_scene_set_light(hmrm_scene *scene, const void *plane, size_t stride_bytes, int32_t format, uint32_t full_scale) {
	return set_light_common(scene, plane, stride_bytes, format, full_scale, false, nullptr);
}

int hmrm_scene_set_light_device(hmrm_scene *scene, const void *d_plane, size_t stride_bytes, int32_t format, uint32_t full_scale,
                                void *hip_stream) {
	return set_light_common(scene, d_plane, stride_bytes, format, full_scale, true, (hipStream_t)hip_stream);
}

int hmrm_scene_clear_light(hmrm_scene *s) {
	if (!s) return fail(HMRM_E_ARG, "light plane: NULL scene");
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	if (const int rc = drain_scene_streams(s, true)) return rc;
	drop_light_plane(s);
	return HMRM_OK;
}

int hmrm_scene_light(const hmrm_scene *cs, uint16_t *out, size_t stride_bytes, uint32_t *full_scale) {
	hmrm_scene *s = const_cast<hmrm_scene *>(cs);
	if (!s) return fail(HMRM_E_ARG, "light plane: NULL scene");
	if (!full_scale) return fail(HMRM_E_ARG, "light plane: NULL full_scale");
	const size_t W = (size_t)s->map_w, H = (size_t)s->map_h;
	if (out && (stride_bytes < 2 * W || (stride_bytes & 1u))) return fail(HMRM_E_ARG, "light plane: stride_bytes must be >= 2 * map_w and even");
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	*full_scale = s->d_baked ? s->baked_scale : 0u;
	if (!out || *full_scale == 0u) return HMRM_OK;
	HIP_TRY(hipMemcpy2DAsync(out, stride_bytes, s->d_baked, W * 2, W * 2, H, hipMemcpyDeviceToHost, s->stream));
	HIP_TRY(hipStreamSynchronize(s->stream));
	return HMRM_OK;
}

int hmrm_debug_reload_env(hmrm_scene *s) {
	if (!s) return fail(HMRM_E_ARG, "NULL argument");
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	s->knobs = read_knobs();
	// A launch order is calibrated for ONE kernel variant and level policy: makespans measured before the knobs
	// changed must not be compared with ones measured after, and an order settled for the old kernel must not be
	// adopted for the new one.  Every record goes back to "uncalibrated" (pixels never depended on any of this).
	s->settled.clear();
	s->choice.reset();
	++s->probe_epoch;
	for (StreamCtx *c : s->ctxs)
		for (FrameSlot &sl : c->slots) {
			if (sl.cal.in_flight >= 0 && sl.measured) HIP_TRY(hipEventSynchronize(sl.measured)); // (its read-back targets the slot's records)
			sl.cal.reset();
			if (c->meas_owner == &sl) c->meas_owner = nullptr;
		}
	return HMRM_OK;
}

int hmrm_scene_read_heights(const hmrm_scene *cs, double *out) {
	hmrm_scene *s = const_cast<hmrm_scene *>(cs);
	if (!s || !out) return fail(HMRM_E_ARG, "NULL argument");
	HIP_TRY(hipSetDevice(s->device));
	const int64_t n = (int64_t)s->map_w * s->map_h;
	double *tmp = nullptr;
	HIP_TRY(hipMalloc((void **)&tmp, (size_t)n * sizeof(double)));
	hipError_t e = hmrm::launch_prepare_heights(s->d_rgb, tmp, n, s->params.lum_r, s->params.lum_g,
	                                            s->params.lum_b, s->params.min_height,
	                                            s->params.max_height, true, nullptr, s->stream);
	if (e == hipSuccess)
		e = hipMemcpyAsync(out, tmp, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
	(void)hipFree(tmp);
	if (e != hipSuccess) return fail(HMRM_E_DEVICE, std::string("read_heights: ") + hipGetErrorString(e));
	return HMRM_OK;
}

// Test hook (no GPU): the pyramid layout hmrm_scene_create would choose for a map, and whether 32-bit BYTE offsets
// would cover it (0: only the kernel's 64-bit offsets do -- informational since round 5).
int hmrm_debug_mip_layout(int32_t map_w, int32_t map_h, int32_t *mip_row, int32_t *plane_shift, int32_t *levels) {
	if (map_w <= 0 || map_h <= 0 || (int64_t)map_w * map_h > ((int64_t)1 << 31) / 4) return fail(HMRM_E_ARG, "bad map dimensions");
	int32_t w[hmrm::kMipLevels], h[hmrm::kMipLevels], row = 0, shift = 0;
	const bool fits = mip_layout(map_w, map_h, w, h, &row, &shift);
	if (mip_row) *mip_row = row;
	if (plane_shift) *plane_shift = shift;
	if (levels) *levels = hmrm::kMipLevels;
	return fits ? 1 : 0;
}

// Test hook: the scene's window records (frame.hpp WindowRecord, 32 bytes each, rec_row(map_w) x ceil(map_h / 4)) and the
// threshold table they were built from (map_w x map_h doubles), copied to the host.  Either pointer may be NULL.
int hmrm_debug_read_records(const hmrm_scene *cs, void *records_out, double *thr_out) {
	hmrm_scene *s = const_cast<hmrm_scene *>(cs);
	if (!s) return fail(HMRM_E_ARG, "NULL argument");
	std::lock_guard<std::mutex> lk(s->mu);
	HIP_TRY(hipSetDevice(s->device));
	HIP_TRY(hipStreamSynchronize(s->stream));
	if (records_out) {
		if (!s->d_records) return fail(HMRM_E_ARG, "this scene has no window records (map too tall)");
		const int rc_r = ensure_records(s);
		if (rc_r) return rc_r;
		HIP_TRY(hipMemcpy(records_out, s->d_records, (size_t)hmrm::rec_row(s->map_w) * (size_t)((s->map_h + 3) / 4) * sizeof(hmrm::WindowRecord),
		                  hipMemcpyDeviceToHost));
	}
	if (thr_out) HIP_TRY(hipMemcpy(thr_out, s->d_thr, (size_t)s->map_w * (size_t)s->map_h * sizeof(double), hipMemcpyDeviceToHost));
	return HMRM_OK;
}

} // extern "C"
