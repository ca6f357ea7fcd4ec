// api_frames.cpp -- the C ABI declared in include/hmrm.h, frame entry points: the synchronous frames, the ticketed ones (the
// asynchronous read-back ring, frames into device memory through the launch lanes), row strips, one frame over several
// scenes, and the kernel timing of bench.py.
#include <algorithm>
#include <cstring>
#include <map>
#include <new>

#include "api_internal.hpp"
#include "host_pool.hpp"

namespace {

thread_local double g_last_kernel_ms = -1.0;

// Antialiasing (hmrm_render_aa, HMRM_AA): factor n in {1, 2, 4, 8} -> *shift = log2 n and *super = the camera of the
// n x n larger "super frame" the kernel marches (everything else unchanged), which must itself pass check_camera.  Needs
// no scene and no device: the rejections are testable without a GPU.
int check_antialias(const hmrm_camera *cam, int32_t factor, hmrm_camera *super, int *shift) {
	const int sh = factor == 1 ? 0 : factor == 2 ? 1 : factor == 4 ? 2 : factor == 8 ? 3 : -1;
	if (sh < 0) return fail(HMRM_E_ARG, "antialias factor must be 1, 2, 4 or 8 (got " + std::to_string(factor) + ")");
	if ((int64_t)cam->width * cam->height * ((int64_t)1 << (2 * sh)) > ((int64_t)1 << 31) / 4)
		return fail(HMRM_E_ARG, "antialias: the " + std::to_string(factor) + "x super frame has more than 2^29 samples (the reference "
		                        "indexes the framebuffer with int)");
	*super = *cam;
	super->width = cam->width << sh;
	super->height = cam->height << sh;
	*shift = sh;
	return HMRM_OK;
}

// The antialias factor of a ticketed call's flags (HMRM_AA), refusing bits the ABI does not define.
int antialias_of_flags(uint32_t flags, int32_t *factor) {
	if (flags & ~(HMRM_NO_PROBE | HMRM_AA_MASK))
		return fail(HMRM_E_ARG, "flags: unknown bits (defined: HMRM_NO_PROBE and the antialias factor HMRM_AA(n))");
	const int32_t n = (int32_t)((flags & HMRM_AA_MASK) >> 8);
	*factor = n == 0 ? 1 : n;
	return HMRM_OK;
}

// hmrm_render's frame into d_out.
FrameRequest plain_request(uint32_t *d_out, int64_t out_stride_px) {
	return FrameRequest{d_out, out_stride_px, nullptr, nullptr, false, false, Interior::kNot, nullptr};
}

// The next lane in turn (lanes are created on first use; call with s->mu held).
int next_lane(hmrm_scene *s, hipStream_t *out) {
	const uint32_t i = s->lane_next++ % kLanes;
	if (!s->lanes[i]) HIP_TRY(hipStreamCreateWithFlags(&s->lanes[i], hipStreamNonBlocking));
	*out = s->lanes[i];
	return HMRM_OK;
}

// What every frame entry point sets up before it launches: the launch state of `stream`, the cached record of `cam` -- the
// camera the kernel marches: the super camera of an antialiased frame, `aa_shift` the log2 of its factor -- and the row map of
// the whole frame (strips and bands: the caller puts its own in its place).  Call with s->mu held.
struct FrameSetup {
	StreamCtx *c = nullptr;
	FrameSlot *slot = nullptr;
	hmrm::DevFrame f;
	hmrm::RowMap rows;
};
int setup_frame(hmrm_scene *s, hipStream_t stream, const hmrm_camera *cam, int aa_shift, FrameSetup *fs) {
	int rc = ctx_for(s, stream, &fs->c);
	if (rc) return rc;
	if ((rc = prepare_frame(s, fs->c, cam, &fs->f, &fs->slot))) return rc;
	fs->f.aa_shift = aa_shift;
	fs->rows = hmrm::RowMap{0, cam->height, 0, 0, 1, {}, {}, nullptr};
	return HMRM_OK;
}

// A frame in the caller's device memory: rows of whole pixels, the stride in pixels an int.
int check_device_stride(const hmrm_camera *cam, size_t stride_bytes) {
	if (stride_bytes < (size_t)cam->width * 4 || (stride_bytes & 3) || stride_bytes / 4 > 0x7fffffffu)
		return fail(HMRM_E_ARG, "stride_bytes must be >= width*4, a multiple of 4 and below 2^33");
	return HMRM_OK;
}

// One plane of a frame with several (geometry frames, lit sums; `prefix` names the family): a stride of whole elements that covers
// the camera's width -- compared only when there is a camera with one: `width` is 0 else, and check_camera refuses right after --
// and, with check_align, a pointer aligned to its elements.  A NULL plane is not wanted and passes.
int check_plane(const char *prefix, const char *name, const void *ptr, size_t stride, size_t elem, size_t width, bool check_align) {
	if (!ptr) return HMRM_OK;
	if (stride < elem * width || (stride % elem) != 0 || stride / elem > 0x7fffffffu)
		return fail(HMRM_E_ARG, std::string(prefix) + name + "_stride must be >= " + std::to_string(elem) + " * width, a multiple of " +
		                            std::to_string(elem) + " and below 2^31 elements");
	if (check_align && ((uintptr_t)ptr % elem) != 0)
		return fail(HMRM_E_ARG, std::string(prefix) + name + " must be " + std::to_string(elem) + "-byte aligned");
	return HMRM_OK;
}
size_t width_or_0(const hmrm_camera *cam) { return (cam && cam->width > 0) ? (size_t)cam->width : 0; }

// A ticket pool (the read-back ring, the device tickets): *idx = the first free slot, else a new one while the pool has fewer
// than kMaxRing, else the refusal `full`.  A new slot joins the pool only once complete() has made it whole -- a half-made slot
// would be picked up as free by the next call -- and is torn down by the function hmrm_scene_destroy uses.  (s->mu held.)
template <class Ticket> int acquire_ticket(std::vector<Ticket *> &pool, const char *who, const char *full, int *idx) {
	for (size_t i = 0; i < pool.size(); ++i)
		if (!pool[i]->busy) {
			*idx = (int)i;
			return HMRM_OK;
		}
	if ((int)pool.size() >= kMaxRing) return fail(HMRM_E_ARG, std::string(who) + ": " + full);
	Ticket *t = new (std::nothrow) Ticket();
	if (!t) return fail(HMRM_E_ARG, "out of memory");
	const hipError_t e = t->complete();
	if (e != hipSuccess) {
		t->teardown();
		delete t;
		return fail(HMRM_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
	}
	pool.push_back(t);
	*idx = (int)pool.size() - 1;
	return HMRM_OK;
}

} // namespace

extern "C" {

// What the synchronous frames differ in.  aa_factor > 1 (hmrm_render_aa): the launch marches the super frame and writes the
// W x H box-filtered frame (no per-pixel arrays then).
struct SyncFrame {
	hmrm_stats *stats;  // hmrm_render_stats' outputs, with want_stats
	uint32_t *steps_pp;
	double *entry_d;
	bool want_stats;
	int32_t aa_factor;
	bool interior; // hmrm_render_interior
	const LitFrame *lit;
	bool baked = false;          // hmrm_render_baked: the hit pixels under the scene's light plane ...
	bool baked_interior = false; // ... and, HMRM_TRACE_INTERIOR, every origin tested by the kernels
};
constexpr SyncFrame kPlainSync{nullptr, nullptr, nullptr, false, 1, false, nullptr};

// The scene's light plane as a baked frame's launch takes it, or the refusal of a scene without one.  (s->mu held.)
static int baked_light_of(const hmrm_scene *s, hmrm::BakedLight *out) {
	if (!s->d_baked || s->baked_scale == 0u) return fail(HMRM_E_ARG, "the scene has no light plane");
	*out = hmrm::BakedLight{s->d_baked, s->baked_scale};
	return HMRM_OK;
}
static int check_baked_flags(uint32_t baked_flags) {
	if (baked_flags & ~HMRM_TRACE_INTERIOR) return fail(HMRM_E_ARG, "baked_flags: undefined bit");
	return HMRM_OK;
}

static int render_common(hmrm_scene *s, const hmrm_camera *cam, uint8_t *rgba, size_t stride_bytes, const SyncFrame &how) {
	const bool want_stats = how.want_stats;
	int rc = check_camera(cam);
	if (rc) return rc;
	hmrm_camera super;
	int aa_shift = 0;
	if ((rc = check_antialias(cam, how.aa_factor, &super, &aa_shift))) return rc;
	if (!s || !rgba) return fail(HMRM_E_ARG, "NULL argument");
	const size_t W = (size_t)cam->width, H = (size_t)cam->height;
	if (stride_bytes < W * 4) return fail(HMRM_E_ARG, "stride_bytes < width*4");
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	const bool per_pixel = want_stats && aa_shift == 0; // (per-pixel arrays are of the plain frame only)
	hmrm::BakedLight baked{nullptr, 0u};
	if (how.baked && (rc = baked_light_of(s, &baked))) return rc;
	if ((rc = s->d_frame.reserve(W * H * sizeof(uint32_t)))) return rc;
	if (per_pixel && ((rc = s->d_steps.reserve(W * H * sizeof(uint32_t))) || (rc = s->d_entry.reserve(W * H * sizeof(double))))) return rc;
	FrameSetup fs;
	if ((rc = setup_frame(s, s->stream, &super, aa_shift, &fs))) return rc;
	StreamCtx *const c = fs.c;
	Interior interior = Interior::kNot; // (decided once per frame where every ray starts at the camera: FrameRequest)
	if (how.interior) {
		const hmrm::DevFrame &f = fs.f;
		const double *o = f.cam;
		const bool cam_inside = f.c0[0] < o[0] && o[0] < f.c1[0] && f.c1[1] < o[1] && o[1] < f.c0[1] && f.c0[2] < o[2] && o[2] < f.c1[2];
		interior = (cam->projection == HMRM_ORTHOGRAPHIC || cam_inside) ? Interior::kByKernels : Interior::kHostSawNone;
	}
	if (want_stats) {
		HIP_TRY(hipMemsetAsync(c->d_counters, 0, 2 * sizeof(unsigned long long), s->stream));
		HIP_TRY(hipMemsetAsync(c->d_counters + 4, 0, 4 * sizeof(unsigned long long), s->stream));
	}
	HIP_TRY(hipEventRecord(s->ev0, s->stream));
	FrameRequest req{s->d_frame.as<uint32_t>(), (int64_t)W, per_pixel ? s->d_steps.as<uint32_t>() : nullptr,
	                 per_pixel ? s->d_entry.as<double>() : nullptr, want_stats, false, interior, how.lit};
	if (how.baked) { // (with the flag every origin is tested by the kernels, whatever the projection: a geometry frame's rule)
		req.baked = &baked;
		req.interior = how.baked_interior ? Interior::kByKernels : Interior::kNot;
	}
	if ((rc = launch_frame(s, c, fs.f, fs.slot, fs.rows, req))) return rc;
	HIP_TRY(hipEventRecord(s->ev1, s->stream));
	HIP_TRY(hipMemcpy2DAsync(rgba, stride_bytes, s->d_frame.ptr, W * 4, W * 4, H, hipMemcpyDeviceToHost, s->stream));
	unsigned long long counters[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	HIP_TRY(hipMemcpyAsync(counters, c->d_counters, sizeof counters, hipMemcpyDeviceToHost, s->stream));
	if (per_pixel && how.steps_pp)
		HIP_TRY(hipMemcpyAsync(how.steps_pp, s->d_steps.ptr, W * H * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
	if (per_pixel && how.entry_d)
		HIP_TRY(hipMemcpyAsync(how.entry_d, s->d_entry.ptr, W * H * sizeof(double), hipMemcpyDeviceToHost, s->stream));
	HIP_TRY(hipStreamSynchronize(s->stream));
	float ms = 0.f;
	HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
	g_last_kernel_ms = ms;
	const unsigned long long capped = new_capped(c, counters[2]);
	if (hmrm_stats *const stats = how.stats) {
		stats->rays = (uint64_t)super.width * (uint64_t)super.height;
		stats->steps = counters[0];
		stats->hits = counters[1];
		stats->capped = capped;
		stats->leap_attempts = counters[4];
		stats->leaps = counters[5];
		stats->groups = counters[6];
		stats->leaped_steps = counters[7];
	}
	return noterm(capped);
}

int hmrm_render(const hmrm_scene *scene, const hmrm_camera *cam, uint8_t *rgba, size_t stride_bytes) {
	return render_common(const_cast<hmrm_scene *>(scene), cam, rgba, stride_bytes, kPlainSync);
}

// Progressive refresh of the reference's frame driver (hmap.cpp:976-983): only pixels
// p = cycle, cycle + cycle_period, ... (p = x + y*width) of the caller's framebuffer are
// rewritten, the rest keeps what earlier frames left there.  The whole frame is rendered on
// the device (sub-millisecond) and the selected pixels are merged on the host.
int hmrm_render_cycle(const hmrm_scene *scene, const hmrm_camera *cam, uint8_t *rgba, size_t stride_bytes,
                      int32_t cycle, int32_t cycle_period) {
	if (cycle_period <= 0 || cycle < 0 || cycle >= cycle_period) return fail(HMRM_E_ARG, "need 0 <= cycle < cycle_period");
	int rc = check_camera(cam);
	if (rc) return rc;
	if (!rgba) return fail(HMRM_E_ARG, "NULL argument");
	if (stride_bytes < (size_t)cam->width * 4) return fail(HMRM_E_ARG, "stride_bytes < width*4");
	const size_t W = (size_t)cam->width, H = (size_t)cam->height;
	std::vector<uint8_t> full(W * H * 4);
	rc = hmrm_render(scene, cam, full.data(), W * 4);
	if (rc != HMRM_OK && rc != HMRM_E_NOTERM) return rc;
	for (size_t p = (size_t)cycle; p < W * H; p += (size_t)cycle_period) {
		const size_t x = p % W, y = p / W; // hmap.cpp:982-983
		memcpy(rgba + y * stride_bytes + x * 4, &full[p * 4], 4);
	}
	return rc;
}

int hmrm_render_aa(const hmrm_scene *scene, const hmrm_camera *cam, int32_t factor, uint8_t *rgba, size_t stride_bytes,
                   hmrm_stats *stats) {
	SyncFrame how = kPlainSync;
	how.stats = stats;
	how.want_stats = stats != nullptr;
	how.aa_factor = factor;
	return render_common(const_cast<hmrm_scene *>(scene), cam, rgba, stride_bytes, how);
}

int hmrm_render_interior(const hmrm_scene *scene, const hmrm_camera *cam, uint8_t *rgba, size_t stride_bytes) {
	SyncFrame how = kPlainSync;
	how.interior = true;
	return render_common(const_cast<hmrm_scene *>(scene), cam, rgba, stride_bytes, how);
}

// ---- geometry frames: hmrm_render's frame (hmrm_render_interior's with HMRM_TRACE_INTERIOR) and up to three more planes -- hit
// cell, range, slope -- from the same launch ----
// The five refusals of the header, in its order; needs no scene and no device.  A stride is compared with the camera's width
// only when there is a camera with one: a camera that check_camera refuses is refused right after.
static int check_geometry_planes(const hmrm_geometry_planes *p, const hmrm_camera *cam, bool device) {
	if (!p) return fail(HMRM_E_ARG, "geometry frame: NULL planes");
	if (p->flags & ~HMRM_TRACE_INTERIOR) return fail(HMRM_E_ARG, "hmrm_geometry_planes.flags: undefined bit");
	if (p->reserved != 0u) return fail(HMRM_E_ARG, "hmrm_geometry_planes.reserved must be 0");
	if (!p->rgba && !p->cell && !p->range && !p->slope) return fail(HMRM_E_ARG, "geometry frame: every plane is NULL");
	// (a host plane of 4-byte elements may sit anywhere; the slope's 8-byte pairs are refused misaligned in host memory too)
	const size_t width = width_or_0(cam);
	const char *const pre = "geometry frame: ";
	int rc;
	if ((rc = check_plane(pre, "rgba", p->rgba, p->rgba_stride, 4, width, device)) ||
	    (rc = check_plane(pre, "cell", p->cell, p->cell_stride, 4, width, device)) ||
	    (rc = check_plane(pre, "range", p->range, p->range_stride, 4, width, device)) ||
	    (rc = check_plane(pre, "slope", p->slope, p->slope_stride, 8, width, true)))
		return rc;
	return HMRM_OK;
}

// Launched the way an interior frame is (FrameRequest::own_kernels): never measured, never the probe, with the scene's current
// kernel.  With the flag every origin is tested by the kernels, whatever the projection.  `device`: p holds device pointers and
// the launch goes to `stream` without a host sync; else the planes are staged through the scene's buffer, slope first (8-byte
// elements), rows packed, and copied to the caller's behind the launch.
static int render_geometry_common(hmrm_scene *s, const hmrm_camera *cam, const hmrm_geometry_planes *p, bool device, hipStream_t stream) {
	int rc = check_geometry_planes(p, cam, device);
	if (rc || (rc = check_camera(cam))) return rc;
	if (!s) return fail(HMRM_E_ARG, "NULL argument");
	const size_t W = (size_t)cam->width, H = (size_t)cam->height;
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	uint32_t *d_rgba = (uint32_t *)p->rgba;
	hmrm::GeomPlanes dev{p->cell, p->range, p->slope, (int64_t)(p->cell_stride / 4), (int64_t)(p->range_stride / 4), (int64_t)(p->slope_stride / 8)};
	int64_t rgba_stride_px = (int64_t)(p->rgba_stride / 4);
	if (!device) {
		const size_t px = W * H;
		if ((rc = s->d_geom.reserve(px * ((p->slope ? 8 : 0) + (p->rgba ? 4 : 0) + (p->cell ? 4 : 0) + (p->range ? 4 : 0))))) return rc;
		uint8_t *at = s->d_geom.as<uint8_t>();
		auto take = [&](const void *wanted, size_t elem) -> void * {
			if (!wanted) return nullptr;
			void *here = at;
			at += px * elem;
			return here;
		};
		dev.slope = (float *)take(p->slope, 8);
		d_rgba = (uint32_t *)take(p->rgba, 4);
		dev.cell = (int32_t *)take(p->cell, 4);
		dev.range = (float *)take(p->range, 4);
		dev.cell_stride = dev.range_stride = dev.slope_stride = rgba_stride_px = (int64_t)W;
		stream = s->stream;
	}
	FrameSetup fs;
	if ((rc = setup_frame(s, stream, cam, 0, &fs))) return rc;
	StreamCtx *const c = fs.c;
	FrameRequest req = plain_request(d_rgba, rgba_stride_px);
	req.interior = (p->flags & HMRM_TRACE_INTERIOR) ? Interior::kByKernels : Interior::kNot;
	req.geom = &dev;
	if ((rc = launch_frame(s, c, fs.f, fs.slot, fs.rows, req)) || device) return rc;
	if (p->slope) HIP_TRY(hipMemcpy2DAsync(p->slope, p->slope_stride, dev.slope, W * 8, W * 8, H, hipMemcpyDeviceToHost, s->stream));
	if (p->rgba) HIP_TRY(hipMemcpy2DAsync(p->rgba, p->rgba_stride, d_rgba, W * 4, W * 4, H, hipMemcpyDeviceToHost, s->stream));
	if (p->cell) HIP_TRY(hipMemcpy2DAsync(p->cell, p->cell_stride, dev.cell, W * 4, W * 4, H, hipMemcpyDeviceToHost, s->stream));
	if (p->range) HIP_TRY(hipMemcpy2DAsync(p->range, p->range_stride, dev.range, W * 4, W * 4, H, hipMemcpyDeviceToHost, s->stream));
	return finish_host_call(s, c);
}

int hmrm_render_geometry(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_geometry_planes *host_planes) {
	return render_geometry_common(const_cast<hmrm_scene *>(scene), cam, host_planes, false, nullptr);
}

int hmrm_render_geometry_device(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_geometry_planes *device_planes, void *hip_stream) {
	return render_geometry_common(const_cast<hmrm_scene *>(scene), cam, device_planes, true, (hipStream_t)hip_stream);
}

// Sun shadows: hmrm_render's frame (hmrm_render_interior's with HMRM_TRACE_INTERIOR), the hit pixels' shadow rays marched
// by the same launch.  The sun is checked before anything else is looked at (check_sun: hmrm_render_lit's three refusals,
// hmrm_render_shaded's too).
static int check_sun(const hmrm_sun *sun) {
	if (!sun) return fail(HMRM_E_ARG, "NULL sun");
	if (sun->flags & ~HMRM_TRACE_INTERIOR) return fail(HMRM_E_ARG, "hmrm_sun.flags: undefined bit");
	for (uint8_t r : sun->reserved)
		if (r) return fail(HMRM_E_ARG, "hmrm_sun.reserved must be 0");
	return HMRM_OK;
}
static LitFrame make_lit_frame(const hmrm_sun *sun, uint32_t shade_flags) {
	return LitFrame{hmrm::SunRules{{sun->dir[0], sun->dir[1], sun->dir[2]}, sun->step_dist, sun->max_steps, sun->ambient},
	                (sun->flags & HMRM_TRACE_INTERIOR) != 0u, shade_flags};
}
static int render_lit_common(const hmrm_scene *scene, const hmrm_camera *cam, const LitFrame *lit, int32_t factor, uint8_t *rgba,
                             size_t stride_bytes) {
	SyncFrame how = kPlainSync;
	how.aa_factor = factor;
	how.lit = lit;
	return render_common(const_cast<hmrm_scene *>(scene), cam, rgba, stride_bytes, how);
}
int hmrm_render_lit(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_sun *sun, uint8_t *rgba, size_t stride_bytes) {
	if (const int rc = check_sun(sun)) return rc;
	const LitFrame lit = make_lit_frame(sun, 0u);
	return render_lit_common(scene, cam, &lit, 1, rgba, stride_bytes);
}

// hmrm_render_lit's three refusals and hmrm_render_shaded's own, in the header's order.
static int check_shaded(const hmrm_sun *sun, uint32_t shade_flags) {
	if (const int rc = check_sun(sun)) return rc;
	if (shade_flags & ~(HMRM_SHADE_DIFFUSE | HMRM_SHADE_NO_SHADOWS)) return fail(HMRM_E_ARG, "shade_flags: undefined bit");
	return HMRM_OK;
}

// Diffuse sun shading: the lit frame whose hit pixels are weighted by their diffuse level, with or without the shadow rays.
// shade_flags = 0 is hmrm_render_lit itself, launch for launch.
int hmrm_render_shaded(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_sun *sun, uint32_t shade_flags, uint8_t *rgba,
                       size_t stride_bytes) {
	if (const int rc = check_shaded(sun, shade_flags)) return rc;
	const LitFrame lit = make_lit_frame(sun, shade_flags);
	return render_lit_common(scene, cam, &lit, 1, rgba, stride_bytes);
}

// The antialiased lit frame: hmrm_render_shaded's of the super camera, box-filtered in the launch.  Factor 1 is
// hmrm_render_shaded, launch for launch.
int hmrm_render_shaded_aa(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_sun *sun, uint32_t shade_flags, int32_t factor,
                          uint8_t *rgba, size_t stride_bytes) {
	if (const int rc = check_shaded(sun, shade_flags)) return rc;
	const LitFrame lit = make_lit_frame(sun, shade_flags);
	return render_lit_common(scene, cam, &lit, factor, rgba, stride_bytes);
}

// ---- accumulated lit frames: the lit frame whose shadow march runs once per direction of a list, the weights summed per pixel ----
// The refusals about the planes, in the header's order; needs no scene and no device.  A stride is compared with the camera's
// width only when there is a camera with one: a camera that check_camera refuses is refused right after.
static int check_light_planes(const hmrm_light_planes *p, const hmrm_camera *cam, bool device) {
	if (!p) return fail(HMRM_E_ARG, "lit sum: NULL planes");
	if (p->reserved[0] != 0u || p->reserved[1] != 0u) return fail(HMRM_E_ARG, "hmrm_light_planes.reserved must be 0");
	if (!p->rgba && !p->light) return fail(HMRM_E_ARG, "lit sum: both planes are NULL");
	// (alignment is the device form's refusal only: host planes are reached by copies)
	const size_t width = width_or_0(cam);
	int rc;
	if ((rc = check_plane("lit sum: ", "rgba", p->rgba, p->rgba_stride, 4, width, device)) ||
	    (rc = check_plane("lit sum: ", "light", p->light, p->light_stride, 2, width, device)))
		return rc;
	return HMRM_OK;
}

// Launched the way a lit frame is (FrameRequest::own_kernels): never measured, never the probe, with the scene's current kernel.
// `device`: dirs and p hold device pointers and the launch goes to `stream` without a host sync; else the directions are staged
// through the scene's target list, the pixels through its frame buffer and the light plane through a buffer of its own, rows
// packed, and copied to the caller's behind the launch.
static int render_lit_sum_common(hmrm_scene *s, const hmrm_camera *cam, const hmrm_sun *sun, const void *dirs, int32_t n_dirs,
                                 uint32_t shade_flags, const hmrm_light_planes *p, bool device, hipStream_t stream) {
	int rc = check_shaded(sun, shade_flags);
	if (rc) return rc;
	if (!dirs) return fail(HMRM_E_ARG, "lit sum: NULL dirs");
	if (n_dirs < 1 || n_dirs > hmrm::kMaxSumDirs) return fail(HMRM_E_ARG, "lit sum: n_dirs must be 1 .. 256 (got " + std::to_string(n_dirs) + ")");
	if ((rc = check_light_planes(p, cam, device))) return rc;
	if (device && ((uintptr_t)dirs & 7u)) return fail(HMRM_E_ARG, "lit sum: d_dirs must be 8-byte aligned");
	if ((rc = check_camera(cam))) return rc;
	if (!s) return fail(HMRM_E_ARG, "NULL argument");
	const size_t W = (size_t)cam->width, H = (size_t)cam->height;
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	uint32_t *d_rgba = (uint32_t *)p->rgba;
	int64_t rgba_stride_px = (int64_t)(p->rgba_stride / 4);
	hmrm::LightSum sum{static_cast<const double *>(dirs), p->light, (int64_t)p->light_stride, n_dirs, shade_flags};
	if (!device) {
		const size_t dirs_bytes = (size_t)n_dirs * 3 * sizeof(double);
		if (p->rgba && (rc = s->d_frame.reserve(W * H * sizeof(uint32_t)))) return rc;
		if (p->light && (rc = s->d_light.reserve(W * H * sizeof(uint16_t)))) return rc;
		if ((rc = s->d_targets.reserve(dirs_bytes))) return rc; // (hmrm_cell_map_sum's staging of its targets)
		d_rgba = p->rgba ? s->d_frame.as<uint32_t>() : nullptr;
		rgba_stride_px = (int64_t)W;
		sum.dirs = s->d_targets.as<double>();
		sum.light = p->light ? s->d_light.as<uint16_t>() : nullptr;
		sum.light_stride = (int64_t)(2 * W);
		stream = s->stream;
		HIP_TRY(hipMemcpyAsync(s->d_targets.ptr, dirs, dirs_bytes, hipMemcpyHostToDevice, s->stream));
	}
	FrameSetup fs;
	if ((rc = setup_frame(s, stream, cam, 0, &fs))) return rc;
	StreamCtx *const c = fs.c;
	LitFrame lit = make_lit_frame(sun, shade_flags);
	lit.sum = &sum;
	FrameRequest req = plain_request(d_rgba, rgba_stride_px);
	req.lit = &lit;
	if ((rc = launch_frame(s, c, fs.f, fs.slot, fs.rows, req)) || device) return rc;
	if (p->rgba) HIP_TRY(hipMemcpy2DAsync(p->rgba, p->rgba_stride, d_rgba, W * 4, W * 4, H, hipMemcpyDeviceToHost, s->stream));
	if (p->light) HIP_TRY(hipMemcpy2DAsync(p->light, p->light_stride, sum.light, W * 2, W * 2, H, hipMemcpyDeviceToHost, s->stream));
	return finish_host_call(s, c);
}

int hmrm_render_lit_sum(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_sun *sun, const double *dirs, int32_t n_dirs,
                        uint32_t shade_flags, const hmrm_light_planes *host_planes) {
	return render_lit_sum_common(const_cast<hmrm_scene *>(scene), cam, sun, dirs, n_dirs, shade_flags, host_planes, false, nullptr);
}

int hmrm_render_lit_sum_device(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_sun *sun, const void *d_dirs, int32_t n_dirs,
                               uint32_t shade_flags, const hmrm_light_planes *device_planes, void *hip_stream) {
	return render_lit_sum_common(const_cast<hmrm_scene *>(scene), cam, sun, d_dirs, n_dirs, shade_flags, device_planes, true,
	                             (hipStream_t)hip_stream);
}

// ---- baked-light frames: hmrm_render's frame (hmrm_render_interior's with HMRM_TRACE_INTERIOR) whose hit pixels take the weight of
// the scene's light plane, antialiased or not ----
int hmrm_render_baked(const hmrm_scene *scene, const hmrm_camera *cam, uint32_t baked_flags, int32_t factor, uint8_t *rgba,
                      size_t stride_bytes) {
	if (const int rc = check_baked_flags(baked_flags)) return rc;
	SyncFrame how = kPlainSync;
	how.aa_factor = factor;
	how.baked = true;
	how.baked_interior = (baked_flags & HMRM_TRACE_INTERIOR) != 0u;
	return render_common(const_cast<hmrm_scene *>(scene), cam, rgba, stride_bytes, how);
}

// ---- water frames: hmrm_render's frame (hmrm_render_interior's with HMRM_TRACE_INTERIOR) whose hit pixels at or below the water
// level take their mirror ray's pixel blended in, marched by the same launch ----
// The three refusals of the header, in its order; needs no scene and no device.
static int check_water(const hmrm_water *w) {
	if (!w) return fail(HMRM_E_ARG, "NULL water");
	if (w->flags & ~(HMRM_TRACE_INTERIOR | HMRM_WATER_OWN_COLOR)) return fail(HMRM_E_ARG, "hmrm_water.flags: undefined bit");
	for (uint8_t r : w->reserved)
		if (r) return fail(HMRM_E_ARG, "hmrm_water.reserved must be 0");
	return HMRM_OK;
}

// Launched the way a lit frame is (FrameRequest::own_kernels): never measured, never the probe, with the scene's current kernel.
// With the flag every origin is tested by the kernels, whatever the projection.  `device`: `target` is device memory and the launch
// goes to `stream` without a host sync; else the frame is staged through the scene's frame buffer, rows packed, and copied to the
// caller's behind the launch.
// `factor`, `water_mode` (hmrm_render_water_aa): the super frame box-filtered inside the launch, as hmrm_render_aa's, and
// HMRM_WATER_BAKED, the frame under the scene's light plane; hmrm_render_water and hmrm_render_water_device come with 1 and 0.
// `sun`, `shade_flags` (hmrm_render_water_lit, `lit`): the sun-lit water frame -- hmrm_render_shaded's four refusals come behind the
// water's three, the primary rays are under the interior rule when either flags word asks, and the launch is the family's own.
static int check_water_mode(uint32_t water_mode) {
	if (water_mode & ~HMRM_WATER_BAKED) return fail(HMRM_E_ARG, "water_mode: undefined bit");
	return HMRM_OK;
}
static hmrm::WaterRules water_rules_of(const hmrm_water *w) {
	return hmrm::WaterRules{w->level, w->step_dist, w->max_steps, (uint32_t)w->reflectivity,
	                        (uint32_t)w->color[0] | ((uint32_t)w->color[1] << 8) | ((uint32_t)w->color[2] << 16),
	                        w->flags & HMRM_WATER_OWN_COLOR};
}
static int render_water_common(hmrm_scene *s, const hmrm_camera *cam, const hmrm_water *w, void *target, size_t stride_bytes,
                               bool device, hipStream_t stream, int32_t factor, uint32_t water_mode, bool lit = false,
                               const hmrm_sun *sun = nullptr, uint32_t shade_flags = 0u) {
	int rc = check_water(w);
	if (!rc && lit) rc = check_shaded(sun, shade_flags);
	if (rc || (rc = check_water_mode(water_mode)) || (rc = check_camera(cam))) return rc;
	hmrm_camera super;
	int aa_shift = 0;
	if ((rc = check_antialias(cam, factor, &super, &aa_shift))) return rc;
	if (!s || !target) return fail(HMRM_E_ARG, "NULL argument");
	const size_t W = (size_t)cam->width, H = (size_t)cam->height;
	if (device) {
		if ((rc = check_device_stride(cam, stride_bytes))) return rc;
	} else if (stride_bytes < W * 4) return fail(HMRM_E_ARG, "stride_bytes < width*4");
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	uint32_t *d_rgba = (uint32_t *)target;
	int64_t stride_px = (int64_t)(stride_bytes / 4);
	hmrm::BakedLight baked{nullptr, 0u};
	if ((water_mode & HMRM_WATER_BAKED) && (rc = baked_light_of(s, &baked))) return rc;
	if (!device) {
		if ((rc = s->d_frame.reserve(W * H * sizeof(uint32_t)))) return rc;
		d_rgba = s->d_frame.as<uint32_t>();
		stride_px = (int64_t)W;
		stream = s->stream;
	}
	FrameSetup fs;
	if ((rc = setup_frame(s, stream, &super, aa_shift, &fs))) return rc;
	StreamCtx *const c = fs.c;
	hmrm::WaterRules rules = water_rules_of(w);
	FrameRequest req = plain_request(d_rgba, stride_px);
	req.interior = (w->flags & HMRM_TRACE_INTERIOR) ? Interior::kByKernels : Interior::kNot;
	req.water = &rules;
	hmrm::SunRules sun_rules{};
	if (lit) {
		sun_rules = hmrm::SunRules{{sun->dir[0], sun->dir[1], sun->dir[2]}, sun->step_dist, sun->max_steps, sun->ambient};
		rules.flags |= ((shade_flags & HMRM_SHADE_DIFFUSE) ? hmrm::kWaterSunDiffuse : 0u) |
		               ((shade_flags & HMRM_SHADE_NO_SHADOWS) ? hmrm::kWaterSunNoShadows : 0u);
		if (sun->flags & HMRM_TRACE_INTERIOR) req.interior = Interior::kByKernels;
		req.water_sun = &sun_rules;
	}
	if (water_mode & HMRM_WATER_BAKED) req.baked = &baked;
	if (!device) HIP_TRY(hipEventRecord(s->ev0, s->stream)); // (the host form is timed like hmrm_render: hmrm_last_kernel_ms)
	if ((rc = launch_frame(s, c, fs.f, fs.slot, fs.rows, req)) || device) return rc;
	HIP_TRY(hipEventRecord(s->ev1, s->stream));
	HIP_TRY(hipMemcpy2DAsync(target, stride_bytes, d_rgba, W * 4, W * 4, H, hipMemcpyDeviceToHost, s->stream));
	rc = finish_host_call(s, c);
	float ms = 0.f;
	HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
	g_last_kernel_ms = ms;
	return rc;
}

int hmrm_render_water(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_water *water, uint8_t *rgba, size_t stride_bytes) {
	return render_water_common(const_cast<hmrm_scene *>(scene), cam, water, rgba, stride_bytes, false, nullptr, 1, 0u);
}

int hmrm_render_water_aa(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_water *water, uint32_t water_mode, int32_t factor,
                         uint8_t *rgba, size_t stride_bytes) {
	return render_water_common(const_cast<hmrm_scene *>(scene), cam, water, rgba, stride_bytes, false, nullptr, factor, water_mode);
}

int hmrm_render_water_device(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_water *water, void *d_rgba,
                             size_t stride_bytes, void *hip_stream) {
	return render_water_common(const_cast<hmrm_scene *>(scene), cam, water, d_rgba, stride_bytes, true, (hipStream_t)hip_stream, 1, 0u);
}

// ---- haze frames: hmrm_render's frame (hmrm_render_interior's with HMRM_TRACE_INTERIOR, hmrm_render_aa's with a factor) whose pixels
// are blended towards one colour by the byte of the caller's table at their range, in the same launch ----
// The five refusals of the header, in its order; needs no scene and no device.
static_assert(sizeof(hmrm_haze) == 32 && offsetof(hmrm_haze, color) == 24, "hmrm_haze has padding");
static int check_haze(const hmrm_haze *h, const void *table) {
	if (!h) return fail(HMRM_E_ARG, "NULL haze");
	if (h->flags & ~(HMRM_TRACE_INTERIOR | HMRM_HAZE_SKY)) return fail(HMRM_E_ARG, "hmrm_haze.flags: undefined bit");
	for (uint8_t r : h->reserved)
		if (r) return fail(HMRM_E_ARG, "hmrm_haze.reserved must be 0");
	if (h->n < 1u || h->n > (uint32_t)hmrm::kMaxHazeEntries)
		return fail(HMRM_E_ARG, "hmrm_haze.n must be 1 .. 4096 (got " + std::to_string(h->n) + ")");
	if (!table) return fail(HMRM_E_ARG, "haze: NULL table");
	return HMRM_OK;
}

// Launched the way an interior frame is (FrameRequest::own_kernels): never measured, never the probe, with the scene's current
// kernel.  With the flag every origin is tested by the kernels, whatever the projection.  `device`: `table` and `target` are device
// memory and the launch goes to `stream` without a host sync; else the table is staged through the scene's target list, as
// hmrm_render_lit_sum's directions are, the frame through the scene's frame buffer, rows packed, and copied to the caller's behind
// the launch.
static int render_haze_common(hmrm_scene *s, const hmrm_camera *cam, const hmrm_haze *h, const void *table, int32_t factor, void *target,
                              size_t stride_bytes, bool device, hipStream_t stream) {
	int rc = check_haze(h, table);
	if (rc) return rc;
	if (factor != 1 && factor != 2 && factor != 4 && factor != 8) // (check_antialias's own refusal, ahead of the camera it needs for the rest)
		return fail(HMRM_E_ARG, "antialias factor must be 1, 2, 4 or 8 (got " + std::to_string(factor) + ")");
	if ((rc = check_camera(cam))) return rc;
	hmrm_camera super;
	int aa_shift = 0;
	if ((rc = check_antialias(cam, factor, &super, &aa_shift))) return rc;
	if (!s || !target) return fail(HMRM_E_ARG, "NULL argument");
	const size_t W = (size_t)cam->width, H = (size_t)cam->height;
	if (device) {
		if ((rc = check_device_stride(cam, stride_bytes))) return rc;
	} else if (stride_bytes < W * 4) return fail(HMRM_E_ARG, "stride_bytes < width*4");
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	uint32_t *d_rgba = (uint32_t *)target;
	int64_t stride_px = (int64_t)(stride_bytes / 4);
	hmrm::HazeRules rules{static_cast<const uint8_t *>(table), h->start, h->scale, h->n,
	                      (uint32_t)h->color[0] | ((uint32_t)h->color[1] << 8) | ((uint32_t)h->color[2] << 16), h->flags & HMRM_HAZE_SKY};
	if (!device) {
		if ((rc = s->d_frame.reserve(W * H * sizeof(uint32_t))) || (rc = s->d_targets.reserve((size_t)h->n))) return rc;
		d_rgba = s->d_frame.as<uint32_t>();
		stride_px = (int64_t)W;
		stream = s->stream;
		rules.table = s->d_targets.as<uint8_t>();
		HIP_TRY(hipMemcpyAsync(s->d_targets.ptr, table, (size_t)h->n, hipMemcpyHostToDevice, s->stream));
	}
	FrameSetup fs;
	if ((rc = setup_frame(s, stream, &super, aa_shift, &fs))) return rc;
	StreamCtx *const c = fs.c;
	FrameRequest req = plain_request(d_rgba, stride_px);
	req.interior = (h->flags & HMRM_TRACE_INTERIOR) ? Interior::kByKernels : Interior::kNot;
	req.haze = &rules;
	if (!device) HIP_TRY(hipEventRecord(s->ev0, s->stream)); // (the host form is timed like hmrm_render: hmrm_last_kernel_ms)
	if ((rc = launch_frame(s, c, fs.f, fs.slot, fs.rows, req)) || device) return rc;
	HIP_TRY(hipEventRecord(s->ev1, s->stream));
	HIP_TRY(hipMemcpy2DAsync(target, stride_bytes, d_rgba, W * 4, W * 4, H, hipMemcpyDeviceToHost, s->stream));
	rc = finish_host_call(s, c);
	float ms = 0.f;
	HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
	g_last_kernel_ms = ms;
	return rc;
}

int hmrm_render_haze(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_haze *haze, const uint8_t *table, int32_t factor,
                     uint8_t *rgba, size_t stride_bytes) {
	return render_haze_common(const_cast<hmrm_scene *>(scene), cam, haze, table, factor, rgba, stride_bytes, false, nullptr);
}

int hmrm_render_haze_device(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_haze *haze, const void *d_table, int32_t factor,
                            void *d_rgba, size_t stride_bytes, void *hip_stream) {
	return render_haze_common(const_cast<hmrm_scene *>(scene), cam, haze, d_table, factor, d_rgba, stride_bytes, true,
	                          (hipStream_t)hip_stream);
}

// ---- view batches: n cameras of one scene in one launch; view k is hmrm_render's frame of cams[k] (hmrm_render_interior's with
// HMRM_TRACE_INTERIOR) ----
// Which spherical tables the views of a batch use, deduplicated within the batch: views that agree in (hang, hfov, width) -- bit
// for bit -- share a pair of column tables, views that agree in (vang, hfov, width, height) a pair of row tables; tables are
// numbered in the order of their first view, whose index goes to *_first.  Another projection has no tables: every index -1.
struct ViewTables {
	std::vector<int32_t> col_of, row_of;       // per view
	std::vector<int32_t> col_first, row_first; // per table: the first view that uses it
};
static uint64_t bits_of(double v) {
	uint64_t b;
	memcpy(&b, &v, sizeof b);
	return b;
}
static void plan_view_tables(const hmrm_camera *cams, int32_t n, ViewTables *t) {
	t->col_of.assign((size_t)n, -1);
	t->row_of.assign((size_t)n, -1);
	t->col_first.clear();
	t->row_first.clear();
	if (cams[0].projection != HMRM_SPHERICAL) return;
	// (width and height are the batch's: the keys are the angles and hfov)
	std::map<std::pair<uint64_t, uint64_t>, int32_t> cols, rows;
	for (int32_t k = 0; k < n; ++k) {
		const uint64_t fov = bits_of(cams[k].hfov);
		auto c = cols.emplace(std::make_pair(bits_of(cams[k].hang), fov), (int32_t)t->col_first.size());
		if (c.second) t->col_first.push_back(k);
		t->col_of[(size_t)k] = c.first->second;
		auto r = rows.emplace(std::make_pair(bits_of(cams[k].vang), fov), (int32_t)t->row_first.size());
		if (r.second) t->row_first.push_back(k);
		t->row_of[(size_t)k] = r.first->second;
	}
}

// The refusals of the header, in its order; needs no scene and no device.
static int check_views(const void *scene, const hmrm_camera *cams, int32_t n, uint32_t flags, const void *target, size_t stride_bytes,
                       size_t view_stride_bytes, bool device) {
	if (!cams) return fail(HMRM_E_ARG, "views: NULL cams");
	if (n < 1 || n > HMRM_MAX_VIEWS) return fail(HMRM_E_ARG, "views: n must be 1 .. 65536 (got " + std::to_string(n) + ")");
	if (flags & ~HMRM_TRACE_INTERIOR) return fail(HMRM_E_ARG, "views: flags: undefined bit");
	for (int32_t k = 1; k < n; ++k) {
		const char *field = cams[k].width != cams[0].width ? "width" : cams[k].height != cams[0].height ? "height"
		                    : cams[k].projection != cams[0].projection ? "projection" : cams[k].sampling != cams[0].sampling ? "sampling" : nullptr;
		if (field) return fail(HMRM_E_ARG, "views: view " + std::to_string(k) + " differs from view 0 in " + field + ", which a batch shares");
	}
	int rc = check_camera(&cams[0]); // (hmrm_render's camera rules look at the four shared fields only)
	if (rc) return rc;
	if (!scene || !target) return fail(HMRM_E_ARG, "NULL argument");
	const size_t W = (size_t)cams[0].width, H = (size_t)cams[0].height;
	if (device) {
		if ((rc = check_device_stride(&cams[0], stride_bytes))) return rc;
	} else if (stride_bytes < W * 4) return fail(HMRM_E_ARG, "stride_bytes < width*4");
	// (the host form takes any stride: the products are made in 128 bits)
	const unsigned __int128 view_bytes = (unsigned __int128)H * stride_bytes;
	if (view_stride_bytes < view_bytes || (device && (view_stride_bytes & 3)))
		return fail(HMRM_E_ARG, device ? "views: view_stride_bytes must be >= height * stride_bytes and a multiple of 4"
		                               : "views: view_stride_bytes must be >= height * stride_bytes");
	if ((unsigned __int128)(n - 1) * view_stride_bytes + (unsigned __int128)(H - 1) * stride_bytes + W * 4 > ((unsigned __int128)1 << 40))
		return fail(HMRM_E_ARG, "views: the batch's last byte lies at or beyond 2^40");
	int tile_w = 1, tile_h = 1;
	hmrm::render_tile_shape(&tile_w, &tile_h);
	if ((int64_t)n * (int64_t)((H + (size_t)tile_h - 1) / (size_t)tile_h) > (int64_t)65535 * 32768)
		return fail(HMRM_E_ARG, "views: the batch has more tile rows than a launch's grid holds (65535 * 32768)");
	return HMRM_OK;
}

// One batch.  `device`: `target` is device memory and everything goes to `stream` without a host wait; else the batch is rendered
// into the scene's frame buffer, views and rows packed, on the scene's stream and copied to the caller's behind the launch.
static int render_views_common(hmrm_scene *s, const hmrm_camera *cams, int32_t n, uint32_t flags, void *target, size_t stride_bytes,
                               size_t view_stride_bytes, bool device, hipStream_t stream) {
	int rc = check_views(s, cams, n, flags, target, stride_bytes, view_stride_bytes, device);
	if (rc) return rc;
	const size_t W = (size_t)cams[0].width, H = (size_t)cams[0].height;
	const bool spherical = cams[0].projection == HMRM_SPHERICAL;
	ViewTables tables;
	plan_view_tables(cams, n, &tables);
	constexpr size_t kRecDoubles = sizeof(hmrm::DevFrame) / sizeof(double);
	static_assert(sizeof(hmrm::DevFrame) % sizeof(double) == 0, "the records are uploaded as doubles");
	const size_t n_col = tables.col_first.size(), n_row = tables.row_first.size();
	const size_t col_base = (size_t)n * kRecDoubles, row_base = col_base + n_col * 2 * W, total = row_base + n_row * 2 * H;
	if (total * sizeof(double) > kMaxViewStagingBytes)
		return fail(HMRM_E_ARG, "views: the batch's records and distinct spherical tables exceed 256 MiB (" + std::to_string(n_col) +
		                            " column and " + std::to_string(n_row) + " row tables)");
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	uint32_t *d_rgba = (uint32_t *)target;
	int64_t stride_px = (int64_t)(stride_bytes / 4), view_stride_px = (int64_t)(view_stride_bytes / 4);
	if (!device) {
		if ((rc = s->d_frame.reserve((size_t)n * W * H * sizeof(uint32_t)))) return rc;
		d_rgba = s->d_frame.as<uint32_t>();
		stride_px = (int64_t)W;
		view_stride_px = (int64_t)(W * H);
		stream = s->stream;
	}
	StreamCtx *c = nullptr;
	if ((rc = ctx_for(s, stream, &c))) return rc;
	if (cams[0].sampling == HMRM_BILINEAR && (rc = ensure_bilinear_pyramid(s))) return rc;
	ViewsKernel kern;
	if ((rc = pick_views_kernel(s, c, cams[0].sampling, &kern))) return rc;
	// the device arena: only grows; one that launches of this stream may still read is retired, not freed
	for (size_t i = c->retired_views.size(); i-- > 0;) {
		const hipError_t e = hipEventQuery(c->retired_views[i].after);
		if (e == hipErrorNotReady) (void)hipGetLastError();
		if (e != hipSuccess) continue;
		(void)hipEventDestroy(c->retired_views[i].after);
		(void)hipFree(c->retired_views[i].ptr);
		c->retired_views.erase(c->retired_views.begin() + (long)i);
	}
	if (total > c->d_views_cap) {
		if (c->d_views) {
			RetiredArena r{c->d_views, nullptr};
			HIP_TRY(hipEventCreateWithFlags(&r.after, hipEventDisableTiming));
			HIP_TRY(hipEventRecord(r.after, c->stream));
			c->retired_views.push_back(r);
			c->d_views = nullptr;
		}
		const size_t cap = std::max(total, 2 * c->d_views_cap);
		c->d_views_cap = 0;
		HIP_TRY(hipMalloc((void **)&c->d_views, cap * sizeof(double)));
		c->d_views_cap = cap;
	}
	ViewStage *stage = nullptr;
	if ((rc = acquire_view_stage(c, total, ++s->clock, &stage))) return rc;
	double *const h = stage->h, *const d = c->d_views;
	const bool interior = (flags & HMRM_TRACE_INTERIOR) != 0;
	const bool records = !kern.literal && kern.kind == hmrm::kRecords;
	// the records: build_frame per camera (glibc's trig: the bits of n single renders), the scene's part and the knobs as a
	// single frame gets them, the tables' places in the arena; spread over the host pool for large n
	hmrm::parallel_ranges(n, 256, [&](int b, int e) {
		for (int k = b; k < e; ++k) {
			hmrm::HostCamera hc;
			to_host_camera(&cams[k], &hc);
			hmrm::DevFrame fr{};
			hmrm::build_frame(hc, s->map_w, s->map_h, s->params.min_height, s->params.max_height, s->params.grid_width, &fr, nullptr, nullptr,
			                  nullptr, nullptr);
			finish_frame_record(s, cams[k].sampling, &fr);
			apply_scene_knobs(s, &fr);
			fr.aa_shift = 0;
			if (records) fr.mipbuf_bil = reinterpret_cast<const float *>(s->d_records); // (launch_common.hpp select_tables)
			if (spherical) {
				const double *cc = d + col_base + (size_t)tables.col_of[(size_t)k] * 2 * W;
				const double *rs = d + row_base + (size_t)tables.row_of[(size_t)k] * 2 * H;
				fr.col_cos_ha = cc;
				fr.col_sin_ha = cc + W;
				fr.row_sin_va = rs;
				fr.row_cos_va = rs + H;
			}
			memcpy(h + (size_t)k * kRecDoubles, &fr, sizeof fr);
		}
	});
	// the distinct tables: items [0, n_col * W) are columns, the rest rows
	if (spherical) {
		const int64_t items = (int64_t)(n_col * W + n_row * H);
		// (W, H <= 2^29 and the arena's limit keep `items` far below 2^31)
		hmrm::parallel_ranges((int)items, 1024, [&](int b, int e) {
			int64_t i = b;
			while (i < e) {
				const bool col = i < (int64_t)(n_col * W);
				const int64_t j = col ? i : i - (int64_t)(n_col * W);
				const int64_t side = col ? (int64_t)W : (int64_t)H;
				const int64_t t = j / side, first = j - t * side;
				const int64_t last = std::min<int64_t>(side, first + (e - i));
				hmrm::HostCamera hc;
				to_host_camera(&cams[col ? tables.col_first[(size_t)t] : tables.row_first[(size_t)t]], &hc);
				if (col) hmrm::fill_col_tables(hc, (int32_t)first, (int32_t)last, h + col_base + (size_t)t * 2 * W, h + col_base + (size_t)t * 2 * W + W);
				else hmrm::fill_row_tables(hc, (int32_t)first, (int32_t)last, h + row_base + (size_t)t * 2 * H, h + row_base + (size_t)t * 2 * H + H);
				i += last - first;
			}
		});
	}
	// stream order puts the upload behind every earlier kernel of this stream that read the arena and in front of the batch's own
	HIP_TRY(hmrm::launch_upload_tables(stage->h_dev, d, total, c->stream));
	HIP_TRY(hipEventRecord(stage->uploaded, c->stream));
	stage->used = true;
	hmrm::DevFrame f0;
	memcpy(&f0, h, sizeof f0);
	if (!device) HIP_TRY(hipEventRecord(s->ev0, s->stream)); // (the host form is timed like hmrm_render: hmrm_last_kernel_ms)
	if ((rc = launch_views(s, c, kern, f0, reinterpret_cast<const hmrm::DevFrame *>(d), n, interior, d_rgba, stride_px, view_stride_px)) || device)
		return rc;
	HIP_TRY(hipEventRecord(s->ev1, s->stream));
	if (view_stride_bytes == H * stride_bytes) // (the views' rows are equally spaced: one copy)
		HIP_TRY(hipMemcpy2DAsync(target, stride_bytes, d_rgba, W * 4, W * 4, (size_t)n * H, hipMemcpyDeviceToHost, s->stream));
	else
		for (int32_t k = 0; k < n; ++k)
			HIP_TRY(hipMemcpy2DAsync((uint8_t *)target + (size_t)k * view_stride_bytes, stride_bytes, d_rgba + (size_t)k * W * H, W * 4, W * 4, H,
			                         hipMemcpyDeviceToHost, s->stream));
	rc = finish_host_call(s, c);
	float ms = 0.f;
	HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
	g_last_kernel_ms = ms;
	return rc;
}

int hmrm_render_views(const hmrm_scene *scene, const hmrm_camera *cams, int32_t n, uint32_t flags, uint8_t *rgba, size_t stride_bytes,
                      size_t view_stride_bytes) {
	return render_views_common(const_cast<hmrm_scene *>(scene), cams, n, flags, rgba, stride_bytes, view_stride_bytes, false, nullptr);
}

int hmrm_render_views_device(const hmrm_scene *scene, const hmrm_camera *cams, int32_t n, uint32_t flags, void *d_rgba, size_t stride_bytes,
                             size_t view_stride_bytes, void *hip_stream) {
	return render_views_common(const_cast<hmrm_scene *>(scene), cams, n, flags, d_rgba, stride_bytes, view_stride_bytes, true,
	                           (hipStream_t)hip_stream);
}

int hmrm_debug_views_tables(const hmrm_camera *cams, int32_t n, int32_t *out_col_index, int32_t *out_row_index) {
	if (!cams || !out_col_index || !out_row_index) return fail(HMRM_E_ARG, "NULL argument");
	if (n < 1 || n > HMRM_MAX_VIEWS) return fail(HMRM_E_ARG, "views: n must be 1 .. 65536 (got " + std::to_string(n) + ")");
	ViewTables t;
	plan_view_tables(cams, n, &t);
	memcpy(out_col_index, t.col_of.data(), (size_t)n * sizeof(int32_t));
	memcpy(out_row_index, t.row_of.data(), (size_t)n * sizeof(int32_t));
	return HMRM_OK;
}

// The sun-lit water frame: hmrm_render_water and hmrm_render_shaded composed, in one launch of a family of its own.
int hmrm_render_water_lit(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_water *water, const hmrm_sun *sun,
                          uint32_t shade_flags, uint8_t *rgba, size_t stride_bytes) {
	return render_water_common(const_cast<hmrm_scene *>(scene), cam, water, rgba, stride_bytes, false, nullptr, 1, 0u, true, sun, shade_flags);
}

int hmrm_render_water_lit_device(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_water *water, const hmrm_sun *sun,
                                 uint32_t shade_flags, void *d_rgba, size_t stride_bytes, void *hip_stream) {
	return render_water_common(const_cast<hmrm_scene *>(scene), cam, water, d_rgba, stride_bytes, true, (hipStream_t)hip_stream, 1, 0u,
	                           true, sun, shade_flags);
}

int hmrm_render_stats(const hmrm_scene *scene, const hmrm_camera *cam, uint8_t *rgba,
                      size_t stride_bytes, hmrm_stats *stats, uint32_t *steps_per_pixel, double *entry_d) {
	return render_common(const_cast<hmrm_scene *>(scene), cam, rgba, stride_bytes,
	                     SyncFrame{stats, steps_per_pixel, entry_d, true, 1, false, nullptr});
}

int hmrm_render_rows_device(const hmrm_scene *scene, const hmrm_camera *cam, void *d_rgba,
                            size_t stride_bytes, int32_t row_begin, int32_t row_end, int32_t band_rows,
                            int32_t band_index, int32_t band_count, void *hip_stream) {
	hmrm_scene *s = const_cast<hmrm_scene *>(scene);
	int rc = check_camera(cam);
	if (rc) return rc;
	if (!s || !d_rgba) return fail(HMRM_E_ARG, "NULL argument");
	if ((rc = check_device_stride(cam, stride_bytes))) return rc;
	hmrm::RowMap rows{};
	if (band_rows > 0) {
		if (band_count <= 0 || band_index < 0 || band_index >= band_count)
			return fail(HMRM_E_ARG, "bad band_index/band_count");
		// bands band_index, band_index+band_count, ... packed back to back; a trailing
		// partial band still occupies band_rows rows of the strip (its tail is not written)
		const int64_t local = hmrm_band_local_rows(cam->height, band_rows, band_index, band_count);
		rows.row_begin = 0;
		rows.local_rows = (int32_t)local;
		rows.band_rows = band_rows;
		rows.band_index = band_index;
		rows.band_count = band_count;
	} else {
		if (row_begin < 0 || row_end > cam->height || row_begin > row_end)
			return fail(HMRM_E_ARG, "bad row range");
		rows.row_begin = row_begin;
		rows.local_rows = row_end - row_begin;
		rows.band_rows = 0;
		rows.band_index = 0;
		rows.band_count = 1;
	}
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	FrameSetup fs;
	if ((rc = setup_frame(s, (hipStream_t)hip_stream, cam, 0, &fs))) return rc;
	return launch_frame(s, fs.c, fs.f, fs.slot, rows, plain_request((uint32_t *)d_rgba, (int64_t)(stride_bytes / 4)));
}

// One frame over several scenes -- one per GPU, same maps (BASELINE config C4's sharding):
// scene i renders the cyclic 16-row bands i, i+n, ... into a strip on its own device and the strip crosses
// its own PCIe link; no exchange between devices (a gather to one GPU first would funnel every byte through
// that GPU's link).  Three passes so that no device ever waits for another one's copy:
//   1. every scene's kernel is launched (asynchronous);
//   2. every scene's device-to-host copy is enqueued behind its kernel.  A copy into PAGEABLE host memory is staged
//      by the runtime and blocks the calling thread until it is done -- device i+1's copy would start after device
//      i's had finished -- so the copies go to the caller's frame directly only when that memory is pinned (the
//      caller registered it, hipHostRegister, or got it from hipHostMalloc), else to a pinned staging strip the
//      scene owns;
//   3. scenes are waited for in order and staged strips are copied into the caller's rows by the host pool while
//      the later devices' copies are still in flight.
int hmrm_render_multi(hmrm_scene *const *scenes, int32_t n_scenes, const hmrm_camera *cam, uint8_t *rgba,
                      size_t stride_bytes) {
	int rc = check_camera(cam);
	if (rc) return rc;
	if (!scenes || n_scenes <= 0 || !rgba) return fail(HMRM_E_ARG, "NULL argument");
	const size_t W = (size_t)cam->width;
	const int H = cam->height;
	if (stride_bytes < W * 4) return fail(HMRM_E_ARG, "stride_bytes < width*4");
	constexpr int kBand = 16;
	const int n = std::min<int>(n_scenes, (H + kBand - 1) / kBand);
	for (int i = 0; i < n; ++i)
		if (!scenes[i]) return fail(HMRM_E_ARG, "NULL scene");
	// is the caller's frame pinned?  (an address the runtime does not know is ordinary pageable memory: the query
	// fails with hipErrorInvalidValue, which is not an error of this call)
	bool pinned_dst = false;
	{
		// (first AND last byte: a frame only partly inside a registered block would send the later bands' copies
		// through the runtime's staging, which blocks the calling thread per band)
		hipPointerAttribute_t attr{}, attr_end{};
		const uint8_t *last = rgba + (size_t)(H - 1) * stride_bytes + W * 4 - 1;
		if (hipPointerGetAttributes(&attr, rgba) == hipSuccess && hipPointerGetAttributes(&attr_end, last) == hipSuccess)
			pinned_dst = attr.type == hipMemoryTypeHost && attr_end.type == hipMemoryTypeHost;
		else (void)hipGetLastError();
	}
	int launched = 0; // scenes with work in flight: drained before an error return (the caller may free `rgba` at once)
	auto drain = [&](int rc_keep) -> int {
		const std::string keep = g_error;
		for (int j = 0; j < launched; ++j)
			if (hipSetDevice(scenes[j]->device) == hipSuccess) (void)hipStreamSynchronize(scenes[j]->stream);
		g_error = keep;
		return rc_keep;
	};
	auto launch = [&](int i) -> int {
		hmrm_scene *s = scenes[i];
		HIP_TRY(hipSetDevice(s->device));
		std::lock_guard<std::mutex> lk(s->mu);
		const int32_t local = hmrm_band_local_rows(H, kBand, i, n);
		int rc2;
		if ((rc2 = s->d_frame.reserve(W * 4 * (size_t)local))) return rc2;
		if (!pinned_dst && (rc2 = s->h_stage.reserve(W * 4 * (size_t)local))) return rc2;
		FrameSetup fs;
		if ((rc2 = setup_frame(s, s->stream, cam, 0, &fs))) return rc2;
		hmrm::RowMap rows{0, local, kBand, i, n, {}, {}, nullptr};
		return launch_frame(s, fs.c, fs.f, fs.slot, rows, plain_request(s->d_frame.as<uint32_t>(), (int64_t)W));
	};
	auto enqueue_copy = [&](int i) -> int {
		hmrm_scene *s = scenes[i];
		HIP_TRY(hipSetDevice(s->device));
		const int32_t local = hmrm_band_local_rows(H, kBand, i, n);
		if (!pinned_dst) { // the whole strip in one transfer
			HIP_TRY(hipMemcpyAsync(s->h_stage.ptr, s->d_frame.ptr, W * 4 * (size_t)local, hipMemcpyDeviceToHost, s->stream));
			return HMRM_OK;
		}
		// band b of this scene's strip is frame rows [(i + b*n) * kBand, ...): contiguous in both
		for (int b = 0; (i + b * n) * kBand < H; ++b) {
			const int row0 = (i + b * n) * kBand, nrows = std::min(kBand, H - row0);
			HIP_TRY(hipMemcpy2DAsync(rgba + (size_t)row0 * stride_bytes, stride_bytes,
			                         s->d_frame.as<uint32_t>() + (size_t)b * kBand * W, W * 4, W * 4, (size_t)nrows,
			                         hipMemcpyDeviceToHost, s->stream));
		}
		return HMRM_OK;
	};
	for (int i = 0; i < n; ++i) {
		rc = launch(i);
		launched = i + 1; // (a failed launch may still have enqueued a table upload)
		if (rc != HMRM_OK) return drain(rc);
	}
	for (int i = 0; i < n; ++i)
		if ((rc = enqueue_copy(i)) != HMRM_OK) return drain(rc);
	unsigned long long capped = 0;
	for (int i = 0; i < n; ++i) {
		hmrm_scene *s = scenes[i];
		hipError_t e = hipSetDevice(s->device);
		if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
		if (e != hipSuccess) return drain(fail(HMRM_E_DEVICE, std::string("hmrm_render_multi: ") + hipGetErrorString(e)));
		if (!pinned_dst) {
			const int bands = (H - i * kBand + n * kBand - 1) / (n * kBand); // bands i, i+n, .. below H
			const uint8_t *src = s->h_stage.as<uint8_t>();
			hmrm::parallel_ranges(bands, 4, [&](int b0, int b1) {
				for (int b = b0; b < b1; ++b) {
					const int row0 = (i + b * n) * kBand, nrows = std::min(kBand, H - row0);
					for (int r = 0; r < nrows; ++r)
						memcpy(rgba + (size_t)(row0 + r) * stride_bytes, src + ((size_t)b * kBand + (size_t)r) * W * 4, W * 4);
				}
			});
		}
		std::lock_guard<std::mutex> lk(s->mu);
		StreamCtx *c = nullptr;
		if ((rc = ctx_for(s, s->stream, &c))) return drain(rc);
		unsigned long long here = 0;
		if ((rc = take_capped(c, &here))) return drain(rc);
		capped += here;
	}
	return noterm(capped);
}

int hmrm_scene_take_capped(const hmrm_scene *scene, void *hip_stream, uint64_t *capped) {
	hmrm_scene *s = const_cast<hmrm_scene *>(scene);
	if (!s || !capped) return fail(HMRM_E_ARG, "NULL argument");
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	*capped = 0;
	for (StreamCtx *c : s->ctxs)
		if (c->stream == (hipStream_t)hip_stream) {
			HIP_TRY(hipStreamSynchronize(c->stream));
			unsigned long long n = 0;
			const int rc = take_capped(c, &n);
			if (rc) return rc;
			*capped = n;
			return noterm(n);
		}
	return HMRM_OK; // nothing was ever launched on that stream
}

// ---- asynchronous frames: kernel k+1 runs while frame k crosses PCIe (the reference's counterpart is
// the blit of the finished framebuffer, SDL_UpdateTexture, hmap.cpp:1082) ----
int hmrm_render_begin(const hmrm_scene *scene, const hmrm_camera *cam, int32_t *ticket) {
	return hmrm_render_begin_flags(scene, cam, 0u, ticket);
}

// What both ticketed begins refuse first, in this order: the camera, the flags and their antialias factor (-> the super camera
// and the log2 of the factor), NULL arguments (`have_target`: the device begin's d_rgba is there).  *ticket is -1 from then on.
static int check_begin(const hmrm_scene *s, const hmrm_camera *cam, uint32_t flags, bool have_target, int32_t *ticket, hmrm_camera *super,
                       int *aa_shift) {
	int rc = check_camera(cam);
	if (rc) return rc;
	int32_t aa_factor = 1;
	if ((rc = antialias_of_flags(flags, &aa_factor)) || (rc = check_antialias(cam, aa_factor, super, aa_shift))) return rc;
	if (!s || !have_target || !ticket) return fail(HMRM_E_ARG, "NULL argument");
	*ticket = -1;
	return HMRM_OK;
}
// The request of a ticketed frame: never instrumented, never interior; HMRM_NO_PROBE from the flags.
static FrameRequest ticket_request(uint32_t *d_out, int64_t out_stride_px, uint32_t flags, const LitFrame *lit) {
	return FrameRequest{d_out, out_stride_px, nullptr, nullptr, false, (flags & HMRM_NO_PROBE) != 0, Interior::kNot, lit};
}

// A baked ticket (hmrm_render_baked_begin, hmrm_render_baked_device_begin).  The plane is looked up under the lock
// and goes into the launch by value: a later hmrm_scene_set_light drains the lane before it touches the plane.
struct BakedTicket {
	bool on = false;
	bool interior = false;
};
static int apply_baked(const hmrm_scene *s, const BakedTicket &bt, hmrm::BakedLight *light, FrameRequest *req) {
	if (!bt.on) return HMRM_OK;
	if (const int rc = baked_light_of(s, light)) return rc;
	req->baked = light;
	req->interior = bt.interior ? Interior::kByKernels : Interior::kNot;
	return HMRM_OK;
}

// A water ticket (hmrm_render_water_begin, hmrm_render_water_device_begin): the rules, made from the caller's hmrm_water before the
// begin and copied into the launch; `baked`: under the light plane, looked up under the lock as a baked ticket's is.
struct WaterTicket {
	const hmrm::WaterRules *rules = nullptr;
	bool baked = false;
	bool interior = false;
};
static int apply_water(const hmrm_scene *s, const WaterTicket &wt, hmrm::BakedLight *light, FrameRequest *req) {
	if (!wt.rules) return HMRM_OK;
	if (wt.baked) {
		if (const int rc = baked_light_of(s, light)) return rc;
		req->baked = light;
	}
	req->water = wt.rules;
	req->interior = wt.interior ? Interior::kByKernels : Interior::kNot;
	return HMRM_OK;
}

// `lit` (hmrm_render_shaded_begin): the ticket's frame is a lit one -- launched the way a lit frame is (launch_frame), on the lane.
static int begin_common(const hmrm_scene *scene, const hmrm_camera *cam, uint32_t flags, int32_t *ticket, const LitFrame *lit,
                        const BakedTicket &bt = BakedTicket{}, const WaterTicket &wt = WaterTicket{}) {
	hmrm_scene *s = const_cast<hmrm_scene *>(scene);
	hmrm_camera super;
	int aa_shift = 0;
	int rc = check_begin(s, cam, flags, true, ticket, &super, &aa_shift);
	if (rc) return rc;
	const size_t W = (size_t)cam->width, H = (size_t)cam->height;
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	hmrm::BakedLight light{nullptr, 0u};
	FrameRequest req = ticket_request(nullptr, (int64_t)W, flags, lit);
	if ((rc = apply_baked(s, bt, &light, &req)) || (rc = apply_water(s, wt, &light, &req))) return rc;
	int idx = -1;
	if ((rc = acquire_ticket(s->ring, "hmrm_render_begin", "every frame of the ring is in use (release one)", &idx))) return rc;
	RingFrame *r = s->ring[(size_t)idx];
	// (the slot is free: nothing in flight touches its buffers)
	if ((rc = r->d_frame.reserve(W * H * 4)) || (rc = r->h_frame.reserve(W * H * 4))) return rc;
	hipStream_t lane = nullptr;
	FrameSetup fs;
	if ((rc = next_lane(s, &lane)) || (rc = setup_frame(s, lane, &super, aa_shift, &fs))) return rc;
	req.d_out = r->d_frame.as<uint32_t>();
	if ((rc = launch_frame(s, fs.c, fs.f, fs.slot, fs.rows, req))) return rc;
	StreamCtx *const c = fs.c;
	r->ctx = c;
	HIP_TRY(hipEventRecord(r->kernel_done, c->stream));
	HIP_TRY(hipStreamWaitEvent(s->copy_stream, r->kernel_done, 0));
	HIP_TRY(hipMemcpyAsync(r->h_frame.ptr, r->d_frame.ptr, W * H * 4, hipMemcpyDeviceToHost, s->copy_stream));
	HIP_TRY(hipMemcpyAsync(r->h_capped, c->d_counters + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost,
	                       s->copy_stream));
	HIP_TRY(hipEventRecord(r->copy_done, s->copy_stream));
	r->width = cam->width;
	r->height = cam->height;
	r->busy = true;
	*ticket = idx;
	return HMRM_OK;
}

int hmrm_render_begin_flags(const hmrm_scene *scene, const hmrm_camera *cam, uint32_t flags, int32_t *ticket) {
	return begin_common(scene, cam, flags, ticket, nullptr);
}

// (the sun goes into the launch by value -- SunRules is a kernel argument -- so the caller's hmrm_sun need not outlive the call)
int hmrm_render_shaded_begin(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_sun *sun, uint32_t shade_flags, uint32_t flags,
                             int32_t *ticket) {
	if (const int rc = check_shaded(sun, shade_flags)) return rc;
	const LitFrame lit = make_lit_frame(sun, shade_flags);
	return begin_common(scene, cam, flags, ticket, &lit);
}

int hmrm_render_wait(const hmrm_scene *scene, int32_t ticket, const uint8_t **rgba, size_t *stride_bytes) {
	hmrm_scene *s = const_cast<hmrm_scene *>(scene);
	if (!s || !rgba) return fail(HMRM_E_ARG, "NULL argument");
	RingFrame *r = nullptr;
	{
		std::lock_guard<std::mutex> lk(s->mu);
		if (ticket < 0 || ticket >= (int)s->ring.size() || !s->ring[(size_t)ticket]->busy)
			return fail(HMRM_E_ARG, "hmrm_render_wait: no such frame in flight");
		r = s->ring[(size_t)ticket];
	}
	HIP_TRY(hipSetDevice(s->device));
	HIP_TRY(hipEventSynchronize(r->copy_done)); // (outside the lock: other threads may begin frames meanwhile)
	*rgba = r->h_frame.as<uint8_t>();
	if (stride_bytes) *stride_bytes = (size_t)r->width * 4;
	std::lock_guard<std::mutex> lk(s->mu);
	return noterm(new_capped(r->ctx, *r->h_capped));
}

void hmrm_render_release(const hmrm_scene *scene, int32_t ticket) {
	hmrm_scene *s = const_cast<hmrm_scene *>(scene);
	if (!s) return;
	std::lock_guard<std::mutex> lk(s->mu);
	if (ticket < 0 || ticket >= (int)s->ring.size()) return;
	RingFrame *r = s->ring[(size_t)ticket];
	if (!r->busy) return;
	(void)hipSetDevice(s->device);
	(void)hipEventSynchronize(r->copy_done); // never hand a slot back while the copy engine writes it
	r->busy = false;
}

// ---- frames into device memory through the launch lanes ----
int hmrm_render_device_begin(const hmrm_scene *scene, const hmrm_camera *cam, void *d_rgba, size_t stride_bytes, int32_t *ticket) {
	return hmrm_render_device_begin_flags(scene, cam, d_rgba, stride_bytes, 0u, ticket);
}

static int device_begin_common(const hmrm_scene *scene, const hmrm_camera *cam, void *d_rgba, size_t stride_bytes, uint32_t flags,
                               int32_t *ticket, const LitFrame *lit, const BakedTicket &bt = BakedTicket{},
                               const WaterTicket &wt = WaterTicket{}) {
	hmrm_scene *s = const_cast<hmrm_scene *>(scene);
	hmrm_camera super;
	int aa_shift = 0;
	int rc = check_begin(s, cam, flags, d_rgba != nullptr, ticket, &super, &aa_shift);
	if (rc || (rc = check_device_stride(cam, stride_bytes))) return rc;
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	hmrm::BakedLight light{nullptr, 0u};
	FrameRequest req = ticket_request((uint32_t *)d_rgba, (int64_t)(stride_bytes / 4), flags, lit);
	if ((rc = apply_baked(s, bt, &light, &req)) || (rc = apply_water(s, wt, &light, &req))) return rc;
	int idx = -1;
	if ((rc = acquire_ticket(s->dev_tickets, "hmrm_render_device_begin", "64 frames in flight (wait for one)", &idx))) return rc;
	DevTicket *t = s->dev_tickets[(size_t)idx];
	hipStream_t lane = nullptr;
	FrameSetup fs;
	if ((rc = next_lane(s, &lane)) || (rc = setup_frame(s, lane, &super, aa_shift, &fs))) return rc;
	if ((rc = launch_frame(s, fs.c, fs.f, fs.slot, fs.rows, req))) return rc;
	StreamCtx *const c = fs.c;
	HIP_TRY(hipMemcpyAsync(t->h_capped, c->d_counters + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipEventRecord(t->done, c->stream));
	t->ctx = c;
	t->busy = true;
	*ticket = idx;
	return HMRM_OK;
}

int hmrm_render_device_begin_flags(const hmrm_scene *scene, const hmrm_camera *cam, void *d_rgba, size_t stride_bytes, uint32_t flags,
                                   int32_t *ticket) {
	return device_begin_common(scene, cam, d_rgba, stride_bytes, flags, ticket, nullptr);
}

int hmrm_render_shaded_device_begin(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_sun *sun, uint32_t shade_flags,
                                    void *d_rgba, size_t stride_bytes, uint32_t flags, int32_t *ticket) {
	if (const int rc = check_shaded(sun, shade_flags)) return rc;
	const LitFrame lit = make_lit_frame(sun, shade_flags);
	return device_begin_common(scene, cam, d_rgba, stride_bytes, flags, ticket, &lit);
}

// Baked tickets: from the same ring, the same lanes and the same device-ticket pool as the plain and the lit ones.
int hmrm_render_baked_begin(const hmrm_scene *scene, const hmrm_camera *cam, uint32_t baked_flags, uint32_t flags, int32_t *ticket) {
	if (const int rc = check_baked_flags(baked_flags)) return rc;
	return begin_common(scene, cam, flags, ticket, nullptr, BakedTicket{true, (baked_flags & HMRM_TRACE_INTERIOR) != 0u});
}

int hmrm_render_baked_device_begin(const hmrm_scene *scene, const hmrm_camera *cam, uint32_t baked_flags, void *d_rgba,
                                   size_t stride_bytes, uint32_t flags, int32_t *ticket) {
	if (const int rc = check_baked_flags(baked_flags)) return rc;
	return device_begin_common(scene, cam, d_rgba, stride_bytes, flags, ticket, nullptr, BakedTicket{true, (baked_flags & HMRM_TRACE_INTERIOR) != 0u});
}

// Water tickets: from the same ring, lanes and pool once more.  HMRM_NO_PROBE is accepted and has no effect: a water frame is
// never the probe.
int hmrm_render_water_begin(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_water *water, uint32_t water_mode, uint32_t flags,
                            int32_t *ticket) {
	int rc = check_water(water);
	if (rc || (rc = check_water_mode(water_mode))) return rc;
	const hmrm::WaterRules rules = water_rules_of(water);
	return begin_common(scene, cam, flags, ticket, nullptr, BakedTicket{},
	                    WaterTicket{&rules, (water_mode & HMRM_WATER_BAKED) != 0u, (water->flags & HMRM_TRACE_INTERIOR) != 0u});
}

int hmrm_render_water_device_begin(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_water *water, uint32_t water_mode,
                                   void *d_rgba, size_t stride_bytes, uint32_t flags, int32_t *ticket) {
	int rc = check_water(water);
	if (rc || (rc = check_water_mode(water_mode))) return rc;
	const hmrm::WaterRules rules = water_rules_of(water);
	return device_begin_common(scene, cam, d_rgba, stride_bytes, flags, ticket, nullptr, BakedTicket{},
	                           WaterTicket{&rules, (water_mode & HMRM_WATER_BAKED) != 0u, (water->flags & HMRM_TRACE_INTERIOR) != 0u});
}

int hmrm_render_device_wait(const hmrm_scene *scene, int32_t ticket) {
	hmrm_scene *s = const_cast<hmrm_scene *>(scene);
	if (!s) return fail(HMRM_E_ARG, "NULL argument");
	DevTicket *t = nullptr;
	{
		std::lock_guard<std::mutex> lk(s->mu);
		if (ticket < 0 || ticket >= (int)s->dev_tickets.size() || !s->dev_tickets[(size_t)ticket]->busy)
			return fail(HMRM_E_ARG, "hmrm_render_device_wait: no such frame in flight");
		t = s->dev_tickets[(size_t)ticket];
	}
	HIP_TRY(hipSetDevice(s->device));
	HIP_TRY(hipEventSynchronize(t->done)); // (outside the lock: other threads may begin frames meanwhile)
	std::lock_guard<std::mutex> lk(s->mu);
	t->busy = false;
	return noterm(new_capped(t->ctx, *t->h_capped));
}

double hmrm_last_kernel_ms(void) { return g_last_kernel_ms; }

double hmrm_bench_kernel_ms(const hmrm_scene *scene, const hmrm_camera *cam, int32_t iters) {
	hmrm_scene *s = const_cast<hmrm_scene *>(scene);
	if (check_camera(cam) || !s || iters <= 0) {
		if (g_error.empty()) g_error = "bad argument";
		return -1.0;
	}
	auto body = [&]() -> int {
		const size_t W = (size_t)cam->width, H = (size_t)cam->height;
		HIP_TRY(hipSetDevice(s->device));
		std::lock_guard<std::mutex> lk(s->mu);
		int rc = s->d_frame.reserve(W * H * sizeof(uint32_t));
		if (rc) return rc;
		FrameSetup fs;
		if ((rc = setup_frame(s, s->stream, cam, 0, &fs))) return rc;
		const FrameRequest req = plain_request(s->d_frame.as<uint32_t>(), (int64_t)W);
		HIP_TRY(hipEventRecord(s->ev0, s->stream));
		for (int i = 0; i < iters; ++i)
			if ((rc = launch_frame(s, fs.c, fs.f, fs.slot, fs.rows, req))) return rc;
		HIP_TRY(hipEventRecord(s->ev1, s->stream));
		HIP_TRY(hipStreamSynchronize(s->stream));
		float ms = 0.f;
		HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
		g_last_kernel_ms = ms / iters;
		return HMRM_OK;
	};
	if (body() != HMRM_OK) return -1.0;
	return g_last_kernel_ms;
}

int32_t hmrm_band_local_rows(int32_t height, int32_t band_rows, int32_t band_index, int32_t band_count) {
	if (height <= 0 || band_rows <= 0 || band_count <= 0 || band_index < 0 || band_index >= band_count) return 0;
	int64_t local = 0;
	for (int64_t b = band_index; b * band_rows < height; b += band_count) local += band_rows;
	return (int32_t)local;
}

} // extern "C"

namespace hmrm {
int check_shaded_args(const hmrm_sun *sun, uint32_t shade_flags) { return check_shaded(sun, shade_flags); } // (record.cpp)
int check_baked_args(uint32_t baked_flags) { return check_baked_flags(baked_flags); }                         // (likewise)
int check_water_args(const hmrm_water *water, uint32_t water_mode) {                                          // (likewise)
	const int rc = check_water(water);
	return rc ? rc : check_water_mode(water_mode);
}
} // namespace hmrm
