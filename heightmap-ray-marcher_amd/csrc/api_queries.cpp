// api_queries.cpp -- the C ABI declared in include/hmrm.h, queries: ray batches, segments, cell maps and their sums, pick.
#include <cmath>
#include <cstdio>

#include "api_internal.hpp"

static_assert(sizeof(hmrm_ray) == sizeof(hmrm::BatchRay) && sizeof(hmrm_ray_hit) == sizeof(hmrm::BatchHit) &&
                  offsetof(hmrm_ray_hit, entry_d) == offsetof(hmrm::BatchHit, entry_d) &&
                  offsetof(hmrm_ray_hit, steps) == offsetof(hmrm::BatchHit, steps) &&
                  offsetof(hmrm_ray_hit, rgba) == offsetof(hmrm::BatchHit, rgba) &&
                  offsetof(hmrm_ray_hit, status) == offsetof(hmrm::BatchHit, status) && sizeof(hmrm_trace_params) == 16 &&
                  sizeof(hmrm_segment_params) == 24 && offsetof(hmrm_segment_params, flags) == 12 &&
                  offsetof(hmrm_segment_params, max_steps) == 16 && offsetof(hmrm_segment_params, reserved) == 20,
              "the kernels' mirrors of hmrm_ray / hmrm_ray_hit (frame.hpp)");
static_assert(sizeof(hmrm_cell_map_params) == 56 && offsetof(hmrm_cell_map_params, max_steps) == 40 &&
                  offsetof(hmrm_cell_map_params, sampling) == 48 && sizeof(hmrm_cell_rect) == 16 &&
                  HMRM_MAP_TOWARDS_POINT == hmrm::kMapTowardsPoint && HMRM_MAP_WEIGHT == hmrm::kMapWeight &&
                  HMRM_MAP_DIFFUSE == hmrm::kMapDiffuse && HMRM_MAP_NO_SHADOWS == hmrm::kMapNoShadows,
              "hmrm_cell_map_params and the kernels' flag bits (frame.hpp CellRules)");

namespace {

// ---- ray batches (hmrm_trace_rays, hmrm_trace_rays_device, hmrm_pick) ----
constexpr int64_t kMaxBatch = (int64_t)1 << 29;

// Needs no scene and no device: the refusals are testable without a GPU.
int check_trace(const hmrm_trace_params *p, const void *rays, int64_t n, const void *hits) {
	if (n < 0) return fail(HMRM_E_ARG, "trace: n must not be negative (got " + std::to_string(n) + ")");
	if (n > kMaxBatch) return fail(HMRM_E_ARG, "trace: at most 2^29 rays per batch (got " + std::to_string(n) + ")");
	if (n > 0 && (!p || !rays || !hits)) return fail(HMRM_E_ARG, "trace: NULL params, rays or hits");
	if (p && p->sampling > HMRM_NEAREST_F32)
		return fail(HMRM_E_ARG, "trace: sampling must be 0 (nearest), 1 (bilinear) or 2 (nearest, float heights)");
	return HMRM_OK;
}

// hmrm_trace_segments' refusals: check_trace's, then the flags and the reserved word.
int check_segments(const hmrm_segment_params *p, const void *rays, int64_t n, const void *hits, hmrm_trace_params *plain) {
	if (p) *plain = hmrm_trace_params{p->step_dist, p->bg_r, p->bg_g, p->bg_b, p->sampling};
	const int rc = check_trace(p ? plain : nullptr, rays, n, hits);
	if (rc) return rc;
	if (p && (p->flags & ~(uint32_t)HMRM_TRACE_INTERIOR)) return fail(HMRM_E_ARG, "trace: unknown flag bits (defined: HMRM_TRACE_INTERIOR)");
	if (p && p->reserved != 0u) return fail(HMRM_E_ARG, "trace: hmrm_segment_params.reserved must be 0");
	return HMRM_OK;
}

// The DevFrame of a launch without a camera (ray batches, cell maps): a zeroed record plus the scene's box, grid and pyramid.
// The leap policy's hints come from a camera's step length in cells for frames (camera.cpp); such a launch's directions have
// any length, so it gets the fine-step defaults: windows from 4 cells on, no pause (HMRM_MIN_LEVEL / HMRM_FINEST_PAUSE apply).
// The caller sets projection and the "frame" (screen_w x screen_h).  Refuses what no kernel of the sampling mode can render.
int cameraless_frame(hmrm_scene *s, double step_dist, int sampling, hmrm::DevFrame *out) {
	const bool huge_side = s->map_w >= (1 << 24) || s->map_h >= (1 << 24);
	if (huge_side && sampling != 0) return fail(HMRM_E_ARG, "maps with a side of 2^24 cells or more support nearest sampling only");
	if (sampling == HMRM_BILINEAR) {
		const int rc_b = ensure_bilinear_pyramid(s);
		if (rc_b) return rc_b;
	}
	hmrm::DevFrame f = hmrm::DevFrame();
	hmrm::fill_scene_fields(s->map_w, s->map_h, s->params.min_height, s->params.max_height, s->params.grid_width, step_dist, &f);
	f.bg[3] = 255;
	f.sampling = sampling;
	f.thr_max = sampling == HMRM_BILINEAR ? s->thr_max_bil : s->thr_max;
	f.mipbuf = s->d_mipbuf;
	f.mipbuf_bil = s->d_mipbuf_bil;
	f.mip_row = s->mip_row;
	f.mip_plane_shift = s->mip_plane_shift;
	f.step_cap = s->knobs.step_cap;
	f.min_window = 4;
	f.min_level = s->knobs.min_level >= 0 ? s->knobs.min_level : 0;
	f.finest_pause = s->knobs.finest_pause >= 0 ? s->knobs.finest_pause : 0;
	*out = f;
	return HMRM_OK;
}
// ... and the kernel such a launch runs: the scene's choice is only READ (HMRM_KERNEL or the probe's verdict, never a probe).
// *literal: the literal loop (HMRM_KERNEL=simple, or a side of 2^24 cells), which only knows the reference's sampling.
int cameraless_kernel(hmrm_scene *s, int sampling, bool *literal, hmrm::FastKernel *k) {
	const bool huge_side = s->map_w >= (1 << 24) || s->map_h >= (1 << 24);
	*literal = (s->knobs.kernel == 2 || huge_side) && sampling == 0;
	*k = hmrm::kLeaps;
	if (*literal) return HMRM_OK;
	const bool use_other = s->knobs.kernel == 0 && s->knobs.try_group && s->choice.use_group;
	*k = (hmrm::FastKernel)hmrm::pick_fast_kernel(s->knobs.kernel, use_other, sampling == 0 && s->d_records, s->choice);
	return *k == hmrm::kRecords ? ensure_records(s) : HMRM_OK;
}

// What every launch without a camera does before its kernel goes out, in this order: the DevFrame (cameraless_frame) laid out as a
// w x h "frame" of the given projection code, the wait -- in stream order -- for a measured launch in flight, and only then the
// kernel (cameraless_kernel: a probe's verdict may have arrived meanwhile).  Such a launch is not a frame: it takes no cached
// record, is never measured, never probes and does not count towards the scene's probe.
struct Cameraless {
	hmrm::DevFrame f;
	bool literal = false;
	hmrm::FastKernel k = hmrm::kLeaps;
};
int cameraless_prologue(hmrm_scene *s, StreamCtx *c, double step_dist, int sampling, int32_t w, int32_t h, int32_t projection, Cameraless *out) {
	int rc = cameraless_frame(s, step_dist, sampling, &out->f);
	if (rc) return rc;
	out->f.screen_w = w;
	out->f.screen_h = h;
	out->f.projection = projection;
	if ((rc = wait_for_measure_fence(s, c))) return rc;
	return cameraless_kernel(s, sampling, &out->literal, &out->k);
}

// One batch on the context's stream, laid out as a frame kBatchW pixels wide (frame.hpp RayBatch).
// `seg` (hmrm_trace_segments; null: hmrm_trace_rays): the segment rules, run by the segment kernels (render_segments.hip).
int launch_batch(hmrm_scene *s, StreamCtx *c, double step_dist, const uint8_t bg[3], int sampling, const hmrm::BatchRay *d_rays,
                 int64_t n, hmrm::BatchHit *d_hits, const hmrm::SegRules *seg = nullptr) {
	Cameraless cl;
	const int rc = cameraless_prologue(s, c, step_dist, sampling, hmrm::kBatchW, (int32_t)((n + hmrm::kBatchW - 1) / hmrm::kBatchW), 4, &cl);
	if (rc) return rc;
	hmrm::DevFrame &f = cl.f;
	f.bg[0] = bg[0];
	f.bg[1] = bg[1];
	f.bg[2] = bg[2];
	const hmrm::RayBatch batch{d_rays, d_hits, n};
	if (cl.literal) {
		if (seg) HIP_TRY(hmrm::launch_trace_segments_literal(f, s->d_thr, s->d_cmap, batch, *seg, c->d_counters, c->stream));
		else HIP_TRY(hmrm::launch_trace_rays_literal(f, s->d_thr, s->d_cmap, batch, c->d_counters, c->stream));
	} else {
		if (seg) HIP_TRY(hmrm::launch_trace_segments(f, s->d_thr, s->d_thr32, s->d_cmap, batch, *seg, c->d_counters, cl.k, s->d_records, c->stream));
		else HIP_TRY(hmrm::launch_trace_rays(f, s->d_thr, s->d_thr32, s->d_cmap, batch, c->d_counters, cl.k, s->d_records, c->stream));
	}
	return HMRM_OK;
}

// ---- cell maps (hmrm_cell_map, hmrm_cell_map_device) ----
// Needs no scene and no device, in hmrm.h's order.
int check_cell_map(const hmrm_cell_map_params *p, const void *out) {
	if (!p) return fail(HMRM_E_ARG, "cell map: NULL params");
	constexpr uint32_t known = HMRM_MAP_TOWARDS_POINT | HMRM_MAP_WEIGHT | HMRM_MAP_DIFFUSE | HMRM_MAP_NO_SHADOWS;
	if (p->flags & ~known)
		return fail(HMRM_E_ARG, "cell map: unknown flag bits (defined: HMRM_MAP_TOWARDS_POINT, _WEIGHT, _DIFFUSE, _NO_SHADOWS)");
	for (uint8_t r : p->reserved)
		if (r != 0) return fail(HMRM_E_ARG, "cell map: hmrm_cell_map_params.reserved must be 0");
	if (p->sampling > HMRM_NEAREST_F32)
		return fail(HMRM_E_ARG, "cell map: sampling must be 0 (nearest), 1 (bilinear) or 2 (nearest, float heights)");
	if ((p->flags & (HMRM_MAP_DIFFUSE | HMRM_MAP_NO_SHADOWS)) && !(p->flags & HMRM_MAP_WEIGHT))
		return fail(HMRM_E_ARG, "cell map: HMRM_MAP_DIFFUSE and HMRM_MAP_NO_SHADOWS need HMRM_MAP_WEIGHT");
	if (!out) return fail(HMRM_E_ARG, "cell map: NULL out");
	return HMRM_OK;
}

// ... and what needs the scene's size: the rect (null: the whole map) and the stride.
int check_cell_rect(const hmrm_scene *s, const hmrm_cell_rect *rect, size_t stride_bytes, hmrm_cell_rect *r) {
	*r = rect ? *rect : hmrm_cell_rect{0, 0, s->map_w, s->map_h};
	if (r->w <= 0 || r->h <= 0 || r->x0 < 0 || r->y0 < 0 || (int64_t)r->x0 + r->w > s->map_w || (int64_t)r->y0 + r->h > s->map_h)
		return fail(HMRM_E_ARG, "cell map: the rect must be non-empty and inside the map");
	if (stride_bytes < (size_t)r->w) return fail(HMRM_E_ARG, "cell map: stride_bytes is below the rect's width");
	return HMRM_OK;
}

// One cell map on the context's stream: a launch without a camera whose "frame" is the rect.
int launch_cells(hmrm_scene *s, StreamCtx *c, const hmrm_cell_map_params *p, const hmrm_cell_rect &r, uint8_t *d_out, size_t stride_bytes) {
	Cameraless cl;
	const int rc = cameraless_prologue(s, c, p->step_dist, p->sampling, r.w, r.h, 5, &cl);
	if (rc) return rc;
	const hmrm::CellRules cells{{p->target[0], p->target[1], p->target[2]}, p->lift, r.x0, r.y0, p->max_steps, p->flags, p->ambient};
	if (cl.literal) HIP_TRY(hmrm::launch_cell_map_literal(cl.f, s->d_thr, d_out, (int64_t)stride_bytes, cells, c->d_counters, c->stream));
	else HIP_TRY(hmrm::launch_cell_map(cl.f, s->d_thr, s->d_thr32, d_out, (int64_t)stride_bytes, cells, c->d_counters, cl.k, s->d_records, c->stream));
	return HMRM_OK;
}

// ---- accumulated cell maps (hmrm_cell_map_sum, hmrm_cell_map_sum_device) ----
// Needs no scene and no device, in hmrm.h's order: hmrm_cell_map's own refusals first.
int check_cell_map_sum(const hmrm_cell_map_params *p, const void *targets, int32_t n_targets, const void *out) {
	if (const int rc = check_cell_map(p, out)) return rc;
	if (!targets) return fail(HMRM_E_ARG, "cell map sum: NULL targets");
	if (n_targets < 1 || n_targets > hmrm::kMaxSumTargets) return fail(HMRM_E_ARG, "cell map sum: n_targets must be 1..256");
	return HMRM_OK;
}

// ... and what needs the scene's size: the rect (null: the whole map) and the stride of its rows of 16-bit words.
int check_cell_sum_rect(const hmrm_scene *s, const hmrm_cell_rect *rect, size_t stride_bytes, hmrm_cell_rect *r) {
	if (const int rc = check_cell_rect(s, rect, (size_t)-1, r)) return rc; // (the rect's own test; the stride's is below)
	if (stride_bytes < 2 * (size_t)r->w) return fail(HMRM_E_ARG, "cell map sum: stride_bytes is below twice the rect's width");
	if (stride_bytes & 1u) return fail(HMRM_E_ARG, "cell map sum: stride_bytes must be even");
	return HMRM_OK;
}

// One accumulated cell map on the context's stream: launch_cells' recipe with the list of targets beside the rules.
int launch_cell_sums(hmrm_scene *s, StreamCtx *c, const hmrm_cell_map_params *p, const double *d_targets, int32_t n_targets,
                     const hmrm_cell_rect &r, uint16_t *d_out, size_t stride_bytes) {
	Cameraless cl;
	const int rc = cameraless_prologue(s, c, p->step_dist, p->sampling, r.w, r.h, 5, &cl);
	if (rc) return rc;
	const hmrm::CellRules cells{{0.0, 0.0, 0.0}, p->lift, r.x0, r.y0, p->max_steps, p->flags, p->ambient}; // (p->target is not looked at)
	const hmrm::CellSums sums{d_targets, n_targets};
	if (cl.literal) HIP_TRY(hmrm::launch_cell_map_sum_literal(cl.f, s->d_thr, d_out, (int64_t)stride_bytes, cells, sums, c->d_counters, c->stream));
	else HIP_TRY(hmrm::launch_cell_map_sum(cl.f, s->d_thr, s->d_thr32, d_out, (int64_t)stride_bytes, cells, sums, c->d_counters, cl.k, s->d_records, c->stream));
	return HMRM_OK;
}

// The host-memory half of hmrm_trace_rays / hmrm_pick: the records of the scene's staging buffer and the stream's capped-ray
// count come back, the stream is drained.  (s->mu held.)
int finish_batch(hmrm_scene *s, StreamCtx *c, hmrm_ray_hit *hits, int64_t n, hmrm_stats *stats) {
	HIP_TRY(hipMemcpyAsync(hits, s->d_hits.ptr, (size_t)n * sizeof(hmrm_ray_hit), hipMemcpyDeviceToHost, s->stream));
	unsigned long long capped = 0;
	const int rc = finish_host_call(s, c, &capped);
	if (rc == HMRM_E_DEVICE) return rc;
	if (stats) {
		*stats = hmrm_stats{};
		stats->rays = (uint64_t)n;
		for (int64_t i = 0; i < n; ++i) {
			stats->steps += hits[i].steps;
			stats->hits += hits[i].status == HMRM_RAY_HIT ? 1u : 0u;
		}
		stats->capped = capped;
	}
	return rc;
}

// hmrm_trace_rays, hmrm_trace_segments and their device forms behind their own argument checks (check_trace, check_segments).
// `sp`: the segment rules (null: plain rays -- or a segment call without params, which check_segments lets through for n == 0
// only); `max_steps`: the segments' per-ray limits or null.  `device`: rays, max_steps and hits are device pointers and the
// launch goes to `stream` without a host sync; else they are staged through the scene's buffers, on its own stream.
int trace_common(hmrm_scene *s, const hmrm_trace_params *p, const hmrm_segment_params *sp, const void *rays, const void *max_steps,
                 int64_t n, void *hits, hmrm_stats *stats, bool device, hipStream_t stream) {
	if (!s) return fail(HMRM_E_ARG, "NULL argument");
	if (n == 0) {
		if (!device && stats) *stats = hmrm_stats{};
		return HMRM_OK;
	}
	if (device && (((uintptr_t)rays | (uintptr_t)hits) & 7u)) return fail(HMRM_E_ARG, "trace: d_rays and d_hits must be 8-byte aligned");
	if (device && ((uintptr_t)max_steps & 3u)) return fail(HMRM_E_ARG, "trace: d_max_steps must be 4-byte aligned");
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	int rc;
	if (!device) {
		if ((rc = s->d_rays.reserve((size_t)n * sizeof(hmrm::BatchRay))) || (rc = s->d_hits.reserve((size_t)n * sizeof(hmrm::BatchHit)))) return rc;
		if (max_steps && (rc = s->d_limits.reserve((size_t)n * sizeof(uint32_t)))) return rc;
		stream = s->stream;
	}
	StreamCtx *c = nullptr;
	if ((rc = ctx_for(s, stream, &c))) return rc;
	if (!device) {
		HIP_TRY(hipMemcpyAsync(s->d_rays.ptr, rays, (size_t)n * sizeof(hmrm_ray), hipMemcpyHostToDevice, s->stream));
		if (max_steps) HIP_TRY(hipMemcpyAsync(s->d_limits.ptr, max_steps, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
		rays = s->d_rays.ptr;
		if (max_steps) max_steps = s->d_limits.ptr;
	}
	hmrm::BatchHit *const d_hits = device ? static_cast<hmrm::BatchHit *>(hits) : s->d_hits.as<hmrm::BatchHit>();
	const uint8_t bg[3] = {p->bg_r, p->bg_g, p->bg_b};
	hmrm::SegRules seg{};
	if (sp) seg = hmrm::SegRules{static_cast<const uint32_t *>(max_steps), sp->max_steps, sp->flags & HMRM_TRACE_INTERIOR};
	rc = launch_batch(s, c, p->step_dist, bg, p->sampling, static_cast<const hmrm::BatchRay *>(rays), n, d_hits, sp ? &seg : nullptr);
	if (rc || device) return rc;
	return finish_batch(s, c, static_cast<hmrm_ray_hit *>(hits), n, stats);
}

// hmrm_cell_map and its device form.  `device`: out is a device pointer and the launch goes to `stream` without a host sync; else
// the rect is staged through the scene's buffer, rows packed, and copied to the caller's behind the launch.
int cell_map_common(const hmrm_scene *scene, const hmrm_cell_map_params *p, const hmrm_cell_rect *rect, void *out, size_t stride_bytes,
                    bool device, hipStream_t stream) {
	hmrm_scene *s = const_cast<hmrm_scene *>(scene);
	int rc = check_cell_map(p, out);
	if (rc) return rc;
	if (!s) return fail(HMRM_E_ARG, "NULL argument");
	hmrm_cell_rect r;
	if ((rc = check_cell_rect(s, rect, stride_bytes, &r))) return rc;
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	const size_t row_bytes = (size_t)r.w;
	if (!device) {
		if ((rc = s->d_cells.reserve(row_bytes * (size_t)r.h))) return rc;
		stream = s->stream;
	}
	StreamCtx *c = nullptr;
	if ((rc = ctx_for(s, stream, &c))) return rc;
	if (device) return launch_cells(s, c, p, r, static_cast<uint8_t *>(out), stride_bytes);
	if ((rc = launch_cells(s, c, p, r, s->d_cells.as<uint8_t>(), row_bytes))) return rc;
	HIP_TRY(hipMemcpy2DAsync(out, stride_bytes, s->d_cells.ptr, row_bytes, row_bytes, (size_t)r.h, hipMemcpyDeviceToHost, s->stream));
	return finish_host_call(s, c);
}

// hmrm_cell_map_sum and its device form, likewise: the host form's targets go through the scene's target list, its words through
// the buffer hmrm_cell_map's bytes use.
int cell_map_sum_common(const hmrm_scene *scene, const hmrm_cell_map_params *p, const void *targets, int32_t n_targets,
                        const hmrm_cell_rect *rect, void *out, size_t stride_bytes, bool device, hipStream_t stream) {
	hmrm_scene *s = const_cast<hmrm_scene *>(scene);
	int rc = check_cell_map_sum(p, targets, n_targets, out);
	if (rc) return rc;
	if (!s) return fail(HMRM_E_ARG, "NULL argument");
	hmrm_cell_rect r;
	if ((rc = check_cell_sum_rect(s, rect, stride_bytes, &r))) return rc;
	if (device && ((uintptr_t)out & 1u)) return fail(HMRM_E_ARG, "cell map sum: d_out must be 2-byte aligned");
	if (device && ((uintptr_t)targets & 7u)) return fail(HMRM_E_ARG, "cell map sum: d_targets must be 8-byte aligned");
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	const size_t row_bytes = 2 * (size_t)r.w, targets_bytes = (size_t)n_targets * 3 * sizeof(double);
	if (!device) {
		if ((rc = s->d_cells.reserve(row_bytes * (size_t)r.h)) || (rc = s->d_targets.reserve(targets_bytes))) return rc;
		stream = s->stream;
	}
	StreamCtx *c = nullptr;
	if ((rc = ctx_for(s, stream, &c))) return rc;
	if (device) return launch_cell_sums(s, c, p, static_cast<const double *>(targets), n_targets, r, static_cast<uint16_t *>(out), stride_bytes);
	HIP_TRY(hipMemcpyAsync(s->d_targets.ptr, targets, targets_bytes, hipMemcpyHostToDevice, s->stream));
	if ((rc = launch_cell_sums(s, c, p, s->d_targets.as<double>(), n_targets, r, s->d_cells.as<uint16_t>(), row_bytes))) return rc;
	HIP_TRY(hipMemcpy2DAsync(out, stride_bytes, s->d_cells.ptr, row_bytes, row_bytes, (size_t)r.h, hipMemcpyDeviceToHost, s->stream));
	return finish_host_call(s, c);
}

} // namespace

extern "C" {

int hmrm_trace_rays(const hmrm_scene *scene, const hmrm_trace_params *p, const hmrm_ray *rays, int64_t n, hmrm_ray_hit *hits,
                    hmrm_stats *stats) {
	if (const int rc = check_trace(p, rays, n, hits)) return rc;
	return trace_common(const_cast<hmrm_scene *>(scene), p, nullptr, rays, nullptr, n, hits, stats, false, nullptr);
}

int hmrm_trace_rays_device(const hmrm_scene *scene, const hmrm_trace_params *p, const void *d_rays, int64_t n, void *d_hits,
                           void *hip_stream) {
	if (const int rc = check_trace(p, d_rays, n, d_hits)) return rc;
	return trace_common(const_cast<hmrm_scene *>(scene), p, nullptr, d_rays, nullptr, n, d_hits, nullptr, true, (hipStream_t)hip_stream);
}

int hmrm_trace_segments(const hmrm_scene *scene, const hmrm_segment_params *p, const hmrm_ray *rays, const uint32_t *max_steps,
                        int64_t n, hmrm_ray_hit *hits, hmrm_stats *stats) {
	hmrm_trace_params plain{};
	if (const int rc = check_segments(p, rays, n, hits, &plain)) return rc;
	return trace_common(const_cast<hmrm_scene *>(scene), &plain, p, rays, max_steps, n, hits, stats, false, nullptr);
}

int hmrm_trace_segments_device(const hmrm_scene *scene, const hmrm_segment_params *p, const void *d_rays, const void *d_max_steps,
                               int64_t n, void *d_hits, void *hip_stream) {
	hmrm_trace_params plain{};
	if (const int rc = check_segments(p, d_rays, n, d_hits, &plain)) return rc;
	return trace_common(const_cast<hmrm_scene *>(scene), &plain, p, d_rays, d_max_steps, n, d_hits, nullptr, true, (hipStream_t)hip_stream);
}

int hmrm_cell_map(const hmrm_scene *scene, const hmrm_cell_map_params *p, const hmrm_cell_rect *rect, uint8_t *out, size_t stride_bytes) {
	return cell_map_common(scene, p, rect, out, stride_bytes, false, nullptr);
}

int hmrm_cell_map_device(const hmrm_scene *scene, const hmrm_cell_map_params *p, const hmrm_cell_rect *rect, void *d_out,
                         size_t stride_bytes, void *hip_stream) {
	return cell_map_common(scene, p, rect, d_out, stride_bytes, true, (hipStream_t)hip_stream);
}

int hmrm_cell_map_sum(const hmrm_scene *scene, const hmrm_cell_map_params *p, const double *targets, int32_t n_targets,
                      const hmrm_cell_rect *rect, uint16_t *out, size_t stride_bytes) {
	return cell_map_sum_common(scene, p, targets, n_targets, rect, out, stride_bytes, false, nullptr);
}

int hmrm_cell_map_sum_device(const hmrm_scene *scene, const hmrm_cell_map_params *p, const void *d_targets, int32_t n_targets,
                             const hmrm_cell_rect *rect, void *d_out, size_t stride_bytes, void *hip_stream) {
	return cell_map_sum_common(scene, p, d_targets, n_targets, rect, d_out, stride_bytes, true, (hipStream_t)hip_stream);
}

// hmrm_cell_map_sum's launch over the whole map, its words written straight into the scene's light plane (hmrm_render_baked
// reads it): the same checks without an `out`, the targets through the scene's target list, on the scene's own stream behind
// a drain of its other streams.  A HIP failure from the drain on leaves the scene without a plane; capped rays leave a valid one.
int hmrm_scene_bake_light(hmrm_scene *s, const hmrm_cell_map_params *p, const double *targets, int32_t n_targets) {
	int rc = check_cell_map_sum(p, targets, n_targets, /* out: the scene's own */ p);
	if (rc) return rc;
	if (!s) return fail(HMRM_E_ARG, "light plane: NULL scene");
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	if ((rc = drain_scene_streams(s, true))) return rc;
	const hmrm_cell_rect whole{0, 0, s->map_w, s->map_h};
	const size_t targets_bytes = (size_t)n_targets * 3 * sizeof(double);
	StreamCtx *c = nullptr;
	auto body = [&]() -> int {
		int rc2;
		if ((rc2 = ensure_light_plane(s)) || (rc2 = s->d_targets.reserve(targets_bytes)) || (rc2 = ctx_for(s, s->stream, &c))) return rc2;
		HIP_TRY(hipMemcpyAsync(s->d_targets.ptr, targets, targets_bytes, hipMemcpyHostToDevice, s->stream));
		return launch_cell_sums(s, c, p, s->d_targets.as<double>(), n_targets, whole, s->d_baked, 2 * (size_t)s->map_w);
	};
	if ((rc = body()) == HMRM_OK) rc = finish_host_call(s, c);
	if (rc == HMRM_E_ARG) return rc; // (a refusal of the launch path, before anything was written: the old plane stays)
	if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
		drop_light_plane(s);
		return rc;
	}
	s->baked_scale = (p->flags & HMRM_MAP_WEIGHT) ? 255u * (uint32_t)n_targets : (uint32_t)n_targets;
	return rc;
}

int hmrm_sky_directions(int32_t rings, int32_t per_ring, double *out_xyz) {
	if (!out_xyz) return fail(HMRM_E_ARG, "sky directions: NULL out_xyz");
	if (rings < 1 || per_ring < 1 || (int64_t)rings * per_ring > hmrm::kMaxSumTargets)
		return fail(HMRM_E_ARG, "sky directions: rings * per_ring must be 1..256");
	const double two_pi = 6.283185307179586476925286766559;
	for (int32_t i = 0; i < rings; ++i) {
		const double u = ((double)i + 0.5) / (double)rings;
		const double z = std::sqrt(u), rad = std::sqrt(1.0 - u);
		for (int32_t j = 0; j < per_ring; ++j) {
			const double a = two_pi * ((double)j + 0.5 * (double)(i & 1)) / (double)per_ring;
			double *o = out_xyz + 3 * ((size_t)i * (size_t)per_ring + (size_t)j);
			o[0] = rad * std::cos(a);
			o[1] = rad * std::sin(a);
			o[2] = z;
		}
	}
	return rings * per_ring;
}

// Picking: GetRay of one pixel on the device (k_probe, as hmrm_debug_ray) and that ray traced as a batch of one.  Like a
// batch it takes no cached per-frame record: the camera's record is built here and dropped, and a spherical camera's tables
// go to the scene's scratch behind the probe's seven doubles.
int hmrm_pick(const hmrm_scene *scene, const hmrm_camera *cam, int32_t px, int32_t py, hmrm_ray_hit *hit) {
	hmrm_scene *s = const_cast<hmrm_scene *>(scene);
	int rc = check_camera(cam);
	if (rc) return rc;
	if (!s || !hit) return fail(HMRM_E_ARG, "NULL argument");
	if (px < 0 || py < 0 || px >= cam->width || py >= cam->height) return fail(HMRM_E_ARG, "pixel out of range");
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	const size_t W = (size_t)cam->width, H = (size_t)cam->height;
	const bool spherical = cam->projection == HMRM_SPHERICAL;
	// (borrowed: the scene's entry-distance scratch holds the probe's doubles and the tables, its hit records the one record)
	if ((rc = s->d_entry.reserve((8 + (spherical ? 2 * W + 2 * H : 0)) * sizeof(double)))) return rc;
	if ((rc = s->d_hits.reserve(sizeof(hmrm::BatchHit)))) return rc;
	StreamCtx *c = nullptr;
	if ((rc = ctx_for(s, s->stream, &c))) return rc;
	hmrm::HostCamera hc;
	to_host_camera(cam, &hc);
	std::vector<double> tables(spherical ? 2 * W + 2 * H : 0);
	double *t = tables.data();
	hmrm::DevFrame f;
	hmrm::build_frame(hc, s->map_w, s->map_h, s->params.min_height, s->params.max_height, s->params.grid_width, &f,
	                  spherical ? t : nullptr, spherical ? t + W : nullptr, spherical ? t + 2 * W : nullptr,
	                  spherical ? t + 2 * W + H : nullptr);
	if (spherical) {
		double *d_t = s->d_entry.as<double>() + 8;
		// (pageable source: the copy is staged before the call returns)
		HIP_TRY(hipMemcpyAsync(d_t, t, tables.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
		f.col_cos_ha = d_t;
		f.col_sin_ha = d_t + W;
		f.row_sin_va = d_t + 2 * W;
		f.row_cos_va = d_t + 2 * W + H;
	}
	// the probe's first six doubles -- pos, dir -- are an hmrm_ray
	HIP_TRY(hmrm::launch_probe(f, px, py, s->d_entry.as<double>(), s->stream));
	const uint8_t bg[3] = {cam->bg_r, cam->bg_g, cam->bg_b};
	if ((rc = launch_batch(s, c, cam->step_dist, bg, cam->sampling, s->d_entry.as<const hmrm::BatchRay>(), 1, s->d_hits.as<hmrm::BatchHit>())))
		return rc;
	return finish_batch(s, c, hit, 1, nullptr);
}

} // extern "C"
