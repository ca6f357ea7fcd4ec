// render.hip -- gfx950 kernels for the reference's hot path and their launchers.
//
//   k_prepare_heights  UpdateHeightmap            main/hmap.cpp:171-191
//   k_render           the pixel loop             main/hmap.cpp:978-1058
//                        ImagePlane::GetRay       src/{Perspective,Spherical,Orthographic}.cpp
//                        intersection/distance    src/AABB.cpp:30-77
//                        SetPixel                 main/hmap.cpp:139-154
//
// Numerical contract: every fp64 operation of the reference is performed once, in
// the reference's order, with IEEE round-to-nearest and NO fused multiply-add
// (this file must be compiled with -ffp-contract=off; hipcc contracts by
// default).  Division and sqrt are the correctly rounded LLVM expansions.  No
// transcendental is evaluated on the device (the host supplies them, frame.hpp).
//
// Bit-preserving departures from the literal loop, each argued where it is made:
//   * heightmap_buf[i] + hmap_c0.z (hmap.cpp:1016) is loop invariant per cell and
//     precomputed into the `thr` table by k_prepare_heights;
//   * step_dist * ray.dir (hmap.cpp:1037) is loop invariant per ray and hoisted;
//   * x / grid_width is evaluated as x * (1/grid_width) only when grid_width is a
//     power of two (exactly representable reciprocal => identical rounding);
//   * the (int) casts + integer range test (hmap.cpp:1001-1011) are evaluated as
//     an fp range test followed by the cast (same predicate, no UB, NaN breaks as
//     on x86 where cvttsd2si gives INT_MIN);
//   * the unbounded while(true) gets a step cap that is reported, never silent.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "device_common.hpp"
#include "launch_common.hpp"
#include "render.hpp"

#pragma clang fp contract(off)

namespace hmrm {

// --------------------------------------------------------------- heights ----
// thr[i] = heightmap_buf[i] + c0.z  with heightmap_buf[i] exactly as
// UpdateHeightmap computes it.  PLAIN = true writes heightmap_buf[i] itself
// (test hook).  Also reduces max(thr) with an order-preserving integer key.
__device__ __forceinline__ unsigned long long f64_order_key(double v) {
	unsigned long long b = (unsigned long long)__double_as_longlong(v);
	return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}

template <bool PLAIN>
__global__ __launch_bounds__(256) void k_prepare_heights(const uint8_t *__restrict__ rgb,
                                                         double *__restrict__ out, int64_t n,
                                                         double lum_r, double lum_g, double lum_b,
                                                         double min_h, double max_h,
                                                         unsigned long long *__restrict__ max_key) {
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	unsigned long long local = 0; // smaller than the key of every double
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
		const double r = (double)rgb[3 * i + 0];
		const double g = (double)rgb[3 * i + 1];
		const double b = (double)rgb[3 * i + 2];
		double value = ((lum_r * r) + (lum_g * g)) + (lum_b * b);
		// Clamp<double>, hmap.cpp:118-124 (NaN falls through both tests)
		if (value < 0.0) value = 0.0;
		else if (value > 255.0) value = 255.0;
		const double hz = (value / 255.0) * (max_h - min_h) + min_h;
		const double v = PLAIN ? hz : hz + min_h; // hmap.cpp:1016: heightmap_z + hmap_c0.z
		out[i] = v;
		if (!PLAIN) {
			const unsigned long long k = f64_order_key(v);
			if (v == v && k > local) local = k;
		}
	}
	if (!PLAIN) {
		for (int off = 32; off > 0; off >>= 1) {
			unsigned long long o = __shfl_xor(local, off);
			if (o > local) local = o;
		}
		if ((threadIdx.x & 63) == 0 && local) atomicMax(max_key, local);
	}
}

// The literal loop for the pixel (or, PROJ 4, the batch ray: hmrm_trace_rays, frame.hpp RayBatch) of one lane.
// AA: the antialiased epilogue (device_common.hpp store_box_filtered, f.aa_shift); the plain instantiations store per lane.
// PROJ 4: the lane's ray comes from `batch` and its hmrm_ray_hit record goes there; `out` is not used.
// SEG: the segment rules (frame.hpp SegRules; hmrm_trace_segments, hmrm_render_interior), as in march.hpp.
// LIT (hmrm_render_lit; frame.hpp SunRules; implies SEG): one of the two passes of a lit pixel, which hand each other `lit` in
// registers and write no pixel themselves.  1: the primary ray -- its pixel, whether it hit, and where and under which
// threshold, go to *lit.  2: the shadow ray of a lane whose primary ray hit, made from *lit and `sun` with the sun's step
// (`seg` holds the sun's limit and the interior rule); a hit darkens lit->rgba.  The other lanes sit that pass out.
// 3 (hmrm_render_shaded): pass 2, but a hit leaves lit->rgba alone and says SHADOWED in lit->phase -- the caller weights the pixel;
// `hit_cell` (pass 1, may be null): where the primary hit's cell index gridx + gridy * W goes, for that caller.
// 4 (hmrm_cell_map): pass 3 for a ray the caller put into *lit itself; the ray's status (HMRM_RAY_*) comes back in lit->phase.
// 5 (hmrm_render_water): pass 2 for a mirror ray -- the caller hands the lane's own direction, step and limit in `sun` -- whose pixel,
// the hit cell's colour or the miss shade of its own dz, comes back in lit->rgba; `hit_cell` (may be null): where the mirror ray's
// hit cell goes, for the light of a water frame under the light plane -- left alone when the ray did not hit.
// 6 (hmrm_render_water_lit): pass 5 that also leaves where the mirror ray hit, and under which threshold, in *lit as pass 1 does --
// the origin of that hit's own shadow ray.  A mode of its own: pass 5's callers keep their instructions.
template <int PROJ, bool STATS, bool AA, bool SEG = false, int LIT = 0>
__device__ __forceinline__ void render_lane_literal(const DevFrame &f, PixelId pid, const double *__restrict__ thr,
                                                    const uint32_t *__restrict__ cmap, uint32_t *__restrict__ out,
                                                    int64_t out_stride_px, const StatsOut &st, const RayBatch &batch,
                                                    const SegRules &seg = SegRules{}, const SunRules &sun = SunRules{},
                                                    LitState<true> *lit = nullptr, unsigned *hit_cell = nullptr,
                                                    double *hit_z = nullptr) { // (hit_z: pass 1, may be null: int_point's z, geometry frames)
	constexpr bool RAYS = PROJ == 4, COUNT = STATS || RAYS;
	static_assert(LIT == 0 || (SEG && !RAYS), "sun shadows: frames, under the segment rules");
	static_assert(!RAYS || (!AA && !STATS), "ray batches: neither antialiased nor instrumented");
	static_assert(!SEG || (!AA && !STATS), "segment rules: production kernels only");
	// (what a batch adds is written as `if constexpr (RAYS)` statements beside the frame kernels' own, which stay as they
	// were: they must keep compiling to the same instructions)
	int64_t ray_index = 0;
	if constexpr (RAYS) {
		ray_index = (int64_t)pid.py * kBatchW + pid.px;
		pid.live = pid.live && ray_index < batch.n;
	}
	if constexpr (LIT >= 2) pid.live = pid.live && lit->primary_hit;
	const int px = pid.px, py = pid.py, lrow = pid.lrow;
	const bool live = pid.live;

	unsigned long long my_steps = 0;
	uint32_t my_hit = 0, my_cap = 0;
	uint32_t aa_rgba = 0; // (AA: this lane's sample, filtered by the whole wave below)

	if (live) {
		DevRay ray = make_ray<PROJ>(f, px, py);
		if constexpr (RAYS) ray = batch_ray(batch, ray_index); // (make_ray<4>'s value is dead)
		if constexpr (LIT >= 2) { // (the camera's ray is dead too: from the surface above the hit point towards the sun)
			ray.px = lit->hx; ray.py = lit->hy; ray.pz = lit->t;
			ray.dx = sun.dir[0]; ray.dy = sun.dir[1]; ray.dz = sun.dir[2];
		}
		const double d_box = slab_distance(ray, f);
		if (STATS && st.entry_d) st.entry_d[(int64_t)py * f.screen_w + px] = d_box;
		double d = d_box;
		SegState<SEG> sg; // (empty unless SEG: device_common.hpp)
		if constexpr (SEG) {
			sg.d_record = d_box; // (a record keeps distance()'s own value, not the d that was used)
			if (seg.interior != 0u && origin_strictly_inside(ray, f)) d = 0.0; // as if distance() had returned +0.0
			sg.budget = segment_budget(seg, RAYS ? ray_index : 0, f.step_cap, &sg.ends);
		}

		uint32_t rgba = 0;
		bool real_hit = false;
		double hx = 0.0, hy = 0.0, hz = 0.0; // (RAYS: where hmap.cpp:1016 fired, and in which cell)
		int hgx = -1, hgy = -1;

		// intersection(): AABB.cpp:33-44
		if (!(d == __builtin_huge_val()) && !(d < 0.0)) {
			double x = ray.px + d * ray.dx;
			double y = ray.py + d * ray.dy;
			double z = ray.pz + d * ray.dz;
			// hmap.cpp:998  int_point += (grid_width*0.01) * dir
			x = x + f.nudge * ray.dx;
			y = y + f.nudge * ray.dy;
			z = z + f.nudge * ray.dz;
			// hmap.cpp:1037  step_dist * dir is the same three products every iteration
			const double step_dist = LIT >= 2 ? sun.step_dist : f.step_dist;
			const double sx = step_dist * ray.dx;
			const double sy = step_dist * ray.dy;
			const double sz = step_dist * ray.dz;
			const double wlim = (double)f.map_w, hlim = (double)f.map_h;
			const double c0x = f.c0[0], c0y = f.c0[1];
			const bool pow2 = f.grid_pow2 != 0;
			int64_t budget = f.step_cap;
			if constexpr (SEG) budget = sg.budget; // (min(step cap, the ray's own limit))

			for (;;) {
				// hmap.cpp:1001-1004
				double qx, qy;
				if (pow2) {
					qx = (x - c0x) * f.inv_grid_width;
					qy = -(y - c0y) * f.inv_grid_width;
				} else {
					qx = (x - c0x) / f.grid_width;
					qy = -(y - c0y) / f.grid_width;
				}
				// hmap.cpp:1006-1011: (int)q >= 0  <=>  q > -1 ;  (int)q < W  <=>  q < W
				if (!(qx > -1.0 && qx < wlim && qy > -1.0 && qy < hlim)) break;
				if (budget-- <= 0) { my_cap = 1; break; }
				const int gridx = (int)qx, gridy = (int)qy;
				const int64_t cell = (int64_t)gridy * f.map_w + gridx;
				const double t = thr[cell]; // hmap.cpp:1013-1014 (+ c0.z folded in)
				if (COUNT) my_steps += 1;
				if (z < t) { // hmap.cpp:1016
					if constexpr (LIT != 4) { // (a cell map has no colours: `cmap` is null)
					const uint32_t c = cmap[cell];
					rgba = ((c >> 24) == 0) ? pack_rgba(f.bg[0], f.bg[1], f.bg[2]) : (c | 0xff000000u);
					}
					real_hit = true;
					if constexpr (RAYS) { hx = x; hy = y; hz = z; hgx = gridx; hgy = gridy; }
					if constexpr (LIT == 1) {
						lit->hx = x; lit->hy = y; lit->t = t;
						if (hit_cell) *hit_cell = (unsigned)cell; // (maps hold at most 2^29 cells)
						if (hit_z) *hit_z = z;
					}
					if constexpr (LIT == 5) {
						if (hit_cell) *hit_cell = (unsigned)cell;
					}
					if constexpr (LIT == 6) {
						lit->hx = x; lit->hy = y; lit->t = t;
						if (hit_cell) *hit_cell = (unsigned)cell;
					}
					break;
				}
				x = x + sx;
				y = y + sy;
				z = z + sz;
			}
		}

		if (!real_hit) {
			// hmap.cpp:1041-1057
			if (ray.dz > 0.0) {
				const double zz = ray.dz * ray.dz; // std::pow(z,2) == z*z under -std=c++98
				const double r_ = 220.0 * zz + (double)f.bg[0];
				const double g_ = 240.0 * zz + (double)f.bg[1];
				const double b_ = 255.0 * ray.dz + (double)f.bg[2];
				rgba = pack_rgba(sky_channel_literal(r_), sky_channel_literal(g_), sky_channel_literal(b_));
			} else {
				rgba = pack_rgba(f.bg[0], f.bg[1], f.bg[2]);
			}
		} else {
			my_hit = 1;
		}
		if constexpr (SEG) { // an END ray is not a capped one: not counted, never HMRM_E_NOTERM
			sg.ended = my_cap != 0u && sg.ends;
			my_cap = sg.ended ? 0u : my_cap;
		}
		if constexpr (LIT == 1) {
			lit->primary_hit = real_hit;
			lit->rgba = rgba;
		} else if constexpr (LIT == 2) {
			if (real_hit) lit->rgba = shade_shadowed(lit->rgba, sun.ambient); // (MISS, END and CAPPED leave the pixel lit)
		} else if constexpr (LIT == 3) {
			if (real_hit) lit->phase = 1;
		} else if constexpr (LIT == 4) {
			lit->phase = real_hit ? 1 : (my_cap != 0u ? 2 : (sg.ended ? 3 : 0));
		} else if constexpr (LIT == 5 || LIT == 6) {
			lit->rgba = rgba;
		} else
		if constexpr (RAYS && SEG) store_batch_hit(batch, ray_index, real_hit, my_cap != 0u, hx, hy, hz, hgx, hgy, sg.d_record, (uint32_t)my_steps, rgba, sg.ended);
		else if constexpr (RAYS) store_batch_hit(batch, ray_index, real_hit, my_cap != 0u, hx, hy, hz, hgx, hgy, d_box, (uint32_t)my_steps, rgba);
		else if constexpr (AA) aa_rgba = rgba;
		else out[(int64_t)lrow * out_stride_px + px] = rgba;
		if (STATS && st.steps_per_pixel)
			st.steps_per_pixel[(int64_t)py * f.screen_w + px] =
			    my_steps > 0xffffffffull ? 0xffffffffu : (uint32_t)my_steps;
	}
	if constexpr (AA) store_box_filtered(out, out_stride_px, f.aa_shift, (int)(threadIdx.x & 63), px, lrow, live, aa_rgba);

	publish_counters<STATS>(st, my_steps, my_hit, my_cap);
}

template <int PROJ, bool STATS, bool AA>
__global__ __launch_bounds__(kBlockThreads) void k_render(const DevFrame f, const RowMap rows,
                                                const double *__restrict__ thr,
                                                const uint32_t *__restrict__ cmap,
                                                uint32_t *__restrict__ out, int64_t out_stride_px,
                                                int tiles_y, StatsOut st) {
	// one small pixel tile per wave (device_common.hpp): neighbouring rays walk neighbouring
	// ground tracks, so a wave's height loads share cache lines and its lanes leave the loop
	// at similar times.
	render_lane_literal<PROJ, STATS, AA>(f, pixel_of_lane(f, rows, tiles_y), thr, cmap, out, out_stride_px, st, RayBatch{});
}

// The literal loop over a ray batch (HMRM_KERNEL=simple): the batch as a frame kBatchW pixels wide (frame.hpp RayBatch), one
// workgroup per 128 consecutive rays, grid rows beyond 32768 in blockIdx.z.
__global__ __launch_bounds__(kBlockThreads) void k_trace_rays_literal(const DevFrame f, const double *__restrict__ thr,
                                                                      const uint32_t *__restrict__ cmap, const RayBatch batch,
                                                                      int tiles_y, StatsOut st) {
	const RowMap rows = whole_frame_rows(f);
	const PixelId pid = pixel_of_tile_lane(f, rows, tiles_y, 0, blockIdx.z * 32768u + blockIdx.x, (int)(threadIdx.x >> 6),
	                                       (int)(threadIdx.x & 63));
	render_lane_literal<4, false, false>(f, pid, thr, cmap, nullptr, 0, st, batch);
}

// The same two under the segment rules (hmrm_render_interior, hmrm_trace_segments with HMRM_KERNEL=simple).
template <int PROJ>
__global__ __launch_bounds__(kBlockThreads) void k_render_interior_literal(const DevFrame f, const RowMap rows,
                                                                           const double *__restrict__ thr,
                                                                           const uint32_t *__restrict__ cmap,
                                                                           uint32_t *__restrict__ out, int64_t out_stride_px,
                                                                           int tiles_y, StatsOut st, const SegRules seg) {
	render_lane_literal<PROJ, false, false, true>(f, pixel_of_lane(f, rows, tiles_y), thr, cmap, out, out_stride_px, st, RayBatch{}, seg);
}
// A lit pixel (hmrm_render_lit with HMRM_KERNEL=simple): the literal loop twice, primary ray and shadow ray, one store.
template <int PROJ>
__global__ __launch_bounds__(kBlockThreads) void k_render_lit_literal(const DevFrame f, const RowMap rows,
                                                                      const double *__restrict__ thr,
                                                                      const uint32_t *__restrict__ cmap,
                                                                      uint32_t *__restrict__ out, int64_t out_stride_px,
                                                                      int tiles_y, StatsOut st, const SegRules seg, const SunRules sun) {
	const PixelId pid = pixel_of_lane(f, rows, tiles_y);
	LitState<true> lt;
	render_lane_literal<PROJ, false, false, true, 1>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{}, seg, sun, &lt);
	render_lane_literal<PROJ, false, false, true, 2>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{},
	                                                 SegRules{nullptr, sun.max_steps, 1u}, sun, &lt);
	if (pid.live) out[(int64_t)pid.lrow * out_stride_px + pid.px] = lt.rgba;
}
// A hill-shaded pixel (hmrm_render_shaded with HMRM_KERNEL=simple): the primary ray, SHADOWS: its shadow ray, then the weight --
// the ambient level for a shadowed pixel, else that of the diffuse level of the hit cell, which pass 1 hands over.
template <int PROJ, bool SHADOWS>
__global__ __launch_bounds__(kBlockThreads) void k_render_shaded_literal(const DevFrame f, const RowMap rows,
                                                                         const double *__restrict__ thr,
                                                                         const uint32_t *__restrict__ cmap,
                                                                         uint32_t *__restrict__ out, int64_t out_stride_px,
                                                                         int tiles_y, StatsOut st, const SegRules seg, const SunRules sun) {
	const PixelId pid = pixel_of_lane(f, rows, tiles_y);
	LitState<true> lt;
	unsigned cell = 0u;
	render_lane_literal<PROJ, false, false, true, 1>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{}, seg, sun, &lt, &cell);
	if constexpr (SHADOWS)
		render_lane_literal<PROJ, false, false, true, 3>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{},
		                                                 SegRules{nullptr, sun.max_steps, 1u}, sun, &lt);
	if (!pid.live) return;
	uint32_t rgba = lt.rgba;
	if (lt.primary_hit) {
		uint32_t w = sun.ambient;
		if (lt.phase == 0) w = shade_weight(sun.ambient, diffuse_level_nearest<false>(f, thr, cell, sun.dir));
		rgba = shade_weighted(rgba, w);
	}
	out[(int64_t)pid.lrow * out_stride_px + pid.px] = rgba;
}
// The antialiased lit and hill-shaded pixels (hmrm_render_shaded_aa with HMRM_KERNEL=simple): the same passes per sample of the
// super frame; the lane's final sample goes to the wave's box filter (store_box_filtered: every lane of the wave calls it,
// so no lane returns before) and not to memory.  Kernels of their own: the two above keep their instructions.
template <int PROJ>
__global__ __launch_bounds__(kBlockThreads) void k_render_lit_literal_aa(const DevFrame f, const RowMap rows,
                                                                         const double *__restrict__ thr,
                                                                         const uint32_t *__restrict__ cmap,
                                                                         uint32_t *__restrict__ out, int64_t out_stride_px,
                                                                         int tiles_y, StatsOut st, const SegRules seg, const SunRules sun) {
	const PixelId pid = pixel_of_lane(f, rows, tiles_y);
	LitState<true> lt;
	render_lane_literal<PROJ, false, false, true, 1>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{}, seg, sun, &lt);
	render_lane_literal<PROJ, false, false, true, 2>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{},
	                                                 SegRules{nullptr, sun.max_steps, 1u}, sun, &lt);
	store_box_filtered(out, out_stride_px, f.aa_shift, (int)(threadIdx.x & 63), pid.px, pid.lrow, pid.live, pid.live ? lt.rgba : 0u);
}
template <int PROJ, bool SHADOWS>
__global__ __launch_bounds__(kBlockThreads) void k_render_shaded_literal_aa(const DevFrame f, const RowMap rows,
                                                                            const double *__restrict__ thr,
                                                                            const uint32_t *__restrict__ cmap,
                                                                            uint32_t *__restrict__ out, int64_t out_stride_px,
                                                                            int tiles_y, StatsOut st, const SegRules seg, const SunRules sun) {
	const PixelId pid = pixel_of_lane(f, rows, tiles_y);
	LitState<true> lt;
	unsigned cell = 0u;
	render_lane_literal<PROJ, false, false, true, 1>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{}, seg, sun, &lt, &cell);
	if constexpr (SHADOWS)
		render_lane_literal<PROJ, false, false, true, 3>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{},
		                                                 SegRules{nullptr, sun.max_steps, 1u}, sun, &lt);
	uint32_t rgba = 0u;
	if (pid.live) {
		rgba = lt.rgba;
		if (lt.primary_hit) {
			uint32_t w = sun.ambient;
			if (lt.phase == 0) w = shade_weight(sun.ambient, diffuse_level_nearest<false>(f, thr, cell, sun.dir));
			rgba = shade_weighted(rgba, w);
		}
	}
	store_box_filtered(out, out_stride_px, f.aa_shift, (int)(threadIdx.x & 63), pid.px, pid.lrow, pid.live, rgba);
}
__global__ __launch_bounds__(kBlockThreads) void k_trace_segments_literal(const DevFrame f, const double *__restrict__ thr,
                                                                          const uint32_t *__restrict__ cmap, const RayBatch batch,
                                                                          const SegRules seg, int tiles_y, StatsOut st) {
	const RowMap rows = whole_frame_rows(f);
	const PixelId pid = pixel_of_tile_lane(f, rows, tiles_y, 0, blockIdx.z * 32768u + blockIdx.x, (int)(threadIdx.x >> 6),
	                                       (int)(threadIdx.x & 63));
	render_lane_literal<4, false, false, true>(f, pid, thr, cmap, nullptr, 0, st, batch, seg);
}

// A cell of a cell map (hmrm_cell_map with HMRM_KERNEL=simple, or on a map with a side of 2^24 cells; frame.hpp CellRules):
// the cell's ray (device_common.hpp cell_ray) through the literal loop as a shadow ray is, then the byte.  The "frame" is the
// rect, tiled like a frame; nearest sampling only, like every literal kernel.
__global__ __launch_bounds__(kBlockThreads) void k_cell_map_literal(const DevFrame f, const double *__restrict__ thr,
                                                                    uint8_t *__restrict__ out, int64_t stride_bytes,
                                                                    const CellRules cells, int tiles_y, StatsOut st) {
	const RowMap rows = whole_frame_rows(f);
	const PixelId pid = pixel_of_lane(f, rows, tiles_y);
	LitState<true> lt;
	DevRay ray{};
	size_t cell = 0; // (gridx + gridy * W of the lane's cell)
	if (pid.live) {
		const int cx = cells.x0 + pid.px, cy = cells.y0 + pid.py;
		cell = (size_t)cy * (size_t)f.map_w + (size_t)cx;
		ray = cell_ray(cells, f, cx, cy, thr[cell]);
	}
	const SunRules sun{{ray.dx, ray.dy, ray.dz}, f.step_dist, cells.max_steps, cells.ambient};
	lt.hx = ray.px; lt.hy = ray.py; lt.t = ray.pz;
	lt.primary_hit = (cells.flags & kMapNoShadows) == 0u; // (without shadows no lane marches)
	render_lane_literal<3, false, false, true, 4>(f, pid, thr, nullptr, nullptr, 0, st, RayBatch{}, SegRules{nullptr, cells.max_steps, 1u},
	                                              sun, &lt);
	if (!pid.live) return;
	uint32_t v = (uint32_t)lt.phase;
	if ((cells.flags & kMapWeight) != 0u) {
		uint32_t q = 0u;
		if ((cells.flags & kMapDiffuse) != 0u && lt.phase != 1)
			q = diffuse_level_nearest<false>(f, thr, (unsigned)cell, sun.dir); // (maps hold at most 2^29 cells)
		v = cell_weight(cells, lt.phase == 1, q);
	}
	out[(int64_t)pid.lrow * stride_bytes + pid.px] = (uint8_t)v;
}

// A cell of an accumulated cell map (hmrm_cell_map_sum; frame.hpp CellSums): the loop over the targets around the same pass --
// the cell's ray towards target k through the literal loop, the value k_cell_map_literal would have stored for it (or 1 for a
// ray that did not hit) added up -- and one 16-bit word at the end.  Every pass publishes its own capped ray.
__global__ __launch_bounds__(kBlockThreads) void k_cell_map_sum_literal(const DevFrame f, const double *__restrict__ thr,
                                                                        uint16_t *__restrict__ out, int64_t stride_bytes,
                                                                        const CellRules cells, const CellSums sums, int tiles_y,
                                                                        StatsOut st) {
	const RowMap rows = whole_frame_rows(f);
	const PixelId pid = pixel_of_lane(f, rows, tiles_y);
	const int cx = cells.x0 + pid.px, cy = cells.y0 + pid.py;
	const size_t cell = pid.live ? (size_t)cy * (size_t)f.map_w + (size_t)cx : 0; // (gridx + gridy * W of the lane's cell)
	uint32_t acc = 0u;
	for (int k = 0; k < sums.n; ++k) {
		CellRules rules = cells;
		rules.target[0] = sums.targets[3 * k];
		rules.target[1] = sums.targets[3 * k + 1];
		rules.target[2] = sums.targets[3 * k + 2];
		LitState<true> lt;
		DevRay ray{};
		if (pid.live) ray = cell_ray(rules, f, cx, cy, thr[cell]);
		const SunRules sun{{ray.dx, ray.dy, ray.dz}, f.step_dist, cells.max_steps, cells.ambient};
		lt.hx = ray.px; lt.hy = ray.py; lt.t = ray.pz;
		lt.primary_hit = (cells.flags & kMapNoShadows) == 0u; // (without shadows no lane marches)
		render_lane_literal<3, false, false, true, 4>(f, pid, thr, nullptr, nullptr, 0, st, RayBatch{},
		                                              SegRules{nullptr, cells.max_steps, 1u}, sun, &lt);
		uint32_t v = lt.phase != 1 ? 1u : 0u;
		if ((cells.flags & kMapWeight) != 0u) {
			uint32_t q = 0u;
			if ((cells.flags & kMapDiffuse) != 0u && lt.phase != 1 && pid.live)
				q = diffuse_level_nearest<false>(f, thr, (unsigned)cell, sun.dir); // (maps hold at most 2^29 cells)
			v = cell_weight(cells, lt.phase == 1, q);
		}
		acc += v;
	}
	if (!pid.live) return;
	*reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(out) + (int64_t)pid.lrow * stride_bytes + 2 * (int64_t)pid.px) = (uint16_t)acc;
}

// A pixel of a geometry frame (hmrm_render_geometry with HMRM_KERNEL=simple, or on a map with a side of 2^24 cells; frame.hpp
// GeomPlanes): the primary ray of a lit pixel -- its colour, whether it hit, where and in which cell -- then the planes, each
// through a pointer that may be null.  Nearest sampling only, like every literal kernel.
template <int PROJ>
__global__ __launch_bounds__(kBlockThreads) void k_render_geometry_literal(const DevFrame f, const RowMap rows,
                                                                           const double *__restrict__ thr,
                                                                           const uint32_t *__restrict__ cmap,
                                                                           uint32_t *__restrict__ out, int64_t out_stride_px,
                                                                           int tiles_y, StatsOut st, const SegRules seg,
                                                                           const GeomPlanes geo) {
	const PixelId pid = pixel_of_lane(f, rows, tiles_y);
	LitState<true> lt;
	unsigned cell = 0u;
	double hz = 0.0;
	render_lane_literal<PROJ, false, false, true, 1>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{}, seg, SunRules{}, &lt, &cell, &hz);
	if (!pid.live) return;
	if (out != nullptr) out[(int64_t)pid.lrow * out_stride_px + pid.px] = lt.rgba;
	store_geometry<PROJ>(f, geo, pid, lt.primary_hit, cell, lt.hx, lt.hy, hz);
	if (geo.slope != nullptr) {
		Gradient g{0.0, 0.0};
		if (lt.primary_hit) g = gradient_nearest<false>(f, thr, cell);
		store_slope(geo, pid, lt.primary_hit, g.gx, g.gy);
	}
}

// A pixel of an accumulated lit frame (hmrm_render_lit_sum with HMRM_KERNEL=simple, or on a map with a side of 2^24 cells;
// frame.hpp LightSum): the primary ray of a lit pixel, then the loop over the directions around pass 3 -- the shadow ray towards
// direction k through the literal loop (unless HMRM_SHADE_NO_SHADOWS), hmrm_render_shaded's weight for it added up -- then the
// pixel under its sum and / or the sum itself, each through a pointer that may be null.  Every pass publishes its own capped ray.
template <int PROJ>
__global__ __launch_bounds__(kBlockThreads) void k_render_lit_sum_literal(const DevFrame f, const RowMap rows,
                                                                          const double *__restrict__ thr,
                                                                          const uint32_t *__restrict__ cmap,
                                                                          uint32_t *__restrict__ out, int64_t out_stride_px,
                                                                          int tiles_y, StatsOut st, const SegRules seg, const SunRules sun,
                                                                          const LightSum lsum) {
	const PixelId pid = pixel_of_lane(f, rows, tiles_y);
	LitState<true> lt;
	unsigned cell = 0u;
	render_lane_literal<PROJ, false, false, true, 1>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{}, seg, sun, &lt, &cell);
	uint32_t acc = 0u;
	for (int k = 0; k < lsum.n; ++k) {
		SunRules sk = sun;
		sk.dir[0] = lsum.dirs[3 * k];
		sk.dir[1] = lsum.dirs[3 * k + 1];
		sk.dir[2] = lsum.dirs[3 * k + 2];
		lt.phase = 0;
		if ((lsum.flags & kShadeNoShadows) == 0u)
			render_lane_literal<PROJ, false, false, true, 3>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{},
			                                                 SegRules{nullptr, sun.max_steps, 1u}, sk, &lt);
		if (pid.live && lt.primary_hit) {
			uint32_t w = lt.phase != 0 ? sun.ambient : 255u;
			if ((lsum.flags & kShadeDiffuse) != 0u && lt.phase == 0) w = shade_weight(sun.ambient, diffuse_level_nearest<false>(f, thr, cell, sk.dir));
			acc += w;
		}
	}
	if (!pid.live) return;
	if (out != nullptr) out[(int64_t)pid.lrow * out_stride_px + pid.px] = lt.primary_hit ? shade_summed(lt.rgba, acc, (uint32_t)lsum.n) : lt.rgba;
	if (lsum.light != nullptr)
		*reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(lsum.light) + (int64_t)pid.lrow * lsum.light_stride + 2 * (int64_t)pid.px) =
		    lt.primary_hit ? (uint16_t)acc : (uint16_t)0xffffu;
}

// A pixel of a baked-light frame (hmrm_render_baked with HMRM_KERNEL=simple, or on a map with a side of 2^24 cells; frame.hpp
// BakedLight): the primary ray of a lit pixel -- its colour, whether it hit and in which cell -- then the pixel under the plane's
// word of that cell.  AA: the lane's sample goes to the wave's box filter (every lane of the wave calls it, so no lane returns
// before) and not to memory.  Nearest sampling only, like every literal kernel.
template <int PROJ, bool AA>
__global__ __launch_bounds__(kBlockThreads) void k_render_baked_literal(const DevFrame f, const RowMap rows,
                                                                        const double *__restrict__ thr,
                                                                        const uint32_t *__restrict__ cmap,
                                                                        uint32_t *__restrict__ out, int64_t out_stride_px,
                                                                        int tiles_y, StatsOut st, const SegRules seg,
                                                                        const BakedLight baked) {
	const PixelId pid = pixel_of_lane(f, rows, tiles_y);
	LitState<true> lt;
	unsigned cell = 0u;
	render_lane_literal<PROJ, false, false, true, 1>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{}, seg, SunRules{}, &lt, &cell);
	uint32_t rgba = 0u;
	if (pid.live) {
		rgba = lt.rgba;
		if (lt.primary_hit) rgba = shade_baked(rgba, baked.plane[cell], baked.full_scale);
	}
	if constexpr (AA) store_box_filtered(out, out_stride_px, f.aa_shift, (int)(threadIdx.x & 63), pid.px, pid.lrow, pid.live, rgba);
	else if (pid.live) out[(int64_t)pid.lrow * out_stride_px + pid.px] = rgba;
}

// A pixel of a water frame (hmrm_render_water with HMRM_KERNEL=simple, or on a map with a side of 2^24 cells; frame.hpp WaterRules):
// the primary ray of a lit pixel -- its colour, whether it hit, where and under which threshold -- then, for a lane that hit at or
// below the water level, the literal loop once more for its mirror ray -- the camera's ray made again, with dz negated -- and the
// blend.  Nearest sampling only, like every literal kernel.
template <int PROJ>
__global__ __launch_bounds__(kBlockThreads) void k_render_water_literal(const DevFrame f, const RowMap rows,
                                                                        const double *__restrict__ thr,
                                                                        const uint32_t *__restrict__ cmap,
                                                                        uint32_t *__restrict__ out, int64_t out_stride_px,
                                                                        int tiles_y, StatsOut st, const SegRules seg,
                                                                        const WaterRules water) {
	const PixelId pid = pixel_of_lane(f, rows, tiles_y);
	LitState<true> lt;
	render_lane_literal<PROJ, false, false, true, 1>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{}, seg, SunRules{}, &lt);
	const bool wet = pid.live && lt.primary_hit && lt.t <= water.level; // (a NaN level: no water)
	LitState<true> mr = lt;
	mr.primary_hit = wet; // (the other lanes sit the pass out)
	SunRules mirror{{0.0, 0.0, 0.0}, water.step_dist, water.max_steps, 0u};
	if (wet) {
		const DevRay primary = make_ray<PROJ>(f, pid.px, pid.py);
		mirror.dir[0] = primary.dx; mirror.dir[1] = primary.dy; mirror.dir[2] = -primary.dz;
	}
	render_lane_literal<PROJ, false, false, true, 5>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{},
	                                                 SegRules{nullptr, water.max_steps, 1u}, mirror, &mr);
	if (pid.live) out[(int64_t)pid.lrow * out_stride_px + pid.px] = wet ? blend_water(lt.rgba, mr.rgba, water) : lt.rgba;
}

// Per-ray parity hook: GetRay + distance() of one pixel -> out[0..2] pos, [3..5] dir, [6] d.
template <int PROJ>
__global__ void k_probe(const DevFrame f, int px, int py, double *__restrict__ out) {
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	const DevRay r = make_ray<PROJ>(f, px, py);
	out[0] = r.px; out[1] = r.py; out[2] = r.pz;
	out[3] = r.dx; out[4] = r.dy; out[5] = r.dz;
	out[6] = slab_distance(r, f);
}

// Accuracy probe for v_rcp_f64 (test hook; device_common.hpp slab_classify rests on the bound it reports).
// For every sample x: r = rcp(x) and e = |fma(r, x, -1)|, which is |r - 1/x| / |1/x| up to a factor 1 + 2^-53
// (r*x - 1 is formed exactly inside the fma and rounded once).  mode 0 walks the leading 32 mantissa bits
// exhaustively (sample i has them = i; the 20 trailing bits are 0, all ones, or hashed, by `seed & 3`; exponent
// exp_lo, positive); mode 1 hashes mantissa, sign and an exponent in [exp_lo, exp_hi]; mode 2 measures what the
// shortcut really forms, t' = n * rcp(d) against the correctly rounded n / d (|t' - q| / |q|: the difference of two
// neighbours is exact), with hashed n of exponent in [exp_lo, exp_hi] and direction-like d (exponent -40..0).
// out[0] = max e as fp64 bits (positive doubles order like integers), hist[k] = samples with e in [2^-k, 2^-(k-1)).
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
	z += 0x9e3779b97f4a7c15ull;
	z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
	z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
	return z ^ (z >> 31);
}
__global__ __launch_bounds__(256) void k_rcp_error(int mode, uint64_t count, uint64_t seed, int exp_lo, int exp_hi,
                                                   unsigned long long *__restrict__ out_max,
                                                   unsigned long long *__restrict__ hist) {
	__shared__ unsigned int lh[64];
	if (threadIdx.x < 64) lh[threadIdx.x] = 0u;
	__syncthreads();
	const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
	double worst = 0.0;
	const unsigned span = (unsigned)(exp_hi - exp_lo + 1);
	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
		const uint64_t h = mix64(i ^ (seed * 0x9e3779b97f4a7c15ull));
		double e;
		if (mode == 2) {
			const uint64_t h2 = mix64(h);
			const uint64_t nb = (h & 0x800fffffffffffffull) | ((uint64_t)(1023 + exp_lo + (int)((h >> 52) % span)) << 52);
			const uint64_t db = (h2 & 0x800fffffffffffffull) | ((uint64_t)(1023 - (int)((h2 >> 52) % 41u)) << 52);
			const double n = __longlong_as_double((long long)nb), d = __longlong_as_double((long long)db);
			const double t = n * __builtin_amdgcn_rcp(d), q = n / d;
			e = __builtin_fabs(t - q) / __builtin_fabs(q);
		} else {
			uint64_t b;
			if (mode == 0) {
				const uint64_t low = (seed & 3) == 0 ? 0ull : ((seed & 3) == 1 ? 0xfffffull : (h & 0xfffffull));
				b = ((uint64_t)(1023 + exp_lo) << 52) | ((i & 0xffffffffull) << 20) | low;
			} else {
				b = (h & 0x800fffffffffffffull) | ((uint64_t)(1023 + exp_lo + (int)((h >> 52) % span)) << 52);
			}
			const double x = __longlong_as_double((long long)b);
			const double r = __builtin_amdgcn_rcp(x);
			e = __builtin_fabs(__builtin_fma(r, x, -1.0));
		}
		worst = __builtin_fmax(worst, e);
		// bin = -exponent of e, clamped to 0..63 (e == 0 -> 63)
		int k = 1023 - (int)((((unsigned long long)__double_as_longlong(e)) >> 52) & 0x7ffu);
		k = e == 0.0 ? 63 : (k < 0 ? 0 : (k > 63 ? 63 : k));
		atomicAdd(&lh[k], 1u);
	}
	for (int off = 32; off > 0; off >>= 1) worst = __builtin_fmax(worst, __shfl_xor(worst, off));
	if ((threadIdx.x & 63) == 0) atomicMax(out_max, (unsigned long long)__double_as_longlong(worst));
	__syncthreads();
	if (threadIdx.x < 64 && lh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)lh[threadIdx.x]);
}

hipError_t launch_rcp_error(int mode, uint64_t count, uint64_t seed, int exp_lo, int exp_hi,
                            unsigned long long *d_out65, hipStream_t stream) {
	// (a block's LDS histogram counts in 32 bits: at most 2^32 / 4096 blocks... keep every block below 2^31 samples)
	hipLaunchKernelGGL(k_rcp_error, dim3(256 * 16), dim3(256), 0, stream, mode, count, seed, exp_lo, exp_hi, d_out65,
	                   d_out65 + 1);
	return hipGetLastError();
}

// Spherical tables, pinned host staging -> device, by a kernel of the launch stream instead of a copy command: a
// DMA copy between two kernels of one stream costs two cross-engine hand-overs (~25 us per frame measured on a
// moving camera); this is one more small dispatch on the same queue, reading 96 KB (4K frame) over PCIe.
__global__ __launch_bounds__(256) void k_upload_tables(const double *__restrict__ host_src, double *__restrict__ dst, int n) {
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (i < n) dst[i] = host_src[i];
}

hipError_t launch_upload_tables(const double *h_pinned, double *d_dst, size_t n, hipStream_t stream) {
	if (n == 0 || n > 0x7fffffffu) return n ? hipErrorInvalidValue : hipSuccess;
	hipLaunchKernelGGL(k_upload_tables, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, h_pinned, d_dst, (int)n);
	return hipGetLastError();
}

// ------------------------------------------------------------- launchers ----
// fn(proj): the projection as the kernels' template argument.
template <class Fn>
static void dispatch_projection(int projection, Fn &&fn) {
	switch (projection) {
	case 1: fn(MarchConst<1>{}); break;
	case 2: fn(MarchConst<2>{}); break;
	default: fn(MarchConst<3>{}); break;
	}
}

hipError_t launch_probe(const DevFrame &f, int px, int py, double *d_out7, hipStream_t stream) {
	dispatch_projection(f.projection, [&](auto proj) { hipLaunchKernelGGL(k_probe<proj()>, dim3(1), dim3(64), 0, stream, f, px, py, d_out7); });
	return hipGetLastError();
}

hipError_t launch_prepare_heights(const uint8_t *d_rgb, double *d_out, int64_t n, double lum_r,
                                  double lum_g, double lum_b, double min_h, double max_h, bool plain,
                                  unsigned long long *d_max_key, hipStream_t stream) {
	int64_t blocks = (n + 255) / 256;
	if (blocks > 256 * 8) blocks = 256 * 8; // grid-stride the rest
	if (blocks < 1) blocks = 1;
	if (plain)
		hipLaunchKernelGGL(k_prepare_heights<true>, dim3((unsigned)blocks), dim3(256), 0, stream, d_rgb,
		                   d_out, n, lum_r, lum_g, lum_b, min_h, max_h, d_max_key);
	else
		hipLaunchKernelGGL(k_prepare_heights<false>, dim3((unsigned)blocks), dim3(256), 0, stream, d_rgb,
		                   d_out, n, lum_r, lum_g, lum_b, min_h, max_h, d_max_key);
	return hipGetLastError();
}

double max_key_to_double(unsigned long long key) {
	unsigned long long b = (key & 0x8000000000000000ull) ? (key & 0x7fffffffffffffffull) : ~key;
	double v;
	__builtin_memcpy(&v, &b, sizeof v);
	return v;
}

hipError_t launch_trace_rays_literal(const DevFrame &f, const double *d_thr, const uint32_t *d_cmap, const RayBatch &batch,
                                     unsigned long long *d_counters, hipStream_t stream) {
	const LaunchGrid g = batch_grid(f, batch);
	if (g.tiles_y == 0) return g.err;
	hipLaunchKernelGGL(k_trace_rays_literal, g.grid, dim3(kBlockThreads), 0, stream, f, d_thr, d_cmap, batch, g.tiles_y,
	                   StatsOut{d_counters, nullptr, nullptr});
	return hipGetLastError();
}

hipError_t launch_trace_segments_literal(const DevFrame &f, const double *d_thr, const uint32_t *d_cmap, const RayBatch &batch,
                                         const SegRules &seg, unsigned long long *d_counters, hipStream_t stream) {
	const LaunchGrid g = batch_grid(f, batch);
	if (g.tiles_y == 0) return g.err;
	hipLaunchKernelGGL(k_trace_segments_literal, g.grid, dim3(kBlockThreads), 0, stream, f, d_thr, d_cmap, batch, seg, g.tiles_y,
	                   StatsOut{d_counters, nullptr, nullptr});
	return hipGetLastError();
}

hipError_t launch_cell_map_literal(const DevFrame &f, const double *d_thr, uint8_t *d_out, int64_t stride_bytes, const CellRules &cells,
                                   unsigned long long *d_counters, hipStream_t stream) {
	const RowMap rows = whole_frame_rows(f);
	const LaunchGrid g = tile_grid(f, rows);
	if (g.tiles_y == 0) return g.err;
	hipLaunchKernelGGL(k_cell_map_literal, g.grid, dim3(kBlockThreads), 0, stream, f, d_thr, d_out, stride_bytes, cells, g.tiles_y,
	                   StatsOut{d_counters, nullptr, nullptr});
	return hipGetLastError();
}

hipError_t launch_cell_map_sum_literal(const DevFrame &f, const double *d_thr, uint16_t *d_out, int64_t stride_bytes,
                                       const CellRules &cells, const CellSums &sums, unsigned long long *d_counters, hipStream_t stream) {
	const RowMap rows = whole_frame_rows(f);
	const LaunchGrid g = tile_grid(f, rows);
	if (g.tiles_y == 0) return g.err;
	hipLaunchKernelGGL(k_cell_map_sum_literal, g.grid, dim3(kBlockThreads), 0, stream, f, d_thr, d_out, stride_bytes, cells, sums,
	                   g.tiles_y, StatsOut{d_counters, nullptr, nullptr});
	return hipGetLastError();
}

// One frame by the literal loop.  `launch(proj, grid, args...)` launches the family's kernel for that projection on that grid
// with `args...` as its leading arguments: frame, row map, table, colours, target, stride, tile rows, counters.
template <class Launch>
static hipError_t launch_literal(const FrameLaunch &l, const StatsOut &st, Launch &&launch) {
	const LaunchGrid g = tile_grid(l.f, l.rows);
	if (g.tiles_y == 0) return g.err;
	dispatch_projection(l.f.projection, [&](auto proj) {
		launch(proj, g.grid, l.f, l.rows, l.d_thr, l.d_cmap, l.d_out, l.out_stride_px, g.tiles_y, st);
	});
	return hipGetLastError();
}

static hipError_t launch_plain_literal(const FrameLaunch &l); // (hmrm_render's frame: below)
static hipError_t launch_geometry_literal(const FrameLaunch &l); // (hmrm_render_geometry's, and behind them hmrm_render_lit_sum's:
static hipError_t launch_lit_sum_literal(const FrameLaunch &l);  //  the last kernels of the code object)
static hipError_t launch_baked_literal(const FrameLaunch &l);    // (hmrm_render_baked's, behind those)
static hipError_t launch_water_literal(const FrameLaunch &l);    // (hmrm_render_water's, behind those)
static hipError_t launch_water_literal_more(const FrameLaunch &l); // (hmrm_render_water_aa's, behind those)
static hipError_t launch_water_lit_literal(const FrameLaunch &l);  // (hmrm_render_water_lit's, behind those)
static hipError_t launch_haze_literal(const FrameLaunch &l);       // (hmrm_render_haze's, behind those)
static hipError_t launch_views_literal(const FrameLaunch &l);      // (hmrm_render_views', the last kernels of the code object)

// The interior family's kernel takes the segment rules behind the common arguments, the lit and shaded ones the sun too; the
// shaded ones are built without shadow rays (kFrameShaded) and with them (kFrameLitShaded).  (The families one by one and in
// this order, which is the order of the kernels in the code object.)
hipError_t launch_frame_literal(const FrameLaunch &l) {
	if (l.family == kFramePlain) return launch_plain_literal(l);
	const StatsOut st{l.d_counters, nullptr, nullptr};
	const SegRules seg = frame_seg_rules(l);
	const dim3 block(kBlockThreads);
	if (l.family == kFrameInterior)
		return launch_literal(l, st, [&](auto proj, dim3 grid, const auto &...args) {
			hipLaunchKernelGGL(k_render_interior_literal<proj()>, grid, block, 0, l.stream, args..., seg);
		});
	if (l.family == kFrameGeometry) return launch_geometry_literal(l);
	if (l.family == kFrameLitSum) return launch_lit_sum_literal(l);
	if (l.family == kFrameBaked) return launch_baked_literal(l);
	if (l.family == kFrameWater) return launch_water_literal(l);
	if (l.family == kFrameWaterAA || l.family == kFrameWaterBaked || l.family == kFrameWaterBakedAA) return launch_water_literal_more(l);
	if (l.family == kFrameWaterLit) return launch_water_lit_literal(l);
	if (l.family == kFrameHaze) return launch_haze_literal(l);
	if (l.family == kFrameViews) return launch_views_literal(l);
	if (l.f.aa_shift == 0) switch (l.family) {
		case kFrameLit:
			return launch_literal(l, st, [&](auto proj, dim3 grid, const auto &...args) {
				hipLaunchKernelGGL(k_render_lit_literal<proj()>, grid, block, 0, l.stream, args..., seg, l.sun);
			});
		case kFrameLitShaded:
			return launch_literal(l, st, [&](auto proj, dim3 grid, const auto &...args) {
				hipLaunchKernelGGL((k_render_shaded_literal<proj(), true>), grid, block, 0, l.stream, args..., seg, l.sun);
			});
		default:
			return launch_literal(l, st, [&](auto proj, dim3 grid, const auto &...args) {
				hipLaunchKernelGGL((k_render_shaded_literal<proj(), false>), grid, block, 0, l.stream, args..., seg, l.sun);
			});
		}
	// The antialiased ones: f is the super frame, d_out the filtered frame's.  Never a measured launch.
	if (l.rows.measure != nullptr) return hipErrorInvalidValue;
	switch (l.family) {
	case kFrameLit:
		return launch_literal(l, st, [&](auto proj, dim3 grid, const auto &...args) {
			hipLaunchKernelGGL(k_render_lit_literal_aa<proj()>, grid, block, 0, l.stream, args..., seg, l.sun);
		});
	case kFrameLitShaded:
		return launch_literal(l, st, [&](auto proj, dim3 grid, const auto &...args) {
			hipLaunchKernelGGL((k_render_shaded_literal_aa<proj(), true>), grid, block, 0, l.stream, args..., seg, l.sun);
		});
	default:
		return launch_literal(l, st, [&](auto proj, dim3 grid, const auto &...args) {
			hipLaunchKernelGGL((k_render_shaded_literal_aa<proj(), false>), grid, block, 0, l.stream, args..., seg, l.sun);
		});
	}
}

// hmrm_render's frame: instrumented or not, antialiased or not.
template <bool STATS, bool AA>
static hipError_t launch_render_t(const FrameLaunch &l) {
	return launch_literal(l, StatsOut{l.d_counters, l.d_steps, l.d_entry}, [&](auto proj, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL((k_render<proj(), STATS, AA>), grid, dim3(kBlockThreads), 0, l.stream, args...);
	});
}
static hipError_t launch_plain_literal(const FrameLaunch &l) {
	if (l.f.aa_shift) return l.stats ? launch_render_t<true, true>(l) : launch_render_t<false, true>(l);
	return l.stats ? launch_render_t<true, false>(l) : launch_render_t<false, false>(l);
}

// A geometry frame: the interior family's arguments and the planes.  No antialiased variant, never a measured launch.
static hipError_t launch_geometry_literal(const FrameLaunch &l) {
	if (l.f.aa_shift != 0 || l.rows.measure != nullptr) return hipErrorInvalidValue;
	const SegRules seg = frame_seg_rules(l);
	return launch_literal(l, StatsOut{l.d_counters, nullptr, nullptr}, [&](auto proj, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL(k_render_geometry_literal<proj()>, grid, dim3(kBlockThreads), 0, l.stream, args..., seg, l.geo);
	});
}

// An accumulated lit frame: the lit family's arguments and the list.  No antialiased variant, never a measured launch.
static hipError_t launch_lit_sum_literal(const FrameLaunch &l) {
	if (l.f.aa_shift != 0 || l.rows.measure != nullptr) return hipErrorInvalidValue;
	if (l.lsum.n < 1 || l.lsum.n > kMaxSumDirs || !l.lsum.dirs || (!l.d_out && !l.lsum.light)) return hipErrorInvalidValue;
	const SegRules seg = frame_seg_rules(l);
	return launch_literal(l, StatsOut{l.d_counters, nullptr, nullptr}, [&](auto proj, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL(k_render_lit_sum_literal<proj()>, grid, dim3(kBlockThreads), 0, l.stream, args..., seg, l.sun, l.lsum);
	});
}

// dst[y * w + x] = src[y * src_stride + x]: one thread per cell, rows in blockIdx.y.
__global__ __launch_bounds__(256) void k_widen_light(const uint8_t *__restrict__ src, size_t src_stride, int w, int h,
                                                     uint16_t *__restrict__ dst) {
	const int x = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	for (int y = (int)blockIdx.y; y < h; y += (int)gridDim.y)
		if (x < w) dst[(size_t)y * (size_t)w + (size_t)x] = (uint16_t)src[(size_t)y * src_stride + (size_t)x];
}
hipError_t launch_widen_light(const uint8_t *d_src, size_t src_stride, int w, int h, uint16_t *d_dst, hipStream_t stream) {
	if (w <= 0 || h <= 0) return hipErrorInvalidValue;
	const dim3 grid((unsigned)((w + 255) / 256), (unsigned)(h < 65535 ? h : 65535));
	hipLaunchKernelGGL(k_widen_light, grid, dim3(256), 0, stream, d_src, src_stride, w, h, d_dst);
	return hipGetLastError();
}

// A baked-light frame: the interior family's arguments and the plane, antialiased or not.  Never a measured launch.
static hipError_t launch_baked_literal(const FrameLaunch &l) {
	if (l.rows.measure != nullptr || !l.d_out) return hipErrorInvalidValue;
	if (!l.baked.plane || l.baked.full_scale < 1u || l.baked.full_scale > 65535u) return hipErrorInvalidValue;
	const SegRules seg = frame_seg_rules(l);
	const bool aa = l.f.aa_shift != 0;
	return launch_literal(l, StatsOut{l.d_counters, nullptr, nullptr}, [&](auto proj, dim3 grid, const auto &...args) {
		if (aa) hipLaunchKernelGGL((k_render_baked_literal<proj(), true>), grid, dim3(kBlockThreads), 0, l.stream, args..., seg, l.baked);
		else hipLaunchKernelGGL((k_render_baked_literal<proj(), false>), grid, dim3(kBlockThreads), 0, l.stream, args..., seg, l.baked);
	});
}

// A water frame: the interior family's arguments and the water's rules.  No antialiased variant, never a measured launch.
static hipError_t launch_water_literal(const FrameLaunch &l) {
	if (l.rows.measure != nullptr || l.f.aa_shift != 0 || !l.d_out) return hipErrorInvalidValue;
	const SegRules seg = frame_seg_rules(l);
	return launch_literal(l, StatsOut{l.d_counters, nullptr, nullptr}, [&](auto proj, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL(k_render_water_literal<proj()>, grid, dim3(kBlockThreads), 0, l.stream, args..., seg, l.water);
	});
}

// A pixel of an antialiased water frame and / or one under the light plane (hmrm_render_water_aa with HMRM_KERNEL=simple, or on a
// map with a side of 2^24 cells): k_render_water_literal's two passes, which also hand back the two hit cells; BAKED: the base --
// the primary pixel, or a wet lane's own colour -- under the plane's word of the primary hit's cell, and the mirror pixel under
// that of the mirror ray's hit cell (MISS, END and CAPPED: the miss shade, untouched), then the blend.  AA: the lane's sample goes
// to the wave's box filter (every lane of the wave calls it, so no lane returns before) and not to memory.  Kernels of their own:
// k_render_water_literal keeps its instructions.
template <int PROJ, bool AA, bool BAKED>
__global__ __launch_bounds__(kBlockThreads) void k_render_water_literal_more(const DevFrame f, const RowMap rows,
                                                                             const double *__restrict__ thr,
                                                                             const uint32_t *__restrict__ cmap,
                                                                             uint32_t *__restrict__ out, int64_t out_stride_px,
                                                                             int tiles_y, StatsOut st, const SegRules seg,
                                                                             const WaterRules water, const BakedLight baked) {
	const PixelId pid = pixel_of_lane(f, rows, tiles_y);
	LitState<true> lt;
	unsigned cell = 0u, mcell = ~0u; // (mcell: the mirror ray's hit cell, if it hit)
	render_lane_literal<PROJ, false, false, true, 1>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{}, seg, SunRules{}, &lt, &cell);
	const bool wet = pid.live && lt.primary_hit && lt.t <= water.level; // (a NaN level: no water)
	LitState<true> mr = lt;
	mr.primary_hit = wet; // (the other lanes sit the pass out)
	SunRules mirror{{0.0, 0.0, 0.0}, water.step_dist, water.max_steps, 0u};
	if (wet) {
		const DevRay primary = make_ray<PROJ>(f, pid.px, pid.py);
		mirror.dir[0] = primary.dx; mirror.dir[1] = primary.dy; mirror.dir[2] = -primary.dz;
	}
	render_lane_literal<PROJ, false, false, true, 5>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{},
	                                                 SegRules{nullptr, water.max_steps, 1u}, mirror, &mr, &mcell);
	uint32_t rgba = 0u;
	if (pid.live) {
		rgba = lt.rgba;
		if constexpr (BAKED) {
			if (lt.primary_hit) {
				rgba = shade_baked(wet ? water_base(rgba, water) : rgba, baked.plane[cell], baked.full_scale) | 0xff000000u;
				if (wet) {
					uint32_t m = mr.rgba;
					if (mcell != ~0u) m = shade_baked(m, baked.plane[mcell], baked.full_scale);
					rgba = blend_water_base(rgba, m, water);
				}
			}
		} else if (wet) rgba = blend_water(rgba, mr.rgba, water);
	}
	if constexpr (AA) store_box_filtered(out, out_stride_px, f.aa_shift, (int)(threadIdx.x & 63), pid.px, pid.lrow, pid.live, rgba);
	else if (pid.live) out[(int64_t)pid.lrow * out_stride_px + pid.px] = rgba;
}

// Such a frame: the water family's arguments and, where the family has it, the plane.  Never a measured launch.
static hipError_t launch_water_literal_more(const FrameLaunch &l) {
	const bool aa = l.family != kFrameWaterBaked, baked = l.family != kFrameWaterAA;
	if (l.rows.measure != nullptr || (l.f.aa_shift != 0) != aa || !l.d_out) return hipErrorInvalidValue;
	if (baked && (!l.baked.plane || l.baked.full_scale < 1u || l.baked.full_scale > 65535u)) return hipErrorInvalidValue;
	const SegRules seg = frame_seg_rules(l);
	return launch_literal(l, StatsOut{l.d_counters, nullptr, nullptr}, [&](auto proj, dim3 grid, const auto &...args) {
		const dim3 block(kBlockThreads);
		if (l.family == kFrameWaterAA) hipLaunchKernelGGL((k_render_water_literal_more<proj(), true, false>), grid, block, 0, l.stream, args..., seg, l.water, l.baked);
		else if (l.family == kFrameWaterBaked) hipLaunchKernelGGL((k_render_water_literal_more<proj(), false, true>), grid, block, 0, l.stream, args..., seg, l.water, l.baked);
		else hipLaunchKernelGGL((k_render_water_literal_more<proj(), true, true>), grid, block, 0, l.stream, args..., seg, l.water, l.baked);
	});
}

// A pixel of a sun-lit water frame (hmrm_render_water_lit with HMRM_KERNEL=simple, or on a map with a side of 2^24 cells): the literal
// loop up to four times -- the primary ray, its hit's shadow ray, a wet lane's mirror ray, that ray's hit's shadow ray -- then
// hmrm_render_shaded's weight on either side of the mirror and hmrm_render_water's blend.  Each pass counts its own capped rays.
// Whether shadow rays are cast and whether the weights are diffuse are the launch's flags (frame.hpp kWaterSun*): scalar branches.
template <int PROJ>
__global__ __launch_bounds__(kBlockThreads) void k_render_water_lit_literal(const DevFrame f, const RowMap rows,
                                                                            const double *__restrict__ thr,
                                                                            const uint32_t *__restrict__ cmap,
                                                                            uint32_t *__restrict__ out, int64_t out_stride_px,
                                                                            int tiles_y, StatsOut st, const SegRules seg,
                                                                            const WaterRules water, const SunRules sun) {
	const PixelId pid = pixel_of_lane(f, rows, tiles_y);
	const bool shadows = (water.flags & kWaterSunNoShadows) == 0u, diffuse = (water.flags & kWaterSunDiffuse) != 0u;
	const SegRules sun_seg{nullptr, sun.max_steps, 1u};
	LitState<true> lt;
	unsigned cell = 0u, mcell = ~0u; // (mcell: the mirror ray's hit cell, if it hit)
	render_lane_literal<PROJ, false, false, true, 1>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{}, seg, sun, &lt, &cell);
	const bool wet = pid.live && lt.primary_hit && lt.t <= water.level; // (a NaN level: no water)
	LitState<true> ps = lt; // (the primary hit's shadow ray: SHADOWED comes back in ps.phase)
	if (shadows) render_lane_literal<PROJ, false, false, true, 3>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{}, sun_seg, sun, &ps);
	LitState<true> mr = lt;
	mr.primary_hit = wet; // (the other lanes sit the pass out)
	SunRules mirror{{0.0, 0.0, 0.0}, water.step_dist, water.max_steps, 0u};
	if (wet) {
		const DevRay primary = make_ray<PROJ>(f, pid.px, pid.py);
		mirror.dir[0] = primary.dx; mirror.dir[1] = primary.dy; mirror.dir[2] = -primary.dz;
	}
	render_lane_literal<PROJ, false, false, true, 6>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{},
	                                                 SegRules{nullptr, water.max_steps, 1u}, mirror, &mr, &mcell);
	LitState<true> ms = mr; // (the mirror hit's shadow ray, from the point and threshold pass 6 left)
	ms.primary_hit = wet && mcell != ~0u;
	ms.phase = 0;
	if (shadows) render_lane_literal<PROJ, false, false, true, 3>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{}, sun_seg, sun, &ms);
	if (!pid.live) return;
	auto weight_of = [&](bool shadowed, unsigned c) -> uint32_t {
		if (shadowed) return sun.ambient;
		return diffuse ? shade_weight(sun.ambient, diffuse_level_nearest<false>(f, thr, c, sun.dir)) : 255u;
	};
	uint32_t rgba = lt.rgba;
	if (lt.primary_hit) {
		rgba = shade_weighted(wet ? water_base(rgba, water) : rgba, weight_of(ps.phase != 0, cell)) | 0xff000000u;
		if (wet) {
			uint32_t m = mr.rgba; // (MISS, END and CAPPED: the miss shade, untouched)
			if (mcell != ~0u) m = shade_weighted(m, weight_of(ms.phase != 0, mcell));
			rgba = blend_water_base(rgba, m, water);
		}
	}
	out[(int64_t)pid.lrow * out_stride_px + pid.px] = rgba;
}

// Such a frame: the water family's arguments and the sun.  No antialiased variant, never a measured launch.
static hipError_t launch_water_lit_literal(const FrameLaunch &l) {
	if (l.rows.measure != nullptr || l.f.aa_shift != 0 || !l.d_out) return hipErrorInvalidValue;
	const SegRules seg = frame_seg_rules(l);
	return launch_literal(l, StatsOut{l.d_counters, nullptr, nullptr}, [&](auto proj, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL(k_render_water_lit_literal<proj()>, grid, dim3(kBlockThreads), 0, l.stream, args..., seg, l.water, l.sun);
	});
}

// A pixel of a haze frame (hmrm_render_haze with HMRM_KERNEL=simple, or on a map with a side of 2^24 cells; frame.hpp HazeRules): the
// primary ray of a lit pixel -- its colour, whether it hit and where -- then the range of a geometry frame, in doubles, the table's
// byte at its index and the blend; with kHazeSky a pixel that did not hit blends at the table's last entry.  AA: the lane's sample
// goes to the wave's box filter (every lane of the wave calls it, so no lane returns before) and not to memory.  Nearest sampling
// only, like every literal kernel.
template <int PROJ, bool AA>
__global__ __launch_bounds__(kBlockThreads) void k_render_haze_literal(const DevFrame f, const RowMap rows,
                                                                       const double *__restrict__ thr,
                                                                       const uint32_t *__restrict__ cmap,
                                                                       uint32_t *__restrict__ out, int64_t out_stride_px,
                                                                       int tiles_y, StatsOut st, const SegRules seg,
                                                                       const HazeRules haze) {
	const PixelId pid = pixel_of_lane(f, rows, tiles_y);
	LitState<true> lt;
	unsigned cell = 0u;
	double hz = 0.0;
	render_lane_literal<PROJ, false, false, true, 1>(f, pid, thr, cmap, out, out_stride_px, st, RayBatch{}, seg, SunRules{}, &lt, &cell, &hz);
	uint32_t rgba = 0u;
	if (pid.live) {
		rgba = lt.rgba;
		if (lt.primary_hit) {
			const DevRay o = make_ray<PROJ>(f, pid.px, pid.py);
			HMRM_RANGE_FROM(o, lt.hx, lt.hy, hz);
			rgba = blend_haze(rgba, haze, haze_index(haze, r));
		} else if ((haze.flags & kHazeSky) != 0u) rgba = blend_haze(rgba, haze, haze.n - 1u);
	}
	if constexpr (AA) store_box_filtered(out, out_stride_px, f.aa_shift, (int)(threadIdx.x & 63), pid.px, pid.lrow, pid.live, rgba);
	else if (pid.live) out[(int64_t)pid.lrow * out_stride_px + pid.px] = rgba;
}

// Such a frame: the interior family's arguments and the haze's rules, antialiased or not.  Never a measured launch.
static hipError_t launch_haze_literal(const FrameLaunch &l) {
	if (l.rows.measure != nullptr || !l.d_out) return hipErrorInvalidValue;
	if (!l.haze.table || l.haze.n < 1u || l.haze.n > (uint32_t)kMaxHazeEntries) return hipErrorInvalidValue;
	const SegRules seg = frame_seg_rules(l);
	const bool aa = l.f.aa_shift != 0;
	return launch_literal(l, StatsOut{l.d_counters, nullptr, nullptr}, [&](auto proj, dim3 grid, const auto &...args) {
		if (aa) hipLaunchKernelGGL((k_render_haze_literal<proj(), true>), grid, dim3(kBlockThreads), 0, l.stream, args..., seg, l.haze);
		else hipLaunchKernelGGL((k_render_haze_literal<proj(), false>), grid, dim3(kBlockThreads), 0, l.stream, args..., seg, l.haze);
	});
}

// A pixel of a view batch (hmrm_render_views with HMRM_KERNEL=simple, or on a map with a side of 2^24 cells): k_render_interior_literal's
// pixel of the view this workgroup belongs to -- the frame record read from the batch's device array at a wave-uniform index, as
// render_views.hip does -- stored into that view's part of the target.  Nearest sampling only, like every literal kernel.
template <int PROJ>
__global__ __launch_bounds__(kBlockThreads) void k_render_views_literal(const DevFrame *__restrict__ frames, int n_views, int tiles_y_view,
                                                                        const double *__restrict__ thr,
                                                                        const uint32_t *__restrict__ cmap,
                                                                        uint32_t *__restrict__ out, int64_t out_stride_px,
                                                                        int64_t view_stride_px, StatsOut st, const SegRules seg) {
	const unsigned gy = blockIdx.z * 32768u + blockIdx.y;
	const unsigned view = (unsigned)__builtin_amdgcn_readfirstlane((int)(gy / (unsigned)tiles_y_view));
	if (view >= (unsigned)n_views) return;
	DevFrame f; // (a copy made of 32-bit words, not a reference: device_common.hpp copy_frame_words)
	copy_frame_words(&f, frames + view);
	const PixelId pid = pixel_of_tile_lane(f, whole_frame_rows(f), tiles_y_view, (int)blockIdx.x, gy - view * (unsigned)tiles_y_view,
	                                       (int)(threadIdx.x >> 6), (int)(threadIdx.x & 63));
	render_lane_literal<PROJ, false, false, true>(f, pid, thr, cmap, out + (int64_t)view * view_stride_px, out_stride_px, st, RayBatch{}, seg);
}

// Such a batch: render_views.hip's grid and arguments.  Never a measured launch.
static hipError_t launch_views_literal(const FrameLaunch &l) {
	if (l.f.aa_shift != 0 || l.rows.measure != nullptr || !l.d_frames || l.n_views < 1 || !l.d_out) return hipErrorInvalidValue;
	const LaunchGrid g = views_grid(l.f, l.n_views);
	if (g.tiles_y == 0) return g.err;
	const SegRules seg = frame_seg_rules(l);
	dispatch_projection(l.f.projection, [&](auto proj) {
		hipLaunchKernelGGL(k_render_views_literal<proj()>, g.grid, dim3(kBlockThreads), 0, l.stream, l.d_frames, l.n_views, g.tiles_y, l.d_thr,
		                   l.d_cmap, l.d_out, l.out_stride_px, l.view_stride_px, StatsOut{l.d_counters, nullptr, nullptr}, seg);
	});
	return hipGetLastError();
}

} // namespace hmrm
