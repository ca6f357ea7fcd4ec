// march.hpp -- the production march for gfx950: render_wave_tile, one wave's 8 x 8 pixels (or 64 batch rays), and its
// tuning constants.  Instantiated by render_fast.hip and render_fast_aa.hip (frames: march_frame.hpp), render_rays.hip,
// render_segments.hip, render_interior.hip, render_lit.hip, render_shaded.hip, render_lit_shaded.hip, their antialiased
// counterparts (march_lit_aa.hpp), render_cells.hip, render_cell_sums.hip, render_geometry.hip, render_lit_sum.hip, render_baked.hip,
// render_baked_aa.hip, render_water.hip, render_water_aa.hip, render_water_baked.hip, render_water_baked_aa.hip, render_water_lit.hip, render_haze.hip and render_haze_aa.hip, each with a __global__ kernel of its own and a family of its own: march_family.hpp, which holds every
// switch and derived constant with its reasons.
//
// Same pixels, same per-ray step counts as k_render (render.hip) and therefore as
// the reference loop main/hmap.cpp:978-1058; two bit-preserving restructurings:
//
// (1) SPECULATIVE GROUPS.  The positions a ray visits do not depend on the heights
//     it loads -- only the decision to stop does.  So U consecutive positions are
//     produced with the reference's sequential adds (hmap.cpp:1037), their U height
//     loads are issued together, and the tests (range :1006, hit :1016) are then
//     resolved in order.  One memory latency per U steps instead of per step.
//
// (2) EXACT LEAPS.  While a coordinate p stays inside one binade [2^E, 2^(E+1)) every
//     value is a multiple of u = 2^(E-52), and fl(p + s) = p + delta with the SAME
//     delta = round_u(s) for every p of that binade (round-to-nearest; on an exact
//     tie the increment is constant too once p has the steady parity: axis_refresh).  Hence the
//     reference's sequential accumulation satisfies p_k = p_0 + k*delta EXACTLY, and
//     both the product k*delta and the sum are exact in fp64.  A pyramid of window
//     maxima over the hit thresholds then lets a ray jump over n steps at once when
//     all n skipped positions provably (a) stay inside the window whose maximum was
//     looked up and (b) stay at or above that maximum (no hit possible: hmap.cpp:1016
//     needs z < threshold), with (c) all three coordinates inside their binades.
//     (a) and (b): the jump length is only ESTIMATED (approximate reciprocals); the landing
//     point is then VERIFIED with exact tests (cell inside the window, z >= max), and
//     monotonicity of each coordinate in k extends the verification from the landing point to
//     every skipped position.  A failed verification just means "no jump".
//     (c): how many further steps stay strictly inside a coordinate's binade is established ONCE
//     per binade (axis_refresh: estimate, shortened, verified at its far end) and counted down
//     with every step leaped or marched (Axis::left): the multiplied part of a jump never exceeds the
//     three counts.  A jump of n steps is n - 1 multiplied steps and then ONE real step fl(p + s) from that
//     exact position (HMRM_CROSS): where a binade's end cut the jump short, that step is the one
//     that carries the coordinate into its next binade -- otherwise a whole group of real steps would
//     have to be marched at every binade boundary (half of all groups before this was done).  The
//     end point after the real step is what (a) and (b) are verified for.
//     Skipped positions are counted as steps: each was inside the grid, so the reference
//     executed its height load there.
//
// Pyramid layout (built by k_build_mip*): level l holds maxima of S x S-cell windows,
// S = 4, 8, 16, .. 256, placed every S/2 cells on the 4-cell level and every S/4 cells above it
// (overlapping), so that a ray can always pick a window in which it has at least S/2 (3S/4) cells of
// room ahead.  Values are floats rounded UP (a larger bound is always safe).  Above them: the whole
// map, the one window of a top plane.  A ray moves two levels at a time until it has made kAdaptAfter
// jumps, then one at a time (performance only: any level sequence gives the same pixels).
#pragma once
#include "device_common.hpp"
#include "leap_common.hpp"
#include "leap_diag.hpp"
#include "launch_common.hpp"
#include "march_dispatch.hpp"
#include "march_family.hpp"
#include "render.hpp"

#pragma clang fp contract(off)

namespace hmrm {

namespace {

// (the group lengths kGroup, kGroupPlain and kGroupRec, and the geometry frames' A/B switches: march_family.hpp, beside U)
// the most refusals in a row the record kernel's back-off counts (attempts every 2^n-th trip at most)
#ifndef HMRM_REC_BACKOFF
#define HMRM_REC_BACKOFF 6
#endif
constexpr int kRecBackoff = HMRM_REC_BACKOFF;
#ifndef HMRM_MIN_LEAP
#define HMRM_MIN_LEAP 2
#endif
constexpr int kMinLeap = HMRM_MIN_LEAP; // a jump shorter than this is not worth its bookkeeping
#ifndef HMRM_UP_RATIO
#define HMRM_UP_RATIO (kLevelStep == 2 ? 4.0 : 2.0)
#endif
constexpr double kUpRatio = HMRM_UP_RATIO; // see the level policy in k_render_fast
// (per-ray adaptive level spacing, kAdaptAfter: frame.hpp, beside the policy's level moves)

// HMRM_EARLY_LOAD (default 1): order of an attempt -- the pyramid look-up is issued first, refreshes and lateral estimates
// run while it is in flight (see the attempt block).  0 = refresh first and estimates after the load, for A/B runs.
#ifndef HMRM_EARLY_LOAD
#define HMRM_EARLY_LOAD 1
#endif
constexpr bool kEarlyLoad = HMRM_EARLY_LOAD != 0;

// ---- bilinear quality mode (HMRM_BILINEAR; a build-side addition, not in the reference) ----
// Same definition, operation for operation, as oracle/hmrm_oracle.c "bilinear quality mode":
// values sit at cell centres; u = q - 0.5, t = u - floor(u), neighbours clamp(floor(u)) and
// clamp(floor(u) + 1); f = a + ty*(b - a), a = f00 + tx*(f10 - f00), b = f01 + tx*(f11 - f01).
struct Bil {
	int c00, c10, c01, c11; // the four neighbour cells (linear indices)
	double tx, ty;
};
__device__ __forceinline__ Bil bil_setup(double qx, double qy, int w, int h) {
	const double u = qx - 0.5, v = qy - 0.5;
	const double fu = __builtin_floor(u), fv = __builtin_floor(v);
	Bil b;
	b.tx = u - fu;
	b.ty = v - fv;
	const int iu = cvt_i32_sat(fu), iv = cvt_i32_sat(fv);
	const int i0 = min(max(iu, 0), w - 1), i1 = min(max(iu + 1, 0), w - 1);
	const int j0 = min(max(iv, 0), h - 1), j1 = min(max(iv + 1, 0), h - 1);
	b.c00 = j0 * w + i0; b.c10 = j0 * w + i1;
	b.c01 = j1 * w + i0; b.c11 = j1 * w + i1;
	return b;
}
__device__ __forceinline__ double bil_mix(const Bil &b, double f00, double f10, double f01, double f11) {
	const double a = f00 + b.tx * (f10 - f00);
	const double c = f01 + b.tx * (f11 - f01);
	return a + b.ty * (c - a);
}
// The gradient of the interpolated surface at a hit point whose neighbours and weights are `b`: that of bil_mix's surface there,
// a = f10 - f00, b = f11 - f01 mixed along y, c = f01 - f00, d = f11 - f10 along x -- and its diffuse level (device_common.hpp
// diffuse_level).  The slope plane of a geometry frame stores the former.
// (A macro that declares gx and gy in its user's scope, for the reason device_common.hpp gives at HMRM_GRADIENT_NEAREST.)
#define HMRM_GRADIENT_BILINEAR(f, thr, b)                                                   \
	const double t00 = thr[b.c00], t10 = thr[b.c10], t01 = thr[b.c01], t11 = thr[b.c11];    \
	const double ax = t10 - t00, bx = t11 - t01;                                            \
	const double gx = (ax + b.ty * (bx - ax)) / f.grid_width;                               \
	const double cy = t01 - t00, dy = t11 - t10;                                            \
	const double gy = (cy + b.tx * (dy - cy)) / f.grid_width
__device__ __forceinline__ Gradient gradient_bilinear(const DevFrame &f, const double *__restrict__ thr, const Bil &b) {
	HMRM_GRADIENT_BILINEAR(f, thr, b);
	return Gradient{gx, gy};
}
__device__ __forceinline__ uint32_t diffuse_level_bilinear(const DevFrame &f, const double *__restrict__ thr, const Bil &b,
                                                           const double (&s)[3]) {
	HMRM_GRADIENT_BILINEAR(f, thr, b);
	return diffuse_level(gx, gy, s);
}
// Colour at a hit: R,G,B interpolated and rounded with floor(f + 0.5); the alpha-0 rule
// (hmap.cpp:1020) keeps looking at the nearest cell.
__device__ __forceinline__ uint32_t shade_hit_bilinear(const DevFrame &f, const uint32_t *__restrict__ cmap,
                                                       int nearest_cell, const Bil &b) {
	const uint32_t tn = cmap[nearest_cell];
	if ((tn >> 24) == 0) return pack_rgba(f.bg[0], f.bg[1], f.bg[2]);
	const uint32_t t00 = cmap[b.c00], t10 = cmap[b.c10], t01 = cmap[b.c01], t11 = cmap[b.c11];
	uint32_t ch[3];
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const int sh = 8 * k;
		double v = bil_mix(b, (double)((t00 >> sh) & 255u), (double)((t10 >> sh) & 255u),
		                   (double)((t01 >> sh) & 255u), (double)((t11 >> sh) & 255u)) + 0.5;
		if (v < 0.0) v = 0.0;
		else if (v > 255.0) v = 255.0;
		ch[k] = (uint32_t)(int)__builtin_floor(v);
	}
	return pack_rgba(ch[0], ch[1], ch[2]);
}
// Baked light at a hit (hmrm_render_baked): the four neighbours' words of the plane mixed like a colour channel and rounded
// with floor(m + 0.5), clamped to the word's range.
__device__ __forceinline__ uint32_t baked_light_bilinear(const uint16_t *__restrict__ plane, const Bil &b) {
	double v = bil_mix(b, (double)plane[b.c00], (double)plane[b.c10], (double)plane[b.c01], (double)plane[b.c11]) + 0.5;
	if (v < 0.0) v = 0.0;
	else if (v > 65535.0) v = 65535.0;
	return (uint32_t)(int)__builtin_floor(v);
}

// Cell maps: the ray of cell (x0 + px, y0 + py) of the rect, made from the cell's entry of the table the sampling mode's
// march reads (`thr`: the float copy for SAMP 2, else the doubles -- the bilinear mode's origin sits on the cell's own value).
template <int SAMP>
__device__ __forceinline__ DevRay cell_ray_of(const CellRules &c, const DevFrame &f, const double *__restrict__ thr, int px, int py) {
	const int cx = c.x0 + px, cy = c.y0 + py;
	const size_t i = (size_t)cy * (size_t)f.map_w + (size_t)cx;
	const double t = SAMP == 2 ? (double)reinterpret_cast<const float *>(thr)[i] : thr[i];
	return cell_ray(c, f, cx, cy, t);
}

} // namespace

#ifndef HMRM_MIN_WAVES
#define HMRM_MIN_WAVES 1
#endif
#ifdef HMRM_WAVES_PER_EU
#define HMRM_OCCUPANCY_ATTR __attribute__((amdgpu_waves_per_eu(HMRM_WAVES_PER_EU, HMRM_WAVES_PER_EU), amdgpu_num_vgpr(512 / HMRM_WAVES_PER_EU / 8 * 8)))
#else
#define HMRM_OCCUPANCY_ATTR
#endif
// One wave's 8 x 8 pixels (cells; or 64 batch rays): wave `wave` of the workgroup-sized tile (tile_x, grid row gy), for the family
// F = Family<TAG, PROJ, GWM, LEAP, SAMP> (march_family.hpp: what each switch and derived constant means) with the tag's arguments
// `a`.  Returns the tile row rendered (-1: the grid row does not exist).  k_render_fast calls it with the tile = blockIdx (one tile
// per workgroup); round 4's persistent-tile experiment (resident waves pulling tiles from queue heads) called it in a loop and was
// 1.4-1.9 x slower: profiles/r04_experiments.txt section 1, code at commit 80527e9.
// Every feature is written as `if constexpr` statements beside the others' own, so that the families without it keep their
// instructions.
template <class F, class... ARGS>
__device__ __forceinline__ int render_wave_tile(const DevFrame &f, const RowMap &rows, const double *__restrict__ thr,
                                                const uint32_t *__restrict__ cmap, uint32_t *__restrict__ out,
                                                int64_t out_stride_px, int tiles_y, const StatsOut &st, int tile_x, unsigned gy,
                                                int wave, int lane, const ARGS &...args) {
	const typename F::Args a{args...}; // (the tag's arguments under their names: references, nothing is copied)
	constexpr int PROJ = F::PROJ, GWM = F::GWM, LEAP = F::LEAP, SAMP = F::SAMP, U = F::U;
	constexpr bool STATS = F::STATS, AA = F::AA, SEG = F::SEG, LIT = F::LIT, SHADE = F::SHADE, SUM = F::SUM, GEOM = F::GEOM, LSUM = F::LSUM;
	constexpr bool BAKED = F::BAKED, CELLS = F::CELLS, RAYS = F::RAYS, COUNT = F::COUNT, BILINEAR = F::BILINEAR, F32 = F::F32, REC = F::REC;
	constexpr bool KEEP_Q = F::KEEP_Q, KEEP_P = F::KEEP_P, CHAIN = F::CHAIN, DEFER = F::DEFER, CARRY = F::CARRY;
	constexpr bool MIRROR = F::MIRROR, SUNLIT = F::SUNLIT;
	[[maybe_unused]] constexpr bool HAZE = F::HAZE, POINT = F::POINT;
	const float *__restrict__ thr32 = reinterpret_cast<const float *>(thr);
	const float *__restrict__ mip = BILINEAR ? f.mipbuf_bil : f.mipbuf; // the pyramid this sampling mode leaps on
	PixelId pid = pixel_of_tile_lane(f, rows, tiles_y, tile_x, gy, wave, lane);
	// (what a batch adds is written as `if constexpr (RAYS)` statements beside the frame kernels' own, which stay as they
	// were: they must keep compiling to the same instructions)
	int64_t ray_index = 0;
	if constexpr (RAYS) {
		ray_index = (int64_t)pid.py * kBatchW + pid.px;
		pid.live = pid.live && ray_index < a.batch.n;
	}
	LoopDiag<STATS> diag; // (empty unless STATS: leap_diag.hpp)
	diag.start();
	unsigned long long my_steps = 0;
	uint32_t my_hit = 0, my_cap = 0;
	uint32_t aa_rgba = 0; // (AA: this lane's sample, filtered by the whole wave below)
	SumState<SUM> sm; // (empty unless SUM: device_common.hpp)
	LitSumState<LSUM> lm; // (empty unless LSUM)

	if (pid.live) {
		DevRay ray = make_ray<PROJ>(f, pid.px, pid.py);
		if constexpr (RAYS) ray = batch_ray(a.batch, ray_index); // (make_ray<4>'s value is dead)
		if constexpr (CELLS) ray = cell_ray_of<SAMP>(a.cells, f, thr, pid.px, pid.py); // (make_ray<5>'s too)
		if constexpr (SUM) { // (... towards the list's first target, not CellRules' own)
			sm.rules = a.cells;
			sum_target(a.sums, 0, &sm.rules);
			ray = cell_ray_of<SAMP>(sm.rules, f, thr, pid.px, pid.py);
		}
		// most rays of a frame never touch the box: prove the miss cheaply where possible (the instrumented
		// variant reports d, so it takes no shortcut for misses); most of the others get their entry distance
		// from one division instead of six (slab_classify: the instrumented variant uses that path too, so the
		// parity tests compare its d with the oracle's bit for bit)
		double d = __builtin_huge_val();
		if constexpr (CELLS) { // (most origins are strictly inside: no slab test unless one is not; no ray at all without shadows)
			if ((a.cells.flags & kMapNoShadows) == 0u) d = shadow_entry(ray, f);
		} else
		if (COUNT || !slab_points_away<PROJ>(ray, f)) {
			const int verdict = slab_classify(ray, f, !COUNT, &d);
			if (verdict == 0) d = slab_distance(ray, f);
		}
		if (STATS && st.entry_d) st.entry_d[(int64_t)pid.py * f.screen_w + pid.px] = d;
		SegState<SEG> sg; // (empty unless SEG: device_common.hpp)
		if constexpr (SEG) {
			sg.d_record = d; // (a record keeps distance()'s own value, not the d that was used)
			if constexpr (!CELLS) // (shadow_entry has applied the rule)
			if (a.seg.interior != 0u && origin_strictly_inside(ray, f)) d = 0.0; // as if distance() had returned +0.0
			sg.budget = segment_budget(a.seg, RAYS ? ray_index : 0, f.step_cap, &sg.ends);
		}

		uint32_t rgba = 0;
		bool real_hit = false;
		double hx = 0.0, hy = 0.0, hz = 0.0; // (RAYS: where hmap.cpp:1016 fired; GEOM, HAZE: hz, beside hqx and hqy)
		// The cell hmap.cpp:1016 fired in (LIT: for the primary ray).  The one thing a hit lane of the nearest-cell modes carries out
		// of the march loop: its colour (below the loop: one load for all hit lanes of the wave, where the loop had one, and a wait
		// for it, in every trip in which any lane hit), SHADE's diffuse level and the ray batches' record are all made from it.
		unsigned hcell = 0u;
		LitState<LIT || MIRROR> lt; // (empty unless LIT or MIRROR: device_common.hpp)
		// (MIRROR: what LitState::rgba holds between the passes -- the primary hit's cell, below 2^29, or its pixel without the alpha
		// byte -- and the two flags beside it)
		[[maybe_unused]] constexpr bool kMirrorKeepsCell = MIRROR && DEFER && !BILINEAR;
		[[maybe_unused]] constexpr uint32_t kMirrorHit = 0x40000000u, kMirrorWet = 0x80000000u, kMirrorValue = kMirrorKeepsCell ? 0x3fffffffu : 0x00ffffffu;
		// (SUNLIT: the keeps-cell form gives up one bit of the value -- a cell is below 2^29 -- for "the primary hit is shadowed"; the
		// keeps-pixel form has "the mirror ray hit" in a free bit above the pixel, the keeps-cell form says that with hcell: all ones = no)
		[[maybe_unused]] constexpr uint32_t kSunShadowed = 0x20000000u, kSunMirrorHit = 0x10000000u, kSunValue = kMirrorKeepsCell ? 0x1fffffffu : 0x00ffffffu;
		double hqx = 0.0, hqy = 0.0; // (bilinear, no LIT: the hit's exact cell coordinates, KEEP_Q, or SHADE's copy of its x and y, KEEP_P)
		bool again = false; // (LIT: the wave has shadow rays to march; SUM: targets)
		// Bilinear mode, behind the march: the exact cell coordinates of a hit point -- the very expressions the group made its
		// QX, QY with (the true division for general grid widths; the literal path's division by a power of two is the same
		// product), so the weights keep their bits -- and the pixel there, with the alpha-0 rule looked up in the hit cell.
		auto cell_coords_of = [&](double px, double py, double &qx, double &qy) {
			qx = GWM == 0 ? px : (GWM == 2 ? px / f.grid_width : px * f.inv_grid_width);
			qy = GWM == 0 ? -py : (GWM == 2 ? -py / f.grid_width : -py * f.inv_grid_width);
		};
		auto bilinear_pixel = [&](double qx, double qy) {
			return shade_hit_bilinear(f, cmap, (int)hcell, bil_setup(qx, qy, f.map_w, f.map_h));
		};

		// LSUM: the weight of a lane that hit under direction `s` -- hmrm_render_shaded's: the ambient level for a shadowed pixel, else
		// 255 or, HMRM_SHADE_DIFFUSE, that of the level of the primary hit.  (The hit cell, or the hit point, goes through an empty
		// statement: the gradient made from it does not depend on the direction, and the compiler would otherwise make it once,
		// before the first pass, and hold it in vector registers across every march -- the lesson of SUM's cell.)
		[[maybe_unused]] auto sum_weight = [&](const SunRules &sun, const LightSum &lsum, bool shadowed, const double (&s)[3]) -> uint32_t {
			uint32_t w = shadowed ? sun.ambient : 255u;
			if constexpr (LSUM) {
				if ((lsum.flags & kShadeDiffuse) != 0u && !shadowed) {
					uint32_t q;
					if constexpr (BILINEAR) {
						double px = lt.hx, py = lt.hy, qxs, qys;
						asm volatile("" : "+v"(px), "+v"(py));
						cell_coords_of(px, py, qxs, qys);
						q = diffuse_level_bilinear(f, thr, bil_setup(qxs, qys, f.map_w, f.map_h), s);
					} else {
						unsigned hc = hcell;
						asm volatile("" : "+v"(hc));
						q = diffuse_level_nearest<F32>(f, thr, hc, s);
					}
					w = shade_weight(sun.ambient, q);
				}
			}
			return w;
		};

		// SUNLIT: the weight of a hit under the sun -- hmrm_render_shaded's: the ambient level for a shadowed hit, else 255 or,
		// kWaterSunDiffuse, that of the level at the hit's cell (nearest-cell modes) or point (bilinear).
		[[maybe_unused]] auto sun_weight = [&](const SunRules &sun, const WaterRules &water, bool shadowed, unsigned cell_at, double px, double py) -> uint32_t {
			uint32_t w = shadowed ? sun.ambient : 255u;
			if constexpr (SUNLIT) {
				if ((water.flags & kWaterSunDiffuse) != 0u && !shadowed) {
					uint32_t q;
					if constexpr (BILINEAR) {
						double qxs, qys;
						cell_coords_of(px, py, qxs, qys);
						q = diffuse_level_bilinear(f, thr, bil_setup(qxs, qys, f.map_w, f.map_h), sun.dir);
					} else q = diffuse_level_nearest<F32>(f, thr, cell_at, sun.dir);
					w = shade_weight(sun.ambient, q);
				}
			}
			return w;
		};
		// SUNLIT: the lane's camera ray, made again from its number in the wave (which goes through an empty statement, so that
		// nothing of it is made before the marches and held across them).
		[[maybe_unused]] auto camera_ray_again = [&]() -> DevRay {
			int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
			asm volatile("" : "+v"(ln));
			const PixelId me = pixel_of_tile_lane(f, rows, tiles_y, tile_x, gy, wave, ln);
			return make_ray<PROJ>(f, me.px, me.py);
		};

		do { // (once; LIT: once more with the shadow rays; SUM: once per target; LSUM: once more per direction)
			if (!(d == __builtin_huge_val()) && !(d < 0.0)) { // intersection(), AABB.cpp:33-44
				double x = ray.px + d * ray.dx;
				double y = ray.py + d * ray.dy;
				double z = ray.pz + d * ray.dz;
				x = x + f.nudge * ray.dx; // hmap.cpp:998
				y = y + f.nudge * ray.dy;
				z = z + f.nudge * ray.dz;
				double step_dist = f.step_dist;
				if constexpr (LIT) step_dist = lt.phase ? a.sun.step_dist : step_dist; // (a shadow ray's own)
				if constexpr (SUNLIT) step_dist = lt.phase == 0 ? step_dist : ((lt.phase & 1) ? a.sun.step_dist : a.water.step_dist); // (passes 1, 3: a shadow ray's; 2: a mirror ray's)
				else
				if constexpr (MIRROR) step_dist = lt.phase ? a.water.step_dist : step_dist; // (a mirror ray's own)
				const double sx = step_dist * ray.dx; // hmap.cpp:1037, loop invariant
				const double sy = step_dist * ray.dy;
				const double sz = step_dist * ray.dz;
				const unsigned wlim = (unsigned)f.map_w, hlim = (unsigned)f.map_h;
				const int budget0 = f.step_cap > 0x7fffffff ? 0x7fffffff : (int)f.step_cap;
				int budget = budget0; // every step taken or leaped comes off it: steps so far = budget0 - budget
				if constexpr (SEG) budget = sg.budget; // (min(step cap, the ray's own limit): steps so far = sg.budget - budget)
				// (int)NaN is INT_MIN on the reference's CPU: the first range test fails, the ray misses
				const bool entry_nan = x != x || y != y;

				// leap state
				// First level to look at: a finer window has a lower maximum, so the finest level whose
				// windows still leave the ray lateral room for its whole descent to the box floor is the
				// best one (steep rays: the finest level at once, instead of walking down from the top);
				// oblique rays start with the whole-map bound.  Performance only.
				int lev = kTopLevel;
				if (sz < 0.0) {
					const double descent = (z - f.c0[2]) * __builtin_amdgcn_rcp(-sz); // steps down to min_height
					const double lateral = descent * __builtin_fmax(__builtin_fabs(sx), __builtin_fabs(sy)) * (GWM == 0 ? 1.0 : f.inv_grid_width);
#pragma unroll
					for (int l = kMipLevels - 1; l >= 0; l -= (kAdaptive ? 2 : 1)) // windows every 1 << hs cells: at least that much room ahead
						lev = (l >= f.min_level && lateral <= (double)((win_strides(l) - 1) << mip_stride_shift(l))) ? l : lev;
				}
				if (REC) lev = lev == kTopLevel ? kTopLevel : kRecLevel; // (the record kernel knows the whole-map bound and the record level)
				// Level state (leap_common.hpp level_state): what an attempt reads of its level besides the number, one word per ray,
				// made again where lev is assigned -- the first level above, the policy's and the record kernel's choice below.
				// (CARRY false: the families a register more would cost a wave per SIMD read the same word off lev at the attempt.)
				uint32_t ls = level_state<CARRY>(lev);
				int cooldown = 0, fails = 0;
				unsigned trip_no = 0; // (REC)
				int young_left = kAdaptAfter; // kAdaptAfter - successful jumps so far (kAdaptive): negative once the ray moves one level at a time
				Axis ax, ay, az;
				ax.delta = ay.delta = az.delta = 0.0;
				if (!kStepsLeft) { // (the counted scheme neither stores nor reads the two)
					ax.key = ay.key = az.key = 0xfffffffeu; // never matches: forces the first refresh
					ax.lim = ay.lim = az.lim = 0.0;
				}
				ax.rdel = ay.rdel = az.rdel = 0.0;
				ax.left = ay.left = az.left = -1; // (kStepsLeft: forces the first refresh)
				// window choice: step back one half-window when the cell index decreases along the ray
				const int offx = sx < 0.0 ? 1 : 0, offy = sy > 0.0 ? 1 : 0; // gy = trunc(-y/gw) falls when y grows
				const double gwid = (GWM == 0) ? 1.0 : f.grid_width;

				// The loop body is written branch-light on purpose: a wave executes every divergent
				// branch any of its lanes takes, and exec-mask juggling per `if` costs as much as
				// the arithmetic it guards.  Values are computed for all lanes and selected.
				bool done = entry_nan;
				while (!done) {
					bool skip_group = false;
					diag.begin_trip();
					// ---------------------------------------------------------- leap
					if (LEAP) {
						// (REC: after `fails` refusals in a row a ray attempts on every 2^fails-th trip of the WAVE's count -- rays that
						// back off do so in step, and on a map that admits no leaps the block is issued once in 64 trips)
						const bool attempt = REC ? (trip_no & ((1u << fails) - 1u)) == 0u : cooldown == 0;
						++trip_no;
						if constexpr (REC) cooldown -= attempt ? 0 : 1;
						else cooldown = (int)__builtin_elementwise_sub_sat((unsigned)cooldown, 1u); // (never negative: 0 stays, the others count down)
						if (attempt) {
							diag.on_attempt();
							// Order of the block (HMRM_EARLY_LOAD): the window look-up depends on the position and the level only, so
							// its load is issued FIRST; the refreshes of stale coordinates and the estimates of lateral room, which
							// do not need the loaded maximum, then run while it is in flight.  For a wave alone on its SIMD -- the
							// long waves at the end of a launch -- a trip is one chain of dependent instructions, and this takes
							// the refreshes and ~20 instructions of the estimate out of the part that waits for the load.
							auto refresh_stale = [&]() {
								const bool stale_x = kStepsLeft ? ax.left < 0 : (hi32(x) >> 20) != ax.key;
								const bool stale_y = kStepsLeft ? ay.left < 0 : (hi32(y) >> 20) != ay.key;
								const bool stale_z = kStepsLeft ? az.left < 0 : (hi32(z) >> 20) != az.key;
								diag.on_refresh_check(f, stale_x, stale_y, stale_z);
								if (stale_x) axis_refresh(ax, x, sx);
								if (stale_y) axis_refresh(ay, y, sy);
								if (stale_z) axis_refresh(az, z, sz);
							};
							if (!kEarlyLoad) refresh_stale();
							bool near0 = false;
							const double qx = cell_coord_fast<GWM>(x, f, near0), qy = cell_coord_fast<GWM>(-y, f, near0);
							// General grid widths: a start or landing point within 2^-20 of a cell boundary would need the true quotient
							// to name its cell.  The START divides for real then (a rare, wave-uniform branch: a coordinate that never
							// moves -- orthographic rays along an axis -- can sit that close to a boundary for a whole ray).  The LANDING
							// point does not: its cell is gxn or gxn - 1 (below), and the jump is accepted when BOTH lie inside the window
							// -- two inlined divisions and their temporaries less at the block's point of highest register pressure.
							// (Refusing such landings outright is wrong for speed: with 1 / grid_width an integer -- 0.05, 0.01 -- every
							// power of two is a cell boundary, the landing point of a binade-limited jump is the first position behind
							// one, always the same whatever the start, and a ray whose crossing step ends within 2^-20 of it was
							// refused again and again until it had MARCHED there: 175 groups instead of one, the launch's last wave.)
							double qx2 = qx, qy2 = qy;
							if (GWM == 2 && __builtin_amdgcn_ballot_w64(near0) != 0ull) {
								qx2 = near0 ? x / f.grid_width : qx;
								qy2 = near0 ? -y / f.grid_width : qy;
							}
							const int gx = cvt_i32_sat(qx2), gy = GWM == 0 ? cvt_i32_sat_neg(y) : cvt_i32_sat(qy2);
							const bool inb0 = (unsigned)gx < wlim && (unsigned)gy < hlim;
							const bool top = lev == kTopLevel;
							// window (ix,iy) of level lev: S = 4 << lev cells wide, one every 1<<hs cells.  The whole map is
							// the one window of the top plane: with hs = 28 every in-grid cell has ix = iy = 0 and the
							// spans below come out as the map's, so nothing else treats that level specially.
							// (levels below kDenseFrom: windows every half window, the others every quarter -- frame.hpp)
							const uint32_t lsa = CARRY ? ls : level_state<false>(lev);
							const int hs = (int)(lsa & 31u);
							const int back = (int)(lsa >> 5); // strides to step back when the cell index falls along the ray
							// (a cell inside the grid is not negative: the unsigned difference saturates at window 0)
							const int ix = (int)__builtin_elementwise_sub_sat((unsigned)(gx >> hs), (unsigned)(offx ? back : 0));
							const int iy = (int)__builtin_elementwise_sub_sat((unsigned)(gy >> hs), (unsigned)(offy ? back : 0));
							const unsigned widx = ((unsigned)lev << f.mip_plane_shift) + (unsigned)index_2d(iy, f.mip_row, ix); // (= mip_index)
							diag.load_begin(f, 17);
#ifndef HMRM_WIDE_MIP
#define HMRM_WIDE_MIP 1
#endif
							// (the element index fits 32 bits -- 8 planes of at most 2^28 floats, api.cpp's map limit -- the byte offset
							// need not: a 64-bit offset, one v_lshl_add_u64 where the 32-bit form had a shift.  Measured equal within the
							// run-to-run spread on C3 / C5 / C2 / C4, profiles/r05_raw/wide_mip_abn.txt; with HMRM_WIDE_MIP 0 -- round 4 --
							// very oblong maps near the 2^29-cell limit, 16385 x 32766, had to be rendered by the literal loop, 85 x slower.)
							float mf = HMRM_WIDE_MIP ? mip[(size_t)((REC ? inb0 && top : inb0) ? widx : 0u)]
							                         : *(const float *)((const char *)mip + (size_t)((inb0 ? widx : 0u) * 4u));
							uint32_t rec_xs0 = ~0u, rec_xs1 = ~0u, rec_ys0 = ~0u, rec_ys1 = ~0u;
							if constexpr (REC) { // the window's record: two 16-byte loads of one 32-byte line
								const WindowRecord *recs = reinterpret_cast<const WindowRecord *>(f.mipbuf_bil);
								const unsigned ridx = (inb0 && !top) ? (unsigned)index_2d(iy, rec_row(f.map_w), ix) : 0u;
								const uint4 r0 = *reinterpret_cast<const uint4 *>(recs + ridx);
								const uint2 r1 = *reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(recs + ridx) + 16);
								mf = top ? mf : __uint_as_float(r0.x);
								rec_xs0 = r0.z; rec_xs1 = r0.w; rec_ys0 = r1.x; rec_ys1 = r1.y;
							}
							diag.load_end(f, 17, mf);
							if (kEarlyLoad) refresh_stale();
							const bool exact = kStepsLeft ? (ax.left | ay.left | az.left) >= 0
							                              : ax.key != 0xffffffffu && ay.key != 0xffffffffu && az.key != 0xffffffffu;
							const int left_min = min(ax.left, min(ay.left, az.left)); // (kStepsLeft)
							const int wx0 = ix << hs, wy0 = iy << hs;
							// (the last windows of a row / column hang over the map's edge: the usable span ends at the edge)
							const int wcells = (back + 1) << hs; // window size S in cells: its strides, each 1 << hs cells
							const int wspan_x = min(wcells, f.map_w - wx0), wspan_y = min(wcells, f.map_h - wy0);
							// estimates of the steps left before each lateral constraint bites; rdel is signed like
							// the motion, so every quotient is >= 0.  Only estimates: verified below.
							// (a coordinate that does not move -- s == 0 or absorbed -- has rdel = 2^40 and is strictly inside
							// of whichever edge it looks at: a huge quotient once its sign is dropped, which costs nothing -- an
							// operand modifier -- and changes nothing for a moving coordinate.  No case distinction needed.)
							const double ex = (double)(offx ? wx0 : wx0 + wspan_x) * gwid;  // x edge ahead
							const double ey = -(double)(offy ? wy0 : wy0 + wspan_y) * gwid; // y edge ahead
							double room_lat = 0.0;
							if (kStepsLeft) {
								room_lat = __builtin_fmin(__builtin_fabs((ex - x) * ax.rdel), __builtin_fabs((ey - y) * ay.rdel));
								// (computed here, not sunk behind the wait for the load: the empty statement reads the estimate
								// and stands between the load and the first use of its result)
								if (kEarlyLoad) asm volatile("" : "+v"(mf) : "v"(room_lat));
							}
							const double m = (double)mf; // (floats rounded up: also bounds every float / interpolated threshold)
							const bool above = z >= m;
							// Nothing below can succeed unless the ray is above this window's maximum: when no
							// lane of the wave is, skip the estimate and the verification (the usual case in
							// the last, nearly empty waves of a launch, which set its duration).
							double room = 0.0, room_b = 0x1p40, room_z = 0.0;
							bool z_bound = false, ok = false, can = false, binade_bound = false;
							int n = 0;
							const bool cand = inb0 && exact && above;
							// (the wave asks for `above` alone: the ballot of one compare is the compare's own lane mask, that of the
							// conjunction a select and a compare more.  A wave whose only lanes above their maximum are no candidates
							// -- outside the grid: a ray's last trip on its way out; or not exact -- now runs the block for nothing
							// where it used to skip it.  How often that happens has not been counted: the headline A/B carries it,
							// DESIGN.md 5.2.  Per lane nothing changes: `can` and `ok` start from `cand`.)
							if (__builtin_amdgcn_ballot_w64(above) != 0ull) {
								if (kStepsLeft) {
									room = room_lat;
								} else {
									room = (ax.lim - x) * ax.rdel;
									room = __builtin_fmin(room, (ay.lim - y) * ay.rdel);
									room = __builtin_fmin(room, (az.lim - z) * az.rdel);
									room_b = room; // steps left inside the three binades
									room = __builtin_fmin(room, sx != 0.0 ? (ex - x) * ax.rdel : 0x1p40);
									room = __builtin_fmin(room, sy != 0.0 ? (ey - y) * ay.rdel : 0x1p40);
								}
								room_z = sz < 0.0 ? (m - z) * az.rdel : 0x1p40;
								z_bound = room_z < room;
								// (a select on the compare just made: the same value as fmin for the lanes that use it -- neither
								// is NaN there (z >= m, finite non-zero reciprocals) -- without fmin's canonicalising v_max)
								room = STATS ? __builtin_fmin(room, room_z) : (z_bound ? room_z : room);
								// (the saturating cast takes care of huge and negative estimates; the step budget caps the
								// integer: a jump never takes more steps than the cap has left)
								n = min(cvt_i32_sat(room * 0.998), budget) - 1;
								if (kStepsLeft) { // (the binades' share is an exact count, not an estimate)
									// (kCross: the jump's last step is a real one and may leave the binade)
									const int left_lim = left_min + (kCross ? 1 : 0);
									binade_bound = left_lim <= n;
									z_bound = z_bound & !binade_bound;
									n = min(n, left_lim);
								} else {
									binade_bound = room_b <= room;
								}
								can = cand && n >= kMinLeap;
								// landing point and its exact verification
								// (kCross: n - 1 steps by multiplication, all inside the three binades by count, then one real step
								// from that exact position.  Coordinates move monotonically, so the tests of the end point below
								// hold for every position before it.)
								const double nn = (double)(kCross ? n - 1 : n);
								const double xm = x + nn * ax.delta, ym = y + nn * ay.delta, zm = z + nn * az.delta;
								const double xn = kCross ? xm + sx : xm, yn = kCross ? ym + sy : ym, zn = kCross ? zm + sz : zm;
								bool nearn = false;
								const double qxn = cell_coord_fast<GWM>(xn, f, nearn), qyn = cell_coord_fast<GWM>(-yn, f, nearn);
								const int gxn = cvt_i32_sat(qxn), gyn = GWM == 0 ? cvt_i32_sat_neg(yn) : cvt_i32_sat(qyn);
								const bool inbn = (unsigned)gxn < wlim && (unsigned)gyn < hlim; // (diagnostics only)
								// (inside the window implies inside the grid: the spans were cut at the map's edge)
								// (kStepsLeft: n <= left of every axis, so the landing point is inside the three binades by count)
								// (general grid widths, nearn: q' + 2^-20 lies in [k, k + 2^-19), so the landing cell is k = gxn or k - 1;
								// both are asked to be inside the window, on both axes -- one flag serves the two)
								const unsigned nm = (GWM == 2 && nearn) ? 1u : 0u;
								ok = can && (unsigned)(gxn - wx0) - nm < (unsigned)wspan_x - nm &&
								     (unsigned)(gyn - wy0) - nm < (unsigned)wspan_y - nm && zn >= m &&
								     (kStepsLeft || (axis_landing_ok(ax, xn) && axis_landing_ok(ay, yn) && axis_landing_ok(az, zn)));
								diag.on_landing_refused(f, can && !ok, inbn,
								                        (unsigned)(gxn - wx0) < (unsigned)wspan_x && (unsigned)(gyn - wy0) < (unsigned)wspan_y, zn >= m);
								if constexpr (REC) {
									// The positions leaped over are x + k delta, k = 0 .. n - 1 (kCross: up to (xm, ym); else up to the landing
									// point): all ON the segment between the first and the last, inside the window, at heights >= max2.  None
									// of them may lie in a recorded cell: segment against each cell's box, in cells relative to the window's
									// corner, float -- values below 32, conversion and product errors below 2^-13 -- with the box grown by
									// 2^-10 and the line test given 2^-9 of slack: conservative, never wrong.  (Separating axes: the
									// segment's extent in x, in y, and the line through it against the box's four corners.)
									const double bxd = kCross ? xm : xn, byd = kCross ? ym : yn;
									const double qbx = GWM == 0 ? bxd : bxd * f.inv_grid_width, qby = GWM == 0 ? -byd : -byd * f.inv_grid_width;
									const float pax = (float)(qx2 - (double)wx0), pay = (float)(qy2 - (double)wy0);
									const float pbx = (float)(qbx - (double)wx0), pby = (float)(qby - (double)wy0);
									constexpr float grow = 0x1p-10f;
									const float ddx = pbx - pax, ddy = pby - pay;
									const float x_lo = __builtin_fminf(pax, pbx) - (1.0f + grow), x_hi = __builtin_fmaxf(pax, pbx) + grow;
									const float y_lo = __builtin_fminf(pay, pby) - (1.0f + grow), y_hi = __builtin_fmaxf(pay, pby) + grow;
									const float reach = (0.5f + grow) * (__builtin_fabsf(ddx) + __builtin_fabsf(ddy)) + 0x1p-9f;
									const float cax = pax - 0.5f, cay = pay - 0.5f; // (cell corner - this = cell centre - start)
									bool touched = false;
#pragma unroll
									for (int k = 0; k < kRecCells; ++k) {
										const uint32_t wxs = k < 4 ? rec_xs0 : rec_xs1, wys = k < 4 ? rec_ys0 : rec_ys1;
										const float cx = (float)((wxs >> (8 * (k & 3))) & 0xffu), cy = (float)((wys >> (8 * (k & 3))) & 0xffu);
										const float ex = cx - cax, ey = cy - cay;
										const float cross = ex * ddy - ey * ddx;
										const bool apart = cx > x_hi || cx < x_lo || cy > y_hi || cy < y_lo || __builtin_fabsf(cross) > reach;
										touched = touched || !apart;
									}
									// (the reference truncates: a coordinate in (-1, 0) -- a ray on its way out through the map's low edge --
									// still names cell 0, which no box says.  Such paths are marched.)
									const bool floor_is_trunc = __builtin_fmin(qx2, qbx) >= 0.0 && __builtin_fmin(qy2, qby) >= 0.0;
									ok = ok && (top || (!touched && floor_is_trunc));
								}
								x = ok ? xn : x;
								y = ok ? yn : y;
								z = ok ? zn : z;
								budget -= ok ? n : 0;
								if (kStepsLeft) {
									const int took = ok ? n : 0;
									ax.left -= took;
									ay.left -= took;
									az.left -= took;
								}
							}
							diag.on_attempt_done(f, inb0, exact, above, n < kMinLeap, z_bound, can, ok, n, lev);
							diag.on_bounds(ok, binade_bound);
							// level policy (performance only; any policy gives the same pixels):
							//   window crossed                    -> coarser next time, if the height bound of this
							//                                        level left room for a window kUpRatio times
							//                                        longer (a coarser maximum is no lower)
							//   jump ended at a binade boundary   -> same level (without kCross: and march a group first)
							//   height bound was the limit        -> finer; without a jump retry at once (the
							//     (z < max, or z-room smallest)      level strictly decreases); at the finest
							//                                        level march 1 + finest_pause groups first
							//   no lateral/binade room, not exact -> coarser (a bigger window has more room),
							//                                        growing pause while attempts keep failing
							const bool height_limited = inb0 && exact && (!above || z_bound);
							// levels per move: two while the ray is young (kAdaptive), then one
							const int lstep = level_step(young_left);
							if (kAdaptive) young_left -= ok ? 1 : 0;
							const int coarser = level_coarser(lev, lstep);
							const int minlev = f.min_level;
#ifndef HMRM_DOWN
#define HMRM_DOWN 1
#endif
							// a failed height test drops HMRM_DOWN levels, a height-limited jump one
							const int drop = (ok ? 1 : HMRM_DOWN) * lstep;
							const int finer = level_finer(lev, drop, minlev);
							const bool at_finest = lev == minlev;
							// (selects, not branches: the three cases are mutually exclusive)
							const bool crossed = ok && !z_bound;
							const bool hl = !crossed && height_limited;
							const bool other = !crossed && !hl;
							// (lane-mask logic: `a ? b : c` on booleans would be materialised in VGPRs)
							// (a window lstep levels up is 2^lstep times as long: the scaling rides on the exponent)
							const double room_up = kAdaptive ? __builtin_ldexp(room, lstep) : kUpRatio * room;
							const bool go_up = (crossed & (room_z >= room_up) & !binade_bound) | other;
							const int fails_before = fails;
							lev = hl ? finer : (go_up ? coarser : lev);
							fails = (crossed | (hl & ok)) ? 0 : fails + (other ? 1 : 0);
							const bool hl_fail = hl & !ok, pause_now = hl_fail & at_finest;
							cooldown = pause_now ? f.finest_pause : (other ? (fails_before < 3 ? fails_before : 3) : 0);
							// retry one level down without marching; after a jump look at the next window straight
							// away -- unless the jump stopped at a binade boundary: only real steps cross it,
							// another attempt here would just fail
							// (kCross: the jump's last step has crossed it)
							skip_group = (hl_fail ^ pause_now) | (ok & (kCross | !binade_bound));
							if constexpr (REC) {
								// two levels only: the whole map while the ray is above everything, then the record level for good.
								// A refusal there is followed by a group; refusals in a row thin the attempts out (see `attempt`).
								lev = lev == kTopLevel ? kTopLevel : kRecLevel;
								fails = (ok | top) ? 0 : (fails_before < kRecBackoff ? fails_before + 1 : kRecBackoff);
								skip_group = (top & hl & !ok) | (ok & (kCross | !binade_bound));
							}
							if constexpr (CARRY) ls = level_state<true>(lev);
						}
					}
					diag.on_trip(f, LEAP, skip_group);
					if (skip_group) continue;

					// --------------------------------------------- speculative group
					diag.on_group();
					double X[U], Y[U], Z[U], T[U];
					unsigned cell[U]; // (unsigned: the 64-bit address needs no sign extension)
					bool inb[U];
					X[0] = x; Y[0] = y; Z[0] = z;
#pragma unroll
					for (int j = 1; j < U; ++j) {
						X[j] = X[j - 1] + sx;
						Y[j] = Y[j - 1] + sy;
						Z[j] = Z[j - 1] + sz;
					}
					// cells of the U positions.  Only the integers are kept: the general-grid-width quotient q' is needed for
					// nothing but its truncation (and the test whether it is too close to an integer to be trusted), and holding
					// U pairs of them cost the general instantiations 12 vector registers (76: 6 waves per SIMD).  The
					// bilinear mode needs the exact quotients themselves (its weights) and keeps them.
					double QX[BILINEAR ? U : 1], QY[BILINEAR ? U : 1];
					bool near = false;
#pragma unroll
					for (int j = 0; j < U; ++j) {
						int gx, gy;
						if constexpr (BILINEAR && GWM != 0) { // (the exact q: true division unless the reciprocal is exact)
							QX[j] = GWM == 2 ? X[j] / f.grid_width : X[j] * f.inv_grid_width;
							QY[j] = GWM == 2 ? -Y[j] / f.grid_width : -Y[j] * f.inv_grid_width;
							gx = cvt_i32_sat(QX[j]);
							gy = cvt_i32_sat(QY[j]);
						} else {
							const double qx = cell_coord_fast<GWM>(X[j], f, near), qy = cell_coord_fast<GWM>(-Y[j], f, near);
							if constexpr (BILINEAR) { QX[j] = qx; QY[j] = qy; }
							gx = cvt_i32_sat(qx);                                       // hmap.cpp:1001-1004
							gy = GWM == 0 ? cvt_i32_sat_neg(Y[j]) : cvt_i32_sat(qy);
						}
						inb[j] = (unsigned)gx < wlim && (unsigned)gy < hlim;      // hmap.cpp:1006-1011
						cell[j] = inb[j] ? (unsigned)index_2d(gy, f.map_w, gx) : 0u;
					}
					if (GWM == 2 && !BILINEAR && near) { // some position is on a cell boundary to within 2^-20: divide for real
#pragma unroll
						for (int j = 0; j < U; ++j) {
							// (one division at a time: interleaved, their temporaries set the kernel's register count)
							__builtin_amdgcn_sched_barrier(0);
							const int gx = cvt_i32_sat(X[j] / f.grid_width);
							__builtin_amdgcn_sched_barrier(0);
							const int gy = cvt_i32_sat(-Y[j] / f.grid_width);
							inb[j] = (unsigned)gx < wlim && (unsigned)gy < hlim;
							cell[j] = inb[j] ? (unsigned)index_2d(gy, f.map_w, gx) : 0u;
						}
						__builtin_amdgcn_sched_barrier(0);
					}
					diag.load_begin(f, 18);
					if constexpr (BILINEAR) {
#pragma unroll
						for (int j = 0; j < U; ++j) {
							const Bil b = bil_setup(inb[j] ? QX[j] : 0.0, inb[j] ? QY[j] : 0.0, f.map_w, f.map_h);
							T[j] = bil_mix(b, thr[b.c00], thr[b.c10], thr[b.c01], thr[b.c11]);
						}
					} else {
#pragma unroll
						// (32-bit byte offsets from the table's base -- api.cpp caps maps at 2^29 cells -- so that the loads can
						// take the base from scalar registers: no 64-bit address arithmetic per sample)
						for (int j = 0; j < U; ++j)
							T[j] = F32 ? (double)*(const float *)((const char *)thr32 + (size_t)(cell[j] * 4u))
							           : *(const double *)((const char *)thr + (size_t)(cell[j] * 8u)); // hmap.cpp:1013-1014 (+ c0.z)
					}
					if constexpr (U == 4) diag.load_end(f, 18, T[0], T[1], T[2], T[3]);
					const bool hit_before = real_hit; // (diagnostics only)
					if (budget >= U) {
						// in order: the first position that leaves the grid (:1006) or hits (:1016) ends the ray
						int first = U, hit_j = 0;
						unsigned hit_cell = 0u;
						bool hit = false, stop = false;
#pragma unroll
						for (int j = U - 1; j >= 0; --j) { // (selects, last write = earliest position)
							const bool h = inb[j] && Z[j] < T[j];
							const bool s = !inb[j] || h;
							if (COUNT) first = s ? j : first;
							stop = stop | s; // (lane masks: no VGPR select)
							hit = s ? h : hit;
							hit_cell = s ? cell[j] : hit_cell;
							hit_j = s ? j : hit_j;
						}
						// loads the reference executed in this group: U unless the ray ends in it.  Only the instrumented kernel
						// and the ray batches read the budget of a ray that has ended (its step count), so only they count the exact
						// share of the last group; the others need the budget of rays that go on, and first + hit = U for those.
						budget -= COUNT ? first + (hit ? 1 : 0) : U;
						done = stop;
						if (hit) {
							if constexpr (BILINEAR) {
								// (the weights are rebuilt for the one position that hit: cheaper than keeping
								// U sets of them alive)
								double qxh = QX[0], qyh = QY[0];
#pragma unroll
								for (int j = 1; j < U; ++j) {
									qxh = hit_j == j ? QX[j] : qxh;
									qyh = hit_j == j ? QY[j] : qyh;
								}
								// (DEFER: the colour's five loads, its weights and mixes come behind the loop, bilinear_pixel below)
								if constexpr (!DEFER && SUNLIT) { // (a shadow ray has no colour, and the mirror pixel in `rgba` outlives pass 3: a scalar branch)
									if ((lt.phase & 1) == 0) rgba = shade_hit_bilinear(f, cmap, (int)hit_cell, bil_setup(qxh, qyh, f.map_w, f.map_h));
								} else
								if constexpr (!DEFER && !CELLS) // (a cell map has no colours: `cmap` is null)
								rgba = shade_hit_bilinear(f, cmap, (int)hit_cell, bil_setup(qxh, qyh, f.map_w, f.map_h));
								if constexpr (KEEP_Q) { hqx = qxh; hqy = qyh; }
							}
							// (DEFER: no colour here, nothing reads it before the pixel is stored -- see hcell)
							if constexpr (!DEFER && !BILINEAR && !CELLS) rgba = shade_hit(f, cmap[hit_cell]);
							if constexpr (LIT) hcell = lt.phase ? hcell : hit_cell; // (the primary ray's)
							else if constexpr (SUNLIT) hcell = (lt.phase & 1) ? hcell : hit_cell; // (the primary ray's, then the mirror ray's)
							else hcell = hit_cell;
							real_hit = true;
							if constexpr (CHAIN) {
								hx = X[0]; hy = Y[0]; hz = Z[0];
#pragma unroll
								for (int j = 1; j < U; ++j) {
									hx = hit_j == j ? X[j] : hx;
									hy = hit_j == j ? Y[j] : hy;
									hz = hit_j == j ? Z[j] : hz;
								}
							}
							if constexpr (KEEP_P) {
								// The shadow ray's origin (P.x, P.y, t): int_point's x and y where :1016 fired and the threshold z was
								// below.  The lane leaves the loop with it in x, y, z, which nothing else reads after a hit, so no
								// register is held across the loop for it; and X[hit_j] is made again from the group's start with
								// the same sequential adds (the same bits) so that X[1 .. U-2] need not outlive the cell indices.
								// (GEOM, HAZE: int_point itself -- z is stepped like x and y, no threshold is kept)
								double ox = x, oy = y, ot = POINT ? z : T[0];
#pragma unroll
								for (int j = 1; j < U; ++j) {
									ox = hit_j >= j ? ox + sx : ox;
									oy = hit_j >= j ? oy + sy : oy;
									if constexpr (POINT) ot = hit_j >= j ? ot + sz : ot;
									else ot = hit_j == j ? T[j] : ot;
								}
								x = ox; y = oy; z = ot;
							}
						}
					} else {
						// (almost never) close to the step cap: the literal loop, one position at a time, cap
						// checked per step; a real loop over scalars so that none of the group's arrays is
						// indexed dynamically
						double xs = x, ys = y, zs = z;
#pragma unroll 1
						for (int j = 0; j < U; ++j) {
							const double qx = (GWM == 0) ? xs : xs / f.grid_width, qy = (GWM == 0) ? -ys : -ys / f.grid_width;
							const int gx = cvt_i32_sat(qx), gy = cvt_i32_sat(qy);
							if (!((unsigned)gx < wlim && (unsigned)gy < hlim)) { done = true; break; }
							if (budget <= 0) { my_cap = 1; done = true; break; }
							--budget;
							const int c = gy * f.map_w + gx;
							Bil b{};
							double t;
							if (BILINEAR) {
								b = bil_setup(qx, qy, f.map_w, f.map_h);
								t = bil_mix(b, thr[b.c00], thr[b.c10], thr[b.c01], thr[b.c11]);
							} else {
								t = F32 ? (double)thr32[c] : thr[c];
							}
							if (zs < t) { // hmap.cpp:1016
								if constexpr (!DEFER && SUNLIT) { // (as in the group)
									if ((lt.phase & 1) == 0) rgba = BILINEAR ? shade_hit_bilinear(f, cmap, c, b) : shade_hit(f, cmap[c]);
								} else
								if constexpr (!DEFER && !CELLS) rgba = BILINEAR ? shade_hit_bilinear(f, cmap, c, b) : shade_hit(f, cmap[c]);
								real_hit = true;
								if constexpr (KEEP_Q) { hqx = qx; hqy = qy; }
								if constexpr (LIT) hcell = lt.phase ? hcell : (unsigned)c; // (as in the group: the colour comes behind the loop)
								else if constexpr (SUNLIT) hcell = (lt.phase & 1) ? hcell : (unsigned)c;
								else hcell = (unsigned)c;
								if constexpr (CHAIN) { hx = xs; hy = ys; hz = zs; }
								if constexpr (KEEP_P) { x = xs; y = ys; z = POINT ? zs : t; } // (as above)
								done = true;
								break;
							}
							xs += sx;
							ys += sy;
							zs += sz;
						}
					}
					diag.on_group_done(f, real_hit && !hit_before);
					if constexpr (KEEP_P) { // (a lane that hit keeps what the hit left in x, y, z)
						x = real_hit ? x : X[U - 1] + sx;
						y = real_hit ? y : Y[U - 1] + sy;
						z = real_hit ? z : Z[U - 1] + sz;
					} else {
						x = X[U - 1] + sx;
						y = Y[U - 1] + sy;
						z = Z[U - 1] + sz;
					}
					if (LEAP && kStepsLeft) { // U real steps further inside (or out of) the binades
						ax.left -= U;
						ay.left -= U;
						az.left -= U;
					}
				}
				if (COUNT) my_steps = (unsigned long long)(unsigned)(budget0 - budget);
				if constexpr (SEG && COUNT) my_steps = (unsigned long long)(unsigned)(sg.budget - budget);
				if constexpr ((LIT && SHADE && BILINEAR) || LSUM) { // (the primary hit's point outlives the shadow march: the gradient is taken there; LSUM: every pass's ray starts there)
					if (lt.phase == 0) { lt.hx = x; lt.hy = y; lt.t = z; }
				} else
				if constexpr (SUNLIT) { // (the primary hit's point outlives pass 1, the mirror hit's pass 3: a shadow ray's own is not kept)
					if ((lt.phase & 1) == 0) { lt.hx = x; lt.hy = y; lt.t = z; }
				} else
				if constexpr (LIT || MIRROR) { lt.hx = x; lt.hy = y; lt.t = z; } // (of a lane that hit: see the end of the loop)
				else if constexpr (POINT && CHAIN) { hqx = hx; hqy = hy; }
				else if constexpr (POINT) { hqx = x; hqy = y; hz = z; } // (int_point of a lane that hit)
				else if constexpr (KEEP_P) { hqx = x; hqy = y; } // (SHADE, bilinear: the same two, for the gradient at P)
			}
			if constexpr (LSUM) {
				// After the primary rays: as LIT below, except that no pixel is kept -- the hit point and hcell are, for every pass -- and
				// that the wave takes direction 0 of the list.  After a shadow pass: a lane that hit folds the weight of this direction
				// into its sum and counts the ray if the step cap stopped it (an END ray is not a capped one; the primary ray counts
				// the same way, once); while directions are left the wave takes the next one, and the ray, its d, its budget, real_hit
				// and the cap state start over -- everything derived from them is computed again by the next pass.
				again = false;
				double sdir[3];
				lm.acc += (my_cap != 0u && !sg.ends) ? 0x10000u : 0u; // (the lanes that sat the pass out have my_cap = 0)
				my_cap = 0u;
				if (lt.phase == 0) {
					lt.primary_hit = real_hit;
					if (__builtin_amdgcn_ballot_w64(real_hit) != 0ull) {
						lt.phase = 1;
						lt.dz = ray.dz;
						if ((a.lsum.flags & kShadeNoShadows) != 0u) { // (no march: the n weights of the lanes that hit, here)
#pragma unroll 1
							for (int k = 0; k < a.lsum.n; ++k) {
								sum_direction(a.lsum, k, sdir);
								if (lt.primary_hit) lm.acc += sum_weight(a.sun, a.lsum, false, sdir);
							}
						} else {
							again = true;
						}
					}
				} else {
					sum_direction(a.lsum, lm.k, sdir); // (loaded again behind the march rather than held across it)
					if (lt.primary_hit) lm.acc += sum_weight(a.sun, a.lsum, real_hit, sdir);
					++lm.k;
					again = lm.k < a.lsum.n;
				}
				if (again) {
					sum_direction(a.lsum, lm.k, sdir);
					ray.px = lt.hx; ray.py = lt.hy; ray.pz = lt.t; // (shadow_ray's, towards direction k)
					ray.dx = sdir[0]; ray.dy = sdir[1]; ray.dz = sdir[2];
					d = __builtin_huge_val();
					if (lt.primary_hit) {
						d = shadow_entry(ray, f);
						sg.budget = segment_budget(SegRules{nullptr, a.sun.max_steps, 1u}, 0, f.step_cap, &sg.ends);
					}
					real_hit = false;
				}
			} else
			if constexpr (LIT) {
				// After the primary rays: the lanes that hit keep their pixel and become their shadow rays -- the ray, its d, its step
				// (above) and its budget min(step cap, L) are replaced, everything derived from them is computed again by the second
				// pass -- the others get d = inf and sit it out.  A wave without a hit is finished.  After the shadow rays: real_hit
				// says SHADOWED for the lanes that marched one.
				again = false;
				if (lt.phase == 0) {
					lt.primary_hit = real_hit;
					if constexpr (BILINEAR && DEFER) { // (the primary pixel, between the two marches: the point is at hand, and LitState::rgba holds it)
						if (real_hit) {
							double qxp, qyp;
							cell_coords_of(lt.hx, lt.hy, qxp, qyp);
							rgba = bilinear_pixel(qxp, qyp);
						}
					}
					lt.rgba = rgba;
					if (__builtin_amdgcn_ballot_w64(real_hit) != 0ull) {
						lt.phase = 1;
						again = true;
						// (every lane takes the new ray -- a lane that keeps its old one would hold it in registers through the
						// second march for nothing -- and only its dz, for the miss shade, is put aside)
						lt.dz = ray.dz;
						ray = shadow_ray(lt, a.sun);
						d = __builtin_huge_val();
						if (real_hit) {
							d = shadow_entry(ray, f);
							sg.budget = segment_budget(SegRules{nullptr, a.sun.max_steps, 1u}, 0, f.step_cap, &sg.ends);
						}
						real_hit = false;
					}
				}
			}
			if constexpr (SUNLIT) {
				// Behind every pass (march_family.hpp SunWater): the lane counts its ray if the step cap stopped it (an END ray is not a
				// capped one), puts what the pass found into its word, and the wave takes the next pass that any of its lanes needs.
				// Behind pass 0 the word is made as MIRROR makes it, "wet" decided by the same comparison; the keeps-pixel form chooses the
				// base there -- a wet lane's own colour in place of its pixel -- and weights it as soon as the weight is known: here
				// without shadow rays, behind pass 1 with them.  Behind pass 1 real_hit says SHADOWED for the lanes that hit, behind
				// pass 2 that the mirror ray hit, behind pass 3 SHADOWED for the mirror hits.
				again = false;
				if (my_cap != 0u && !sg.ends) atomicAdd(&st.counters[2], 1ull);
				my_cap = 0u;
				const bool shadows = (a.water.flags & kWaterSunNoShadows) == 0u;
				int next = 4;
				if (lt.phase == 0) {
					uint32_t keep;
					if constexpr (kMirrorKeepsCell) keep = hcell;
					else {
						if constexpr (DEFER) { // (BILINEAR)
							if (real_hit) {
								double qxp, qyp;
								cell_coords_of(lt.hx, lt.hy, qxp, qyp);
								rgba = bilinear_pixel(qxp, qyp);
							}
						}
						keep = rgba;
					}
					const bool wet = real_hit && lt.t <= a.water.level; // (a NaN level: no water)
					if constexpr (!kMirrorKeepsCell) {
						keep = wet ? water_base(keep, a.water) : keep;
						if (!shadows && real_hit) keep = shade_weighted(keep, sun_weight(a.sun, a.water, false, hcell, lt.hx, lt.hy));
					}
					lt.rgba = (keep & kSunValue) | (real_hit ? kMirrorHit : 0u) | (wet ? kMirrorWet : 0u);
					if (shadows && __builtin_amdgcn_ballot_w64(real_hit) != 0ull) next = 1;
					else if (__builtin_amdgcn_ballot_w64(wet) != 0ull) next = 2;
				} else if (lt.phase == 1) {
					if constexpr (kMirrorKeepsCell) lt.rgba |= real_hit ? kSunShadowed : 0u;
					else if ((lt.rgba & kMirrorHit) != 0u)
						lt.rgba = (shade_weighted(lt.rgba, sun_weight(a.sun, a.water, real_hit, hcell, lt.hx, lt.hy)) & kSunValue) | (lt.rgba & ~kSunValue);
					if (__builtin_amdgcn_ballot_w64((lt.rgba & kMirrorWet) != 0u) != 0ull) next = 2;
				} else if (lt.phase == 2) {
					if constexpr (kMirrorKeepsCell) hcell = real_hit ? hcell : ~0u;
					else lt.rgba |= real_hit ? kSunMirrorHit : 0u;
					if (shadows && __builtin_amdgcn_ballot_w64(real_hit) != 0ull) next = 3;
				}
				if (next < 4) {
					// The next pass's rays: a shadow ray from the kept point towards the sun (1: of a lane that hit; 3: of a lane whose
					// mirror ray just hit -- real_hit still says so), or (2) the mirror ray of a wet lane, MIRROR's: the primary direction
					// with dz negated, from the same point.  Every lane takes the new ray, the lanes without one at d = inf.
					const bool marches = next == 2 ? (lt.rgba & kMirrorWet) != 0u : real_hit;
					lt.phase = next;
					again = true;
					ray.px = lt.hx; ray.py = lt.hy; ray.pz = lt.t;
					uint32_t limit = a.sun.max_steps;
					if (next == 2) {
						const DevRay primary = camera_ray_again();
						ray.dx = primary.dx; ray.dy = primary.dy; ray.dz = -primary.dz;
						limit = a.water.max_steps;
					} else {
						ray.dx = a.sun.dir[0]; ray.dy = a.sun.dir[1]; ray.dz = a.sun.dir[2];
					}
					d = __builtin_huge_val();
					if (marches) {
						d = shadow_entry(ray, f);
						sg.budget = segment_budget(SegRules{nullptr, limit, 1u}, 0, f.step_cap, &sg.ends);
					}
					real_hit = false;
				}
			} else
			if constexpr (MIRROR) {
				// After the primary rays: the lanes that hit at or below the water level become their mirror rays -- origin, dz, the step
				// (above) and the budget min(step cap, L) are replaced, dx and dy stay -- and the others get d = inf and sit the pass out.
				// A wave without a water lane is finished.  What a lane keeps of its primary ray is ONE word, LitState::rgba: the hit
				// cell (nearest-cell modes with the colour behind the loop: the colour is fetched there, behind both marches, as LIT
				// does) or the pixel itself (the bilinear mode: made here, where the point is at hand; the in-loop fetch: it is there
				// already), with "hit" and "water" in the bits the value leaves free -- two lane masks in scalar registers less across
				// the mirror march, in kernels that sit on the scalar registers' limit.  So hcell and the point are
				// free for the mirror pass.  Every lane negates its dz, the dry ones too: negated once more behind the loop it is the
				// primary ray's again, bit for bit, and nothing is put aside for the miss shade.  After the mirror rays: real_hit says
				// that the mirror ray hit.
				again = false;
				if (lt.phase == 0) {
					uint32_t keep;
					if constexpr (kMirrorKeepsCell) keep = hcell;
					else {
						if constexpr (DEFER) { // (BILINEAR)
							if (real_hit) {
								double qxp, qyp;
								cell_coords_of(lt.hx, lt.hy, qxp, qyp);
								rgba = bilinear_pixel(qxp, qyp);
							}
						}
						keep = rgba;
					}
					const bool wet = real_hit && lt.t <= a.water.level; // (a NaN level: no water)
					if constexpr (BAKED && !kMirrorKeepsCell) {
						// (under baked light, keeps-pixel form: the base -- the primary pixel, or for a wet lane with its own colour that
						// colour -- takes the weight of the primary hit's light here, where the point and the cell are at hand; A stays
						// 255, so the packing below holds.  The keeps-cell form weights behind both marches, from the kept cell.)
						if (real_hit) {
							uint32_t light;
							if constexpr (BILINEAR) {
								double qxl, qyl;
								cell_coords_of(lt.hx, lt.hy, qxl, qyl);
								light = baked_light_bilinear(a.baked.plane, bil_setup(qxl, qyl, f.map_w, f.map_h));
							} else light = a.baked.plane[hcell];
							keep = shade_baked(wet ? water_base(keep, a.water) : keep, light, a.baked.full_scale);
						}
					}
					lt.rgba = (keep & kMirrorValue) | (real_hit ? kMirrorHit : 0u) | (wet ? kMirrorWet : 0u);
					if (__builtin_amdgcn_ballot_w64(wet) != 0ull) {
						lt.phase = 1;
						again = true;
						ray.px = lt.hx; ray.py = lt.hy; ray.pz = lt.t;
						ray.dz = -ray.dz;
						d = __builtin_huge_val();
						if (wet) {
							d = shadow_entry(ray, f);
							sg.budget = segment_budget(SegRules{nullptr, a.water.max_steps, 1u}, 0, f.step_cap, &sg.ends);
						}
						real_hit = false;
					}
				}
			}
			if constexpr (SUM) {
				// After a pass: the lane folds the value of this target's ray into its sum -- the very byte k_cell_map's epilogue below
				// would store for it, or 1 for a ray that did not hit -- and counts the pass if the step cap stopped it (an END ray is
				// not a capped one).  While targets are left the wave then takes the next one: the cell's ray is made again from the
				// cell index, as the epilogue makes it, and d, the budget, real_hit and the cap state start over; everything derived
				// from them is computed again by the next pass.  The target's index is the same for the whole wave.
				// (The lane's cell is made again per pass from its number in the wave, which goes through an empty statement: what
				// is made from it -- the cell's position, its threshold, its gradient -- does not depend on the target, and the
				// compiler would otherwise make all that once, before the first pass, and hold it in vector registers across every
				// march: 104 instead of 73 of them in the production instantiation.)
				int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
				asm volatile("" : "+v"(ln));
				const PixelId me = pixel_of_tile_lane(f, rows, tiles_y, tile_x, gy, wave, ln);
				const int spx = me.px, spy = me.py;
				const bool capped = my_cap != 0u && !sg.ends;
				sm.acc += capped ? 0x10000u : 0u; // (the sum is below 2^16: the passes the step cap stopped are counted above it)
				my_cap = 0u;
				uint32_t v = real_hit ? 0u : 1u;
				if ((a.cells.flags & kMapWeight) != 0u) {
					uint32_t q = 0u;
					if ((a.cells.flags & kMapDiffuse) != 0u && !real_hit) { // the level of the cell under its direction towards this target
						const DevRay own = cell_ray_of<SAMP>(sm.rules, f, thr, spx, spy);
						const double s[3] = {own.dx, own.dy, own.dz};
						if constexpr (BILINEAR) {
							double qxc, qyc;
							cell_coords_of(own.px, own.py, qxc, qyc);
							q = diffuse_level_bilinear(f, thr, bil_setup(qxc, qyc, f.map_w, f.map_h), s);
						} else {
							q = diffuse_level_nearest<F32>(f, thr, (unsigned)index_2d(a.cells.y0 + spy, f.map_w, a.cells.x0 + spx), s);
						}
					}
					v = cell_weight(a.cells, real_hit, q);
				}
				sm.acc += v;
				++sm.k;
				again = sm.k < a.sums.n;
				if (again) {
					sum_target(a.sums, sm.k, &sm.rules);
					ray = cell_ray_of<SAMP>(sm.rules, f, thr, spx, spy);
					d = __builtin_huge_val();
					if ((a.cells.flags & kMapNoShadows) == 0u) d = shadow_entry(ray, f);
					sg.budget = segment_budget(a.seg, 0, f.step_cap, &sg.ends);
					real_hit = false;
				}
			}
		} while ((LIT || SUM || MIRROR) && again); // (LSUM implies LIT)
		// The hit lanes' colour: fetched here, once, behind the march (LIT, nearest-cell modes: behind both marches).
		double qxh = hqx, qyh = hqy; // (bilinear: the hit's cell coordinates, for the colour and SHADE's gradient)
		if constexpr (BILINEAR && (KEEP_P || POINT) && !LIT && !MIRROR) cell_coords_of(hqx, hqy, qxh, qyh);
		if constexpr (GEOM) {
			if (out != nullptr && real_hit) rgba = BILINEAR ? bilinear_pixel(qxh, qyh) : shade_hit(f, cmap[hcell]);
		} else
		if constexpr (DEFER && !LIT && !MIRROR) {
			if (real_hit) rgba = BILINEAR ? bilinear_pixel(qxh, qyh) : shade_hit(f, cmap[hcell]);
		}
		if constexpr (SUNLIT) {
			// Behind the last pass.  A lane that hit: its base -- its pixel, or a wet lane's own colour -- at the weight of the primary hit
			// (keeps-cell form: colour and level fetched here from the kept cell; keeps-pixel form: done behind pass 1).  A wet lane: its
			// mirror ray's pixel -- the colour at the mirror hit's cell (the bilinear mode: and point) at the weight of THAT hit, whose
			// shadow ray pass 3 marched (real_hit: shadowed), or for MISS, END and CAPPED the miss shade of the mirror ray's own dz,
			// untouched -- blended in.  The primary direction's dz is made again for the miss shades.
			const double primary_dz = lt.phase == 0 ? ray.dz : camera_ray_again().dz;
			if ((lt.rgba & kMirrorHit) != 0u) {
				const bool wet = (lt.rgba & kMirrorWet) != 0u;
				uint32_t kept;
				if constexpr (kMirrorKeepsCell) {
					const unsigned pcell = lt.rgba & kSunValue;
					kept = shade_hit(f, cmap[pcell]);
					kept = shade_weighted(wet ? water_base(kept, a.water) : kept, sun_weight(a.sun, a.water, (lt.rgba & kSunShadowed) != 0u, pcell, 0.0, 0.0)) | 0xff000000u;
				} else kept = lt.rgba | 0xff000000u;
				if (wet) {
					uint32_t m = rgba; // (the in-loop fetch's, where the family keeps that)
					bool mirror_hit;
					if constexpr (kMirrorKeepsCell) mirror_hit = hcell != ~0u;
					else mirror_hit = (lt.rgba & kSunMirrorHit) != 0u;
					if (mirror_hit) {
						if constexpr (DEFER) {
							if constexpr (BILINEAR) {
								double qxm, qym;
								cell_coords_of(lt.hx, lt.hy, qxm, qym);
								m = bilinear_pixel(qxm, qym);
							} else m = shade_hit(f, cmap[hcell]);
						}
						m = shade_weighted(m, sun_weight(a.sun, a.water, lt.phase == 3 && real_hit, hcell, lt.hx, lt.hy));
					} else m = shade_miss(f, -primary_dz);
					kept = blend_water_base(kept, m, a.water);
				}
				rgba = kept;
				real_hit = true;
			} else real_hit = false;
			ray.dz = primary_dz; // (for the miss shade)
		} else
		if constexpr (MIRROR) {
			// A water lane: its mirror ray's pixel -- the colour of the cell that ray hit, fetched here from the mirror pass's own hcell
			// (the bilinear mode: and hit point), or for MISS, END and CAPPED the miss shade of the mirror ray's own dz -- blended into
			// the primary pixel or the water's own colour.  A dry lane that hit keeps its primary pixel.
			if ((lt.rgba & kMirrorHit) != 0u) {
				uint32_t kept;
				if constexpr (kMirrorKeepsCell) kept = shade_hit(f, cmap[lt.rgba & kMirrorValue]);
				else kept = lt.rgba | 0xff000000u;
				if constexpr (BAKED && kMirrorKeepsCell) { // (the base under the primary hit's light: the plane's word beside the colour, from the kept cell)
					const uint32_t light = a.baked.plane[lt.rgba & kMirrorValue];
					kept = shade_baked((lt.rgba & kMirrorWet) != 0u ? water_base(kept, a.water) : kept, light, a.baked.full_scale) | 0xff000000u;
				}
				if ((lt.rgba & kMirrorWet) != 0u) {
					uint32_t m = rgba; // (the in-loop fetch's, where the family keeps that)
					if constexpr (DEFER) {
						if (real_hit) {
							if constexpr (BILINEAR) {
								cell_coords_of(lt.hx, lt.hy, qxh, qyh);
								m = bilinear_pixel(qxh, qyh);
							} else m = shade_hit(f, cmap[hcell]);
						}
					}
					if constexpr (BAKED) { // (the mirror pixel under the light of the mirror ray's own hit: its cell, or its point)
						if (real_hit) {
							uint32_t light;
							if constexpr (BILINEAR) {
								cell_coords_of(lt.hx, lt.hy, qxh, qyh);
								light = baked_light_bilinear(a.baked.plane, bil_setup(qxh, qyh, f.map_w, f.map_h));
							} else light = a.baked.plane[hcell];
							m = shade_baked(m, light, a.baked.full_scale);
						}
					}
					if (!real_hit) m = shade_miss(f, ray.dz);
					if constexpr (BAKED) kept = blend_water_base(kept, m, a.water); // (the base is chosen and weighted already)
					else
					kept = blend_water(kept, m, a.water);
				}
				rgba = kept;
				real_hit = true;
			}
			ray.dz = lt.phase ? -ray.dz : ray.dz; // (the primary ray's, for the miss shade)
		}
		if constexpr (LSUM) { // (the colour once, behind every march, and only for a colour target; then the pixel under its sum)
			real_hit = lt.primary_hit;
			if (out != nullptr && real_hit) {
				uint32_t lit_rgba;
				if constexpr (BILINEAR) {
					cell_coords_of(lt.hx, lt.hy, qxh, qyh);
					lit_rgba = bilinear_pixel(qxh, qyh);
				} else lit_rgba = shade_hit(f, cmap[hcell]);
				rgba = shade_summed(lit_rgba, lm.acc & 0xffffu, (uint32_t)a.lsum.n);
			}
			ray.dz = lt.phase ? lt.dz : ray.dz; // (the primary ray's, for the miss shade)
		} else
		if constexpr (LIT) {
			if (lt.primary_hit) { // MISS, END and CAPPED shadow rays leave the pixel lit
				uint32_t lit_rgba = lt.rgba;
				if constexpr (DEFER && !BILINEAR) lit_rgba = shade_hit(f, cmap[hcell]);
				if constexpr (SHADE) { // ... at the weight of its diffuse level; a shadowed pixel keeps the ambient weight
					uint32_t w = a.sun.ambient;
					if (!real_hit) {
						if constexpr (BILINEAR) {
							cell_coords_of(lt.hx, lt.hy, qxh, qyh);
							w = shade_weight(a.sun.ambient, diffuse_level_bilinear(f, thr, bil_setup(qxh, qyh, f.map_w, f.map_h), a.sun.dir));
						} else {
							w = shade_weight(a.sun.ambient, diffuse_level_nearest<F32>(f, thr, hcell, a.sun.dir));
						}
					}
					rgba = shade_weighted(lit_rgba, w);
				} else
				rgba = real_hit ? shade_shadowed(lit_rgba, a.sun.ambient) : lit_rgba;
				real_hit = true;
			}
			ray.dz = lt.phase ? lt.dz : ray.dz; // (the primary ray's, for the miss shade)
		} else if constexpr (SHADE) { // (no shadow rays: every hit pixel at the weight of its level)
			if (real_hit) {
				uint32_t q;
				if constexpr (BILINEAR) {
					q = diffuse_level_bilinear(f, thr, bil_setup(qxh, qyh, f.map_w, f.map_h), a.sun.dir);
				} else q = diffuse_level_nearest<F32>(f, thr, hcell, a.sun.dir);
				rgba = shade_weighted(rgba, shade_weight(a.sun.ambient, q));
			}
		}
		if constexpr (BAKED && !MIRROR) { // (every hit pixel at the weight of its baked light; an alpha-0 hit cell's background too; MIRROR has weighted its own)
			if (real_hit) {
				uint32_t light;
				if constexpr (BILINEAR) light = baked_light_bilinear(a.baked.plane, bil_setup(qxh, qyh, f.map_w, f.map_h));
				else light = a.baked.plane[hcell];
				rgba = shade_baked(rgba, light, a.baked.full_scale);
			}
		}
		if constexpr (HAZE) { // (every hit pixel towards the haze colour by the table's byte at its range; an alpha-0 hit cell's background too)
			if (real_hit) {
				// (the ray's origin is made again here rather than held across the march, as store_geometry makes it)
				const DevRay o = make_ray<PROJ>(f, pid.px, pid.py);
				HMRM_RANGE_FROM(o, hqx, hqy, hz);
				rgba = blend_haze(rgba, a.haze, haze_index(a.haze, r));
			}
		}

		// (CELLS: a cell map has no pixel and counts no hits -- `rgba`, the miss shade and my_hit are dead there and compile to
		// nothing; the family's entry passes SegRules::interior = 1 for the record, the rule itself is shadow_entry's above)
		if (real_hit) my_hit = 1;
		else rgba = shade_miss(f, ray.dz);
		if constexpr (HAZE) { // (the sky as hazy as the farthest terrain: a scalar branch; capped rays are non-hits here too)
			if ((a.haze.flags & kHazeSky) != 0u && !real_hit) rgba = blend_haze(rgba, a.haze, a.haze.n - 1u);
		}
		if constexpr (SEG) { // an END ray is not a capped one: not counted, never HMRM_E_NOTERM
			sg.ended = my_cap != 0u && sg.ends;
			my_cap = sg.ended ? 0u : my_cap;
		}
		// (row and pitch are below 2^31, api.cpp: one 32 x 32 -> 64-bit multiply-add)
		if constexpr (LSUM) { // (the lane's pixel is made again from its number in the wave; each pointer test is a scalar branch)
			const PixelId me = pixel_of_tile_lane(f, rows, tiles_y, tile_x, gy, wave, (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)));
			if (out != nullptr) out[(uint64_t)(uint32_t)me.lrow * (uint32_t)out_stride_px + (uint32_t)me.px] = rgba;
			if (a.lsum.light != nullptr) {
				uint8_t *row = reinterpret_cast<uint8_t *>(a.lsum.light) + (uint64_t)(uint32_t)me.lrow * (uint64_t)a.lsum.light_stride;
				reinterpret_cast<uint16_t *>(row)[(uint32_t)me.px] = real_hit ? (uint16_t)lm.acc : (uint16_t)0xffffu;
			}
		} else
		if constexpr (SUM) { // (one 16-bit store per lane: hmrm.h fixes the alignment at 2 bytes, so a wave's row is not widened further)
			const PixelId me = pixel_of_tile_lane(f, rows, tiles_y, tile_x, gy, wave, (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)));
			uint8_t *row = reinterpret_cast<uint8_t *>(out) + (uint64_t)(uint32_t)me.lrow * (uint64_t)out_stride_px;
			reinterpret_cast<uint16_t *>(row)[(uint32_t)me.px] = (uint16_t)sm.acc;
		} else
		if constexpr (CELLS) {
			uint32_t v = real_hit ? 1u : (my_cap != 0u ? 2u : (sg.ended ? 3u : 0u)); // HMRM_RAY_*
			if ((a.cells.flags & kMapWeight) != 0u) {
				uint32_t q = 0u;
				if ((a.cells.flags & kMapDiffuse) != 0u && !real_hit) { // the level of the cell under its own direction
					const DevRay own = cell_ray_of<SAMP>(a.cells, f, thr, pid.px, pid.py);
					const double s[3] = {own.dx, own.dy, own.dz};
					if constexpr (BILINEAR) {
						double qxc, qyc;
						cell_coords_of(own.px, own.py, qxc, qyc);
						q = diffuse_level_bilinear(f, thr, bil_setup(qxc, qyc, f.map_w, f.map_h), s);
					} else {
						q = diffuse_level_nearest<F32>(f, thr, (unsigned)index_2d(a.cells.y0 + pid.py, f.map_w, a.cells.x0 + pid.px), s);
					}
				}
				v = cell_weight(a.cells, real_hit, q);
			}
			reinterpret_cast<uint8_t *>(out)[(uint64_t)(uint32_t)pid.lrow * (uint64_t)out_stride_px + (uint32_t)pid.px] = (uint8_t)v;
		} else
		if constexpr (GEOM) { // (a capped ray is no hit in any plane; its pixel is the miss shade, as in every frame)
			if (out != nullptr) out[(uint64_t)(uint32_t)pid.lrow * (uint32_t)out_stride_px + (uint32_t)pid.px] = rgba;
			store_geometry<PROJ>(f, a.geo, pid, real_hit, hcell, hqx, hqy, hz);
			if (a.geo.slope != nullptr) {
				Gradient g{0.0, 0.0};
				if (real_hit) {
					if constexpr (BILINEAR) g = gradient_bilinear(f, thr, bil_setup(qxh, qyh, f.map_w, f.map_h));
					else g = gradient_nearest<F32>(f, thr, hcell);
				}
				store_slope(a.geo, pid, real_hit, g.gx, g.gy);
			}
		} else
		if constexpr (RAYS) {
			const unsigned cy = hcell / (unsigned)f.map_w; // (gridx, gridy of hmap.cpp:1001-1004 from gridx + gridy * W)
			if constexpr (SEG) {
				store_batch_hit(a.batch, ray_index, real_hit, my_cap != 0u, hx, hy, hz, (int)(hcell - cy * (unsigned)f.map_w), (int)cy,
				                sg.d_record, (uint32_t)my_steps, rgba, sg.ended);
			} else
			store_batch_hit(a.batch, ray_index, real_hit, my_cap != 0u, hx, hy, hz, (int)(hcell - cy * (unsigned)f.map_w), (int)cy, d,
			                (uint32_t)my_steps, rgba);
		} else if constexpr (SUNLIT) { // (the lane's pixel is made again from its number in the wave, as LSUM's: not held across four marches)
			int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
			asm volatile("" : "+v"(ln));
			const PixelId me = pixel_of_tile_lane(f, rows, tiles_y, tile_x, gy, wave, ln);
			out[(uint64_t)(uint32_t)me.lrow * (uint32_t)out_stride_px + (uint32_t)me.px] = rgba;
		} else if constexpr (AA) aa_rgba = rgba;
		else out[(uint64_t)(uint32_t)pid.lrow * (uint32_t)out_stride_px + (uint32_t)pid.px] = rgba;
		if (STATS && st.steps_per_pixel)
			st.steps_per_pixel[(int64_t)pid.py * f.screen_w + pid.px] = diag.pixel_value(f, my_steps);
	}
	// (the sun-lit families make the lane's number again instead of holding it across their marches)
	if constexpr (AA && SEG)
		store_box_filtered(out, out_stride_px, f.aa_shift, (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)), pid.px, pid.lrow, pid.live, aa_rgba);
	else if constexpr (AA) store_box_filtered(out, out_stride_px, f.aa_shift, lane, pid.px, pid.lrow, pid.live, aa_rgba);
	// (SUM: capped rays are counted per ray, up to n per lane -- publish_counters' production path adds one per lane)
	if constexpr (LSUM) { // (likewise: the primary ray once and every shadow ray, up to 1 + n per lane)
		if ((lm.acc >> 16) != 0u) atomicAdd(&st.counters[2], (unsigned long long)(lm.acc >> 16));
	} else
	if constexpr (SUM) {
		if ((sm.acc >> 16) != 0u) atomicAdd(&st.counters[2], (unsigned long long)(sm.acc >> 16));
	} else
	publish_counters<STATS>(st, my_steps, my_hit, my_cap);
	diag.publish(st, f);
	return pid.tile_y;
}

} // namespace hmrm