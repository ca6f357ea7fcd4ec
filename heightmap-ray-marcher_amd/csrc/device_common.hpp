// device_common.hpp -- device helpers shared by the render kernels: ray
// generation (src/{Perspective,Spherical,Orthographic}.cpp GetRay), the slab test
// (src/AABB.cpp:49-77), pixel packing (main/hmap.cpp:139-154) and the sky shade
// (main/hmap.cpp:1041-1057).  Include only from .hip files compiled with
// -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frame.hpp"

#pragma clang fp contract(off)

namespace hmrm {

// ----------------------------------------------------------------- render ----
struct DevRay {
	double px, py, pz;
	double dx, dy, dz;
};

template <int PROJ>
__device__ __forceinline__ DevRay make_ray(const DevFrame &f, int px, int py) {
	DevRay r;
	if (PROJ == 2) {
		// Spherical.cpp:23-25; sin/cos come from the host tables
		const double sva = f.row_sin_va[py], cva = f.row_cos_va[py];
		const double cha = f.col_cos_ha[px], sha = f.col_sin_ha[px];
		r.px = f.cam[0]; r.py = f.cam[1]; r.pz = f.cam[2];
		r.dx = sva * cha;
		r.dy = sva * sha;
		r.dz = cva;
	} else {
		// hmap.cpp:985-988
		const double w = (double)px / (double)(f.screen_w - 1);
		const double h = (double)py / (double)(f.screen_h - 1);
		// upper_left + w*plane_right + h*plane_down  (Perspective.cpp:27, Orthographic.cpp:20)
		const double ox = (f.upper_left[0] + w * f.plane_right[0]) + h * f.plane_down[0];
		const double oy = (f.upper_left[1] + w * f.plane_right[1]) + h * f.plane_down[1];
		const double oz = (f.upper_left[2] + w * f.plane_right[2]) + h * f.plane_down[2];
		if (PROJ == 1) {
			const double vx = ox - f.cam[0], vy = oy - f.cam[1], vz = oz - f.cam[2];
			// glm::normalize: v * (1 / sqrt(dot(v,v))), dot = (x*x + y*y) + z*z
			const double tx = vx * vx, ty = vy * vy, tz = vz * vz;
			const double inv = 1.0 / __builtin_sqrt((tx + ty) + tz);
			r.px = f.cam[0]; r.py = f.cam[1]; r.pz = f.cam[2];
			r.dx = vx * inv;
			r.dy = vy * inv;
			r.dz = vz * inv;
		} else {
			r.px = ox; r.py = oy; r.pz = oz;
			r.dx = f.look[0]; r.dy = f.look[1]; r.dz = f.look[2];
		}
	}
	return r;
}

// Ray batches (hmrm_trace_rays; PROJ == 4 in the kernels, frame.hpp RayBatch): ray `index` of the batch, the caller's, used
// as given -- the reference's loop takes any Ray {pos, dir} (hmap.cpp:989-1038) and never normalises.
__device__ __forceinline__ DevRay batch_ray(const RayBatch &b, int64_t index) {
	const BatchRay *__restrict__ in = b.rays + index;
	DevRay r;
	r.px = in->pos[0]; r.py = in->pos[1]; r.pz = in->pos[2];
	r.dx = in->dir[0]; r.dy = in->dir[1]; r.dz = in->dir[2];
	return r;
}
// The record of a batch ray (hmrm.h hmrm_ray_hit): `hit` with the position and the cell at which hmap.cpp:1016 fired,
// `capped` for a ray stopped by the step cap (`rgba` is the miss shade then, like a miss).
__device__ __forceinline__ void store_batch_hit(const RayBatch &b, int64_t index, bool hit, bool capped, double x, double y,
                                                double z, int cell_x, int cell_y, double d, uint32_t steps, uint32_t rgba,
                                                bool ended = false) { // (ended: HMRM_RAY_END, segment batches only)
	BatchHit *__restrict__ out = b.hits + index;
	out->point[0] = hit ? x : 0.0;
	out->point[1] = hit ? y : 0.0;
	out->point[2] = hit ? z : 0.0;
	out->entry_d = d;
	out->steps = steps;
	out->cell_x = hit ? cell_x : -1;
	out->cell_y = hit ? cell_y : -1;
	__builtin_memcpy(out->rgba, &rgba, 4);
	out->status = hit ? 1u : (capped ? 2u : (ended ? 3u : 0u));
	out->reserved = 0u;
}

// The segment rules (frame.hpp SegRules; hmrm_trace_segments, hmrm_render_interior).  Strictly inside the box: all six
// comparisons true, NaN fails them; an origin exactly on a face is not inside.  (c1.y = -map_h * gw is the LOW end of y.)
__device__ __forceinline__ bool origin_strictly_inside(const DevRay &r, const DevFrame &f) {
	return f.c0[0] < r.px && r.px < f.c1[0] && f.c1[1] < r.py && r.py < f.c0[1] && f.c0[2] < r.pz && r.pz < f.c1[2];
}
// What a lane keeps for the rules (SEG in the kernels); empty in every other instantiation, which stay as they were.
template <bool SEG> struct SegState {};
template <> struct SegState<true> {
	double d_record = 0.0; // distance()'s own value, for the record
	int budget = 0;        // min(step cap, the ray's own limit)
	bool ends = false;     // running out of it is the ray's own end (HMRM_RAY_END), not the step cap
	bool ended = false;
};
// A ray's step budget under the rules: min(step cap, L), L = the smaller of the non-zero values among the batch's limit and
// the ray's own (0 = none).  *ends: running out of it is the ray's own end (L != 0 && L < step cap), not the step cap.
__device__ __forceinline__ int segment_budget(const SegRules &seg, int64_t index, int64_t step_cap, bool *ends) {
	const uint32_t own = seg.max_steps ? seg.max_steps[index] : 0u;
	const uint32_t l = seg.limit == 0u ? own : (own == 0u ? seg.limit : (own < seg.limit ? own : seg.limit));
	const int cap = step_cap > 0x7fffffff ? 0x7fffffff : (int)step_cap;
	*ends = l != 0u && (int64_t)l < (int64_t)cap;
	return *ends ? (int)l : cap;
}

// Sun shadows (frame.hpp SunRules; hmrm_render_lit, LIT in the kernels): what a lane keeps between its primary ray and its
// shadow ray; empty in every other instantiation, as SegState is.
template <bool LIT> struct LitState {};
template <> struct LitState<true> {
	int phase = 0;             // 0: the primary rays, 1: the shadow rays of the lanes that hit (the same for a whole wave)
	bool primary_hit = false;  // hmap.cpp:1016 fired for the primary ray
	uint32_t rgba = 0;         // ... and this is its pixel
	double hx = 0.0, hy = 0.0; // where it fired (int_point's x and y) ...
	double t = 0.0;            // ... and the threshold z was compared with there (set once the march loop has ended)
	double dz = 0.0;           // the primary ray's dir.z (the miss shade wants it after the shadow march)
};
// R, G and B of a shadowed pixel: (c * ambient + 127) / 255 in integers; A stays 255.  ambient = 255 gives c back.
__device__ __forceinline__ uint32_t shade_shadowed(uint32_t rgba, uint32_t ambient) {
	const uint32_t r = ((rgba & 255u) * ambient + 127u) / 255u;
	const uint32_t g = (((rgba >> 8) & 255u) * ambient + 127u) / 255u;
	const uint32_t b = (((rgba >> 16) & 255u) * ambient + 127u) / 255u;
	return r | (g << 8) | (b << 16) | (rgba & 0xff000000u);
}

// Water frames (frame.hpp WaterRules; hmrm_render_water, MIRROR in the kernels): the stored pixel of a water lane -- the base b,
// the primary pixel or the water's own colour, and the mirror ray's pixel m mixed per channel, (b * (255 - r) + m * r + 127) / 255
// in integers; A stays 255.  r = 0 gives b back, r = 255 gives m.
// (blend_water_base: the mix alone, over a base the caller has chosen -- and, under baked light, weighted -- already.)
__device__ __forceinline__ uint32_t water_base(uint32_t primary, const WaterRules &w) {
	return (w.flags & kWaterOwnColor) != 0u ? w.own : primary;
}
__device__ __forceinline__ uint32_t blend_water_base(uint32_t b, uint32_t mirror, const WaterRules &w) {
	const uint32_t r = w.reflectivity, k = 255u - r;
	const uint32_t c0 = ((b & 255u) * k + (mirror & 255u) * r + 127u) / 255u;
	const uint32_t c1 = (((b >> 8) & 255u) * k + ((mirror >> 8) & 255u) * r + 127u) / 255u;
	const uint32_t c2 = (((b >> 16) & 255u) * k + ((mirror >> 16) & 255u) * r + 127u) / 255u;
	return c0 | (c1 << 8) | (c2 << 16) | 0xff000000u;
}
__device__ __forceinline__ uint32_t blend_water(uint32_t primary, uint32_t mirror, const WaterRules &w) {
	const uint32_t b = (w.flags & kWaterOwnColor) != 0u ? w.own : primary;
	const uint32_t r = w.reflectivity, k = 255u - r;
	const uint32_t c0 = ((b & 255u) * k + (mirror & 255u) * r + 127u) / 255u;
	const uint32_t c1 = (((b >> 8) & 255u) * k + ((mirror >> 8) & 255u) * r + 127u) / 255u;
	const uint32_t c2 = (((b >> 16) & 255u) * k + ((mirror >> 16) & 255u) * r + 127u) / 255u;
	return c0 | (c1 << 8) | (c2 << 16) | 0xff000000u;
}
// Haze frames (hmrm_render_haze; frame.hpp HazeRules).  The table's entry of a range r: u = (r - start) * scale -- one subtract,
// one multiply -- then n - 1 for u >= n - 1, else the truncation of a positive u, else 0 (a NaN u fails both tests).  And the pixel
// under the entry's byte f: the water's blend with the haze colour for a mirror pixel and f for the reflectivity.
__device__ __forceinline__ uint32_t haze_index(const HazeRules &h, double r) {
	const double u = (r - h.start) * h.scale;
	const uint32_t last = h.n - 1u;
	return u >= (double)last ? last : (u > 0.0 ? (uint32_t)(int)u : 0u);
}
__device__ __forceinline__ uint32_t blend_haze(uint32_t rgba, const HazeRules &h, uint32_t index) {
	const uint32_t amount = h.table[index];
	return blend_water_base(rgba, h.color, WaterRules{0.0, 0.0, 0u, amount, 0u, 0u});
}

// The diffuse level q in 0..255 of a surface with the gradient (gx, gy) -- gy along the rows, which grow towards decreasing
// world y -- under the sun direction s as given: n = (-gx, gy, 1), q = round(255 * clamp(n.s / (|n| |s|), 0, 1)), every
// operation a plain IEEE double one in the order of hmrm.h, NaN -> 0.  Nothing is special-cased.
__device__ __forceinline__ uint32_t diffuse_level(double gx, double gy, const double (&s)[3]) {
	const double nx = -gx, ny = gy;
	const double dot = (nx * s[0] + ny * s[1]) + s[2];
	const double len = __builtin_sqrt(((nx * nx + ny * ny) + 1.0) * ((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]));
	double k = dot / len;
	k = k > 0.0 ? (k < 1.0 ? k : 1.0) : 0.0;
	return (uint32_t)(k * 255.0 + 0.5);
}
// The gradient (gx, gy) of the hit cell `cell` for the nearest-cell modes: central differences of the threshold table the march
// reads (F32: its float copy, widened), one-sided on the map's border, 0 along a side of one cell.  The one expression behind
// the diffuse level and the slope plane of a geometry frame -- written as a macro that declares gx and gy in its user's scope,
// not as a function: a helper between diffuse_level_nearest and these loads, whichever way it handed the two doubles back (by
// reference, by value, to a callable; inlining forced or not), made the compiler order the existing kernels' instructions
// differently, and those kernels keep theirs.
#define HMRM_GRADIENT_NEAREST(F32, f, thr, cell)                                                                    \
	const float *__restrict__ thr32 = reinterpret_cast<const float *>(thr);                                         \
	const int w = f.map_w, h = f.map_h;                                                                             \
	const int cy = (int)(cell / (unsigned)w), cx = (int)(cell - (unsigned)cy * (unsigned)w);                        \
	const int xm = max(cx - 1, 0), xp = min(cx + 1, w - 1), ym = max(cy - 1, 0), yp = min(cy + 1, h - 1);           \
	const size_t row = (size_t)cy * (size_t)w, ixm = row + (size_t)xm, ixp = row + (size_t)xp;                      \
	const size_t iym = (size_t)ym * (size_t)w + (size_t)cx, iyp = (size_t)yp * (size_t)w + (size_t)cx;              \
	const double txm = F32 ? (double)thr32[ixm] : thr[ixm], txp = F32 ? (double)thr32[ixp] : thr[ixp];              \
	const double tym = F32 ? (double)thr32[iym] : thr[iym], typ = F32 ? (double)thr32[iyp] : thr[iyp];              \
	const double gx = xp > xm ? (txp - txm) / ((double)(xp - xm) * f.grid_width) : 0.0;                             \
	const double gy = yp > ym ? (typ - tym) / ((double)(yp - ym) * f.grid_width) : 0.0
struct Gradient { double gx, gy; };
template <bool F32>
__device__ __forceinline__ Gradient gradient_nearest(const DevFrame &f, const double *__restrict__ thr, unsigned cell) {
	HMRM_GRADIENT_NEAREST(F32, f, thr, cell);
	return Gradient{gx, gy};
}
// ... and the diffuse level of that cell.
template <bool F32>
__device__ __forceinline__ uint32_t diffuse_level_nearest(const DevFrame &f, const double *__restrict__ thr, unsigned cell,
                                                          const double (&s)[3]) {
	HMRM_GRADIENT_NEAREST(F32, f, thr, cell);
	return diffuse_level(gx, gy, s);
}
// The weight w in 0..255 of a hit pixel that is not shadowed, from its level, and the pixel under a weight:
// (c * w + 127) / 255 per channel (w = ambient for a shadowed pixel; w = 255 gives c back).
__device__ __forceinline__ uint32_t shade_weight(uint32_t ambient, uint32_t q) {
	return ambient + ((255u - ambient) * q + 127u) / 255u;
}
__device__ __forceinline__ uint32_t shade_weighted(uint32_t rgba, uint32_t w) { return shade_shadowed(rgba, w); }

// AABB.cpp:49-77, axis order x,y,z, same comparisons (NaN => every test false).
__device__ __forceinline__ double slab_distance(const DevRay &r, const DevFrame &f) {
	const double inf = __builtin_huge_val();
	double lo = -inf, hi = inf;
	const double ro[3] = {r.px, r.py, r.pz};
	const double rd[3] = {r.dx, r.dy, r.dz};
#pragma unroll
	for (int i = 0; i < 3; ++i) {
		double dim_lo = (f.c0[i] - ro[i]) / rd[i];
		double dim_hi = (f.c1[i] - ro[i]) / rd[i];
		if (dim_lo > dim_hi) {
			const double t = dim_lo;
			dim_lo = dim_hi;
			dim_hi = t;
		}
		if (dim_hi < lo || dim_lo > hi) return inf;
		if (dim_lo > lo) lo = dim_lo;
		if (dim_hi < hi) hi = dim_hi;
	}
	return (lo > hi) ? inf : lo;
}
// The shadow ray of a lane whose primary ray hit: from the surface above the hit point towards the sun ...
__device__ __forceinline__ DevRay shadow_ray(const LitState<true> &lt, const SunRules &sun) {
	DevRay r;
	r.px = lt.hx; r.py = lt.hy; r.pz = lt.t;
	r.dx = sun.dir[0]; r.dy = sun.dir[1]; r.dz = sun.dir[2];
	return r;
}
// ... and the d it enters the loop with: +0.0 when its origin is strictly inside the box (the interior rule, always on for
// shadow rays), else distance()'s own value -- an origin on or above max_height, t >= c1.z, is not inside and goes through
// distance() as written.
__device__ __forceinline__ double shadow_entry(const DevRay &r, const DevFrame &f) {
	return origin_strictly_inside(r, f) ? 0.0 : slab_distance(r, f);
}

// Cell maps (hmrm_cell_map; frame.hpp CellRules): the ray of cell (cx, cy) whose threshold is t -- from `lift` above the
// surface at the cell's centre towards the target, a direction used as given or a point -- hmrm.h's operations in hmrm.h's order.
__device__ __forceinline__ DevRay cell_ray(const CellRules &c, const DevFrame &f, int cx, int cy, double t) {
	DevRay r;
	r.px = ((double)cx + 0.5) * f.grid_width;
	r.py = -(((double)cy + 0.5) * f.grid_width);
	r.pz = t + c.lift;
	const bool point = (c.flags & kMapTowardsPoint) != 0u; // (uniform)
	r.dx = point ? c.target[0] - r.px : c.target[0];
	r.dy = point ? c.target[1] - r.py : c.target[1];
	r.dz = point ? c.target[2] - r.pz : c.target[2];
	return r;
}
// ... and the byte of a cell whose ray ended with `status` (HMRM_RAY_*): the status itself, or with HMRM_MAP_WEIGHT the weight
// of hmrm_render_shaded -- ambient for a shadowed cell (status HIT), else 255 or, HMRM_MAP_DIFFUSE, that of the level q.
__device__ __forceinline__ uint32_t cell_weight(const CellRules &c, bool shadowed, uint32_t q) {
	return shadowed ? c.ambient : ((c.flags & kMapDiffuse) != 0u ? shade_weight(c.ambient, q) : 255u);
}
// Accumulated cell maps (hmrm_cell_map_sum; frame.hpp CellSums): what a lane keeps across its passes; empty in every other
// instantiation, as SegState is.  `rules` is the launch's CellRules with the current target in place; it and `k` are the same
// for a whole wave.
template <bool SUM> struct SumState {};
template <> struct SumState<true> {
	CellRules rules;
	int k = 0;         // the pass = the target's index
	uint32_t acc = 0;  // v_0 + .. + v_{k-1} (at most 256 * 255) + 2^16 * the passes of this lane that the step cap stopped (at most 256)
};
// Target k of the list, for every lane of the wave: the index is made a scalar so that the three doubles are scalar loads.
__device__ __forceinline__ void sum_target(const CellSums &sums, int k, CellRules *rules) {
	const double *__restrict__ t = sums.targets + 3 * (size_t)(unsigned)__builtin_amdgcn_readfirstlane(k);
	rules->target[0] = t[0];
	rules->target[1] = t[1];
	rules->target[2] = t[2];
}

// Accumulated lit frames (hmrm_render_lit_sum; frame.hpp LightSum): what a lane keeps across its shadow passes beside LitState's
// hit point; empty in every other instantiation, as SegState is.  `k` is the same for a whole wave.
template <bool LSUM> struct LitSumState {};
template <> struct LitSumState<true> {
	int k = 0;        // the shadow pass = the direction's index
	uint32_t acc = 0; // w_0 + .. + w_{k-1} (at most 256 * 255) + 2^16 * the rays of this lane that the step cap stopped (at most 257)
};
// Direction k of the list, for every lane of the wave: the index is made a scalar so that the three doubles are scalar loads.
__device__ __forceinline__ void sum_direction(const LightSum &ls, int k, double (&s)[3]) {
	const double *__restrict__ t = ls.dirs + 3 * (size_t)(unsigned)__builtin_amdgcn_readfirstlane(k);
	s[0] = t[0];
	s[1] = t[1];
	s[2] = t[2];
}
// The pixel of a hit under the sum S of its n weights: (c * S + (255 n) / 2) / (255 n) per channel in integers, A stays 255.
// c * S <= 255 * 65280 < 2^24; the divisor is the same for the whole launch.
// n copies of one weight w give (c * w + 127) / 255, the pixel of that weight alone, for every n.  Proof: let c * w = 255 q + r,
// 0 <= r <= 254; that pixel is q + [r >= 128].  With S = n w the numerator is 255 n q + (n r + floor(255 n / 2)), so the quotient
// is q + floor((n r + floor(127.5 n)) / (255 n)).  For r >= 128: n r + floor(127.5 n) >= 128 n + 127 n = 255 n, and with
// r <= 254 it is below 254 n + 127.5 n + 1 <= 510 n: the floor is 1.  For r <= 127: n r + floor(127.5 n) <= 254.5 n < 255 n:
// the floor is 0.
__device__ __forceinline__ uint32_t shade_summed(uint32_t rgba, uint32_t sum, uint32_t n) {
	const uint32_t den = 255u * n, half = den / 2u;
	const uint32_t r = ((rgba & 255u) * sum + half) / den;
	const uint32_t g = (((rgba >> 8) & 255u) * sum + half) / den;
	const uint32_t b = (((rgba >> 16) & 255u) * sum + half) / den;
	return r | (g << 8) | (b << 16) | (rgba & 0xff000000u);
}
// The pixel of a hit under the baked light L of full scale D (hmrm_render_baked): min(255, (c * L + D / 2) / D) per channel in
// unsigned 32-bit integers, A stays 255.  c * L + D / 2 <= 255 * 65535 + 32767 < 2^24; the divisor is the same for the whole
// launch.  L = D gives c back: (c D + floor(D / 2)) / D = c, the remainder being below D.
__device__ __forceinline__ uint32_t shade_baked(uint32_t rgba, uint32_t light, uint32_t full_scale) {
	const uint32_t half = full_scale / 2u;
	const uint32_t r = min(255u, ((rgba & 255u) * light + half) / full_scale);
	const uint32_t g = min(255u, (((rgba >> 8) & 255u) * light + half) / full_scale);
	const uint32_t b = min(255u, (((rgba >> 16) & 255u) * light + half) / full_scale);
	return r | (g << 8) | (b << 16) | (rgba & 0xff000000u);
}

// Relative error of the hardware reciprocal.  MEASURED on gfx950 (tools/rcp_accuracy.py over 1.6e11 inputs: the
// leading 32 mantissa bits exhaustively in six binades, hashed mantissas / signs / exponents 2^-1000..2^1000, and the
// product n * rcp(d) against n / d; profiles/r03_rcp_accuracy.txt): |rcp(x) * x - 1| <= 2^-24.36 everywhere, the same
// in every binade -- a 24-bit result, as AMD's ISA guides say ("(2**29) ULP").  tests/test_parity_gpu.py
// re-measures a slice in every GPU run and fails if the device at hand exceeds kRcpRelErr.
constexpr double kRcpRelErr = 0x1p-24;
// ... and the margin every ordering decision below keeps between two approximate slab parameters, as a fraction of
// the largest of them: 16 x kRcpRelErr.  (Needed: 2 x (kRcpRelErr + 2^-53), one error bar per operand.)
constexpr double kSlabMargin = 16.0 * kRcpRelErr; // 2^-20

// Cheap classification of a ray against the box from approximate reciprocals (one v_rcp_f64 and two multiplies per
// axis).  With every direction component and every product of moderate magnitude (2^-500..2^500: no overflow, no
// underflow, no zero) an approximate slab parameter is t' = t (1 + e), |e| <= kRcpRelErr + 2^-53, of the exact real
// quotient t: same sign, and two of them that differ by more than kSlabMargin * max|t'| are ordered like the exact
// quotients -- hence, rounding being monotonic, their correctly rounded values (the reference's) are ordered the same
// way or equal.  So a MISS is proven when
//   (A) min_i hi'_i < 0          => the exact hi is negative => d <= hi < 0 or d = inf;
//   (B) max_i lo'_i exceeds min_i hi'_i by more than the error bars (2^-12 of the largest: far more) => the exact
//       intervals do not overlap => distance() returns inf (early or at its last line).
// Either way the pixel is a miss (AABB.cpp:33-40); nothing else about d is used for a miss.  "Don't know" (take the
// exact path) whenever a direction component or a parameter is zero, tiny, huge or not finite.
// The same approximate parameters also settle most HITS with one division instead of six.  For finite
// quotients distance() returns lo = max_i min(t0_i, t1_i) when lo <= hi = min_i max(t0_i, t1_i), else inf
// (its early returns are that comparison on a prefix of the axes).  If the approximate values show, by more than
// the margin, (a) that the intervals overlap, (b) which axis holds the maximum of the lower ends and (c) which of its
// two quotients is the lower end, then the exact result is that ONE quotient, correctly rounded (where two rounded
// lower ends coincide the value is the same whichever axis supplied it).  Rays through an edge or a corner of the
// box (lower ends within 2^-20 of each other) stay undecided and take the reference's six divisions.
// Returns 0: undecided, take slab_distance(); 1: surely a miss (only when `may_report_miss`; d is not set);
// 2: *d is distance()'s value, bit for bit (it may be negative: the caller's d < 0 test applies as usual).
__device__ __forceinline__ int slab_classify(const DevRay &r, const DevFrame &f, bool may_report_miss, double *d) {
	const double ro[3] = {r.px, r.py, r.pz};
	const double rd[3] = {r.dx, r.dy, r.dz};
	const double inf = __builtin_huge_val();
	double LO = -inf, LO2 = -inf, HI = inf, mag = 0.0, least = inf;
	double num = 0.0, den = 1.0, span = 0.0; // of the axis that holds LO: entry numerator, direction, |t0' - t1'|
	bool fine = true;
#pragma unroll
	for (int i = 0; i < 3; ++i) {
		fine = fine & (__builtin_fabs(rd[i]) > 0x1p-500) & (__builtin_fabs(rd[i]) < 0x1p500);
		const double inv = __builtin_amdgcn_rcp(rd[i]);
		const double n0 = f.c0[i] - ro[i], n1 = f.c1[i] - ro[i];
		const double t0 = n0 * inv, t1 = n1 * inv;
		const bool first = t0 < t1;
		const double lo_i = first ? t0 : t1, hi_i = first ? t1 : t0;
		const bool bigger = lo_i > LO;
		LO2 = bigger ? LO : __builtin_fmax(LO2, lo_i);
		num = bigger ? (first ? n0 : n1) : num;
		den = bigger ? rd[i] : den;
		span = bigger ? hi_i - lo_i : span;
		LO = bigger ? lo_i : LO;
		HI = __builtin_fmin(HI, hi_i);
		const double a0 = __builtin_fabs(t0), a1 = __builtin_fabs(t1);
		mag = __builtin_fmax(mag, __builtin_fmax(a0, a1));
		least = __builtin_fmin(least, __builtin_fmin(a0, a1)); // (NaN operands drop out here and are caught by mag / fine below)
		fine = fine & !__builtin_isunordered(t0, t1);
	}
	// every parameter finite and of moderate magnitude: the relative-error model above holds for each of them
	if (!(fine & (mag < 0x1p500) & (least > 0x1p-500))) return 0;
	if (may_report_miss && (HI < 0.0 || (LO - HI) > mag * 0x1p-12)) return 1;
	const double margin = mag * kSlabMargin;
	if ((HI - LO) > margin && (LO - LO2) > margin && span > margin) {
		*d = num / den;
		return 2;
	}
	return 0;
}

// Cheaper still, from sign and exponent bits alone: on some axis the whole box lies on one
// side of the origin (c0-o and c1-o have the same sign) and the ray points the other way.
// With all three numbers finite, non-zero and of moderate exponent (2^-500 .. 2^499) both
// exact quotients are finite, non-zero and negative, so that axis' dim_hi < 0 and
// distance() (AABB.cpp:49-77) ends in inf or in an entry distance <= hi < 0: a miss.
// PROJ 1 / 2: the origin is the camera for every ray, so the two box-side tests are done once per frame on the
// host (camera.cpp, DevFrame::box_side) and a ray only adds the sign and the exponent of its direction.
template <int PROJ>
__device__ __forceinline__ bool slab_points_away(const DevRay &r, const DevFrame &f) {
	const double ro[3] = {r.px, r.py, r.pz};
	const double rd[3] = {r.dx, r.dy, r.dz};
	bool away = false;
	if (PROJ == 1 || PROJ == 2) { // (orthographic frames and ray batches, PROJ 4: an origin per ray, the tests below)
#pragma unroll
		for (int i = 0; i < 3; ++i) {
			if (!f.box_side_known[i]) continue; // (uniform)
			const uint32_t hd = (uint32_t)((unsigned long long)__double_as_longlong(rd[i]) >> 32);
			away = away | ((((hd >> 20) & 0x7ffu) - 523u) < 1000u & ((f.box_side[i] ^ hd) >> 31) != 0u);
		}
		return away;
	}
#pragma unroll
	for (int i = 0; i < 3; ++i) {
		const uint32_t h0 = (uint32_t)((unsigned long long)__double_as_longlong(f.c0[i] - ro[i]) >> 32);
		const uint32_t h1 = (uint32_t)((unsigned long long)__double_as_longlong(f.c1[i] - ro[i]) >> 32);
		const uint32_t hd = (uint32_t)((unsigned long long)__double_as_longlong(rd[i]) >> 32);
		const bool moderate = (((h0 >> 20) & 0x7ffu) - 523u) < 1000u && (((h1 >> 20) & 0x7ffu) - 523u) < 1000u &&
		                      (((hd >> 20) & 0x7ffu) - 523u) < 1000u;
		away = away || (moderate && ((h0 ^ h1) >> 31) == 0u && ((h0 ^ hd) >> 31) != 0u);
	}
	return away;
}

__device__ __forceinline__ uint32_t pack_rgba(uint32_t r, uint32_t g, uint32_t b) {
	return r | (g << 8) | (b << 16) | 0xff000000u; // bytes R,G,B,A=255 (hmap.cpp:150-153)
}

// Clamp<double>(v,0,255) then floor then (Uint8), hmap.cpp:1049-1051, as written there (the literal kernel's)
__device__ __forceinline__ uint32_t sky_channel_literal(double v) {
	if (v < 0.0) v = 0.0;
	else if (v > 255.0) v = 255.0;
	return (uint32_t)(int)__builtin_floor(v);
}
// The same for the values shade_miss produces: v is
// a sum of non-negative terms (a weight times z or z*z with z > 0, plus a colour byte), never NaN and never
// negative, possibly +inf.  So the lower clamp never acts, min(v, 255) is the upper one, and the truncating
// cast equals the floor.
__device__ __forceinline__ uint32_t sky_channel(double v) {
	return (uint32_t)__builtin_fmin(v, 255.0);
}

struct StatsOut {
	unsigned long long *counters; // [0] steps [1] hits [2] capped
	uint32_t *steps_per_pixel;    // screen_w*screen_h or null
	double *entry_d;              // screen_w*screen_h or null
};


// A frame record fetched from device memory at a wave-uniform address (view batches: render_views.hip, render.hip), as a copy made
// of 32-bit words.  Every field then comes out of scalar loads, the background's bytes too: the scalar unit of gfx950 has no byte
// loads, and read through a reference to the device record f.bg[i] became vector loads.  The compiler keeps no
// copy in memory: the words live in scalar registers like a kernel argument's.
typedef uint32_t __attribute__((may_alias)) FrameWord;
__device__ __forceinline__ void copy_frame_words(DevFrame *dst, const DevFrame *__restrict__ src) {
	static_assert(sizeof(DevFrame) % sizeof(uint32_t) == 0 && alignof(DevFrame) >= alignof(uint32_t), "whole words");
#pragma unroll
	for (unsigned i = 0; i < sizeof(DevFrame) / sizeof(uint32_t); ++i)
		reinterpret_cast<FrameWord *>(dst)[i] = reinterpret_cast<const FrameWord *>(src)[i];
}

// Miss shade: hmap.cpp:1041-1057.
__device__ __forceinline__ uint32_t shade_miss(const DevFrame &f, double dz) {
	if (dz > 0.0) {
		const double zz = dz * dz; // std::pow(z,2) == z*z under -std=c++98 (__builtin_powi)
		const double r_ = 220.0 * zz + (double)f.bg[0];
		const double g_ = 240.0 * zz + (double)f.bg[1];
		const double b_ = 255.0 * dz + (double)f.bg[2];
		return pack_rgba(sky_channel(r_), sky_channel(g_), sky_channel(b_));
	}
	return pack_rgba(f.bg[0], f.bg[1], f.bg[2]);
}

// Hit shade: hmap.cpp:1018-1031 (alpha 0 -> background colour).
__device__ __forceinline__ uint32_t shade_hit(const DevFrame &f, uint32_t texel) {
	return ((texel >> 24) == 0) ? pack_rgba(f.bg[0], f.bg[1], f.bg[2]) : (texel | 0xff000000u);
}

// Which pixel a lane owns.  A wave covers kWaveW x kWaveH pixels (kWaveW * kWaveH = 64), a
// workgroup a kWavesX x kWavesY arrangement of waves (default 2 x 2 = 256 threads).
#ifndef HMRM_WAVE_W
#define HMRM_WAVE_W 8
#endif
#ifndef HMRM_WAVES_X
#define HMRM_WAVES_X 1
#endif
#ifndef HMRM_WAVES_Y
#define HMRM_WAVES_Y 2
#endif
constexpr int kWaveW = HMRM_WAVE_W, kWaveH = 64 / HMRM_WAVE_W;
constexpr int kWavesX = HMRM_WAVES_X, kWavesY = HMRM_WAVES_Y;          // waves per workgroup
constexpr int kBlockThreads = 64 * kWavesX * kWavesY;
constexpr int kTileW = kWavesX * kWaveW, kTileH = kWavesY * kWaveH;
static_assert(kBatchW == kWaveW, "a wave's 64 lanes hold 64 consecutive rays of a batch (frame.hpp RayBatch)");
struct PixelId {
	int px, py, lrow;
	int tile_y; // tile row of the launch this workgroup renders (wave-uniform)
	bool live;
};
// The row map of a launch that renders the whole frame in frame order: no bands, no launch order, no calibration records.
__host__ __device__ __forceinline__ RowMap whole_frame_rows(const DevFrame &f) {
	return RowMap{0, f.screen_h, 0, 0, 1, {0x7fffffff, 0x7fffffff, 0x7fffffff}, {0, 0, 0, 0}, nullptr};
}
// Frame row of local row `lrow` of the launch's output (contiguous strip or cyclic bands).
__device__ __forceinline__ int frame_row_of(const RowMap &rows, int lrow) {
	if (rows.band_rows > 0) {
		const int band = lrow / rows.band_rows, within = lrow - band * rows.band_rows;
		return (rows.band_index + band * rows.band_count) * rows.band_rows + within;
	}
	return rows.row_begin + lrow;
}

// Pixel of lane `lane` of wave `wave` of the workgroup-sized tile (tile_x, grid row gy).
__device__ __forceinline__ PixelId pixel_of_tile_lane(const DevFrame &f, const RowMap &rows, int tiles_y, int tile_x, unsigned gy,
                                                      int wave, int lane) {
	// Grid of tiles: x = tile column (fastest, so workgroups still start row by row), y (+ z for
	// frames taller than 32768 tile rows) = grid row; grid rows are handed to tile rows piece by piece so that the
	// costliest tile rows start first (RowMap::seg_first / seg_delta).  Scalar work, no integer division per wave.
	const bool row_exists = gy < (unsigned)tiles_y; // (the last z-slab may be partly empty)
	int delta = rows.seg_delta[0];
#pragma unroll
	for (int k = 1; k < kOrderSegs; ++k) delta = gy >= (unsigned)rows.seg_first[k - 1] ? rows.seg_delta[k] : delta;
	unsigned ty = gy + (unsigned)delta;
	if (ty >= (unsigned)tiles_y) ty -= (unsigned)tiles_y;
	const int tile_y = (int)ty;
	PixelId p;
	p.tile_y = row_exists ? tile_y : -1;
	p.px = tile_x * kTileW + (wave % kWavesX) * kWaveW + (lane % kWaveW);
	p.lrow = tile_y * kTileH + (wave / kWavesX) * kWaveH + (lane / kWaveW);
	p.py = frame_row_of(rows, p.lrow);
	p.live = row_exists && p.px < f.screen_w && p.lrow < rows.local_rows && p.py < f.screen_h;
	return p;
}
// ... of the launch's own workgroup (one workgroup per tile: blockIdx is the tile)
__device__ __forceinline__ PixelId pixel_of_lane(const DevFrame &f, const RowMap &rows, int tiles_y) {
	return pixel_of_tile_lane(f, rows, tiles_y, (int)blockIdx.x, blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6),
	                          (int)(threadIdx.x & 63));
}

// Wave-reduce and publish the per-launch counters {steps, hits, capped}.
template <bool STATS>
__device__ __forceinline__ void publish_counters(const StatsOut &st, unsigned long long steps,
                                                 uint32_t hit, uint32_t cap) {
	if (STATS) {
		unsigned long long s = steps, h = hit, c = cap;
		for (int off = 32; off > 0; off >>= 1) {
			s += __shfl_xor(s, off);
			h += __shfl_xor(h, off);
			c += __shfl_xor(c, off);
		}
		if ((threadIdx.x & 63) == 0) {
			if (s) atomicAdd(&st.counters[0], s);
			if (h) atomicAdd(&st.counters[1], h);
			if (c) atomicAdd(&st.counters[2], c);
		}
	} else if (cap) {
		atomicAdd(&st.counters[2], 1ull);
	}
}

// Epilogue of the antialiased instantiations (hmrm_render_aa, hmrm.h HMRM_AA): the launch marches the super frame of
// n x n samples per output pixel, n = 1 << shift <= 8, and each n x n block of samples -- always inside one wave's 8 x 8
// pixels, lane = kWaveW * row + column, blocks aligned to n -- is box-filtered across the wave's lanes.  R | B << 16 and
// G are summed in 16-bit fields (64 x 255 fits) by xor shuffles over the lane bits of x, then of y (the masks are
// constants, the shift is uniform); the sums are rounded half up; the block's first lane writes the pixel to
// out[(lrow >> shift) * stride + (px >> shift)].  Every lane of the wave calls this: a block is wholly live or wholly
// dead (api.cpp makes the super frame's sides multiples of n), the shuffles of a dead block carry values nobody writes.
__device__ __forceinline__ void store_box_filtered(uint32_t *__restrict__ out, int64_t out_stride_px, int shift, int lane,
                                                   int px, int lrow, bool live, uint32_t rgba) {
	static_assert(kWaveW == 8 && kWaveH == 8, "an n x n block (n <= 8) must lie inside one wave's pixels");
	uint32_t rb = rgba & 0x00ff00ffu, g = (rgba >> 8) & 0xffu;
#pragma unroll
	for (int k = 0; k < 3; ++k) { // lane bits of x
		if (shift > k) {
			rb += (uint32_t)__shfl_xor((int)rb, 1 << k);
			g += (uint32_t)__shfl_xor((int)g, 1 << k);
		}
	}
#pragma unroll
	for (int k = 0; k < 3; ++k) { // lane bits of y
		if (shift > k) {
			rb += (uint32_t)__shfl_xor((int)rb, kWaveW << k);
			g += (uint32_t)__shfl_xor((int)g, kWaveW << k);
		}
	}
	const int s2 = 2 * shift;
	const uint32_t half = (1u << s2) >> 1;
	const uint32_t r = ((rb & 0xffffu) + half) >> s2, b = ((rb >> 16) + half) >> s2, gg = (g + half) >> s2;
	const int corner = ((1 << shift) - 1) * (kWaveW + 1); // lane bits that must be zero in a block's first lane
	if (live && (lane & corner) == 0)
		out[(uint64_t)(uint32_t)(lrow >> shift) * (uint64_t)out_stride_px + (uint32_t)(px >> shift)] = pack_rgba(r, gg, b);
}

// Epilogue of the geometry frames (hmrm_render_geometry; frame.hpp GeomPlanes): the cell and range planes of a lane whose ray
// hit in cell `cell` at int_point = (x, y, z), or did not hit.  The pointers are kernel arguments: each test is a scalar branch.
// The ray's origin is made again here rather than held across the march (it is per pixel only for orthographic frames); the
// range is hmrm.h's: sqrt((ex * ex + ey * ey) + ez * ez) in doubles, correctly rounded, then rounded to float.
// (The range as a macro that declares ex, ey, ez and r in its user's scope: store_geometry and the haze frames' epilogue
// (march.hpp) share the very expression, and render_geometry.hip keeps its instructions.)
#define HMRM_RANGE_FROM(o, x, y, z)                                             \
	const double ex = (x) - (o).px, ey = (y) - (o).py, ez = (z) - (o).pz;       \
	const double r = __builtin_sqrt((ex * ex + ey * ey) + ez * ez)
template <int PROJ>
__device__ __forceinline__ void store_geometry(const DevFrame &f, const GeomPlanes &geo, const PixelId &pid, bool hit, unsigned cell,
                                               double x, double y, double z) {
	if (geo.cell != nullptr) geo.cell[(uint64_t)(uint32_t)pid.lrow * (uint64_t)geo.cell_stride + (uint32_t)pid.px] = hit ? (int32_t)cell : -1;
	if (geo.range != nullptr) {
		const DevRay o = make_ray<PROJ>(f, pid.px, pid.py);
		HMRM_RANGE_FROM(o, x, y, z);
		geo.range[(uint64_t)(uint32_t)pid.lrow * (uint64_t)geo.range_stride + (uint32_t)pid.px] = hit ? (float)r : __builtin_huge_valf();
	}
}
// ... and the slope plane: one 8-byte store per lane.
__device__ __forceinline__ void store_slope(const GeomPlanes &geo, const PixelId &pid, bool hit, double gx, double gy) {
	const float2 v = hit ? make_float2((float)gx, (float)gy) : make_float2(0.0f, 0.0f);
	reinterpret_cast<float2 *>(geo.slope)[(uint64_t)(uint32_t)pid.lrow * (uint64_t)geo.slope_stride + (uint32_t)pid.px] = v;
}

} // namespace hmrm
