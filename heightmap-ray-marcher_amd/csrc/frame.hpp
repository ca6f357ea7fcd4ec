// frame.hpp -- the per-frame record the host hands to the render kernel.
//
// The reference rebuilds an ImagePlane object and the two box corners every
// frame on the host (main/hmap.cpp:661-672, :952-974) and the pixel loop reads
// them.  Here the same quantities are computed once per frame on the host (with
// glibc's sin/cos/tan, so the bits match the reference's libm calls) and passed
// BY VALUE as a kernel argument: they live in SGPRs / the scalar cache, no
// per-pixel memory traffic.
#pragma once
#include <stdint.h>

namespace hmrm {

struct DevFrame {
	// framebuffer (main/hmap.cpp:31-32)
	int32_t screen_w, screen_h;
	int32_t projection;          // 1 perspective, 2 spherical, 3 orthographic (:104-106)
	// heightmap / colormap dimensions (:54-55,:60-61; equal by :503-515)
	int32_t map_w, map_h;
	uint8_t bg[4];               // bg_r,bg_g,bg_b,255 (:110-112)
	// Ray origin for perspective/spherical = cam_pos (Perspective.cpp:26, Spherical.cpp:21)
	double cam[3];
	// Perspective.cpp:16-22 / Orthographic.cpp:13-16
	double upper_left[3], plane_right[3], plane_down[3];
	// Orthographic.cpp:5 (float-rounded look), used as ray.dir
	double look[3];
	// Spherical.cpp:23-25 is separable: sin/cos(va) depend on the row only,
	// sin/cos(ha) on the column only.  Host-built tables (glibc), device memory.
	const double *col_cos_ha, *col_sin_ha;   // screen_w entries
	const double *row_sin_va, *row_cos_va;   // screen_h entries
	// box corners (hmap.cpp:968-974)
	double c0[3], c1[3];
	double grid_width;           // :65
	double nudge;                // grid_width * 0.01 (:998)
	double step_dist;            // :68
	// ---- derived, bit-preserving helpers (not in the reference) ----
	double inv_grid_width;       // fl(1/grid_width); exact iff grid_pow2 != 0
	int32_t grid_pow2;           // grid_width is a normal power of two: x/gw == x*(1/gw) exactly
	int32_t grid_mode;           // 0: grid_width == 1.0, 1: power of two, 2: general
	double thr_max;              // max over cells of heightmap_buf[i] + c0.z (informational; the kernel uses the pyramid's top plane)
	int64_t step_cap;            // guard for the reference's unbounded while(true) (:1000)
	// window-maximum pyramid over the thr table (render_fast.hip): level l holds the maximum
	// of thr (NaN ignored: z < NaN never hits) over S x S-cell windows, S = 4, 8, 16, .. 256,
	// placed every S/2 cells; floats rounded up.  One buffer of kMipLevels + 1 planes of
	// 1 << mip_plane_shift floats: window (ix, iy) of level l is element
	// (l << mip_plane_shift) + iy * mip_row + ix -- every level uses level 0's row pitch, so the
	// kernel needs no per-level table -- and plane kMipLevels holds one element, the whole-map
	// bound (thr_max rounded up).
	const float *mipbuf;
	const float *mipbuf_bil;     // the same pyramid over the 3x3-dilated table (bilinear quality mode); the record kernel
	                             // (nearest sampling only) finds its WindowRecord table here instead -- see below
	int32_t mip_row;             // row pitch of every plane (windows per row of level 0)
	int32_t mip_plane_shift;     // log2 of the plane pitch
	// Perspective / spherical: every ray starts at cam, so on which side of the origin the box lies per axis
	// is a property of the frame (device_common.hpp slab_points_away): box_side[i] = high word of
	// c0[i] - cam[i] when c0[i] - cam[i] and c1[i] - cam[i] are finite, non-zero, of moderate exponent and
	// of one sign (its sign bit is the side), else 0 with box_side_known[i] = 0.
	// (Kept inside the struct's old size on purpose.  The struct is the kernel argument; a field appended at its
	// end that the miss shade reads -- the background as doubles -- made EVERY wave wait for one more 64-byte
	// line of it at start-up, the compiler hoists scalar loads to the entry: +3...5 % on the all-terrain frames.)
	uint32_t box_side[3];
	int32_t box_side_known[3];
	int32_t diag_mode;           // tools only: what the instrumented kernel writes per pixel
	int32_t sampling;            // 0 nearest cell (the reference), 1 bilinear quality mode, 2 nearest cell with float thresholds
	int32_t min_level;           // finest pyramid level worth an attempt (api_launch.cpp, from min_window)
	int32_t min_window;          // ... as a window size in cells (camera.cpp)
	int32_t finest_pause;        // extra groups marched after a refused attempt at that level (camera.cpp)
	int32_t aa_shift;            // antialiasing (hmrm_render_aa): log2 n of the n x n samples box-filtered into one output
	                             // pixel, 0 = off.  Set per launch by api_frames.cpp, not part of the cached record; the kernels read
	                             // it only in their antialiased instantiations (device_common.hpp store_box_filtered).
};

// Window sizes S = 4 * 2^(kLevelStep*l) cells, placed every S/2 cells.  kLevelStep 1 (the build): S = 4, 8, 16, 32,
// 64, 128, 256 -- a ray moves two levels at a time (4, 16, 64, 256) until it has made a few jumps and then one at a time
// (kAdaptAfter below); kLevelStep 2: only S = 4, 16, 64, 256 exist (round 2's pyramid, kept for A/B runs).
#ifndef HMRM_LEVEL_STEP
#define HMRM_LEVEL_STEP 1
#endif
constexpr int kLevelStep = HMRM_LEVEL_STEP;
#ifndef HMRM_MIP_LEVELS
#define HMRM_MIP_LEVELS (HMRM_LEVEL_STEP == 2 ? 4 : 7)
#endif
constexpr int kMipLevels = HMRM_MIP_LEVELS;
// Windows of S cells are placed every S/2 cells on the levels below kDenseFrom (a ray always finds a window with at
// least S/2 cells of room ahead) and every S/4 cells from that level on (at least 3S/4 of room: longer jumps for four
// times the entries, which the coarse levels can afford and the 4-cell level, one entry per cell then, cannot --
// C3, the one BASELINE config that uses it, got slower).  HMRM_DENSE_FROM: 0 = every level dense, 99 = none.
#ifndef HMRM_DENSE_FROM
#define HMRM_DENSE_FROM 1
#endif
constexpr int kDenseFrom = HMRM_DENSE_FROM;
#if defined(__HIPCC__)
__host__ __device__
#endif
constexpr int win_strides(int l) { return l < kDenseFrom ? 2 : 4; }                        // strides per window
#if defined(__HIPCC__)
__host__ __device__
#endif
constexpr int win_cells(int l) { return 4 << (kLevelStep * l); }                             // S
#if defined(__HIPCC__)
__host__ __device__
#endif
constexpr int mip_stride_shift(int l) { return kLevelStep * l + (l < kDenseFrom ? 1 : 0); } // log2(S / strides per window)
// Level state byte (leap_common.hpp level_state): mip_stride_shift in bits 0-4, win_strides - 1 in bits 5-6.  The whole map,
// level kMipLevels, is the one window of its plane: shift 28 and 4 strides, a window of 1 << 30 cells that no level treats specially.
#if defined(__HIPCC__)
__host__ __device__
#endif
constexpr uint32_t level_state_byte(int l) {
	return l >= kMipLevels ? (28u | (3u << 5)) : ((uint32_t)mip_stride_shift(l) | ((uint32_t)(win_strides(l) - 1) << 5));
}
#if defined(__HIPCC__)
__host__ __device__
#endif
constexpr uint64_t level_state_table() {
	uint64_t k = 0;
	for (int l = 0; l <= kMipLevels; ++l) k |= (uint64_t)level_state_byte(l) << (8 * l);
	return k;
}
static_assert(kMipLevels + 1 <= 8 && mip_stride_shift(kMipLevels - 1) < 28, "level state: one byte per level, eight levels");
// (the sweep: every level's byte against the formulas above, at whatever HMRM_LEVEL_STEP / HMRM_DENSE_FROM this is compiled with)
constexpr bool level_state_table_ok() {
	for (int l = 0; l <= kMipLevels; ++l) {
		const uint32_t b = (uint32_t)(level_state_table() >> (8 * l)) & 0xffu;
		const int hs = (int)(b & 31u), back = (int)(b >> 5);
		if (l < kMipLevels && (hs != mip_stride_shift(l) || back + 1 != win_strides(l) || ((back + 1) << hs) != win_cells(l))) return false;
		if (l == kMipLevels && (hs != 28 || ((back + 1) << hs) != (1 << 30))) return false;
	}
	return true;
}
static_assert(level_state_table_ok(), "level state bytes disagree with win_strides / win_cells / mip_stride_shift");

// Per-ray adaptive level spacing (pyramids with windows doubling per level, HMRM_LEVEL_STEP=1): a ray moves two
// levels at a time -- windows of 4, 16, 64, 256 cells, which is what ordinary rays want (fewer level changes) --
// until it has made more than HMRM_ADAPT_AFTER successful jumps; from then on one level at a time, so that the few
// long rays skimming the terrain (the launch's tail) can use the 8-, 32- and 128-cell windows in between: where a
// 16-cell window clears the ray and the 64-cell one does not, the 32-cell one often does and the jump doubles.
// 0 = off (every ray one level at a time).  Performance only: any level sequence gives the same pixels.
#ifndef HMRM_ADAPT_AFTER
#define HMRM_ADAPT_AFTER 8
#endif
constexpr int kAdaptAfter = (kLevelStep == 1) ? HMRM_ADAPT_AFTER : 0;
constexpr bool kAdaptive = kAdaptAfter > 0;
// The level moves of the policy (march.hpp): levels per move -- two while the ray is young, `young_left` = kAdaptAfter - its
// jumps so far not negative -- and the targets of a move up and of a move down by `drop` levels, clamped at the coarsest
// pyramid level and at the frame's finest; the whole map (level kMipLevels) always steps down to the coarsest level.
#if defined(__HIPCC__)
__host__ __device__
#endif
constexpr int level_step(int young_left) { return kAdaptive ? 2 + (young_left >> 31) : 1; }
#if defined(__HIPCC__)
__host__ __device__
#endif
constexpr int level_coarser(int lev, int lstep) { return lev + lstep > kMipLevels - 1 ? kMipLevels - 1 : lev + lstep; }
#if defined(__HIPCC__)
__host__ __device__
#endif
constexpr int level_finer(int lev, int drop, int minlev) {
	return lev == kMipLevels ? kMipLevels - 1 : (lev - drop > minlev ? lev - drop : minlev);
}
// Element of window (ix, iy) inside a plane (row-major with level 0's pitch; 8 x 4-window tiles per
// 128-byte line were tried and change nothing, profiles/r02_experiments.txt).
#if defined(__HIPCC__)
__host__ __device__
#endif
inline unsigned mip_index(int ix, int iy, int pitch) { return (unsigned)(iy * pitch + ix); }

// Window records (march.hpp, the record kernel; built by render_fast.hip): one per window of level kRecLevel (16 x 16 cells, one every 4
// cells, row pitch rec_row(map_w)).  `max2` is the window's maximum with its kRecCells highest cells left out (rounded up
// to float like the pyramid, NaN ignored), xs / ys the places of those cells inside the window, one byte each (255: slot
// not used -- fewer than kRecCells cells stand above max2).  A ray at or above max2 crosses the window without a load if
// its path misses the recorded cells: maps whose windows all hold a few tall cells (needles on a plateau) defeat a flat
// maximum, not this.  Performance only: the kernel that uses the records renders the same pixels.
constexpr int kRecLevel = 2;
constexpr int kRecCells = 8;
struct WindowRecord {
	float max2;
	uint32_t spare0;
	uint32_t xs[2], ys[2];
	uint32_t spare1[2];
};
static_assert(sizeof(WindowRecord) == 32, "two 16-byte loads");
static_assert(kRecLevel >= kDenseFrom && kLevelStep == 1, "the record level's windows: 16 cells, every 4");
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int rec_row(int map_w) { return (map_w + 3) >> 2; }

// Which framebuffer rows a launch covers and where they land in the output.
struct RowMap {
	int32_t row_begin;     // contiguous mode: first global row
	int32_t local_rows;    // rows held by the output buffer
	int32_t band_rows;     // 0 = contiguous; else cyclic bands of this many rows
	int32_t band_index, band_count;
	// Launch order (api_launch.cpp choose_tile_order): the grid's rows are handed out to tile rows in up to kOrderSegs
	// contiguous pieces.  Grid row j belongs to the last piece k with j >= seg_first[k] (seg_first[0] = 0 is
	// implicit; unused pieces have seg_first = INT32_MAX) and renders tile row (j + seg_delta[k]) mod tile rows --
	// the last piece may wrap around the end of the frame.  Together the pieces cover every tile row once.
	int32_t seg_first[3];  // pieces 1..3
	int32_t seg_delta[4];  // pieces 0..3
	// Calibration launch (api_launch.cpp, launch order from measurement): when not null, every wave folds its duration, and
	// a tile row's first wave its start time (s_memrealtime ticks, 10 ns), into the row's record: kMeasureStride words
	// per tile row (march_frame.hpp k_render_fast).  Scheduling aid only.
	unsigned long long *measure;
};
constexpr int kMeasureStride = 33;
constexpr int kOrderSegs = 4;

// The struct is the first kernel argument of every render kernel; what reads past its old end costs every wave a
// scalar-cache line at start-up (see box_side above).  A field that is needed goes into a slot that is free.
static_assert(sizeof(DevFrame) == 352,"DevFrame must not grow");

// ---- ray batches (hmrm_trace_rays, hmrm.h): caller-supplied rays through the same march, PROJ == 4 in the kernels ----
// Mirrors of hmrm_ray / hmrm_ray_hit (api_queries.cpp asserts the sizes agree), and what a launch is handed beside the
// DevFrame -- extra arguments of the batch kernels' own __global__ entry points (render_rays.hip, render.hip), so
// that neither DevFrame nor the frame kernels' argument lists change.  The DevFrame of a batch has no camera:
// projection = 4, the plane fields zero, and the batch laid out as a "frame" kWaveW (8) pixels wide and
// ceil(n / 8) rows tall -- ray 8 * py + px belongs to pixel (px, py), so a wave's 64 lanes hold 64 consecutive rays
// and their 48-byte loads / 56-byte stores cover contiguous memory.
struct BatchRay { double pos[3], dir[3]; };
struct BatchHit {
	double point[3];
	double entry_d;
	uint32_t steps;
	int32_t cell_x, cell_y;
	uint8_t rgba[4];
	uint32_t status;    // 0 miss, 1 hit, 2 stopped by the step cap (HMRM_RAY_*)
	uint32_t reserved;
};
static_assert(sizeof(BatchRay) == 48 && sizeof(BatchHit) == 56, "hmrm_ray / hmrm_ray_hit");
struct RayBatch {
	const BatchRay *rays;
	BatchHit *hits;
	int64_t n;
};
constexpr int kBatchW = 8; // (= device_common.hpp kWaveW, asserted there)

// ---- segment rules (hmrm_trace_segments, hmrm_render_interior; SEG in the kernels) ----
// interior: a ray whose origin lies strictly inside the box (c0.x < x < c1.x, c1.y < y < c0.y, c0.z < z < c1.z; NaN fails)
// runs the body of hmap.cpp:989-1057 as if distance() had returned +0.0 -- the reference makes it a miss (AABB.cpp:37-39).
// limit / max_steps[i]: the ray ends after L height loads (hmap.cpp:1013) when the L-th did not hit, L = the smaller of the
// non-zero values of the two (0 = none); inside the grid then: HMRM_RAY_END, unless L >= the step cap (CAPPED as before).
// An extra argument of the segment kernels' own __global__ entry points, like RayBatch: nothing existing changes.
struct SegRules {
	const uint32_t *max_steps; // per ray (batches), device memory, may be null
	uint32_t limit;            // for every ray
	uint32_t interior;         // != 0: the interior rule is on
};

// ---- sun shadows (hmrm_render_lit; LIT in the kernels) ----
// Every pixel whose primary ray HIT casts a shadow ray from (P.x, P.y, t) -- P the hit point, t the threshold the hitting load
// compared z with -- along `dir` (as given, not normalised): a segment ray under the interior rule with step_dist and the limit
// max_steps (0 = none).  A pixel whose shadow ray hits keeps (c * ambient + 127) / 255 of its R, G and B.  The primary rays'
// own rules travel in a SegRules beside it.  An extra argument of the lit kernels' own __global__ entry points, like SegRules.
struct SunRules {
	double dir[3];
	double step_dist;
	uint32_t max_steps;
	uint32_t ambient; // 0..255
};

// ---- cell maps (hmrm_cell_map; PROJ == 5 in the kernels) ----
// A lane owns one map cell of the rect instead of a pixel: cell (x0 + px, y0 + py) of the launch's "frame", which is the
// rect (DevFrame::screen_w x screen_h = the rect's w x h, no camera).  Its ray starts `lift` above the cell's threshold, at the
// cell's centre, towards `target` (flags & 1: a point, else a direction as given) -- a segment ray under the interior rule with
// DevFrame::step_dist and the limit max_steps -- and the lane writes ONE BYTE: the ray's status, or (flags & 2) the weight of
// hmrm_render_shaded.  flags are hmrm.h's HMRM_MAP_*.  An extra argument of the cell kernels' own __global__ entry points,
// like SegRules.
struct CellRules {
	double target[3];
	double lift;
	int32_t x0, y0;
	uint32_t max_steps;
	uint32_t flags;
	uint32_t ambient; // 0..255
};
constexpr uint32_t kMapTowardsPoint = 1u, kMapWeight = 2u, kMapDiffuse = 4u, kMapNoShadows = 8u;

// ---- accumulated cell maps (hmrm_cell_map_sum; PROJ == 5 with SUM in the kernels) ----
// The cell kernels' march run n times per lane over a list of targets (device memory, n x 3 doubles, the same for every lane:
// the index is wave-uniform) -- CellRules::target is not looked at, target k takes its place for pass k -- with the lane's
// values summed in a register and ONE 16-bit word stored at the end: n * 255 <= 65280 for n <= 256.  A sibling of CellRules in
// the sum kernels' own __global__ entry points: k_cell_map's arguments do not change.
struct CellSums {
	const double *targets;
	int32_t n; // 1 .. 256
};
constexpr int kMaxSumTargets = 256;

// ---- geometry frames (hmrm_render_geometry; GEOM in the kernels) ----
// What the march knows about a pixel besides its colour, stored by the same launch: the hit cell gridx + gridy * W (-1: no
// hit), the distance from the ray's origin to int_point as a float (+inf: no hit), and the surface gradient (gx, gy) of
// hmrm_render_shaded's level as two floats (+0, +0: no hit).  Every pointer may be null -- that plane is not written; so may
// the kernel's colour target, and the colour is not fetched then.  Strides count ELEMENTS per local row: int32s, floats,
// pairs of floats.  An extra argument of the geometry kernels' own __global__ entry points, like SegRules.
struct GeomPlanes {
	int32_t *cell;
	float *range;
	float *slope; // pairs, 8-byte aligned
	int64_t cell_stride, range_stride, slope_stride;
};

// ---- accumulated lit frames (hmrm_render_lit_sum; LSUM in the kernels) ----
// The lit kernels' shadow march run n times per hit pixel over a list of directions (device memory, n x 3 doubles, the same for
// every lane: the index is wave-uniform) -- SunRules::dir is not looked at, direction k takes its place for pass k -- with the
// pixel's weights w_k of hmrm_render_shaded under `flags` (HMRM_SHADE_*) summed in a register: S <= 255 n <= 65280.  One pixel
// at the weight S / (255 n) is stored at the end, and / or S itself as a 16-bit word at (char *)light + row * light_stride +
// 2 * column (0xFFFF: no hit).  `light` may be null, and so may the kernel's colour target: the colour is not fetched then.  A
// sibling of SunRules in the sum kernels' own __global__ entry points: k_render_lit's arguments do not change.
struct LightSum {
	const double *dirs;
	uint16_t *light;
	int64_t light_stride; // bytes per local row, even
	int32_t n;            // 1 .. 256
	uint32_t flags;       // kShadeDiffuse | kShadeNoShadows (march_dispatch.hpp)
};
constexpr int kMaxSumDirs = 256;

// ---- baked-light frames (hmrm_render_baked; BAKED in the kernels) ----
// The scene's light plane (hmrm_scene_set_light, hmrm_scene_bake_light): map_w x map_h native uint16, rows packed like the
// threshold table, and its full scale D in 1 .. 65535.  A pixel whose primary ray hit keeps (c * L + D / 2) / D of its R, G and
// B, at most 255: L the plane's word of the hit cell, or -- bilinear sampling -- the four neighbours' words mixed like the colour.
// An extra argument of the baked kernels' own __global__ entry points, like SegRules.
struct BakedLight {
	const uint16_t *plane;
	uint32_t full_scale;
};

// ---- water frames (hmrm_render_water; MIRROR in the kernels) ----
// Every pixel whose primary ray HIT with t <= level -- t the threshold the hitting load compared z with, as in SunRules -- casts a
// mirror ray from (P.x, P.y, t) along the primary ray's direction with dir.z negated: a segment ray under the interior rule with
// step_dist and the limit max_steps (0 = none).  Its pixel m -- the hit cell's colour, or the miss shade of its own dir.z -- is
// blended into the base b, the primary pixel or `own` with kWaterOwnColor: (b * (255 - r) + m * r + 127) / 255 per channel.  The
// primary rays' own rules travel in a SegRules beside it.  An extra argument of the water kernels' own __global__ entry points,
// like SegRules.
struct WaterRules {
	double level;
	double step_dist;
	uint32_t max_steps;
	uint32_t reflectivity; // r, 0..255
	uint32_t own;          // R | G << 8 | B << 16, with kWaterOwnColor in `flags`
	uint32_t flags;        // kWaterOwnColor or 0
};
// (r and the colour packed into one word, a scalar register less, made the compiler take a scratch slot in 30 of the 63
// instantiations instead of 9: DESIGN.md 5.20)
constexpr uint32_t kWaterOwnColor = 2u; // (= hmrm.h HMRM_WATER_OWN_COLOR)
// The sun-lit water frame (hmrm_render_water_lit; SUNLIT in the kernels) takes its sun in a SunRules beside the WaterRules and
// hmrm_render_shaded's two flags in `flags`, above the water's own: read at run time, the same for the whole launch.
constexpr uint32_t kWaterSunDiffuse = 0x100u, kWaterSunNoShadows = 0x200u;

// ---- haze frames (hmrm_render_haze; HAZE in the kernels) ----
// Every pixel whose primary ray HIT is blended towards `color` by the byte of `table` (device memory, n entries) at its range:
// r = sqrt((ex * ex + ey * ey) + ez * ez) in doubles, e = int_point - the ray's origin -- the geometry frame's range before its
// rounding to float -- u = (r - start) * scale, entry n - 1 for u >= n - 1, else (int)u for u > 0, else 0 (NaN: 0); the blend is
// the water's, (c * (255 - f) + h * f + 127) / 255 per channel.  With kHazeSky the pixels that did not hit take entry n - 1.  The
// primary rays' own rules travel in a SegRules beside it.  An extra argument of the haze kernels' own __global__ entry points,
// like SegRules.
struct HazeRules {
	const uint8_t *table;
	double start, scale;
	uint32_t n;     // 1 .. 4096
	uint32_t color; // R | G << 8 | B << 16
	uint32_t flags; // kHazeSky or 0
};
constexpr uint32_t kHazeSky = 2u; // (= hmrm.h HMRM_HAZE_SKY)
constexpr int kMaxHazeEntries = 4096;

// Host: fill everything except the table pointers / thr_max / step_cap.
// Also fills the spherical tables (host arrays of screen_w / screen_h doubles) when
// projection == 2 and the pointers are not null.
struct HostCamera {
	int32_t width, height, projection;
	uint8_t bg_r, bg_g, bg_b, sampling;
	double hfov, hang, vang, pos[3], ortho_width, step_dist;
};

void build_frame(const HostCamera &cam, int32_t map_w, int32_t map_h,
                 double min_height, double max_height, double grid_width,
                 DevFrame *out,
                 double *col_cos_ha, double *col_sin_ha,   // width entries each (spherical) or null
                 double *row_sin_va, double *row_cos_va);  // height entries each (spherical) or null

// The part of build_frame that needs no camera (camera.cpp): map size, box corners (hmap.cpp:968-974), nudge (:998),
// step_dist (:68) and the grid_width helpers.  A ray batch's DevFrame is a zeroed one plus these (api_queries.cpp).
void fill_scene_fields(int32_t map_w, int32_t map_h, double min_height, double max_height, double grid_width,
                       double step_dist, DevFrame *out);

// The separable halves of Spherical::GetRay (src/Spherical.cpp:18-25), entries [begin, end): cos / sin of ha per
// column (depend on hang, hfov, width), sin / cos of va per row (depend on vang, hfov, width, height).
void fill_col_tables(const HostCamera &cam, int32_t begin, int32_t end, double *col_cos_ha, double *col_sin_ha);
void fill_row_tables(const HostCamera &cam, int32_t begin, int32_t end, double *row_sin_va, double *row_cos_va);

// Scheduling aid, approximate arithmetic: for every block of `rows_per_sample` screen rows the
// longest in-box ray length (in steps) over a few sample columns of the block's middle row.
// out has ceil(screen_h / rows_per_sample) entries.  Tables as filled by build_frame.
void estimate_row_costs(const DevFrame &f, const double *col_cos_ha, const double *col_sin_ha,
                        const double *row_sin_va, const double *row_cos_va, int rows_per_sample, float *out);

} // namespace hmrm
