// march_family.hpp -- which march a unit instantiates, as one type: Family<TAG, PROJ, GWM, LEAP, SAMP>.  The tag names what the
// family turns on and the arguments it brings (TAG::Args, from frame.hpp); Family adds the four values the launch dispatches on
// (march_dispatch.hpp) and every constant derived from them that decides which code of march.hpp's render_wave_tile exists.
// A new family is a tag here and its `if constexpr` statements there.
#pragma once
#include "frame.hpp"

namespace hmrm {

namespace {

#ifndef HMRM_GROUP
#define HMRM_GROUP 4
#endif
constexpr int kGroup = HMRM_GROUP; // U: positions per speculative group of the production kernel
// ... and of the plain-groups instantiation (LEAP = false: no leaps, every height load of the reference is executed --
// what the scene's probe picks on content that admits no jumps, and the kernel SURVEY 8(d)'s byte roofline is defined
// for).  That kernel waits for its gathers 70 % of the time at 17 % VALU busy (profiles/r05_C3_group_rocprof.txt): more
// loads in flight per lane pay until the registers cost resident waves -- C3 2.61 ms with 4, 2.37 with 6, 2.57 with 8
// (profiles/r05_raw/group_len_ab.txt).  Deciding the hit test from a float copy of the table, doubles only where that is
// unsafe, halves the bytes and changes little: the gathers are bound by lanes, not bytes (r05_experiments.txt section 4).
#ifndef HMRM_GROUP_PLAIN
#define HMRM_GROUP_PLAIN 6
#endif
constexpr int kGroupPlain = HMRM_GROUP_PLAIN;
// ... and of the record kernel
#ifndef HMRM_GROUP_REC
#define HMRM_GROUP_REC 6
#endif
constexpr int kGroupRec = HMRM_GROUP_REC;
// Geometry frames (GEOM below), for A/B builds of render_geometry.hip: HMRM_GEOM_CHAIN 1 keeps the hit point the way the ray
// batches do (a select chain over the group's positions into three doubles held across the loop) instead of KEEP_P's re-add;
// HMRM_GEOM_CARRY 0 reads the level state off the level at every attempt instead of carrying it.  The defaults are what the
// registers decided: DESIGN.md 5.16.
#ifndef HMRM_GEOM_CHAIN
#define HMRM_GEOM_CHAIN 0
#endif
#ifndef HMRM_GEOM_CARRY
#define HMRM_GEOM_CARRY 0
#endif
constexpr bool kGeomChain = HMRM_GEOM_CHAIN != 0, kGeomCarry = HMRM_GEOM_CARRY != 0;
// Haze frames (HAZE below), for A/B builds of render_haze.hip and render_haze_aa.hip: HMRM_HAZE_CHAIN and HMRM_HAZE_CARRY as the
// geometry frames' two; HMRM_HAZE_DEFER 1 fetches the colour behind the loop in every instantiation, as GEOM does, 0 leaves the
// interior family's choice.  The defaults are what the registers decided: DESIGN.md 5.23.
#ifndef HMRM_HAZE_CHAIN
#define HMRM_HAZE_CHAIN 0
#endif
#ifndef HMRM_HAZE_CARRY
#define HMRM_HAZE_CARRY 0
#endif
#ifndef HMRM_HAZE_DEFER
#define HMRM_HAZE_DEFER 1
#endif
constexpr bool kHazeChain = HMRM_HAZE_CHAIN != 0, kHazeCarry = HMRM_HAZE_CARRY != 0, kHazeDefer = HMRM_HAZE_DEFER != 0;

} // namespace

// ---- the tags: the default with everything off, and one per family that turns on only what it needs ----
// Every feature is written in render_wave_tile as `if constexpr` statements beside the others' own, so that the families that do
// not have it keep their instructions.
// Frames (k_render_fast, march_frame.hpp): a camera's frame, one pixel per lane.  FramesOf<STATS, AA> is that kernel's own pair:
// STATS: the instrumented instantiation (leap_diag.hpp), which also reports every ray's d and exact step count.
// AA: the antialiased epilogue (device_common.hpp store_box_filtered; render_fast_aa.hip and, Antialiased<> below, the sun-lit and
// baked-light units' counterparts).  It comes after the LIT / SHADE epilogues -- a sample is lit and shaded on its own, then
// filtered -- and outside `if (pid.live)`: every lane of the wave reaches it together, whatever the lanes did in the LIT loop,
// whose ballot only the live lanes take part in.
struct Frames {
	static constexpr bool STATS = false, AA = false, SEG = false, LIT = false, SHADE = false, SUM = false, GEOM = false, LSUM = false,
	                      BAKED = false, MIRROR = false, SUNLIT = false, HAZE = false;
	struct Args {};
};
template <bool STATS_, bool AA_> struct FramesOf : Frames {
	static constexpr bool STATS = STATS_, AA = AA_;
};
template <class TAG> struct Antialiased : TAG {
	static constexpr bool AA = true;
};
// Rays (PROJ 4, render_rays.hip; hmrm_trace_rays, frame.hpp RayBatch): a batch of caller-supplied rays -- the lane's ray is loaded
// from `batch`, not made from a camera, and instead of a pixel the lane writes its hmrm_ray_hit record, which wants distance()'s
// value for misses too and the ray's exact step count: the two things the instrumented instantiation computes (COUNT below),
// without its diagnostics or its wave-wide counters.  The tile's `out` is not used then.
struct Rays : Frames {
	struct Args { const RayBatch &batch; };
};
// SEG (Segments: PROJ 4, render_segments.hip, hmrm_trace_segments; Interior: render_interior.hip, hmrm_render_interior): the two
// segment rules of frame.hpp SegRules -- a ray whose origin is strictly inside the box enters it at d = +0.0 instead of missing,
// and a ray ends after its own number of height loads (HMRM_RAY_END).  The loop needs nothing new: it is position based and each
// lane has its budget.
struct Segments : Frames {
	static constexpr bool SEG = true;
	struct Args { const RayBatch &batch; const SegRules &seg; };
};
struct Interior : Frames {
	static constexpr bool SEG = true;
	struct Args { const SegRules &seg; };
};
// LIT (render_lit.hip; hmrm_render_lit, frame.hpp SunRules; implies SEG): sun shadows.  "Entry, then the march loop" runs a second
// time for the wave: a lane whose primary ray hit keeps its pixel and marches its shadow ray -- a segment ray under the interior
// rule from (P.x, P.y, t) towards the sun -- through the SAME loop; the other lanes sit the second pass out.  Nothing per pixel
// goes through memory between the two.  The per-lane struct is empty unless LIT (device_common.hpp LitState).
// SHADE (render_shaded.hip, render_lit_shaded.hip; hmrm_render_shaded; implies SEG): diffuse sun shading.  An epilogue: a lane
// whose primary ray hit -- and, LIT, whose shadow ray did not -- computes its diffuse level from the threshold table
// (device_common.hpp diffuse_level) and keeps a weighted pixel; `sun` brings the direction and the ambient level.  Across the loop
// it keeps the hit's cell index (nearest-cell modes: hcell, which every family keeps for the colour) or the hit point (bilinear:
// LitState's, or hqx / hqy, which the leap kernels keep for the colour too).  (LIT: computing the level at the phase switch instead
// and carrying it through the shadow march in the saved pixel's alpha byte holds no cell index, but the compiler then keeps more
// across the march, not less: DESIGN.md 5.12.)
template <bool LIT_, bool SHADE_> struct Sun : Frames {
	static constexpr bool SEG = true, LIT = LIT_, SHADE = SHADE_;
	struct Args { const SegRules &seg; const SunRules &sun; };
};
using Lit = Sun<true, false>;
using Shaded = Sun<false, true>;
using LitShaded = Sun<true, true>;
// Cells (PROJ 5, render_cells.hip; hmrm_cell_map, frame.hpp CellRules; needs SEG): a cell map.  The "frame" is the rect, a lane owns
// one map cell, a wave 8 x 8 of them; the lane's ray is made from the cell index and the cell's own entry of `thr`
// (device_common.hpp cell_ray), enters the loop like a shadow ray (shadow_entry: the interior rule is always on), and the epilogue
// stores ONE BYTE -- the ray's status, or the weight of SHADE's arithmetic -- through `out`, which points at bytes then
// (`out_stride_px` counts bytes).  HMRM_MAP_NO_SHADOWS gives every lane d = inf: the wave skips the loop.  The ray is made again in
// the epilogue rather than held across the march.
struct Cells : Frames {
	static constexpr bool SEG = true;
	struct Args { const SegRules &seg; const CellRules &cells; };
};
// SUM (render_cell_sums.hip; hmrm_cell_map_sum, frame.hpp CellSums; needs PROJ 5): an accumulated cell map.  LIT's "entry, then the
// march loop, once more" generalised: the wave runs it once per target of a wave-uniform list, the lane folds each pass's value --
// k_cell_map's byte for that target, or 1 for a ray that did not hit -- into a register, and the epilogue stores ONE 16-bit WORD
// through `out` (`out_stride_px` counts bytes).  Capped rays are counted per pass.
struct CellSum : Frames {
	static constexpr bool SEG = true, SUM = true;
	struct Args { const SegRules &seg; const CellRules &cells; const CellSums &sums; };
};
// GEOM (render_geometry.hip; hmrm_render_geometry, frame.hpp GeomPlanes; implies SEG): a geometry frame.  An epilogue: beside the
// pixel the lane stores its hit cell, the distance from its ray's origin to int_point and the surface gradient SHADE takes its level
// from, each through a pointer of `geo` that may be null -- and so may `out`: the colour is not fetched then.  A lane that hit
// leaves the loop with int_point in x, y, z (KEEP_P's re-add, with z stepped like x and y) and with hcell; the ray's origin is made
// again in the epilogue.
struct Geometry : Frames {
	static constexpr bool SEG = true, GEOM = true;
	struct Args { const SegRules &seg; const GeomPlanes &geo; };
};
// LSUM (render_lit_sum.hip; hmrm_render_lit_sum, frame.hpp LightSum; needs LIT, without SHADE -- whether the weights are diffuse is
// a run-time flag): an accumulated lit frame, LIT and SUM joined.  The primary march runs once; then the wave runs "entry, then the
// march loop" once per direction of a wave-uniform list for the lanes whose primary ray hit, each of which folds the pass's weight
// -- hmrm_render_shaded's for that direction -- into a register; the epilogue stores ONE pixel at the weight sum / (255 n) through
// `out` and / or the sum as ONE 16-bit word through `lsum.light`, either of which may be null.  Across the passes a lane keeps
// LitState's hit point, hcell, the sum and (wave-uniform) the pass; the gradient and the lane's pixel are made again.  With
// HMRM_SHADE_NO_SHADOWS no shadow pass runs: the n levels are computed behind the primary march.
// Termination: every pass is the march loop with a budget of its own, min(step cap, the shadow rays' limit) <= the step cap, and
// the outer loop runs at most 1 + n times -- the primary pass and one per direction, the pass number only ever grows.
struct LitSum : Frames {
	static constexpr bool SEG = true, LIT = true, LSUM = true;
	struct Args { const SegRules &seg; const SunRules &sun; const LightSum &lsum; };
};
// BAKED (render_baked.hip, render_baked_aa.hip; hmrm_render_baked, frame.hpp BakedLight; implies SEG): a baked-light frame.  An
// epilogue: a lane whose primary ray hit fetches its colour behind the loop, as GEOM and LSUM do, loads its light from the scene's
// plane -- one 16-bit load at hcell, or four at the bilinear mode's neighbours of the kept hit point, mixed like the colour -- and
// keeps the pixel at that weight (device_common.hpp shade_baked).  With AA the weighted sample goes to the box filter.
struct Baked : Frames {
	static constexpr bool SEG = true, BAKED = true;
	struct Args { const SegRules &seg; const BakedLight &baked; };
};
// MIRROR (render_water.hip; hmrm_render_water, frame.hpp WaterRules; implies SEG): a water frame.  LIT's second pass with a ray of
// the lane's own and a colour for a result: a lane whose primary ray hit at or below the water level keeps its pixel and marches its
// mirror ray -- a segment ray under the interior rule from (P.x, P.y, t) along the primary direction with dz negated -- through the
// SAME loop; the other lanes sit the second pass out.  Between the passes the lane keeps LitState's hit point, as a lit lane
// does, and ONE word of its primary ray -- the hit cell or the pixel, with "hit" and "water" in its free bits (march.hpp); the
// mirror pass leaves its own hit cell in hcell and its own hit point in x, y (KEEP_P), from which the mirror colour is fetched
// behind the loop; the primary ray's dz is the mirror ray's
// negated once more, so nothing is put aside for the miss shade.
// Termination: the outer loop runs at most twice -- the phase only goes from 0 to 1 -- and each pass is the march loop with a budget
// of its own, the step cap or min(step cap, the mirror rays' limit).
struct Water : Frames {
	static constexpr bool SEG = true, MIRROR = true;
	struct Args { const SegRules &seg; const WaterRules &water; };
};
// MIRROR and BAKED (render_water_baked.hip, render_water_baked_aa.hip; hmrm_render_water_aa with HMRM_WATER_BAKED): the water frame
// under the scene's light plane.  The two definitions composed: the primary pixel (or the water's own colour) takes the weight of the
// primary hit's light, the mirror pixel that of the mirror ray's hit, then the blend.  In the keeps-cell form (march.hpp
// kMirrorKeepsCell) both lights are loaded behind the marches, beside the colours, from the kept cell and from hcell -- nothing new
// is held across the mirror march; in the keeps-pixel form the primary pixel is weighted at the phase switch, where its point or
// cell is at hand, before it goes into the kept word.  BAKED's own epilogue does not run (the pixel would be weighted twice).
// DEFER and CARRY are MIRROR's.  Antialiased<Water> and Antialiased<BakedWater> (render_water_aa.hip, render_water_baked_aa.hip): every
// sample decides "water" on its own, casts its own mirror ray and is weighted and blended before the box filter.
struct BakedWater : Frames {
	static constexpr bool SEG = true, MIRROR = true, BAKED = true;
	struct Args { const SegRules &seg; const WaterRules &water; const BakedLight &baked; };
};
// MIRROR and SUNLIT (render_water_lit.hip; hmrm_render_water_lit): the sun-lit water frame, hmrm_render_water and hmrm_render_shaded
// composed.  "Entry, then the march loop" runs up to four times for the wave: (0) the primary rays, (1) the shadow rays of the lanes
// that hit, (2) the mirror rays of the wet lanes, (3) the shadow rays of the wet lanes whose mirror ray hit; a lane without a ray sits
// a pass out at d = inf, a pass no lane needs is skipped by a ballot.  SUNLIT is a switch of its own, not LIT: LIT's blocks (its phase
// switch, its epilogue, its hcell and lt rules) are written for two passes and collide with MIRROR's.  Whether the weights are
// diffuse and whether the shadow passes run are run-time flags, as in LSUM -- they travel in WaterRules::flags (frame.hpp
// kWaterSunDiffuse, kWaterSunNoShadows), wave-uniform scalar branches -- so this is one family, not four.
// Between the marches a lane keeps LitState's hit point -- the primary hit's outlives pass 1, as LSUM's does: the mirror ray starts
// there; the mirror hit's replaces it in pass 2 and outlives pass 3 -- and ONE word per hit.  Keeps-cell form: the primary hit's cell
// with "hit", "wet" and "shadowed" in its three free bits, and the mirror hit's cell in hcell (all ones: the mirror ray did not hit);
// colours and diffuse levels are fetched behind the marches.  Keeps-pixel form (bilinear): the primary pixel, weighted behind pass 1
// where its point is still at hand, with "hit", "wet" and "mirror ray hit" beside it.  The primary direction is not kept at all: the
// lane makes its camera ray again from its number in the wave, for the mirror ray and for the miss shades -- the same operations,
// the same bits.  A capped ray is counted behind the pass it belongs to; nothing is held for that.
// DEFER and CARRY are MIRROR's choices, taken over with its structure and not decided again.
// Termination: the pass number is wave-uniform and only grows -- 0, then 1 or 2 or the end, ... -- so the outer loop runs at most four
// times, and each pass is the march loop with a budget of its own: the step cap, min(step cap, the sun's limit) for passes 1 and 3,
// min(step cap, the water's limit) for pass 2.
struct SunWater : Frames {
	static constexpr bool SEG = true, MIRROR = true, SUNLIT = true;
	struct Args { const SegRules &seg; const WaterRules &water; const SunRules &sun; };
};
// HAZE (render_haze.hip, render_haze_aa.hip; hmrm_render_haze, frame.hpp HazeRules; implies SEG): a haze frame.  An epilogue: a lane
// whose primary ray hit leaves the loop with int_point in x, y, z as a geometry lane does, makes its ray's origin again, computes
// the range with the geometry frame's expression -- in doubles, not rounded to float -- loads ONE byte of the table at the index
// made from it and blends its pixel towards the haze colour with the water's blend; with kHazeSky the lanes that did not hit blend
// their miss shade at the table's last entry.  With AA the hazed sample goes to the box filter.  The kernel evaluates no
// transcendental: the table is the caller's.
struct Haze : Frames {
	static constexpr bool SEG = true, HAZE = true;
	struct Args { const SegRules &seg; const HazeRules &haze; };
};

// ---- a family: its tag's switches, the four dispatched values, and what follows from them ----
// SAMP: 0 nearest cell (the reference), 1 bilinear quality mode, 2 nearest cell with float thresholds (`thr` then points at the
// float copy of the table).
template <class TAG, int PROJ_, int GWM_, int LEAP_, int SAMP_> struct Family {
	using Args = typename TAG::Args;
	static constexpr int PROJ = PROJ_, GWM = GWM_, LEAP = LEAP_, SAMP = SAMP_;
	static constexpr bool STATS = TAG::STATS, AA = TAG::AA, SEG = TAG::SEG, LIT = TAG::LIT, SHADE = TAG::SHADE, SUM = TAG::SUM,
	                      GEOM = TAG::GEOM, LSUM = TAG::LSUM, BAKED = TAG::BAKED, MIRROR = TAG::MIRROR;
	static constexpr bool SUNLIT = TAG::SUNLIT; // (shadowed and shaded on both sides of the mirror: the one tag with MIRROR and a sun)
	static constexpr bool HAZE = TAG::HAZE;
	static constexpr bool CELLS = PROJ == 5;
	static constexpr bool POINT = GEOM || HAZE; // (a hit lane leaves the loop with int_point in full: z stepped like x and y)
	static_assert(!HAZE || (SEG && !CELLS && PROJ != 4 && !STATS && !LIT && !SHADE && !GEOM && !BAKED && !MIRROR),
	              "haze frames: plain frames under the segment rules, antialiased or not");
	static_assert(!MIRROR || SEG, "water frames: under the segment rules");
	static_assert(!MIRROR || !CELLS, "water frames: a camera's frame, not a cell map");
	static_assert(!MIRROR || PROJ != 4, "water frames: a camera's frame, not a ray batch");
	static_assert(!MIRROR || !STATS, "water frames: production kernels only");
	static_assert(!MIRROR || !LIT, "water frames: no sun shadows by LIT's two passes (SUNLIT has its own four)");
	static_assert(!MIRROR || !SHADE, "water frames: no sun shading by SHADE's epilogue (SUNLIT weights both sides itself)");
	static_assert(!SUNLIT || (MIRROR && !BAKED && !AA), "sun-lit water frames: water frames, neither under the light plane nor antialiased");
	static_assert(!MIRROR || !GEOM, "water frames: no geometry planes");
	static_assert(!BAKED || (SEG && !CELLS && PROJ != 4 && !STATS && !LIT && !SHADE && !GEOM), "baked-light frames: plain or water frames under the segment rules");
	static_assert(!LSUM || (LIT && !SHADE && !AA), "accumulated lit frames: the lit kernels' marches, the weights by a run-time flag");
	static_assert(!GEOM || (SEG && !CELLS && PROJ != 4 && !STATS && !AA && !LIT && !SHADE), "geometry frames: plain frames under the segment rules");
	static_assert(!SUM || CELLS, "accumulated cell maps: the cell kernels' march, once per target");
	static_assert(!CELLS || (SEG && !STATS && !AA && !LIT && !SHADE), "cell maps: segment rays, one byte per cell");
	static_assert(!LIT || (SEG && PROJ != 4), "sun shadows: frames, under the segment rules");
	static_assert(!SHADE || (SEG && PROJ != 4), "sun shading: frames, under the segment rules");
	static constexpr bool BILINEAR = SAMP == 1, F32 = SAMP == 2;
	// KEEP_P: a lane that hit leaves the loop with its hit point in x, y (LIT: and t in z).  SHADE with bilinear sampling wants
	// the point too; without LIT the plain groups take it that way, the leap kernels keep the hit's exact cell coordinates
	// instead (KEEP_Q) -- each the cheaper of the two in registers for its family, DESIGN.md 5.12 -- and from them they also
	// mix the pixel behind the loop (DEFER), shaded or not.
	// GEOM wants the whole point, in every sampling mode: KEEP_P with z stepped like x and y (no threshold is kept), which holds
	// nothing across the loop -- RAYS' select chain keeps three doubles more.  HAZE wants the same (POINT), for
	// its range; its own answers: DESIGN.md 5.23.
	static constexpr bool KEEP_Q = BILINEAR && !CELLS && !LIT && !MIRROR && LEAP != 0 && !POINT;
	// BAKED with bilinear sampling wants the point like SHADE: KEEP_Q in the leap kernels, KEEP_P in the plain groups.
	// MIRROR wants the point and the threshold like LIT, for the mirror ray's origin -- and the mirror ray's own hit point for its colour.
	static constexpr bool KEEP_P = LIT || MIRROR || ((SHADE || BAKED) && BILINEAR && !KEEP_Q) || (GEOM && !kGeomChain) || (HAZE && !kHazeChain);
	static constexpr bool CHAIN = PROJ == 4 || (GEOM && kGeomChain) || (HAZE && kHazeChain); // (the hit point by RAYS' select chain: hx, hy, hz)
	static constexpr bool RAYS = PROJ == 4, COUNT = STATS || RAYS;
	// DEFER: a hit lane's colour is fetched behind the march loop, from the hit cell it leaves the loop with (hcell; the
	// bilinear mode: and from the hit point, KEEP_P / KEEP_Q), not inside it.  Two exceptions keep the in-loop form.  The record
	// kernels of the interior and the shaded frames without shadow rays: two of them sit on the scalar registers' limit and the
	// epilogue's load costs them a spill slot (profiles/r09_registers.txt).  And the bilinear mode of the plain groups: leaving
	// the loop with the hit point made that kernel 20 % SLOWER where it was measured (0.263 -> 0.316 ms, profiles/r09_ab.txt).
	// (GEOM: always behind the loop -- a null colour target skips the fetch there, a scalar branch)
	// (LSUM: always behind the loop, like GEOM -- and behind every march: the hit point outlives them)
	// (BAKED: behind the loop too -- the light is loaded beside the colour, from the same cell or point -- except in its record
	// kernels, which keep the interior family's in-loop fetch: deferred, the orthographic one with power-of-two grid widths took
	// 36 bytes of scratch)
	// (MIRROR: as LIT -- behind the loop in its record kernels too, in the loop for the bilinear mode of the plain groups, where a
	// pass's colour simply lands in `rgba`: DESIGN.md 5.20; with BAKED too: MIRROR's choice stands)
	// (HAZE: behind the loop in every instantiation, like GEOM -- what that costs the two kinds the interior family keeps in the
	// loop: DESIGN.md 5.23)
	static constexpr bool DEFER = GEOM || LSUM || (HAZE && kHazeDefer) || (BAKED && !MIRROR && LEAP != 2) || (!CELLS && !(LEAP == 2 && SEG && !LIT && !MIRROR && !RAYS) && !(BILINEAR && LEAP == 0));
	static_assert(!RAYS || (!AA && !STATS), "ray batches: neither antialiased nor instrumented");
	static_assert(!SEG || !STATS, "segment rules: production kernels only");
	static_assert(!SEG || !AA || LIT || SHADE || BAKED || MIRROR || HAZE, "segment rules: antialiased for the sun-lit, baked-light, water and haze frames only");
	static constexpr bool REC = LEAP == 2; // leaps over window records instead of the pyramid (frame.hpp WindowRecord)
	// CARRY: a ray holds its level state in a register (see the leap state in the march loop).  The cell maps, the sun shadows, the
	// ray batches and the shaded record kernels sit on a register granule: a register more would cost them a resident wave per SIMD
	// -- as it would six of the geometry kernels (general grid widths: 73 against 71 vector registers, 81 against 80 with window
	// records).  (MIRROR: LIT's choice, taken over with its two-pass structure; DESIGN.md 5.20 has the counts.)
	static constexpr bool CARRY = LEAP != 0 && !CELLS && !LIT && !MIRROR && !RAYS && !((SHADE || BAKED) && REC) && !(GEOM && !kGeomCarry) && !(HAZE && !kHazeCarry);
	static constexpr int U = LEAP == 1 ? kGroup : (REC ? kGroupRec : kGroupPlain); // positions per speculative group
	static_assert(!REC || SAMP == 0, "records bound the nearest cell's double thresholds only");
};

} // namespace hmrm
