// march_dispatch.hpp -- from the run-time values that pick a march kernel (projection, grid mode, kernel kind, sampling)
// to its template arguments <PROJ, GWM, LEAP, SAMP>: the one ladder of every unit that instantiates render_wave_tile
// (march.hpp).  The callable gets the four values as std::integral_constants and is called exactly once.  In front of it,
// route_frame: from what a frame asks for to the family of kernels that renders it.  Host code only, nothing from HIP:
// tests/fuzz_host_logic.cpp compiles it with g++.
#pragma once
#include <type_traits>

namespace hmrm {

// kPlainGroups: speculative step groups; kLeaps: plus exact leaps over empty pyramid windows; kRecords: leaps over windows
// of the record level that are empty but for a few recorded cells (render.hpp launch_frame_march).
enum FastKernel { kPlainGroups = 0, kLeaps = 1, kRecords = 2 };

// Which kernels render a frame (render.hpp FrameLaunch): hmrm_render's, or the ones built with the interior rule, with
// shadow rays, with diffuse shading without or with shadow rays, or the ones that store the geometry planes too.
// (kFrameGeometry is no result of route_frame: a geometry frame takes the literal-or-march decision from it and sets the
// family itself, api_launch.cpp.)  kFrameLitSum: the accumulated lit frame's (hmrm_render_lit_sum), one family for its four
// `shade_flags`, which its kernels read at run time.  kFrameBaked: the baked-light frame's (hmrm_render_baked), set by the launch
// path like kFrameGeometry.  kFrameWater: the water frame's (hmrm_render_water), set by the launch path likewise,
// as are its antialiased form, its form under the light plane and both (hmrm_render_water_aa): kFrameWaterAA, kFrameWaterBaked and
// kFrameWaterBakedAA.  kFrameWaterLit: the sun-lit water frame's (hmrm_render_water_lit), set by the launch path too; one family for
// its four `shade_flags`, which its kernels read at run time.  kFrameHaze: the haze frame's (hmrm_render_haze), set by the launch
// path like kFrameGeometry; its antialiased form is its launchers' matter, as the baked-light family's is, beside which it stands.  kFrameViews: a view batch's
// (hmrm_render_views), set by its own launch path (api_launch.cpp launch_views); it stands beside kFrameHaze.
enum FrameFamily { kFramePlain = 0, kFrameInterior, kFrameLit, kFrameShaded, kFrameLitShaded, kFrameGeometry, kFrameLitSum, kFrameBaked, kFrameHaze, kFrameViews, kFrameWater,
                   kFrameWaterAA, kFrameWaterBaked, kFrameWaterBakedAA, kFrameWaterLit };

// Which launch a frame gets.  `forced`: HMRM_KERNEL (2: simple); `huge_side`: a map side of 2^24 cells or more -- the production
// kernel indexes cells and windows with 24-bit multiplies, leap_common.hpp index_2d; `interior`: hmrm_render_interior's frame
// whose rays may start inside the box; `lit`: the frame has a sun, with hmrm_render_shaded's `shade_flags` (the values of
// HMRM_SHADE_*; 0: hmrm_render_lit's frame, by its kernels).  A sun takes precedence over `interior`: such a frame carries
// the rule in FrameLaunch::primary_interior.  `aa` (the frame has an antialias factor) changes no route: the antialiased variant
// of a family is its launchers' matter (f.aa_shift), and the one family without such kernels, the interior one, has no entry
// point that takes a factor.  `sum` (with `lit`): hmrm_render_lit_sum's frame -- one family whatever the flags, the caller's sun.
constexpr unsigned kShadeDiffuse = 1u, kShadeNoShadows = 2u;
struct FrameRoute {
	bool refused;     // no kernel renders this frame: a huge side with another sampling than nearest
	bool literal;     // the literal loop (which only knows the reference's sampling), else a march kernel
	FrameFamily family;
	bool shadows;     // the launch marches shadow rays
	bool ambient_sun; // the sun handed to the launch is the caller's with ambient = 255
};
inline FrameRoute route_frame(int forced, bool huge_side, int sampling, bool /*aa*/, bool interior, bool lit, unsigned shade_flags,
                              bool sum = false) {
	FrameRoute r{huge_side && sampling != 0, (forced == 2 || huge_side) && sampling == 0, kFramePlain, false, false};
	if (lit && sum) {
		r.family = kFrameLitSum;
		r.shadows = !(shade_flags & kShadeNoShadows);
	} else if (lit) {
		// (HMRM_SHADE_NO_SHADOWS without HMRM_SHADE_DIFFUSE is hmrm_render's frame by definition.  It goes through the shaded kernel
		// with every weight 255 all the same, not through the interior / plain kernels: the interior launcher always sets the
		// interior rule, which this frame has only with HMRM_TRACE_INTERIOR, and the plain one belongs to frames that may be
		// measured or be the probe, which no frame of this entry point is.  The levels it computes for nothing are the price of
		// one route; the combination is an identity for tests, not something to render with.)
		r.shadows = !(shade_flags & kShadeNoShadows);
		r.family = !r.shadows ? kFrameShaded : shade_flags ? kFrameLitShaded : kFrameLit; // (kFrameLitShaded: HMRM_SHADE_DIFFUSE alone)
		// Without HMRM_SHADE_DIFFUSE a pixel that is not shadowed has the weight 255: the kernels without shadow rays get that
		// from ambient = 255, whatever the level.
		r.ambient_sun = !r.shadows && !(shade_flags & kShadeDiffuse);
	} else if (interior) {
		r.family = kFrameInterior;
	}
	return r;
}

template <int V>
using MarchConst = std::integral_constant<int, V>;

template <class Fn>
void dispatch_sampling(int sampling, Fn &&fn) {
	if (sampling == 1) fn(MarchConst<1>{});
	else if (sampling == 2) fn(MarchConst<2>{});
	else fn(MarchConst<0>{});
}

// Ray batches: the projection is fixed (PROJ == 4).  fn(gwm, leap, samp).
// The record kernel is built for nearest sampling only (its records bound the nearest cell's double thresholds), which
// keeps the instantiations at 7 and not 9 per (PROJ, GWM): kRecords arrives with SAMP 0 whatever `sampling` says.  The
// launchers have refused the other combinations before they come here (launch_common.hpp select_tables).
template <class Fn>
void dispatch_march(int grid_mode, int kernel, int sampling, Fn &&fn) {
	auto kind = [&](auto gwm) {
		if (kernel == kRecords) fn(gwm, MarchConst<kRecords>{}, MarchConst<0>{});
		else if (kernel == kLeaps) dispatch_sampling(sampling, [&](auto samp) { fn(gwm, MarchConst<kLeaps>{}, samp); });
		else dispatch_sampling(sampling, [&](auto samp) { fn(gwm, MarchConst<kPlainGroups>{}, samp); });
	};
	switch (grid_mode) {
	case 0: kind(MarchConst<0>{}); break;
	case 1: kind(MarchConst<1>{}); break;
	default: kind(MarchConst<2>{}); break;
	}
}

// Frames: fn(proj, gwm, leap, samp).
template <class Fn>
void dispatch_march(int projection, int grid_mode, int kernel, int sampling, Fn &&fn) {
	auto rest = [&](auto proj) {
		dispatch_march(grid_mode, kernel, sampling, [&](auto gwm, auto leap, auto samp) { fn(proj, gwm, leap, samp); });
	};
	switch (projection) {
	case 1: rest(MarchConst<1>{}); break;
	case 2: rest(MarchConst<2>{}); break;
	default: rest(MarchConst<3>{}); break;
	}
}

} // namespace hmrm
