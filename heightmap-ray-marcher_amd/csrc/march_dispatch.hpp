// march_dispatch.hpp -- from the run-time values that pick a march kernel (projection, grid mode, kernel kind, sampling)
// to its template arguments <PROJ, GWM, LEAP, SAMP>: the one ladder of every unit that instantiates render_wave_tile
// (march.hpp).  The callable gets the four values as std::integral_constants and is called exactly once.  Host code
// only, nothing from HIP: tests/fuzz_host_logic.cpp compiles it with g++.
#pragma once
#include <type_traits>

namespace hmrm {

// kPlainGroups: speculative step groups; kLeaps: plus exact leaps over empty pyramid windows; kRecords: leaps over windows
// of the record level that are empty but for a few recorded cells (render.hpp launch_render_fast).
enum FastKernel { kPlainGroups = 0, kLeaps = 1, kRecords = 2 };

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
