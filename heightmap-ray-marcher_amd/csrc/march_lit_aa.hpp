// march_lit_aa.hpp -- what the three antialiased sun-lit units (render_lit_aa.hip, render_shaded_aa.hip, render_lit_shaded_aa.hip;
// hmrm_render_shaded_aa, hmrm.h) share: the wave's tile with the AA epilogue behind the LIT / SHADE ones, and the launcher.  A
// unit adds its __global__ kernel -- one template argument pair <LIT, SHADE> apart from the other two's -- and names it to
// launch_lit_aa.  The launch marches the super frame (f.screen_w x f.screen_h samples) with the launch shape of the
// non-antialiased counterpart and writes the box-filtered frame (device_common.hpp store_box_filtered); no sample is stored.
#pragma once
#include "march.hpp"

namespace hmrm {

template <bool LIT, bool SHADE, int PROJ, int GWM, int LEAP, int SAMP>
__device__ __forceinline__ void lit_aa_wave_tile(const DevFrame &f, const RowMap &rows, const double *__restrict__ thr,
                                                 const uint32_t *__restrict__ cmap, uint32_t *__restrict__ out, int64_t out_stride_px,
                                                 int tiles_y, const StatsOut &st, const SegRules &seg, const SunRules &sun) {
	(void)render_wave_tile<PROJ, false, GWM, LEAP, SAMP, true, true, LIT, SHADE>(f, rows, thr, cmap, out, out_stride_px, tiles_y, st, (int)blockIdx.x,
	                                                                           blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6),
	                                                                           (int)(threadIdx.x & 63), RayBatch{}, seg, sun);
}

// `launch(proj, gwm, leap, samp, grid, frame, thr, tiles_y, stats, seg)` launches the unit's kernel with those template
// arguments.  Refuses what the non-antialiased launchers accept: a frame without a factor; and, as they do, a measured launch.
template <class Launch>
hipError_t launch_lit_aa(const DevFrame &f, const RowMap &rows, const double *d_thr_f64, const float *d_thr32,
                         unsigned long long *d_counters, FastKernel kernel, const WindowRecord *d_records, bool primary_interior,
                         Launch &&launch) {
	if (f.aa_shift == 0 || rows.measure != nullptr) return hipErrorInvalidValue;
	DevFrame fr = f;
	const double *d_thr = nullptr;
	if (const hipError_t e = select_tables(&fr, kernel, d_thr_f64, d_thr32, d_records, &d_thr); e != hipSuccess) return e;
	const LaunchGrid g = tile_grid(f, rows);
	if (g.tiles_y == 0) return g.err;
	const StatsOut st{d_counters, nullptr, nullptr};
	const SegRules seg{nullptr, 0u, primary_interior ? 1u : 0u};
	dispatch_march(f.projection, f.grid_mode, kernel, f.sampling,
	               [&](auto proj, auto gwm, auto leap, auto samp) { launch(proj, gwm, leap, samp, g.grid, fr, d_thr, g.tiles_y, st, seg); });
	return hipGetLastError();
}

} // namespace hmrm
