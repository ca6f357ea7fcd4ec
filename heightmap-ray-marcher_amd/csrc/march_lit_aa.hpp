// march_lit_aa.hpp -- what the three antialiased sun-lit units (render_lit_aa.hip, render_shaded_aa.hip, render_lit_shaded_aa.hip;
// hmrm_render_shaded_aa, hmrm.h) share: the wave's tile with the AA epilogue behind the LIT / SHADE ones.  A unit adds its
// __global__ kernel -- one template argument pair <LIT, SHADE> apart from the other two's -- and names it to the launcher
// body it shares with the units that are not antialiased (launch_common.hpp launch_march_family).  The launch marches the
// super frame (f.screen_w x f.screen_h samples) with the launch shape of the non-antialiased counterpart and writes the
// box-filtered frame (device_common.hpp store_box_filtered); no sample is stored.
#pragma once
#include "march.hpp"

namespace hmrm {

template <bool LIT, bool SHADE, int PROJ, int GWM, int LEAP, int SAMP>
__device__ __forceinline__ void lit_aa_wave_tile(const DevFrame &f, const RowMap &rows, const double *__restrict__ thr,
                                                 const uint32_t *__restrict__ cmap, uint32_t *__restrict__ out, int64_t out_stride_px,
                                                 int tiles_y, const StatsOut &st, const SegRules &seg, const SunRules &sun) {
	(void)render_wave_tile<Family<Antialiased<Sun<LIT, SHADE>>, PROJ, GWM, LEAP, SAMP>>(f, rows, thr, cmap, out, out_stride_px, tiles_y, st,
	                                                                                     (int)blockIdx.x, blockIdx.z * 32768u + blockIdx.y,
	                                                                                     (int)(threadIdx.x >> 6), (int)(threadIdx.x & 63), seg, sun);
}

} // namespace hmrm
