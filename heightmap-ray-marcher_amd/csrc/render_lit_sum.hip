// render_lit_sum.hip -- accumulated lit frames (hmrm_render_lit_sum, hmrm.h): the lit kernels of render_lit.hip instantiated once
// more with LSUM (march.hpp render_wave_tile): the primary march once, then one shadow march per direction of a wave-uniform list
// for the lanes that hit, the weights of hmrm_render_shaded summed per lane, and one weighted pixel and / or the 16-bit sum stored
// at the end.  Whether the weights are diffuse is a run-time flag of the list (frame.hpp LightSum): one family of kernels.  A
// translation unit of its own: the existing kernels keep their argument lists and their instructions.
#include "march.hpp"

namespace hmrm {

// k_render_lit's launch shape and arguments, and the list; never a calibration launch.
template <int PROJ, int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_render_lit_sum(const DevFrame f, const RowMap rows,
                                                                                                       const double *__restrict__ thr,
                                                                                                       const uint32_t *__restrict__ cmap,
                                                                                                       uint32_t *__restrict__ out,
                                                                                                       int64_t out_stride_px, int tiles_y,
                                                                                                       StatsOut st, const SegRules seg, const SunRules sun,
                                                                                                       const LightSum lsum) {
	(void)render_wave_tile<Family<LitSum, PROJ, GWM, LEAP, SAMP>>(
	    f, rows, thr, cmap, out, out_stride_px, tiles_y, st, (int)blockIdx.x, blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6),
	    (int)(threadIdx.x & 63), seg, sun, lsum);
}

hipError_t launch_render_lit_sum(const FrameLaunch &l, FastKernel kernel) {
	if (l.lsum.n < 1 || l.lsum.n > kMaxSumDirs || !l.lsum.dirs || (!l.d_out && !l.lsum.light)) return hipErrorInvalidValue;
	return launch_march_family(l, kernel, false, [&](auto proj, auto gwm, auto leap, auto samp, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL((k_render_lit_sum<proj(), gwm(), leap(), samp()>), grid, dim3(kBlockThreads), 0, l.stream, args..., l.sun, l.lsum);
	});
}

} // namespace hmrm
