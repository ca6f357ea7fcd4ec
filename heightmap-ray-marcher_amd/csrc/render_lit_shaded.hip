// render_lit_shaded.hip -- hill-shaded frames with sun shadows (hmrm_render_shaded with HMRM_SHADE_DIFFUSE, hmrm.h): the lit
// kernels of render_lit.hip instantiated once more with SHADE (march.hpp render_wave_tile): after the shadow march a pixel
// that hit and is not shadowed takes its diffuse level from the neighbours of its primary hit in the threshold table and
// keeps a weighted pixel; a shadowed one keeps the ambient weight as before.  The hit's cell index (the hit point for
// bilinear sampling) is what survives the second pass for it.  A translation unit of its own: the existing kernels keep
// their argument lists and their instructions.
#include "march.hpp"

namespace hmrm {

// k_render_lit's launch shape and arguments; never a calibration launch.
template <int PROJ, int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_render_lit_shaded(const DevFrame f, const RowMap rows,
                                                                                                          const double *__restrict__ thr,
                                                                                                          const uint32_t *__restrict__ cmap,
                                                                                                          uint32_t *__restrict__ out,
                                                                                                          int64_t out_stride_px, int tiles_y,
                                                                                                          StatsOut st, const SegRules seg, const SunRules sun) {
	(void)render_wave_tile<Family<LitShaded, PROJ, GWM, LEAP, SAMP>>(f, rows, thr, cmap, out, out_stride_px, tiles_y, st, (int)blockIdx.x,
	                                                                  blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6),
	                                                                  (int)(threadIdx.x & 63), seg, sun);
}

hipError_t launch_render_lit_shaded(const FrameLaunch &l, FastKernel kernel) {
	return launch_march_family(l, kernel, false, [&](auto proj, auto gwm, auto leap, auto samp, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL((k_render_lit_shaded<proj(), gwm(), leap(), samp()>), grid, dim3(kBlockThreads), 0, l.stream, args..., l.sun);
	});
}

} // namespace hmrm
