// render_shaded.hip -- hill-shaded frames without shadow rays (hmrm_render_shaded with HMRM_SHADE_NO_SHADOWS, hmrm.h): the
// production march kernel under the segment rules, as render_interior.hip's, instantiated once more with SHADE (march.hpp
// render_wave_tile): a pixel whose ray hit takes its diffuse level from the neighbours of the hit in the threshold table the
// march reads and keeps a weighted pixel.  One pass, nothing added to the march loop but the hit's cell index (its cell
// coordinates for bilinear sampling).  The production kernels only -- three projections, three grid modes, leaps and plain
// groups in the three sampling modes, window records for nearest sampling -- in a translation unit of their own: the
// existing kernels keep their argument lists and their instructions.
#include "march.hpp"

namespace hmrm {

// k_render_fast's launch shape (one workgroup per tile, grid rows beyond 32768 in blockIdx.z); never a calibration launch.
// `sun`: the direction and the ambient level; its step and limit are not looked at.
template <int PROJ, int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_render_shaded(const DevFrame f, const RowMap rows,
                                                                                                      const double *__restrict__ thr,
                                                                                                      const uint32_t *__restrict__ cmap,
                                                                                                      uint32_t *__restrict__ out,
                                                                                                      int64_t out_stride_px, int tiles_y,
                                                                                                      StatsOut st, const SegRules seg, const SunRules sun) {
	(void)render_wave_tile<Family<Shaded, PROJ, GWM, LEAP, SAMP>>(f, rows, thr, cmap, out, out_stride_px, tiles_y, st, (int)blockIdx.x,
	                                                               blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6),
	                                                               (int)(threadIdx.x & 63), seg, sun);
}

hipError_t launch_render_shaded(const FrameLaunch &l, FastKernel kernel) {
	return launch_march_family(l, kernel, false, [&](auto proj, auto gwm, auto leap, auto samp, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL((k_render_shaded<proj(), gwm(), leap(), samp()>), grid, dim3(kBlockThreads), 0, l.stream, args..., l.sun);
	});
}

} // namespace hmrm
