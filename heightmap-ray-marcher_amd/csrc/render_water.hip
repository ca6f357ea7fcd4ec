// render_water.hip -- water frames (hmrm_render_water, hmrm.h): the production march kernel instantiated once more with MIRROR
// (frame.hpp WaterRules; march.hpp render_wave_tile): a pixel whose primary ray hit at or below the water level marches its
// mirror ray -- the primary direction with dz negated, from the surface above the hit point -- through the same loop in the
// same launch, and that ray's pixel is blended into its own.  No hit point, threshold or record goes through memory.
// The production kernels only, as render_lit.hip's -- three projections, three grid modes, leaps and plain groups in the
// three sampling modes, window records for nearest sampling -- in a translation unit of their own: the existing kernels keep
// their argument lists and their instructions.
#include "march.hpp"

namespace hmrm {

// k_render_fast's launch shape (one workgroup per tile, grid rows beyond 32768 in blockIdx.z); never a calibration launch.
template <int PROJ, int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_render_water(const DevFrame f, const RowMap rows,
                                                                                                     const double *__restrict__ thr,
                                                                                                     const uint32_t *__restrict__ cmap,
                                                                                                     uint32_t *__restrict__ out,
                                                                                                     int64_t out_stride_px, int tiles_y,
                                                                                                     StatsOut st, const SegRules seg,
                                                                                                     const WaterRules water) {
	(void)render_wave_tile<Family<Water, PROJ, GWM, LEAP, SAMP>>(f, rows, thr, cmap, out, out_stride_px, tiles_y, st, (int)blockIdx.x,
	                                                              blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6),
	                                                              (int)(threadIdx.x & 63), seg, water);
}

hipError_t launch_render_water(const FrameLaunch &l, FastKernel kernel) {
	if (!l.d_out) return hipErrorInvalidValue;
	return launch_march_family(l, kernel, false, [&](auto proj, auto gwm, auto leap, auto samp, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL((k_render_water<proj(), gwm(), leap(), samp()>), grid, dim3(kBlockThreads), 0, l.stream, args..., l.water);
	});
}

} // namespace hmrm
