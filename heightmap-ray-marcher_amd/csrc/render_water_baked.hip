// render_water_baked.hip -- water frames under the scene's light plane (hmrm_render_water_aa with HMRM_WATER_BAKED, hmrm.h): the
// production march kernel instantiated with MIRROR and BAKED (march_family.hpp BakedWater; march.hpp render_wave_tile): the primary
// pixel, or the water's own colour, takes the weight of the primary hit's light, the mirror ray's pixel that of its own hit, then
// the blend.  Each light is one 16-bit load beside the colour it weights (the bilinear mode: four, mixed like the colour); no third
// march.  The production kernels only, as render_water.hip's, in a translation unit of their own: the existing kernels keep their
// argument lists and their instructions.
#include "march.hpp"

namespace hmrm {

// k_render_water's launch shape (one workgroup per tile, grid rows beyond 32768 in blockIdx.z); never a calibration launch.
template <int PROJ, int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_render_water_baked(const DevFrame f, const RowMap rows,
		const double *__restrict__ thr, const uint32_t *__restrict__ cmap, uint32_t *__restrict__ out, int64_t out_stride_px, int tiles_y,
		StatsOut st, const SegRules seg, const WaterRules water, const BakedLight baked) {
	(void)render_wave_tile<Family<BakedWater, PROJ, GWM, LEAP, SAMP>>(
	    f, rows, thr, cmap, out, out_stride_px, tiles_y, st, (int)blockIdx.x, blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6),
	    (int)(threadIdx.x & 63), seg, water, baked);
}

hipError_t launch_render_water_baked(const FrameLaunch &l, FastKernel kernel) {
	if (!l.baked.plane || l.baked.full_scale < 1u || l.baked.full_scale > 65535u || !l.d_out) return hipErrorInvalidValue;
	return launch_march_family(l, kernel, false, [&](auto proj, auto gwm, auto leap, auto samp, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL((k_render_water_baked<proj(), gwm(), leap(), samp()>), grid, dim3(kBlockThreads), 0, l.stream, args..., l.water,
		                   l.baked);
	});
}

} // namespace hmrm
