// render_water_baked_aa.hip -- water frames under the scene's light plane, antialiased (hmrm_render_water_aa with HMRM_WATER_BAKED
// and a factor, hmrm.h): the kernels of render_water_baked.hip with the AA epilogue behind theirs (device_common.hpp
// store_box_filtered): every sample is weighted and blended on its own, then the wave box-filters its n x n blocks; no sample is
// stored.  A translation unit of its own: the existing kernels keep their instructions.
#include "march.hpp"

namespace hmrm {

// k_render_water_baked's launch shape and arguments; never a calibration launch.
template <int PROJ, int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_render_water_baked_aa(const DevFrame f, const RowMap rows,
		const double *__restrict__ thr, const uint32_t *__restrict__ cmap, uint32_t *__restrict__ out, int64_t out_stride_px, int tiles_y,
		StatsOut st, const SegRules seg, const WaterRules water, const BakedLight baked) {
	(void)render_wave_tile<Family<Antialiased<BakedWater>, PROJ, GWM, LEAP, SAMP>>(
	    f, rows, thr, cmap, out, out_stride_px, tiles_y, st, (int)blockIdx.x, blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6),
	    (int)(threadIdx.x & 63), seg, water, baked);
}

hipError_t launch_render_water_baked_aa(const FrameLaunch &l, FastKernel kernel) {
	if (!l.baked.plane || l.baked.full_scale < 1u || l.baked.full_scale > 65535u || !l.d_out) return hipErrorInvalidValue;
	return launch_march_family(l, kernel, true, [&](auto proj, auto gwm, auto leap, auto samp, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL((k_render_water_baked_aa<proj(), gwm(), leap(), samp()>), grid, dim3(kBlockThreads), 0, l.stream, args..., l.water,
		                   l.baked);
	});
}

} // namespace hmrm
