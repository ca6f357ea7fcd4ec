// render_water_lit.hip -- sun-lit water frames (hmrm_render_water_lit, hmrm.h): the production march kernel instantiated with MIRROR
// and SUNLIT (march_family.hpp SunWater; march.hpp render_wave_tile): hmrm_render_water and hmrm_render_shaded composed in one
// launch.  A wave marches up to four times -- the primary rays, the shadow rays of the lanes that hit, the mirror rays of the wet
// lanes, the shadow rays of the wet lanes whose mirror ray hit -- and weights either side of the mirror by its own hit's weight
// before the blend.  No hit point, threshold or record goes through memory.  Whether the weights are diffuse and whether shadow
// rays are cast are flags of the launch (frame.hpp kWaterSunDiffuse, kWaterSunNoShadows), read at run time: one family.
// The production kernels only, as render_water.hip's, in a translation unit of their own: the existing kernels keep their
// argument lists and their instructions.
#include "march.hpp"

namespace hmrm {

// k_render_water's launch shape (one workgroup per tile, grid rows beyond 32768 in blockIdx.z); never a calibration launch.
template <int PROJ, int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_render_water_lit(const DevFrame f, const RowMap rows,
		const double *__restrict__ thr, const uint32_t *__restrict__ cmap, uint32_t *__restrict__ out, int64_t out_stride_px, int tiles_y,
		StatsOut st, const SegRules seg, const WaterRules water, const SunRules sun) {
	(void)render_wave_tile<Family<SunWater, PROJ, GWM, LEAP, SAMP>>(
	    f, rows, thr, cmap, out, out_stride_px, tiles_y, st, (int)blockIdx.x, blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6),
	    (int)(threadIdx.x & 63), seg, water, sun);
}

hipError_t launch_render_water_lit(const FrameLaunch &l, FastKernel kernel) {
	if (!l.d_out || l.sun.ambient > 255u) return hipErrorInvalidValue;
	return launch_march_family(l, kernel, false, [&](auto proj, auto gwm, auto leap, auto samp, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL((k_render_water_lit<proj(), gwm(), leap(), samp()>), grid, dim3(kBlockThreads), 0, l.stream, args..., l.water,
		                   l.sun);
	});
}

} // namespace hmrm
