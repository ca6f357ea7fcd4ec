// render_shaded_aa.hip -- hill-shaded frames without shadow rays, antialiased (hmrm_render_shaded_aa with HMRM_SHADE_NO_SHADOWS, hmrm.h): the kernels of
// render_shaded.hip with the AA epilogue behind theirs (march_lit_aa.hpp): every sample that hit takes the weight of its own diffuse level, then the wave
// box-filters its n x n blocks.  A translation unit of its own: the existing kernels keep their instructions.
#include "march_lit_aa.hpp"

namespace hmrm {

// k_render_shaded's launch shape and arguments; never a calibration launch.
template <int PROJ, int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_render_shaded_aa(const DevFrame f, const RowMap rows,
		const double *__restrict__ thr, const uint32_t *__restrict__ cmap, uint32_t *__restrict__ out, int64_t out_stride_px, int tiles_y,
		StatsOut st, const SegRules seg, const SunRules sun) {
	lit_aa_wave_tile<false, true, PROJ, GWM, LEAP, SAMP>(f, rows, thr, cmap, out, out_stride_px, tiles_y, st, seg, sun);
}

hipError_t launch_render_shaded_aa(const FrameLaunch &l, FastKernel kernel) {
	return launch_march_family(l, kernel, true, [&](auto proj, auto gwm, auto leap, auto samp, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL((k_render_shaded_aa<proj(), gwm(), leap(), samp()>), grid, dim3(kBlockThreads), 0, l.stream, args..., l.sun);
	});
}

} // namespace hmrm
