// render_haze_aa.hip -- haze frames, antialiased (hmrm_render_haze with a factor, hmrm.h): the kernels of render_haze.hip with the AA
// epilogue behind theirs (device_common.hpp store_box_filtered): every sample is hazed at its own range -- a sample that did not hit
// at the table's last entry, with HMRM_HAZE_SKY -- then the wave box-filters its n x n blocks; no sample is stored.  A translation
// unit of its own: the existing kernels keep their instructions.
#include "march.hpp"

namespace hmrm {

// k_render_haze's launch shape and arguments; never a calibration launch.
template <int PROJ, int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_render_haze_aa(const DevFrame f, const RowMap rows,
		const double *__restrict__ thr, const uint32_t *__restrict__ cmap, uint32_t *__restrict__ out, int64_t out_stride_px, int tiles_y,
		StatsOut st, const SegRules seg, const HazeRules haze) {
	(void)render_wave_tile<Family<Antialiased<Haze>, PROJ, GWM, LEAP, SAMP>>(
	    f, rows, thr, cmap, out, out_stride_px, tiles_y, st, (int)blockIdx.x, blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6),
	    (int)(threadIdx.x & 63), seg, haze);
}

hipError_t launch_render_haze_aa(const FrameLaunch &l, FastKernel kernel) {
	if (!l.haze.table || l.haze.n < 1u || l.haze.n > (uint32_t)kMaxHazeEntries || !l.d_out) return hipErrorInvalidValue;
	return launch_march_family(l, kernel, true, [&](auto proj, auto gwm, auto leap, auto samp, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL((k_render_haze_aa<proj(), gwm(), leap(), samp()>), grid, dim3(kBlockThreads), 0, l.stream, args..., l.haze);
	});
}

} // namespace hmrm
