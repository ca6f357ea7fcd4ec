// render_haze.hip -- haze frames (hmrm_render_haze, hmrm.h): the production march kernel instantiated once more with HAZE (frame.hpp
// HazeRules): hmrm_render's pixel -- hmrm_render_interior's under the interior rule -- blended towards the haze colour by the byte of
// the caller's table at the pixel's range, before it is stored; with HMRM_HAZE_SKY the pixels that did not hit at the table's last
// entry.  The production kernels only -- three projections, three grid modes, leaps and plain groups in the three sampling modes,
// window records for nearest sampling; no instrumented ones -- in a translation unit of their own, as render_interior.hip is: the
// existing frame kernels keep their argument lists and their instructions.
#include "march.hpp"

namespace hmrm {

// k_render_fast's launch shape (one workgroup per tile, grid rows beyond 32768 in blockIdx.z); never a calibration launch.
template <int PROJ, int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_render_haze(const DevFrame f, const RowMap rows,
		const double *__restrict__ thr, const uint32_t *__restrict__ cmap, uint32_t *__restrict__ out, int64_t out_stride_px, int tiles_y,
		StatsOut st, const SegRules seg, const HazeRules haze) {
	(void)render_wave_tile<Family<Haze, PROJ, GWM, LEAP, SAMP>>(
	    f, rows, thr, cmap, out, out_stride_px, tiles_y, st, (int)blockIdx.x, blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6),
	    (int)(threadIdx.x & 63), seg, haze);
}

hipError_t launch_render_haze(const FrameLaunch &l, FastKernel kernel) {
	if (!l.haze.table || l.haze.n < 1u || l.haze.n > (uint32_t)kMaxHazeEntries || !l.d_out) return hipErrorInvalidValue;
	return launch_march_family(l, kernel, false, [&](auto proj, auto gwm, auto leap, auto samp, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL((k_render_haze<proj(), gwm(), leap(), samp()>), grid, dim3(kBlockThreads), 0, l.stream, args..., l.haze);
	});
}

} // namespace hmrm
