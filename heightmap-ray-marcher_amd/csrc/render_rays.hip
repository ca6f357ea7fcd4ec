// render_rays.hip -- ray batches (hmrm_trace_rays, hmrm.h): the production march kernel instantiated for caller-supplied
// rays.  render_fast.hip compiled once more for its march alone (as render_fast_aa.hip does), with the fourth ray source,
// PROJ == 4: a lane loads its hmrm_ray from the batch instead of making it from a camera, marches it through the SAME
// loop -- speculative groups, leaps over the pyramid or the window records, the one-division slab shortcut, the three
// sampling modes -- and writes its hmrm_ray_hit record instead of a pixel.  The frame kernels are not touched: they live
// in their own translation units and take no new argument.
#undef HMRM_TIMELINE
#define HMRM_RENDER_RAYS 1
#include "render_fast.hip"

namespace hmrm {

// One workgroup = 2 waves = 128 consecutive rays (the batch as a frame kBatchW pixels wide, frame.hpp RayBatch: tile
// column 0 only, identity row map -- no launch order, no calibration records).  Grid rows beyond 32768 go to blockIdx.z,
// as for tall frames.
template <int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_trace_rays(const DevFrame f, const double *__restrict__ thr,
                                                                                              const uint32_t *__restrict__ cmap,
                                                                                              const RayBatch batch, int tiles_y, StatsOut st) {
	const RowMap rows{0, f.screen_h, 0, 0, 1, {0x7fffffff, 0x7fffffff, 0x7fffffff}, {0, 0, 0, 0}, nullptr};
	(void)render_wave_tile<4, false, GWM, LEAP, SAMP, false>(f, rows, thr, cmap, nullptr, 0, tiles_y, st, 0, blockIdx.z * 32768u + blockIdx.x,
	                                                          (int)(threadIdx.x >> 6), (int)(threadIdx.x & 63), batch);
}

template <int GWM, int LEAP>
static void launch_samp(const DevFrame &f, const double *d_thr, const uint32_t *d_cmap, const RayBatch &batch, int tiles_y,
                        StatsOut st, dim3 grid, hipStream_t stream) {
	if constexpr (LEAP == kRecords) { // (nearest sampling only: launch_trace_rays has checked)
		hipLaunchKernelGGL((k_trace_rays<GWM, LEAP, 0>), grid, dim3(kBlockThreads), 0, stream, f, d_thr, d_cmap, batch, tiles_y, st);
	} else {
		if (f.sampling == 1)
			hipLaunchKernelGGL((k_trace_rays<GWM, LEAP, 1>), grid, dim3(kBlockThreads), 0, stream, f, d_thr, d_cmap, batch, tiles_y, st);
		else if (f.sampling == 2) // (d_thr is the float table here)
			hipLaunchKernelGGL((k_trace_rays<GWM, LEAP, 2>), grid, dim3(kBlockThreads), 0, stream, f, d_thr, d_cmap, batch, tiles_y, st);
		else
			hipLaunchKernelGGL((k_trace_rays<GWM, LEAP, 0>), grid, dim3(kBlockThreads), 0, stream, f, d_thr, d_cmap, batch, tiles_y, st);
	}
}

template <int GWM>
static void launch_kind(FastKernel kernel, const DevFrame &f, const double *d_thr, const uint32_t *d_cmap, const RayBatch &batch,
                        int tiles_y, StatsOut st, dim3 grid, hipStream_t stream) {
	if (kernel == kLeaps) launch_samp<GWM, kLeaps>(f, d_thr, d_cmap, batch, tiles_y, st, grid, stream);
	else if (kernel == kRecords) launch_samp<GWM, kRecords>(f, d_thr, d_cmap, batch, tiles_y, st, grid, stream);
	else launch_samp<GWM, kPlainGroups>(f, d_thr, d_cmap, batch, tiles_y, st, grid, stream);
}

hipError_t launch_trace_rays(const DevFrame &f, const double *d_thr_f64, const float *d_thr32, const uint32_t *d_cmap,
                             const RayBatch &batch, unsigned long long *d_counters, FastKernel kernel,
                             const WindowRecord *d_records, hipStream_t stream) {
	if (kernel == kRecords && (f.sampling != 0 || !d_records)) return hipErrorInvalidValue;
	if (batch.n <= 0) return hipSuccess;
	if (batch.n > ((int64_t)1 << 29) || f.screen_w != kBatchW || (int64_t)f.screen_h * kBatchW < batch.n) return hipErrorInvalidValue;
	DevFrame fr = f;
	if (kernel == kRecords) fr.mipbuf_bil = reinterpret_cast<const float *>(d_records); // (as launch_fast does)
	const double *d_thr = f.sampling == 2 ? reinterpret_cast<const double *>(d_thr32) : d_thr_f64;
	const int tiles_y = (f.screen_h + kTileH - 1) / kTileH;
	const dim3 grid((unsigned)(tiles_y < 32768 ? tiles_y : 32768), 1u, (unsigned)((tiles_y + 32767) / 32768));
	const StatsOut st{d_counters, nullptr, nullptr};
	switch (f.grid_mode) {
	case 0: launch_kind<0>(kernel, fr, d_thr, d_cmap, batch, tiles_y, st, grid, stream); break;
	case 1: launch_kind<1>(kernel, fr, d_thr, d_cmap, batch, tiles_y, st, grid, stream); break;
	default: launch_kind<2>(kernel, fr, d_thr, d_cmap, batch, tiles_y, st, grid, stream); break;
	}
	return hipGetLastError();
}

} // namespace hmrm
