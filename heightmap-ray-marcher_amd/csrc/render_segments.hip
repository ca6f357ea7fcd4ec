// render_segments.hip -- segment batches (hmrm_trace_segments, hmrm.h): the ray batches' march (render_rays.hip, PROJ == 4)
// instantiated once more under the segment rules (SEG; frame.hpp SegRules) -- a ray that starts strictly inside the box
// enters it at d = +0.0 instead of missing, and a ray ends after its own number of height loads with HMRM_RAY_END.  Kernels
// and an argument struct of their own: k_trace_rays and the frame kernels keep their arguments and their instructions.
#undef HMRM_TIMELINE
#define HMRM_RENDER_SEGMENTS 1
#include "render_fast.hip"

namespace hmrm {

// The launch shape of k_trace_rays: one workgroup = 2 waves = 128 consecutive rays, grid rows beyond 32768 in blockIdx.z.
template <int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_trace_segments(const DevFrame f, const double *__restrict__ thr,
                                                                                                  const uint32_t *__restrict__ cmap,
                                                                                                  const RayBatch batch, const SegRules seg,
                                                                                                  int tiles_y, StatsOut st) {
	const RowMap rows{0, f.screen_h, 0, 0, 1, {0x7fffffff, 0x7fffffff, 0x7fffffff}, {0, 0, 0, 0}, nullptr};
	(void)render_wave_tile<4, false, GWM, LEAP, SAMP, false, true>(f, rows, thr, cmap, nullptr, 0, tiles_y, st, 0,
	                                                                blockIdx.z * 32768u + blockIdx.x, (int)(threadIdx.x >> 6),
	                                                                (int)(threadIdx.x & 63), batch, seg);
}

template <int GWM, int LEAP>
static void launch_samp(const DevFrame &f, const double *d_thr, const uint32_t *d_cmap, const RayBatch &batch, const SegRules &seg,
                        int tiles_y, StatsOut st, dim3 grid, hipStream_t stream) {
	if constexpr (LEAP == kRecords) { // (nearest sampling only: launch_trace_segments has checked)
		hipLaunchKernelGGL((k_trace_segments<GWM, LEAP, 0>), grid, dim3(kBlockThreads), 0, stream, f, d_thr, d_cmap, batch, seg, tiles_y, st);
	} else {
		if (f.sampling == 1)
			hipLaunchKernelGGL((k_trace_segments<GWM, LEAP, 1>), grid, dim3(kBlockThreads), 0, stream, f, d_thr, d_cmap, batch, seg, tiles_y, st);
		else if (f.sampling == 2) // (d_thr is the float table here)
			hipLaunchKernelGGL((k_trace_segments<GWM, LEAP, 2>), grid, dim3(kBlockThreads), 0, stream, f, d_thr, d_cmap, batch, seg, tiles_y, st);
		else
			hipLaunchKernelGGL((k_trace_segments<GWM, LEAP, 0>), grid, dim3(kBlockThreads), 0, stream, f, d_thr, d_cmap, batch, seg, tiles_y, st);
	}
}

template <int GWM>
static void launch_kind(FastKernel kernel, const DevFrame &f, const double *d_thr, const uint32_t *d_cmap, const RayBatch &batch,
                        const SegRules &seg, int tiles_y, StatsOut st, dim3 grid, hipStream_t stream) {
	if (kernel == kLeaps) launch_samp<GWM, kLeaps>(f, d_thr, d_cmap, batch, seg, tiles_y, st, grid, stream);
	else if (kernel == kRecords) launch_samp<GWM, kRecords>(f, d_thr, d_cmap, batch, seg, tiles_y, st, grid, stream);
	else launch_samp<GWM, kPlainGroups>(f, d_thr, d_cmap, batch, seg, tiles_y, st, grid, stream);
}

hipError_t launch_trace_segments(const DevFrame &f, const double *d_thr_f64, const float *d_thr32, const uint32_t *d_cmap,
                                 const RayBatch &batch, const SegRules &seg, unsigned long long *d_counters, FastKernel kernel,
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
	case 0: launch_kind<0>(kernel, fr, d_thr, d_cmap, batch, seg, tiles_y, st, grid, stream); break;
	case 1: launch_kind<1>(kernel, fr, d_thr, d_cmap, batch, seg, tiles_y, st, grid, stream); break;
	default: launch_kind<2>(kernel, fr, d_thr, d_cmap, batch, seg, tiles_y, st, grid, stream); break;
	}
	return hipGetLastError();
}

} // namespace hmrm
