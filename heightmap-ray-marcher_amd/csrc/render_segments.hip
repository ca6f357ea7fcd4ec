// render_segments.hip -- segment batches (hmrm_trace_segments, hmrm.h): the ray batches' march (render_rays.hip, PROJ == 4)
// instantiated once more under the segment rules (SEG; frame.hpp SegRules) -- a ray that starts strictly inside the box
// enters it at d = +0.0 instead of missing, and a ray ends after its own number of height loads with HMRM_RAY_END.  Kernels
// and an argument struct of their own: k_trace_rays and the frame kernels keep their arguments and their instructions.
#include "march.hpp"

namespace hmrm {

// The launch shape of k_trace_rays: one workgroup = 2 waves = 128 consecutive rays, grid rows beyond 32768 in blockIdx.z.
template <int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_trace_segments(const DevFrame f, const double *__restrict__ thr,
                                                                                                  const uint32_t *__restrict__ cmap,
                                                                                                  const RayBatch batch, const SegRules seg,
                                                                                                  int tiles_y, StatsOut st) {
	const RowMap rows = whole_frame_rows(f);
	(void)render_wave_tile<Family<Segments, 4, GWM, LEAP, SAMP>>(f, rows, thr, cmap, nullptr, 0, tiles_y, st, 0,
	                                                              blockIdx.z * 32768u + blockIdx.x, (int)(threadIdx.x >> 6),
	                                                              (int)(threadIdx.x & 63), batch, seg);
}

hipError_t launch_trace_segments(const DevFrame &f, const double *d_thr_f64, const float *d_thr32, const uint32_t *d_cmap,
                                 const RayBatch &batch, const SegRules &seg, unsigned long long *d_counters, FastKernel kernel,
                                 const WindowRecord *d_records, hipStream_t stream) {
	DevFrame fr = f;
	const double *d_thr = nullptr;
	if (const hipError_t e = select_tables(&fr, kernel, d_thr_f64, d_thr32, d_records, &d_thr); e != hipSuccess) return e;
	const LaunchGrid g = batch_grid(f, batch);
	if (g.tiles_y == 0) return g.err;
	const StatsOut st{d_counters, nullptr, nullptr};
	dispatch_march(f.grid_mode, kernel, f.sampling, [&](auto gwm, auto leap, auto samp) {
		hipLaunchKernelGGL((k_trace_segments<gwm(), leap(), samp()>), g.grid, dim3(kBlockThreads), 0, stream, fr, d_thr, d_cmap,
		                   batch, seg, g.tiles_y, st);
	});
	return hipGetLastError();
}

} // namespace hmrm
