// render_rays.hip -- ray batches (hmrm_trace_rays, hmrm.h): the production march (march.hpp) instantiated for caller-supplied
// rays, the fourth ray source, PROJ == 4: a lane loads its hmrm_ray from the batch instead of making it from a camera, marches it through the SAME
// loop -- speculative groups, leaps over the pyramid or the window records, the one-division slab shortcut, the three
// sampling modes -- and writes its hmrm_ray_hit record instead of a pixel.  The frame kernels are not touched: they live
// in their own translation units and take no new argument.
#include "march.hpp"

namespace hmrm {

// One workgroup = 2 waves = 128 consecutive rays (the batch as a frame kBatchW pixels wide, frame.hpp RayBatch: tile
// column 0 only, identity row map -- no launch order, no calibration records).  Grid rows beyond 32768 go to blockIdx.z,
// as for tall frames.
template <int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_trace_rays(const DevFrame f, const double *__restrict__ thr,
                                                                                              const uint32_t *__restrict__ cmap,
                                                                                              const RayBatch batch, int tiles_y, StatsOut st) {
	const RowMap rows = whole_frame_rows(f);
	(void)render_wave_tile<Family<Rays, 4, GWM, LEAP, SAMP>>(f, rows, thr, cmap, nullptr, 0, tiles_y, st, 0, blockIdx.z * 32768u + blockIdx.x,
	                                                          (int)(threadIdx.x >> 6), (int)(threadIdx.x & 63), batch);
}

hipError_t launch_trace_rays(const DevFrame &f, const double *d_thr_f64, const float *d_thr32, const uint32_t *d_cmap,
                             const RayBatch &batch, unsigned long long *d_counters, FastKernel kernel,
                             const WindowRecord *d_records, hipStream_t stream) {
	DevFrame fr = f;
	const double *d_thr = nullptr;
	if (const hipError_t e = select_tables(&fr, kernel, d_thr_f64, d_thr32, d_records, &d_thr); e != hipSuccess) return e;
	const LaunchGrid g = batch_grid(f, batch);
	if (g.tiles_y == 0) return g.err;
	const StatsOut st{d_counters, nullptr, nullptr};
	dispatch_march(f.grid_mode, kernel, f.sampling, [&](auto gwm, auto leap, auto samp) {
		hipLaunchKernelGGL((k_trace_rays<gwm(), leap(), samp()>), g.grid, dim3(kBlockThreads), 0, stream, fr, d_thr, d_cmap, batch,
		                   g.tiles_y, st);
	});
	return hipGetLastError();
}

} // namespace hmrm
