// march_frame.hpp -- the frame kernel of the march (k_render_fast) and its launcher, for the two units that share them:
// render_fast.hip instantiates the plain kernels, render_fast_aa.hip the antialiased ones (launch_fast<false> / <true>),
// so that the two halves compile in parallel.
#pragma once
#include "march.hpp"

namespace hmrm {

// The tool-only wave timeline (-DHMRM_TIMELINE, tools/timeline.py) covers the plain frame kernels only: render_fast.hip
// defines these two hooks, render_fast_aa.hip undefines the flag before it includes this header, and the other units of
// the march do not include it.
#ifdef HMRM_TIMELINE
__device__ __forceinline__ void timeline_wave_done(unsigned long long t0);
static void timeline_before_launch(dim3 grid, int tiles_y, const RowMap &rows);
#endif

template <int PROJ, bool STATS, int GWM, int LEAP, int SAMP, bool AA>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_render_fast(const DevFrame f, const RowMap rows,
                                                     const double *__restrict__ thr,
                                                     const uint32_t *__restrict__ cmap,
                                                     uint32_t *__restrict__ out, int64_t out_stride_px,
                                                     int tiles_y, StatsOut st) {
#ifdef HMRM_TIMELINE
	const unsigned long long tl_t0 = __builtin_amdgcn_s_memrealtime();
#endif
	// calibration launches only (RowMap::measure): when did this wave start
	unsigned long long wave_t0 = 0;
	if (!STATS && rows.measure) wave_t0 = __builtin_amdgcn_s_memrealtime();
	const int tile_y = render_wave_tile<Family<FramesOf<STATS, AA>, PROJ, GWM, LEAP, SAMP>>(
	    f, rows, thr, cmap, out, out_stride_px, tiles_y, st, (int)blockIdx.x, blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6),
	    (int)(threadIdx.x & 63));
	if (!STATS && rows.measure && tile_y >= 0 && (threadIdx.x & 63) == 0) {
		// record of a tile row: [0] start of its first workgroup (rows are handed out left to right), [1 + k] longest
		// wave among the tile columns = k mod 32 (32 addresses per row: the atomics of a row's 2 x 480 waves spread out)
		const unsigned long long took = __builtin_amdgcn_s_memrealtime() - wave_t0;
		unsigned long long *rec = rows.measure + (size_t)tile_y * kMeasureStride;
		if (blockIdx.x == 0 && threadIdx.x == 0) rec[0] = wave_t0;
		atomicMax(&rec[1 + (blockIdx.x & 31u)], took);
	}
#ifdef HMRM_TIMELINE
	if (!STATS) timeline_wave_done(tl_t0);
#endif
}

template <bool AA>
static hipError_t launch_fast(const DevFrame &f, const RowMap &rows, const double *d_thr_f64, const float *d_thr32,
                              const uint32_t *d_cmap, uint32_t *d_out, int64_t out_stride_px,
                              unsigned long long *d_counters, uint32_t *d_steps, double *d_entry, bool stats,
                              FastKernel kernel, const WindowRecord *d_records, hipStream_t stream) {
	DevFrame fr = f;
	const double *d_thr = nullptr;
	if (const hipError_t e = select_tables(&fr, kernel, d_thr_f64, d_thr32, d_records, &d_thr); e != hipSuccess) return e;
	const LaunchGrid g = tile_grid(f, rows);
	if (g.tiles_y == 0) return g.err;
	const StatsOut st{d_counters, d_steps, d_entry};
#ifdef HMRM_TIMELINE
	if (!stats) timeline_before_launch(g.grid, g.tiles_y, rows);
#endif
	auto launch = [&](auto instrumented) {
		dispatch_march(f.projection, f.grid_mode, kernel, f.sampling, [&](auto proj, auto gwm, auto leap, auto samp) {
			hipLaunchKernelGGL((k_render_fast<proj(), decltype(instrumented)::value, gwm(), leap(), samp(), AA>), g.grid,
			                   dim3(kBlockThreads), 0, stream, fr, rows, d_thr, d_cmap, d_out, out_stride_px, g.tiles_y, st);
		});
	};
	if (stats) launch(std::true_type{});
	else launch(std::false_type{});
	return hipGetLastError();
}

} // namespace hmrm
