// render_cells.hip -- cell maps (hmrm_cell_map, hmrm.h): the march of the segment batches (render_segments.hip) with one more
// source of rays (PROJ == 5; frame.hpp CellRules) -- a lane owns one map cell of the rect, makes its own segment ray from the
// cell index and the threshold table, marches it under the interior rule and writes one byte: the ray's status, or the light
// weight of hmrm_render_shaded.  Nothing per ray comes from memory but the cell's own threshold, nothing goes back but the byte.
// Kernels and an argument struct of their own: every other kernel keeps its arguments and its instructions.
#include "march.hpp"

namespace hmrm {

// The launch shape of a frame (launch_common.hpp tile_grid) over the rect: one workgroup = 2 waves = 8 x 16 cells, a wave
// 8 x 8 of them -- 2-D locality in the table, and per tile row eight lanes that store eight contiguous bytes -- tile columns
// in blockIdx.x, tile rows in y, beyond 32768 in z.  Byte stores: `out` and its stride need no alignment (hmrm.h), so a
// wave's row cannot be widened into one store; a wave writes 64 bytes per march, which is no cost beside the march.
template <int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_cell_map(const DevFrame f, const double *__restrict__ thr,
                                                                                            uint8_t *__restrict__ out, int64_t stride_bytes,
                                                                                            const CellRules cells, int tiles_y, StatsOut st) {
	const RowMap rows = whole_frame_rows(f);
	(void)render_wave_tile<Family<Cells, 5, GWM, LEAP, SAMP>>(f, rows, thr, nullptr, reinterpret_cast<uint32_t *>(out), stride_bytes, tiles_y, st,
	                                                           (int)blockIdx.x, blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6),
	                                                           (int)(threadIdx.x & 63), SegRules{nullptr, cells.max_steps, 1u}, cells);
}

hipError_t launch_cell_map(const DevFrame &f, const double *d_thr_f64, const float *d_thr32, uint8_t *d_out, int64_t stride_bytes,
                           const CellRules &cells, unsigned long long *d_counters, FastKernel kernel, const WindowRecord *d_records,
                           hipStream_t stream) {
	DevFrame fr = f;
	const double *d_thr = nullptr;
	if (const hipError_t e = select_tables(&fr, kernel, d_thr_f64, d_thr32, d_records, &d_thr); e != hipSuccess) return e;
	const RowMap rows = whole_frame_rows(f);
	const LaunchGrid g = tile_grid(f, rows);
	if (g.tiles_y == 0) return g.err;
	const StatsOut st{d_counters, nullptr, nullptr};
	dispatch_march(f.grid_mode, kernel, f.sampling, [&](auto gwm, auto leap, auto samp) {
		hipLaunchKernelGGL((k_cell_map<gwm(), leap(), samp()>), g.grid, dim3(kBlockThreads), 0, stream, fr, d_thr, d_out, stride_bytes,
		                   cells, g.tiles_y, st);
	});
	return hipGetLastError();
}

} // namespace hmrm
