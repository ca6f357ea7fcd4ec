// render_cell_sums.hip -- accumulated cell maps (hmrm_cell_map_sum, hmrm.h): the cell kernels of render_cells.hip with the march
// run once per target of a list (SUM; frame.hpp CellSums) -- many suns, sky directions or observers in one launch.  A lane owns
// one map cell of the rect, makes the cell's ray towards target k from the cell index, marches it under the interior rule, adds
// the value k_cell_map would have written for it (or 1 for a ray that did not hit) to a register and, after the last target,
// writes one 16-bit word.  Nothing per ray comes from memory but the cell's own threshold and the wave-uniform target.
// Kernels and argument structs of their own: every other kernel keeps its arguments and its instructions.
#include "march.hpp"

namespace hmrm {

// k_cell_map's launch shape (render_cells.hip): one workgroup = 2 waves = 8 x 16 cells; per tile row eight lanes store eight
// contiguous words.  `out` and its stride are 2-byte aligned and no more (hmrm.h), so a wave's row is not widened into one store.
template <int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_cell_map_sum(const DevFrame f, const double *__restrict__ thr,
                                                                                                uint16_t *__restrict__ out, int64_t stride_bytes,
                                                                                                const CellRules cells, const CellSums sums,
                                                                                                int tiles_y, StatsOut st) {
	const RowMap rows = whole_frame_rows(f);
	(void)render_wave_tile<Family<CellSum, 5, GWM, LEAP, SAMP>>(
	    f, rows, thr, nullptr, reinterpret_cast<uint32_t *>(out), stride_bytes, tiles_y, st, (int)blockIdx.x,
	    blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6), (int)(threadIdx.x & 63), SegRules{nullptr, cells.max_steps, 1u}, cells, sums);
}

hipError_t launch_cell_map_sum(const DevFrame &f, const double *d_thr_f64, const float *d_thr32, uint16_t *d_out, int64_t stride_bytes,
                               const CellRules &cells, const CellSums &sums, unsigned long long *d_counters, FastKernel kernel,
                               const WindowRecord *d_records, hipStream_t stream) {
	DevFrame fr = f;
	const double *d_thr = nullptr;
	if (const hipError_t e = select_tables(&fr, kernel, d_thr_f64, d_thr32, d_records, &d_thr); e != hipSuccess) return e;
	const RowMap rows = whole_frame_rows(f);
	const LaunchGrid g = tile_grid(f, rows);
	if (g.tiles_y == 0) return g.err;
	const StatsOut st{d_counters, nullptr, nullptr};
	dispatch_march(f.grid_mode, kernel, f.sampling, [&](auto gwm, auto leap, auto samp) {
		hipLaunchKernelGGL((k_cell_map_sum<gwm(), leap(), samp()>), g.grid, dim3(kBlockThreads), 0, stream, fr, d_thr, d_out, stride_bytes,
		                   cells, sums, g.tiles_y, st);
	});
	return hipGetLastError();
}

} // namespace hmrm
