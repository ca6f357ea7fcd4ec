// render_views.hip -- view batches (hmrm_render_views, hmrm.h): N cameras of one scene in ONE launch.  The production march kernel
// of render_interior.hip -- the interior family carries plain frames (seg.interior == 0) and interior ones -- whose workgroup
// reads its camera's frame record from a device array instead of from the kernel arguments: grid row gy belongs to view
// gy / tiles_y_view, a wave-uniform index, so the record arrives through the scalar cache as the argument does.
// The production kernels only -- three projections, three grid modes, leaps and plain groups in the three sampling modes, window
// records for nearest sampling; no instrumented and no antialiased ones -- in a translation unit of their own: the existing frame
// kernels keep their argument lists and their instructions.
#include "march.hpp"

namespace hmrm {

// One workgroup per tile: tile columns in x, the n_views * tiles_y_view tile rows of the batch in y (beyond 32768 in blockIdx.z).
// View k's pixels land at out + k * view_stride_px; its row map is the identity of one whole view (no bands, one piece, no
// calibration records).  Grid rows past the last view (the last z-slab may be partly empty) render nothing.
template <int PROJ, int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_render_views(
		const DevFrame *__restrict__ frames, int n_views, int tiles_y_view, const double *__restrict__ thr,
		const uint32_t *__restrict__ cmap, uint32_t *__restrict__ out, int64_t out_stride_px, int64_t view_stride_px, StatsOut st,
		const SegRules seg) {
	const unsigned gy = blockIdx.z * 32768u + blockIdx.y;
	// (blockIdx is uniform already; the builtin says so to the compiler wherever the quotient travels, so that frames[view] is
	// fetched with scalar loads and never per lane)
	const unsigned view = (unsigned)__builtin_amdgcn_readfirstlane((int)(gy / (unsigned)tiles_y_view));
	if (view >= (unsigned)n_views) return;
	const unsigned local_row = gy - view * (unsigned)tiles_y_view;
	// (a copy made of 32-bit words, not a reference: device_common.hpp copy_frame_words)
	DevFrame f;
	copy_frame_words(&f, frames + view);
	const RowMap rows = whole_frame_rows(f);
	(void)render_wave_tile<Family<Interior, PROJ, GWM, LEAP, SAMP>>(f, rows, thr, cmap, out + (int64_t)view * view_stride_px, out_stride_px,
	                                                                 tiles_y_view, st, (int)blockIdx.x, local_row, (int)(threadIdx.x >> 6),
	                                                                 (int)(threadIdx.x & 63), seg);
}

// l.f is view 0's record as the host built it (what the launch dispatches on: projection, grid mode, sampling, size -- the same
// for every view of a batch); l.d_frames the n_views records in device memory, which already name the tables the kernel kind
// reads (the host path has done select_tables' substitution in every record: api_launch.cpp launch_views).
hipError_t launch_render_views(const FrameLaunch &l, FastKernel kernel) {
	if (l.f.aa_shift != 0 || l.rows.measure != nullptr || !l.d_frames || l.n_views < 1 || !l.d_out) return hipErrorInvalidValue;
	DevFrame fr = l.f;
	const double *d_thr = nullptr;
	if (const hipError_t e = select_tables(&fr, kernel, l.d_thr, l.d_thr32, l.d_records, &d_thr); e != hipSuccess) return e;
	const LaunchGrid g = views_grid(l.f, l.n_views);
	if (g.tiles_y == 0) return g.err;
	const StatsOut st{l.d_counters, nullptr, nullptr};
	const SegRules seg = frame_seg_rules(l);
	dispatch_march(l.f.projection, l.f.grid_mode, kernel, l.f.sampling, [&](auto proj, auto gwm, auto leap, auto samp) {
		hipLaunchKernelGGL((k_render_views<proj(), gwm(), leap(), samp()>), g.grid, dim3(kBlockThreads), 0, l.stream, l.d_frames, l.n_views,
		                   g.tiles_y, d_thr, l.d_cmap, l.d_out, l.out_stride_px, l.view_stride_px, st, seg);
	});
	return hipGetLastError();
}

} // namespace hmrm
