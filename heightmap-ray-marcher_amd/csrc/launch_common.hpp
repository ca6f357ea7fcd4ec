// launch_common.hpp -- what the launchers of the march kernels (march.hpp's users) and of the literal loop (render.hip)
// do before they launch: the grid of a frame, the grid of a ray batch, the tables a kernel kind and a sampling mode read.
#pragma once
#include "device_common.hpp"
#include "render.hpp"

namespace hmrm {

struct LaunchGrid {
	dim3 grid;
	int tiles_y;    // 0: nothing to launch, the launcher returns `err`
	hipError_t err;
};

// grid rows beyond 32768 go to blockIdx.z (the kernels read blockIdx.z * 32768 + the row's own index)
inline unsigned folded_rows(int tiles_y) { return (unsigned)(tiles_y < 32768 ? tiles_y : 32768); }
inline unsigned row_folds(int tiles_y) { return (unsigned)((tiles_y + 32767) / 32768); }

// A frame: one workgroup per pixel tile, tile columns in x, the row map's grid rows in y.
inline LaunchGrid tile_grid(const DevFrame &f, const RowMap &rows) {
	const int tiles_x = (f.screen_w + kTileW - 1) / kTileW;
	const int tiles_y = (rows.local_rows + kTileH - 1) / kTileH;
	if (tiles_x <= 0 || tiles_y <= 0) return {dim3(), 0, hipSuccess};
	return {dim3((unsigned)tiles_x, folded_rows(tiles_y), row_folds(tiles_y)), tiles_y, hipSuccess};
}

// A view batch (hmrm_render_views): one workgroup per tile of every view, tile columns in x, the n_views * tiles_y_view tile rows
// in y, folded like a frame's.  tiles_y is ONE view's tile rows.  The row count is made in 64 bits: a batch whose rows do not
// fit the grid (65535 slabs of 32768) is refused.
constexpr int64_t kMaxViewTileRows = (int64_t)65535 * 32768;
inline LaunchGrid views_grid(const DevFrame &f, int n_views) {
	const int tiles_x = (f.screen_w + kTileW - 1) / kTileW;
	const int tiles_y = (f.screen_h + kTileH - 1) / kTileH;
	if (tiles_x <= 0 || tiles_y <= 0 || n_views <= 0) return {dim3(), 0, hipSuccess};
	const int64_t rows = (int64_t)n_views * tiles_y;
	if (rows > kMaxViewTileRows) return {dim3(), 0, hipErrorInvalidValue};
	return {dim3((unsigned)tiles_x, (unsigned)(rows < 32768 ? rows : 32768), (unsigned)((rows + 32767) / 32768)), tiles_y, hipSuccess};
}

// A ray batch: the batch as a frame kBatchW pixels wide (frame.hpp RayBatch), one workgroup per 128 consecutive rays,
// grid rows in x.  An empty batch is no error; one that is too long, or whose frame does not hold it, is.
inline LaunchGrid batch_grid(const DevFrame &f, const RayBatch &batch) {
	if (batch.n <= 0) return {dim3(), 0, hipSuccess};
	if (batch.n > ((int64_t)1 << 29) || f.screen_w != kBatchW || (int64_t)f.screen_h * kBatchW < batch.n)
		return {dim3(), 0, hipErrorInvalidValue};
	const int tiles_y = (f.screen_h + kTileH - 1) / kTileH;
	return {dim3(folded_rows(tiles_y), 1u, row_folds(tiles_y)), tiles_y, hipSuccess};
}

// The tables of a march kernel.  Records need nearest sampling and a table, and the record kernel finds that table where
// the bilinear mode finds its pyramid (frame.hpp: `*f` is the launcher's copy); sampling 2 reads the float copy of the
// threshold table through the kernel's `thr` argument.
inline hipError_t select_tables(DevFrame *f, FastKernel kernel, const double *d_thr_f64, const float *d_thr32,
                                const WindowRecord *d_records, const double **d_thr) {
	if (kernel == kRecords && (f->sampling != 0 || !d_records)) return hipErrorInvalidValue;
	if (kernel == kRecords) f->mipbuf_bil = reinterpret_cast<const float *>(d_records);
	*d_thr = f->sampling == 2 ? reinterpret_cast<const double *>(d_thr32) : d_thr_f64;
	return hipSuccess;
}

// The march units' own frame launchers, one per family and AA variant (launch_frame_march, render_fast.hip, picks): each
// translation unit instantiates its kernels, so that the units compile side by side.  The plain ones may be instrumented
// and measured (march_frame.hpp launch_fast); the others refuse a measured launch, and a frame whose f.aa_shift is not their kind.
hipError_t launch_render_fast(const FrameLaunch &l, FastKernel kernel);          // render_fast.hip
hipError_t launch_render_fast_aa(const FrameLaunch &l, FastKernel kernel);       // render_fast_aa.hip
hipError_t launch_render_interior(const FrameLaunch &l, FastKernel kernel);      // render_interior.hip (no AA variant)
hipError_t launch_render_lit(const FrameLaunch &l, FastKernel kernel);           // render_lit.hip
hipError_t launch_render_lit_aa(const FrameLaunch &l, FastKernel kernel);        // render_lit_aa.hip
hipError_t launch_render_shaded(const FrameLaunch &l, FastKernel kernel);        // render_shaded.hip
hipError_t launch_render_shaded_aa(const FrameLaunch &l, FastKernel kernel);     // render_shaded_aa.hip
hipError_t launch_render_lit_shaded(const FrameLaunch &l, FastKernel kernel);    // render_lit_shaded.hip
hipError_t launch_render_lit_shaded_aa(const FrameLaunch &l, FastKernel kernel); // render_lit_shaded_aa.hip
hipError_t launch_render_geometry(const FrameLaunch &l, FastKernel kernel);      // render_geometry.hip (no AA variant)
hipError_t launch_render_lit_sum(const FrameLaunch &l, FastKernel kernel);       // render_lit_sum.hip (no AA variant)
hipError_t launch_render_baked(const FrameLaunch &l, FastKernel kernel);         // render_baked.hip
hipError_t launch_render_baked_aa(const FrameLaunch &l, FastKernel kernel);      // render_baked_aa.hip
hipError_t launch_render_water(const FrameLaunch &l, FastKernel kernel);         // render_water.hip
hipError_t launch_render_water_aa(const FrameLaunch &l, FastKernel kernel);      // render_water_aa.hip
hipError_t launch_render_water_baked(const FrameLaunch &l, FastKernel kernel);   // render_water_baked.hip
hipError_t launch_render_water_baked_aa(const FrameLaunch &l, FastKernel kernel); // render_water_baked_aa.hip
hipError_t launch_render_water_lit(const FrameLaunch &l, FastKernel kernel);     // render_water_lit.hip (no AA variant)
hipError_t launch_render_haze(const FrameLaunch &l, FastKernel kernel);          // render_haze.hip
hipError_t launch_render_haze_aa(const FrameLaunch &l, FastKernel kernel);       // render_haze_aa.hip
hipError_t launch_render_views(const FrameLaunch &l, FastKernel kernel);         // render_views.hip (view batches; no AA variant)

// The segment rules of a frame launch: no limits, the interior rule for the interior family and where the sun's flags ask.
inline SegRules frame_seg_rules(const FrameLaunch &l) {
	return SegRules{nullptr, 0u, (l.family == kFrameInterior || l.primary_interior) ? 1u : 0u};
}

// The launcher body of the interior, lit and shaded units, antialiased (`aa`) or not: k_render_fast's launch shape (one
// workgroup per tile, grid rows beyond 32768 in blockIdx.z).  `launch(proj, gwm, leap, samp, grid, args...)` launches the
// unit's kernel with those template arguments on that grid, with `args...` as its leading arguments: frame, row map, table,
// colours, target, stride, tile rows, counters, segment rules (a unit whose kernel takes the sun adds it).
template <class Launch>
hipError_t launch_march_family(const FrameLaunch &l, FastKernel kernel, bool aa, Launch &&launch) {
	if ((l.f.aa_shift != 0) != aa || l.rows.measure != nullptr) return hipErrorInvalidValue;
	DevFrame fr = l.f;
	const double *d_thr = nullptr;
	if (const hipError_t e = select_tables(&fr, kernel, l.d_thr, l.d_thr32, l.d_records, &d_thr); e != hipSuccess) return e;
	const LaunchGrid g = tile_grid(l.f, l.rows);
	if (g.tiles_y == 0) return g.err;
	const StatsOut st{l.d_counters, nullptr, nullptr};
	const SegRules seg = frame_seg_rules(l);
	dispatch_march(l.f.projection, l.f.grid_mode, kernel, l.f.sampling, [&](auto proj, auto gwm, auto leap, auto samp) {
		launch(proj, gwm, leap, samp, g.grid, fr, l.rows, d_thr, l.d_cmap, l.d_out, l.out_stride_px, g.tiles_y, st, seg);
	});
	return hipGetLastError();
}

} // namespace hmrm
