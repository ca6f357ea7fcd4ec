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

} // namespace hmrm
