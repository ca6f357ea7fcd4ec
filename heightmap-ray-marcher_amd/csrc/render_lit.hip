// render_lit.hip -- frames with sun shadows (hmrm_render_lit, hmrm.h): the production march kernel instantiated once more with
// LIT (frame.hpp SunRules; render_fast.hip render_wave_tile): a pixel whose primary ray hit marches its shadow ray through the
// same loop in the same launch, and is darkened when that ray hits.  No hit point, threshold or record goes through memory.
// The production kernels only, as render_interior.hip's -- three projections, three grid modes, leaps and plain groups in the
// three sampling modes, window records for nearest sampling -- in a translation unit of their own: the existing kernels keep
// their argument lists and their instructions.
#undef HMRM_TIMELINE
#define HMRM_RENDER_LIT 1
#include "render_fast.hip"

namespace hmrm {

// k_render_fast's launch shape (one workgroup per tile, grid rows beyond 32768 in blockIdx.z); never a calibration launch.
template <int PROJ, int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_render_lit(const DevFrame f, const RowMap rows,
                                                                                                   const double *__restrict__ thr,
                                                                                                   const uint32_t *__restrict__ cmap,
                                                                                                   uint32_t *__restrict__ out,
                                                                                                   int64_t out_stride_px, int tiles_y,
                                                                                                   StatsOut st, const SegRules seg, const SunRules sun) {
	(void)render_wave_tile<PROJ, false, GWM, LEAP, SAMP, false, true, true>(f, rows, thr, cmap, out, out_stride_px, tiles_y, st, (int)blockIdx.x,
	                                                                   blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6),
	                                                                   (int)(threadIdx.x & 63), RayBatch{}, seg, sun);
}

namespace {
struct Launch {
	const DevFrame &f;
	const RowMap &rows;
	const double *d_thr;
	const uint32_t *d_cmap;
	uint32_t *d_out;
	int64_t out_stride_px;
	StatsOut st;
	SegRules seg;
	SunRules sun;
	dim3 grid;
	int tiles_y;
	hipStream_t stream;
};

template <int PROJ, int GWM, int LEAP, int SAMP>
void launch_one(const Launch &l) {
	hipLaunchKernelGGL((k_render_lit<PROJ, GWM, LEAP, SAMP>), l.grid, dim3(kBlockThreads), 0, l.stream, l.f, l.rows, l.d_thr,
	                   l.d_cmap, l.d_out, l.out_stride_px, l.tiles_y, l.st, l.seg, l.sun);
}

template <int PROJ, int GWM>
void launch_kind(FastKernel kernel, const Launch &l) {
	if (kernel == kRecords) { // (nearest sampling only: launch_render_lit has checked)
		launch_one<PROJ, GWM, kRecords, 0>(l);
	} else if (kernel == kLeaps) {
		if (l.f.sampling == 1) launch_one<PROJ, GWM, kLeaps, 1>(l);
		else if (l.f.sampling == 2) launch_one<PROJ, GWM, kLeaps, 2>(l); // (d_thr is the float table here)
		else launch_one<PROJ, GWM, kLeaps, 0>(l);
	} else {
		if (l.f.sampling == 1) launch_one<PROJ, GWM, kPlainGroups, 1>(l);
		else if (l.f.sampling == 2) launch_one<PROJ, GWM, kPlainGroups, 2>(l);
		else launch_one<PROJ, GWM, kPlainGroups, 0>(l);
	}
}

template <int PROJ>
void launch_gwm(FastKernel kernel, const Launch &l) {
	switch (l.f.grid_mode) {
	case 0: launch_kind<PROJ, 0>(kernel, l); break;
	case 1: launch_kind<PROJ, 1>(kernel, l); break;
	default: launch_kind<PROJ, 2>(kernel, l); break;
	}
}
} // namespace

// `primary_interior`: the primary rays are under the interior rule too (HMRM_TRACE_INTERIOR; the kernel tests each origin).
hipError_t launch_render_lit(const DevFrame &f, const RowMap &rows, const double *d_thr_f64, const float *d_thr32,
                             const uint32_t *d_cmap, uint32_t *d_out, int64_t out_stride_px, unsigned long long *d_counters,
                             FastKernel kernel, const WindowRecord *d_records, const SunRules &sun, bool primary_interior,
                             hipStream_t stream) {
	if (kernel == kRecords && (f.sampling != 0 || !d_records)) return hipErrorInvalidValue;
	if (f.aa_shift != 0 || rows.measure != nullptr) return hipErrorInvalidValue;
	DevFrame fr = f;
	if (kernel == kRecords) fr.mipbuf_bil = reinterpret_cast<const float *>(d_records); // (as launch_fast does)
	const double *d_thr = f.sampling == 2 ? reinterpret_cast<const double *>(d_thr32) : d_thr_f64;
	const int tiles_x = (f.screen_w + kTileW - 1) / kTileW;
	const int tiles_y = (rows.local_rows + kTileH - 1) / kTileH;
	if (tiles_x <= 0 || tiles_y <= 0) return hipSuccess;
	const dim3 grid((unsigned)tiles_x, (unsigned)(tiles_y < 32768 ? tiles_y : 32768), (unsigned)((tiles_y + 32767) / 32768));
	const Launch l{fr, rows, d_thr, d_cmap, d_out, out_stride_px, StatsOut{d_counters, nullptr, nullptr},
	               SegRules{nullptr, 0u, primary_interior ? 1u : 0u}, sun, grid, tiles_y, stream};
	switch (f.projection) {
	case 1: launch_gwm<1>(kernel, l); break;
	case 2: launch_gwm<2>(kernel, l); break;
	default: launch_gwm<3>(kernel, l); break;
	}
	return hipGetLastError();
}

} // namespace hmrm
