// render_fast_aa.hip -- the antialiased instantiations of the production march kernel (hmrm_render_aa, hmrm.h HMRM_AA):
// march_frame.hpp's kernel with its AA epilogue (device_common.hpp store_box_filtered) and nothing else -- a translation
// unit of its own, so that the plain kernels keep their compile and both halves build in parallel.
#undef HMRM_TIMELINE // (the tool-only wave timeline covers the plain kernels: march_frame.hpp)
#include "march_frame.hpp"

namespace hmrm {

hipError_t launch_render_fast_aa(const DevFrame &f, const RowMap &rows, const double *d_thr_f64, const float *d_thr32,
                                 const uint32_t *d_cmap, uint32_t *d_out, int64_t out_stride_px,
                                 unsigned long long *d_counters, uint32_t *d_steps, double *d_entry, bool stats,
                                 FastKernel kernel, const WindowRecord *d_records, hipStream_t stream) {
	return launch_fast<true>(f, rows, d_thr_f64, d_thr32, d_cmap, d_out, out_stride_px, d_counters, d_steps, d_entry, stats,
	                         kernel, d_records, stream);
}

} // namespace hmrm
