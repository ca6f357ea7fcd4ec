// render_fast_aa.hip -- the antialiased instantiations of the production march kernel (hmrm_render_aa, hmrm.h HMRM_AA):
// march_frame.hpp's kernel with its AA epilogue (device_common.hpp store_box_filtered) and nothing else -- a translation
// unit of its own, so that the plain kernels keep their compile and both halves build in parallel.
#undef HMRM_TIMELINE // (the tool-only wave timeline covers the plain kernels: march_frame.hpp)
#include "march_frame.hpp"

namespace hmrm {

hipError_t launch_render_fast_aa(const FrameLaunch &l, FastKernel kernel) {
	return launch_fast<true>(l.f, l.rows, l.d_thr, l.d_thr32, l.d_cmap, l.d_out, l.out_stride_px, l.d_counters, l.d_steps, l.d_entry,
	                         l.stats, kernel, l.d_records, l.stream);
}

} // namespace hmrm
