// render_fast_aa.hip -- the antialiased instantiations of the production march kernel (hmrm_render_aa, hmrm.h HMRM_AA):
// render_fast.hip compiled a second time with its AA epilogue (device_common.hpp store_box_filtered) and nothing else --
// a translation unit of its own, so that the plain kernels keep their compile and both halves build in parallel.
// The tool-only wave timeline (HMRM_TIMELINE) covers the plain kernels.
#undef HMRM_TIMELINE
#define HMRM_RENDER_FAST_AA 1
#include "render_fast.hip"
