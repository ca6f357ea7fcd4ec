// render_baked.hip -- baked-light frames (hmrm_render_baked, hmrm.h): the production march kernel instantiated once more with
// BAKED (march.hpp render_wave_tile; frame.hpp BakedLight): hmrm_render's pixel -- hmrm_render_interior's under the interior
// rule -- and, for a pixel whose primary ray hit, the weight of the scene's light plane at the hit cell (bilinear sampling: mixed
// at the hit point) applied behind the march.  The production kernels only -- three projections, three grid modes, leaps and
// plain groups in the three sampling modes, window records for nearest sampling; the antialiased ones are render_baked_aa.hip's
// -- in a translation unit of their own: the existing kernels keep their argument lists and their instructions.
#include "march.hpp"

namespace hmrm {

// k_render_interior's launch shape and arguments, and the plane; never a calibration launch.
template <int PROJ, int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_render_baked(const DevFrame f, const RowMap rows,
                                                                                                 const double *__restrict__ thr,
                                                                                                 const uint32_t *__restrict__ cmap,
                                                                                                 uint32_t *__restrict__ out,
                                                                                                 int64_t out_stride_px, int tiles_y,
                                                                                                 StatsOut st, const SegRules seg,
                                                                                                 const BakedLight baked) {
	(void)render_wave_tile<Family<Baked, PROJ, GWM, LEAP, SAMP>>(
	    f, rows, thr, cmap, out, out_stride_px, tiles_y, st, (int)blockIdx.x, blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6),
	    (int)(threadIdx.x & 63), seg, baked);
}

hipError_t launch_render_baked(const FrameLaunch &l, FastKernel kernel) {
	if (!l.baked.plane || l.baked.full_scale < 1u || l.baked.full_scale > 65535u || !l.d_out) return hipErrorInvalidValue;
	return launch_march_family(l, kernel, false, [&](auto proj, auto gwm, auto leap, auto samp, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL((k_render_baked<proj(), gwm(), leap(), samp()>), grid, dim3(kBlockThreads), 0, l.stream, args..., l.baked);
	});
}

} // namespace hmrm
