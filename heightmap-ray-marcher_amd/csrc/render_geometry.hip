// render_geometry.hip -- geometry frames (hmrm_render_geometry, hmrm.h): the production march kernel instantiated once more with
// GEOM (frame.hpp GeomPlanes): beside hmrm_render's pixel -- hmrm_render_interior's under the interior rule -- the same launch
// stores the hit cell, the range to int_point and the surface gradient of every pixel, each plane optional.  The production
// kernels only -- three projections, three grid modes, leaps and plain groups in the three sampling modes, window records for
// nearest sampling; no instrumented and no antialiased ones -- in a translation unit of their own, as render_interior.hip is:
// the existing frame kernels keep their argument lists and their instructions.
#include "march.hpp"

namespace hmrm {

// k_render_fast's launch shape (one workgroup per tile, grid rows beyond 32768 in blockIdx.z); never a calibration launch.
template <int PROJ, int GWM, int LEAP, int SAMP>
__global__ __launch_bounds__(kBlockThreads, HMRM_MIN_WAVES) HMRM_OCCUPANCY_ATTR void k_render_geometry(const DevFrame f, const RowMap rows,
                                                                                                   const double *__restrict__ thr,
                                                                                                   const uint32_t *__restrict__ cmap,
                                                                                                   uint32_t *__restrict__ out,
                                                                                                   int64_t out_stride_px, int tiles_y,
                                                                                                   StatsOut st, const SegRules seg,
                                                                                                   const GeomPlanes geo) {
	(void)render_wave_tile<Family<Geometry, PROJ, GWM, LEAP, SAMP>>(
	    f, rows, thr, cmap, out, out_stride_px, tiles_y, st, (int)blockIdx.x, blockIdx.z * 32768u + blockIdx.y, (int)(threadIdx.x >> 6),
	    (int)(threadIdx.x & 63), seg, geo);
}

hipError_t launch_render_geometry(const FrameLaunch &l, FastKernel kernel) {
	return launch_march_family(l, kernel, false, [&](auto proj, auto gwm, auto leap, auto samp, dim3 grid, const auto &...args) {
		hipLaunchKernelGGL((k_render_geometry<proj(), gwm(), leap(), samp()>), grid, dim3(kBlockThreads), 0, l.stream, args..., l.geo);
	});
}

} // namespace hmrm
