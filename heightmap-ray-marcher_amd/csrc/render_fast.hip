// render_fast.hip -- the plain frame instantiations of the production march kernel (march.hpp, march_frame.hpp), and what
// is this unit's alone: the pyramid, record, calibration and float-table kernels with their launchers, and the tool-only
// wave timeline.
#ifdef HMRM_TIMELINE
#include <cstdio>
#include <cstdlib>
#endif
#include "march_frame.hpp"

namespace hmrm {

// Tool build only (-DHMRM_TIMELINE, tools/timeline.py): every wave of the production (non-instrumented) kernel
// stores its start and end time (s_memrealtime) and the XCD it ran on into a device buffer (not pinned host memory:
// 129 600 records per 0.1 ms launch were 24 GB/s of PCIe writes, which disturbed what they measured); the library
// copies the last launch's records out to $HMRM_TIMELINE_FILE when the process ends.  Not compiled into the product.
#ifdef HMRM_TIMELINE
struct TimelineRec { unsigned long long t0, t1; unsigned int xcc, pad; };
__device__ TimelineRec *g_timeline = nullptr;
__device__ __forceinline__ void timeline_wave_done(unsigned long long t0) {
	if (!g_timeline || (threadIdx.x & 63) != 0) return;
	unsigned xcc;
	asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
	const size_t wave = ((size_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (kBlockThreads / 64) + (threadIdx.x >> 6);
	g_timeline[wave] = TimelineRec{t0, (unsigned long long)__builtin_amdgcn_s_memrealtime(), xcc, 0u};
}
static void timeline_before_launch(dim3 grid, int tiles_y, const RowMap &rows) {
	static TimelineRec *host = nullptr, *devbuf = nullptr;
	static size_t cap = 0, used = 0;
	static int gx = 0, gy = 0, ty = 0, segs[7] = {0, 0, 0, 0, 0, 0, 0};
	const size_t waves = (size_t)grid.x * grid.y * grid.z * (kBlockThreads / 64);
	if (waves > cap) {
		(void)hipDeviceSynchronize();
		free(host);
		if (devbuf) (void)hipFree(devbuf);
		host = (TimelineRec *)malloc(waves * sizeof(TimelineRec));
		(void)hipMalloc((void **)&devbuf, waves * sizeof(TimelineRec));
		cap = waves;
		(void)hipMemcpyToSymbol(HIP_SYMBOL(g_timeline), &devbuf, sizeof devbuf);
		static bool registered = false;
		if (!registered) {
			registered = true;
			atexit([] {
				const char *path = getenv("HMRM_TIMELINE_FILE");
				if (!path || !host || !devbuf) return;
				(void)hipDeviceSynchronize();
				if (hipMemcpy(host, devbuf, used * sizeof(TimelineRec), hipMemcpyDeviceToHost) != hipSuccess) return;
				if (FILE *fp = fopen(path, "wb")) {
					const int hdr[12] = {gx, gy, kBlockThreads / 64, (int)used, ty, segs[0], segs[1], segs[2], segs[3], segs[4], segs[5], segs[6]};
					fwrite(hdr, sizeof hdr, 1, fp);
					fwrite(host, sizeof(TimelineRec), used, fp);
					fclose(fp);
				}
			});
		}
	}
	used = waves;
	gx = (int)grid.x;
	gy = (int)(grid.y * grid.z);
	for (int k = 0; k < 3; ++k) segs[k] = rows.seg_first[k];
	for (int k = 0; k < 4; ++k) segs[3 + k] = rows.seg_delta[k];
	ty = tiles_y;
}
#endif

// ---------------------------------------------------------------- pyramid ----
__host__ __device__ __forceinline__ float round_up_to_float(double v) {
	float r = (float)v;
	if ((double)r < v) { // conversion rounded down (v finite): next float towards +inf
		uint32_t b;
		__builtin_memcpy(&b, &r, sizeof b);
		if (r == 0.0f) b = 1u;                 // smallest positive subnormal
		else if (b & 0x80000000u) b -= 1u;     // negative: magnitude shrinks
		else b += 1u;                          // positive: magnitude grows (max float -> +inf)
		__builtin_memcpy(&r, &b, sizeof r);
	}
	return r;
}
float round_up_to_float_host(double v) { return round_up_to_float(v); }

// Level 0: window (ix,iy) = max of thr over the 4 x 4 cells from (S0 ix, S0 iy), clipped; NaN ignored.
__global__ __launch_bounds__(256) void k_build_mip0(const double *__restrict__ thr, int map_w, int map_h,
                                                    float *__restrict__ dst, int dst_w, int dst_h, int pitch) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (int64_t)dst_w * dst_h) return;
	const int ix = (int)(i % dst_w), iy = (int)(i / dst_w);
	double m = -__builtin_huge_val();
	constexpr int S0 = 1 << mip_stride_shift(0); // level 0: 4-cell windows every S0 cells
	for (int yy = S0 * iy; yy < S0 * iy + 4 && yy < map_h; ++yy)
		for (int xx = S0 * ix; xx < S0 * ix + 4 && xx < map_w; ++xx) {
			const double v = thr[(int64_t)yy * map_w + xx];
			if (v > m) m = v;
		}
	dst[mip_index(ix, iy, pitch)] = round_up_to_float(m);
}

// Level l+1 from level l.  A level-l window is src_strides strides of level l wide; the window F = 2^kLevelStep times
// as large that starts at stride i of level l+1 (= stride_ratio * i of level l) is the union of the level-l windows with
// indices stride_ratio * i + {0, src_strides, .., src_strides * (F - 1)} per axis.
__global__ __launch_bounds__(256) void k_build_mip_up(const float *__restrict__ src, int src_w, int src_h,
                                                      float *__restrict__ dst, int dst_w, int dst_h, int pitch,
                                                      int stride_ratio, int src_strides) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (int64_t)dst_w * dst_h) return;
	const int ix = (int)(i % dst_w), iy = (int)(i / dst_w);
	constexpr int F = 1 << kLevelStep;
	float m = -__builtin_huge_valf();
	for (int b = 0; b < F; ++b) {
		const int yy = stride_ratio * iy + src_strides * b;
		if (yy >= src_h) break;
		for (int a = 0; a < F; ++a) {
			const int xx = stride_ratio * ix + src_strides * a;
			if (xx >= src_w) break;
			const float v = src[mip_index(xx, yy, pitch)];
			if (v > m) m = v;
		}
	}
	dst[mip_index(ix, iy, pitch)] = m;
}

// 3x3 maximum filter of the thr table (edges clamped, NaN ignored) plus a rounding margin:
// every bilinear interpolation that a position inside cell c can see mixes four cells of c's
// 3x3 neighbourhood, so in exact arithmetic it is at most their maximum m; the six roundings
// of bil_mix can push it above m by a few ulp of the largest magnitude A involved (differences
// reach 2A), hence the bound m + A * 2^-45.  A pyramid built from these values bounds the
// interpolated thresholds of all positions whose cell lies in a window.
__global__ __launch_bounds__(256) void k_dilate3x3(const double *__restrict__ thr, int w, int h,
                                                   double *__restrict__ dst) {
	const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (int64_t)w * h) return;
	const int x = (int)(i % w), y = (int)(i / w);
	double m = -__builtin_huge_val(), a = 0.0;
	for (int yy = max(y - 1, 0); yy <= min(y + 1, h - 1); ++yy)
		for (int xx = max(x - 1, 0); xx <= min(x + 1, w - 1); ++xx) {
			const double v = thr[(int64_t)yy * w + xx];
			if (v > m) m = v;
			if (__builtin_fabs(v) > a) a = __builtin_fabs(v);
		}
	dst[i] = m + a * 0x1p-45; // (inf stays inf; all-NaN neighbourhoods give -inf: never a hit there)
}

hipError_t launch_dilate3x3(const double *d_thr, int w, int h, double *d_dst, hipStream_t stream) {
	const int64_t n = (int64_t)w * h;
	hipLaunchKernelGGL(k_dilate3x3, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_thr, w, h, d_dst);
	return hipGetLastError();
}

hipError_t launch_build_mip0(const double *d_thr, int map_w, int map_h, float *d_dst, int dst_w, int dst_h,
                             int pitch, hipStream_t stream) {
	const int64_t n = (int64_t)dst_w * dst_h;
	hipLaunchKernelGGL(k_build_mip0, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_thr, map_w,
	                   map_h, d_dst, dst_w, dst_h, pitch);
	return hipGetLastError();
}

hipError_t launch_build_mip_up(const float *d_src, int src_w, int src_h, float *d_dst, int dst_w, int dst_h,
                               int pitch, int src_level, hipStream_t stream) {
	const int64_t n = (int64_t)dst_w * dst_h;
	const int stride_ratio = 1 << (mip_stride_shift(src_level + 1) - mip_stride_shift(src_level));
	hipLaunchKernelGGL(k_build_mip_up, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_src, src_w,
	                   src_h, d_dst, dst_w, dst_h, pitch, stride_ratio, win_strides(src_level));
	return hipGetLastError();
}

// ---------------------------------------------------------------- window records ----
// One thread per window of the record level: the nine highest cells of its 16 x 16 (clipped at the map's edge, NaN ignored
// as in the pyramid), kept sorted by insertion.  The ninth is max2; the eight above it are recorded where they are
// strictly higher.
__global__ __launch_bounds__(256) void k_build_records(const double *__restrict__ thr, int map_w, int map_h,
                                                       WindowRecord *__restrict__ dst, int rw, int rh) {
	const int ix = (int)(blockIdx.x * 16u + (threadIdx.x & 15u)), iy = (int)(blockIdx.y * 16u + (threadIdx.x >> 4));
	if (ix >= rw || iy >= rh) return;
	constexpr int S = win_cells(kRecLevel), N = kRecCells + 1;
	const int wx0 = ix << mip_stride_shift(kRecLevel), wy0 = iy << mip_stride_shift(kRecLevel);
	double t[N];
	uint32_t at[N]; // row << 8 | column inside the window
#pragma unroll
	for (int j = 0; j < N; ++j) {
		t[j] = -__builtin_huge_val();
		at[j] = 0xffffu;
	}
	// A row at a time: its 16 loads are in flight together (one load per trip of a cell loop left the kernel waiting for
	// memory 256 times per window), and a row whose maximum does not reach the ninth-highest so far -- most rows -- costs
	// 16 maxima and one comparison.
	const int cols = min(S, map_w - wx0); // (>= 1)
	for (int r = 0; r < S && wy0 + r < map_h; ++r) {
		const double *row = thr + (size_t)(wy0 + r) * (size_t)map_w + wx0;
		double v[S];
#pragma unroll
		for (int c = 0; c < S; ++c) {
			const double x = row[c < cols ? c : cols - 1]; // (never past the row's end)
			v[c] = c < cols ? x : -__builtin_huge_val();
		}
		double m = v[0];
#pragma unroll
		for (int c = 1; c < S; ++c) m = __builtin_fmax(m, v[c]); // (fmax skips NaN, as the pyramid does)
		if (!(m > t[N - 1])) continue;
#pragma unroll
		for (int c = 0; c < S; ++c) {
			if (!(v[c] > t[N - 1])) continue; // (NaN too)
			t[N - 1] = v[c];
			at[N - 1] = (uint32_t)(r << 8 | c);
#pragma unroll
			for (int j = N - 1; j > 0; --j) {
				const bool up = t[j] > t[j - 1];
				const double tv = t[j];
				const uint32_t ta = at[j];
				t[j] = up ? t[j - 1] : t[j];
				at[j] = up ? at[j - 1] : at[j];
				t[j - 1] = up ? tv : t[j - 1];
				at[j - 1] = up ? ta : at[j - 1];
			}
		}
	}
	WindowRecord rec;
	rec.max2 = round_up_to_float(t[N - 1]);
	rec.spare0 = 0u;
	rec.spare1[0] = rec.spare1[1] = 0u;
	uint32_t xs[2] = {0u, 0u}, ys[2] = {0u, 0u};
#pragma unroll
	for (int j = 0; j < kRecCells; ++j) {
		const bool keep = t[j] > t[N - 1];
		xs[j >> 2] |= (keep ? (at[j] & 0xffu) : 0xffu) << (8 * (j & 3));
		ys[j >> 2] |= (keep ? (at[j] >> 8) : 0xffu) << (8 * (j & 3));
	}
	rec.xs[0] = xs[0]; rec.xs[1] = xs[1];
	rec.ys[0] = ys[0]; rec.ys[1] = ys[1];
	dst[(size_t)iy * (size_t)rw + ix] = rec;
}

hipError_t launch_build_records(const double *d_thr, int map_w, int map_h, WindowRecord *d_dst, hipStream_t stream) {
	const int rw = rec_row(map_w), rh = (map_h + 3) >> 2;
	const dim3 grid((unsigned)((rw + 15) / 16), (unsigned)((rh + 15) / 16));
	if (grid.y > 65535u) return hipErrorInvalidValue; // (api_scene.cpp does not build records for such maps)
	hipLaunchKernelGGL(k_build_records, grid, dim3(256), 0, stream, d_thr, map_w, map_h, d_dst, rw, rh);
	return hipGetLastError();
}

// Calibration records (RowMap::measure): kMeasureStride words per tile row, see k_render_fast's last lines.
__global__ __launch_bounds__(256) void k_measure_init(unsigned long long *rec, int n_words) {
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (i < n_words) rec[i] = 0ull;
}
// -> host_dst[2 t] = start of tile row t, host_dst[2 t + 1] = its longest wave
__global__ __launch_bounds__(256) void k_measure_readback(const unsigned long long *__restrict__ rec, unsigned long long *__restrict__ host_dst, int tile_rows) {
	const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (t >= tile_rows) return;
	const unsigned long long *r = rec + (size_t)t * kMeasureStride;
	unsigned long long m = 0;
	for (int k = 1; k < kMeasureStride; ++k) m = r[k] > m ? r[k] : m;
	host_dst[2 * t] = r[0];
	host_dst[2 * t + 1] = m;
}
hipError_t launch_measure_init(unsigned long long *d_rec, int tile_rows, hipStream_t stream) {
	const int n = tile_rows * kMeasureStride;
	hipLaunchKernelGGL(k_measure_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_rec, n);
	return hipGetLastError();
}
hipError_t launch_measure_readback(const unsigned long long *d_rec, unsigned long long *h_pinned_dev, int tile_rows, hipStream_t stream) {
	hipLaunchKernelGGL(k_measure_readback, dim3((unsigned)((tile_rows + 255) / 256)), dim3(256), 0, stream, d_rec, h_pinned_dev, tile_rows);
	return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_thr_to_float(const double *__restrict__ thr, float *__restrict__ dst, int64_t n) {
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = (float)thr[i];
}

hipError_t launch_thr_to_float(const double *d_thr, float *d_thr32, int64_t n, hipStream_t stream) {
	int64_t blocks = (n + 255) / 256;
	if (blocks > 256 * 16) blocks = 256 * 16;
	hipLaunchKernelGGL(k_thr_to_float, dim3((unsigned)(blocks < 1 ? 1 : blocks)), dim3(256), 0, stream, d_thr, d_thr32, n);
	return hipGetLastError();
}

hipError_t launch_render_fast(const FrameLaunch &l, FastKernel kernel) {
	return launch_fast<false>(l.f, l.rows, l.d_thr, l.d_thr32, l.d_cmap, l.d_out, l.out_stride_px, l.d_counters, l.d_steps, l.d_entry,
	                          l.stats, kernel, l.d_records, l.stream);
}

// The family's unit, and its antialiased one for a frame with a factor (launch_common.hpp).
hipError_t launch_frame_march(const FrameLaunch &l, FastKernel kernel) {
	const bool aa = l.f.aa_shift != 0;
	switch (l.family) {
	case kFrameInterior: return launch_render_interior(l, kernel); // (refuses a factor)
	case kFrameLit: return aa ? launch_render_lit_aa(l, kernel) : launch_render_lit(l, kernel);
	case kFrameShaded: return aa ? launch_render_shaded_aa(l, kernel) : launch_render_shaded(l, kernel);
	case kFrameLitShaded: return aa ? launch_render_lit_shaded_aa(l, kernel) : launch_render_lit_shaded(l, kernel);
	case kFrameGeometry: return launch_render_geometry(l, kernel); // (refuses a factor)
	case kFrameLitSum: return launch_render_lit_sum(l, kernel); // (refuses a factor)
	case kFrameBaked: return aa ? launch_render_baked_aa(l, kernel) : launch_render_baked(l, kernel);
	case kFrameWater: return launch_render_water(l, kernel); // (refuses a factor)
	case kFrameWaterAA: return launch_render_water_aa(l, kernel); // (refuses a frame without one)
	case kFrameWaterBaked: return launch_render_water_baked(l, kernel); // (refuses a factor)
	case kFrameWaterBakedAA: return launch_render_water_baked_aa(l, kernel); // (refuses a frame without one)
	case kFrameWaterLit: return launch_render_water_lit(l, kernel); // (refuses a factor)
	case kFrameHaze: return aa ? launch_render_haze_aa(l, kernel) : launch_render_haze(l, kernel);
	case kFrameViews: return launch_render_views(l, kernel); // (refuses a factor)
	default: return aa ? launch_render_fast_aa(l, kernel) : launch_render_fast(l, kernel);
	}
}

void render_tile_shape(int *tile_w, int *tile_h) {
	*tile_w = kTileW;
	*tile_h = kTileH;
}

} // namespace hmrm
