// render.hpp -- launch interface of the device code (render.hip and the march units) for the host side (api_*.cpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "frame.hpp"
#include "march_dispatch.hpp" // (enum FastKernel, enum FrameFamily)

namespace hmrm {

// UpdateHeightmap on the device.  plain=false writes thr[i] = heightmap_buf[i] + min_h and
// folds max(thr) into *d_max_key (order-preserving key, zero-initialised by the caller);
// plain=true writes heightmap_buf[i] itself (test hook).
hipError_t launch_prepare_heights(const uint8_t *d_rgb, double *d_out, int64_t n, double lum_r,
                                  double lum_g, double lum_b, double min_h, double max_h, bool plain,
                                  unsigned long long *d_max_key, hipStream_t stream);
double max_key_to_double(unsigned long long key);

// One frame launch: a pass of the pixel loop over the rows described by `rows`, into d_out (uint32 RGBA per pixel,
// out_stride_px pixels per local row).  Everything a frame launcher takes, named: a launcher reads what its family needs.
// f.aa_shift != 0 selects the family's antialiased kernels: f is then the super frame, every sample is rendered (lit, shaded)
// on its own and the launch writes the box-filtered frame, (f.screen_w >> f.aa_shift) pixels wide, into d_out.
struct FrameLaunch {
	// the tables the scene owns: f.sampling == 2 reads the float copy of the table (d_thr32, launch_thr_to_float) instead of
	// d_thr; d_records (launch_build_records) is read by kRecords only
	const double *d_thr;
	const float *d_thr32;
	const uint32_t *d_cmap;
	const WindowRecord *d_records;
	// the target.  d_counters: 3 x uint64 {steps, hits, capped} (+ diagnostics); steps / hits and the per-pixel d_steps / d_entry
	// are only filled when stats, and only by the plain family; [2] counts capped primary and capped shadow rays, per sample
	uint32_t *d_out;
	int64_t out_stride_px;
	unsigned long long *d_counters;
	uint32_t *d_steps;
	double *d_entry;
	bool stats;
	const DevFrame &f;
	const RowMap &rows;
	// kFramePlain may be a measured launch (rows.measure); the others refuse one.  kFrameInterior (hmrm_render_interior): every
	// primary ray under the interior rule.  kFrameLit (hmrm_render_lit): a hit pixel's shadow ray is marched in the same launch.
	// kFrameShaded (hmrm_render_shaded): no shadow rays, neither sun.step_dist nor sun.max_steps is looked at, every hit pixel
	// at the weight of its diffuse level.  kFrameLitShaded: kFrameLit whose lit pixels get that weight.
	FrameFamily family;
	SunRules sun;          // the lit and shaded families: direction, shadow march and ambient level (frame.hpp)
	bool primary_interior; // ... and whether their primary rays are under the interior rule too (the geometry family's as well)
	// kFrameGeometry (hmrm_render_geometry): the frame of the plain or, with primary_interior, the interior family, and the planes
	// of `geo` the same launch stores beside it (frame.hpp GeomPlanes; d_out may be null then: no colour plane)
	GeomPlanes geo;
	hipStream_t stream;
	// kFrameLitSum (hmrm_render_lit_sum): kFrameLit whose shadow march runs once per direction of the list, the weights summed;
	// sun.dir is not looked at, d_out may be null (no colour plane) and so may lsum.light (frame.hpp LightSum)
	LightSum lsum = LightSum{nullptr, nullptr, 0, 0, 0u};
	// kFrameBaked (hmrm_render_baked): the frame of the plain or, with primary_interior, the interior family, whose hit pixels
	// take the weight of the scene's light plane (frame.hpp BakedLight); antialiased with f.aa_shift
	BakedLight baked = BakedLight{nullptr, 0u};
	// kFrameWater (hmrm_render_water): the frame of the plain or, with primary_interior, the interior family, whose hit pixels at
	// or below water.level march a mirror ray in the same launch and take its pixel blended in (frame.hpp WaterRules).
	// kFrameWaterAA, kFrameWaterBaked, kFrameWaterBakedAA (hmrm_render_water_aa): that frame antialiased with f.aa_shift, under
	// `baked` (both the primary and the mirror pixel take the weight of their own hit's light before the blend), and both
	// kFrameWaterLit (hmrm_render_water_lit): kFrameWater's frame under `sun`, both sides of the mirror at hmrm_render_shaded's weight;
	// the two shade flags travel in water.flags (frame.hpp kWaterSunDiffuse, kWaterSunNoShadows); no AA
	WaterRules water = WaterRules{0.0, 0.0, 0u, 0u, 0u, 0u};
	// kFrameHaze (hmrm_render_haze): the frame of the plain or, with primary_interior, the interior family, whose pixels are blended
	// towards the haze colour by the table's byte at their range (frame.hpp HazeRules); antialiased with f.aa_shift
	HazeRules haze = HazeRules{nullptr, 0.0, 0.0, 0u, 0u, 0u};
	// kFrameViews (hmrm_render_views): n_views frames of the plain or, with primary_interior, the interior family in one launch.
	// d_frames: their records in device memory, complete (tables, pyramid -- or, for kRecords, the record table -- and knobs); `f` is
	// view 0's record on the host, for what the launch dispatches on; view k lands at d_out + k * view_stride_px; `rows` is the
	// identity of one view
	const DevFrame *d_frames = nullptr;
	int32_t n_views = 0;
	int64_t view_stride_px = 0;
};
// The production kernels (march.hpp; one translation unit per family and AA variant, launch_common.hpp): speculative step groups
// (kPlainGroups), plus exact leaps over empty pyramid windows (kLeaps), or over windows of the record level that are empty but
// for a few recorded cells the ray's path misses (kRecords: nearest sampling only).
hipError_t launch_frame_march(const FrameLaunch &l, FastKernel kernel);
// The literal one-step-at-a-time loop (render.hip), nearest sampling only.  Same outputs.
hipError_t launch_frame_literal(const FrameLaunch &l);
// Ray batches (hmrm_trace_rays; render_rays.hip): batch.n caller-supplied rays through the same march, one hmrm_ray_hit
// record per ray.  `f` is a DevFrame without a camera -- projection 4, kBatchW pixels wide, at least ceil(n / kBatchW) rows
// (frame.hpp RayBatch); the row map is the identity.  d_counters[2] counts the rays stopped by the step cap, nothing else
// is counted.  launch_trace_rays_literal (render.hip): the literal loop, nearest sampling only.
hipError_t launch_trace_rays(const DevFrame &f, const double *d_thr, const float *d_thr32, const uint32_t *d_cmap,
                             const RayBatch &batch, unsigned long long *d_counters, FastKernel kernel,
                             const WindowRecord *d_records, hipStream_t stream);
hipError_t launch_trace_rays_literal(const DevFrame &f, const double *d_thr, const uint32_t *d_cmap, const RayBatch &batch,
                                     unsigned long long *d_counters, hipStream_t stream);
// The same two under the segment rules (frame.hpp SegRules; hmrm_trace_segments -- render_segments.hip, kernels of its own --
// and the literal loop in render.hip).  Records: status 3 (HMRM_RAY_END) for a ray ended by its own limit inside the grid;
// d_counters[2] counts CAPPED rays only.
hipError_t launch_trace_segments(const DevFrame &f, const double *d_thr, const float *d_thr32, const uint32_t *d_cmap,
                                 const RayBatch &batch, const SegRules &seg, unsigned long long *d_counters, FastKernel kernel,
                                 const WindowRecord *d_records, hipStream_t stream);
hipError_t launch_trace_segments_literal(const DevFrame &f, const double *d_thr, const uint32_t *d_cmap, const RayBatch &batch,
                                         const SegRules &seg, unsigned long long *d_counters, hipStream_t stream);
// Cell maps (hmrm_cell_map; frame.hpp CellRules; render_cells.hip: the segment march with a lane per map cell, and the literal
// loop in render.hip, nearest sampling only).  `f` is a DevFrame without a camera whose "frame" is the rect: projection 5,
// screen_w x screen_h = the rect's w x h, step_dist the rays'.  One byte per cell at d_out[row * stride_bytes + column] (no
// alignment asked); d_counters[2] counts CAPPED rays only.
hipError_t launch_cell_map(const DevFrame &f, const double *d_thr, const float *d_thr32, uint8_t *d_out, int64_t stride_bytes,
                           const CellRules &cells, unsigned long long *d_counters, FastKernel kernel, const WindowRecord *d_records,
                           hipStream_t stream);
hipError_t launch_cell_map_literal(const DevFrame &f, const double *d_thr, uint8_t *d_out, int64_t stride_bytes, const CellRules &cells,
                                   unsigned long long *d_counters, hipStream_t stream);
// Accumulated cell maps (hmrm_cell_map_sum; frame.hpp CellSums; render_cell_sums.hip, and the literal loop in render.hip, nearest
// sampling only): the same launch with the march run once per target of sums.targets (device memory) and one uint16 per cell at
// (char *)d_out + row * stride_bytes + 2 * column (2-byte aligned); cells.target is not looked at.  d_counters[2] counts CAPPED
// rays, one per ray: up to sums.n per cell.
hipError_t launch_cell_map_sum(const DevFrame &f, const double *d_thr, const float *d_thr32, uint16_t *d_out, int64_t stride_bytes,
                               const CellRules &cells, const CellSums &sums, unsigned long long *d_counters, FastKernel kernel,
                               const WindowRecord *d_records, hipStream_t stream);
hipError_t launch_cell_map_sum_literal(const DevFrame &f, const double *d_thr, uint16_t *d_out, int64_t stride_bytes,
                                       const CellRules &cells, const CellSums &sums, unsigned long long *d_counters, hipStream_t stream);
// The record table of the thr table: rec_row(map_w) x ceil(map_h / 4) WindowRecords.
hipError_t launch_build_records(const double *d_thr, int map_w, int map_h, WindowRecord *d_dst, hipStream_t stream);
// thr32[i] = (float)thr[i], round to nearest (the "float heights" mode).
hipError_t launch_thr_to_float(const double *d_thr, float *d_thr32, int64_t n, hipStream_t stream);
// 3x3 maximum filter of the thr table (bounds every bilinear interpolation: render_fast.hip k_dilate3x3).
hipError_t launch_dilate3x3(const double *d_thr, int w, int h, double *d_dst, hipStream_t stream);
// Window-maximum pyramid (see march.hpp): level 0 from the thr table, level l+1 from level l.
// `pitch` = row pitch (floats) of every plane of the pyramid buffer (DevFrame::mip_row).
hipError_t launch_build_mip0(const double *d_thr, int map_w, int map_h, float *d_dst, int dst_w, int dst_h,
                             int pitch, hipStream_t stream);
hipError_t launch_build_mip_up(const float *d_src, int src_w, int src_h, float *d_dst, int dst_w, int dst_h,
                               int pitch, int src_level, hipStream_t stream);
// A light plane of bytes widened to 16-bit words (hmrm_scene_set_light_device, HMRM_LIGHT_U8; render.hip): w x h bytes, rows
// src_stride bytes apart, into w x h packed uint16.
hipError_t launch_widen_light(const uint8_t *d_src, size_t src_stride, int w, int h, uint16_t *d_dst, hipStream_t stream);
// round-up-to-float of a double (the pyramid's rounding), on the host: for the whole-map element
float round_up_to_float_host(double v);

// Pixel tile (= workgroup) shape of the frame launches.
void render_tile_shape(int *tile_w, int *tile_h);

// GetRay + distance() of pixel (px,py): d_out7 = pos[3], dir[3], d.
hipError_t launch_probe(const DevFrame &f, int px, int py, double *d_out7, hipStream_t stream);

// Launch-order calibration (RowMap::measure): device records of tile_rows x kMeasureStride words, zeroed before a
// measured launch and reduced afterwards to {start of the row's first workgroup, longest wave of the row} per tile row
// in pinned (device-mapped) host memory -- both small kernels of the launch stream.
hipError_t launch_measure_init(unsigned long long *d_rec, int tile_rows, hipStream_t stream);
hipError_t launch_measure_readback(const unsigned long long *d_rec, unsigned long long *h_pinned_dev, int tile_rows, hipStream_t stream);

// n doubles from pinned (device-mapped) host memory into device memory, as a kernel on `stream` (render.hip).
hipError_t launch_upload_tables(const double *h_pinned, double *d_dst, size_t n, hipStream_t stream);

// v_rcp_f64 accuracy probe (render.hip k_rcp_error): d_out65[0] = max relative error as fp64 bits, [1..64] = histogram
// by binary order of magnitude; the caller zeroes d_out65.
hipError_t launch_rcp_error(int mode, uint64_t count, uint64_t seed, int exp_lo, int exp_hi,
                            unsigned long long *d_out65, hipStream_t stream);

} // namespace hmrm
