// api_internal.hpp -- what the translation units behind the C ABI (api_*.cpp) share: the grow-only scratch buffer, the scene and
// the launch state it keeps per stream, the ticket kinds, the request a frame entry point hands to the launch path, and the
// functions that cross those files.  Not installed and not included by include/hmrm.h.
//   api_scene.cpp    scene lifetime: create, update, destroy; knobs, stream contexts, pyramids, records, the light plane, read-backs; the
//                    per-thread error text
//   api_launch.cpp   the frame launch path: the cached per-camera record, calibration and probe, launch_frame; the capped-ray
//                    count and the tail of a host-memory call
//   api_frames.cpp   the frame entry points: synchronous, tickets (and their pool), rows, multi, bench; the plane checker
//   api_queries.cpp  ray batches, segments, cell maps and their sums, pick
//   api_aux.cpp      config, image IO and the debug hooks
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hmrm.h"
#include "frame.hpp"
#include "launch_order.hpp"
#include "render.hpp"

// (internal to the library: none of this is exported)
#pragma GCC visibility push(hidden)
namespace hmrm {
extern thread_local std::string g_error; // hmrm_last_error's text: one per thread for the whole library (api_scene.cpp)
int fail(int code, const std::string &msg);
} // namespace hmrm
using namespace hmrm; // (the api_*.cpp units only: their entry points are C functions outside the namespace)

#define HIP_TRY(expr)                                                                         \
	do {                                                                                      \
		hipError_t e_ = (expr);                                                               \
		if (e_ != hipSuccess)                                                                 \
			return fail(HMRM_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));    \
	} while (0)

// Environment knobs: read ONCE per scene at creation; the launch path never calls
// getenv.  hmrm_debug_reload_env() re-reads them for a scene (tests and tools switch kernels on a
// live scene).
struct Knobs {
	int64_t step_cap = (int64_t)1 << 26; // HMRM_STEP_CAP
	int kernel = 0;                      // HMRM_KERNEL: 0 leap, 1 group, 2 simple, 3 rec (window records; nearest sampling, else the plain groups)
	bool tile_order = true;              // HMRM_TILE_ORDER=0 -> row-major launch order
	int order_mode = 2;                  // HMRM_TILE_ORDER=1 -> plain rotation; 2 (default) -> rotation, then calibrated from measurement
	int diag_mode = 0;                   // HMRM_DIAG_ITERS (tools)
	int min_level = -1;                  // HMRM_MIN_LEVEL (tools)
	int finest_pause = -1;               // HMRM_FINEST_PAUSE (tools)
	bool order_verbose = false;          // HMRM_ORDER_VERBOSE=1 (tools): report every calibration on stderr
	bool try_group = true;               // HMRM_TRY_GROUP=0: the calibration does not time the plain-groups kernel against the leap kernel
	int min_plane_shift = 0;             // HMRM_DEBUG_PLANE_SHIFT (tests): log2 of the pyramid's plane pitch is at least this
	int seg_n = 0;                       // HMRM_TILE_SEGMENTS=b0:c0,b1:c1,.. (tools): tile-row pieces to start first, in this order
	int seg_b[3] = {0, 0, 0}, seg_c[3] = {0, 0, 0};
};

// A grow-only allocation, capacity in BYTES: the staging of the host-memory entry points (device memory) and of the frames that
// cross PCIe behind the caller's back (pinned host memory).  reserve() keeps what is there when it is large enough; else it frees
// first -- nothing in flight may use the buffer: s->mu held, the stream drained by the previous host call or the slot free --
// and an allocation that fails leaves an empty buffer.  A plain member: hmrm_scene_destroy releases by hand, after hipSetDevice.
template <bool kPinned> struct Scratch {
	void *ptr = nullptr;
	size_t cap = 0;
	int reserve(size_t bytes) {
		if (bytes <= cap) return HMRM_OK;
		release();
		if (kPinned) HIP_TRY(hipHostMalloc(&ptr, bytes, hipHostMallocDefault));
		else HIP_TRY(hipMalloc(&ptr, bytes));
		cap = bytes;
		return HMRM_OK;
	}
	template <class T> T *as() const { return static_cast<T *>(ptr); }
	void release() {
		if (ptr) (void)(kPinned ? hipHostFree(ptr) : hipFree(ptr));
		ptr = nullptr;
		cap = 0;
	}
};
using DeviceScratch = Scratch<false>;
using PinnedScratch = Scratch<true>;

constexpr int kFrameSlots = 64;  // cached per-frame records (and spherical tables) per stream: a 64-frame orbit fits
constexpr int kMaxMeasRows = 512;  // tile rows (8192 frame rows) a launch order is calibrated for; taller frames keep the rotation
constexpr int kProbeAfterFrames = 6; // full frames of never-repeating cameras before the scene's shadow probe
constexpr int kMaxStreamCtx = 32; // streams a scene keeps launch state for (more: the least recently used one is recycled, behind a device sync)

// One cached per-frame record: the result of the host set-up (camera.cpp) for one camera, and for
// spherical cameras its sin/cos tables on the device.  A pure function of (camera, scene params,
// map size, thr_max), so a repeated camera re-renders without the libm calls or the upload.
struct FrameSlot {
	bool valid = false;
	uint64_t stamp = 0; // last use (LRU)
	hmrm_camera cam{};
	hmrm_scene_params params{};
	uint64_t thr_max_bits = 0;
	hmrm::DevFrame frame{};
	std::vector<float> row_cost; // per kCostRows screen rows: longest in-box ray, in steps (launch order hint)
	double *d_tables = nullptr;  // spherical sin/cos tables: this slot's piece of the context's arenas
	double *h_tables = nullptr;  // pinned staging, likewise
	hipEvent_t uploaded = nullptr; // after the H2D copy out of h_tables: the host may rewrite them then
	// launch order calibrated by measurement, and -- for one record per scene -- the kernel probe: launch_order.hpp
	hmrm::OrderCalibration cal;
	int meas_rows = 0;             // tile rows of the measured launch in flight
	hipEvent_t measured = nullptr; // after the read-back of a measured launch
};

// View batches (hmrm_render_views): a batch's frame records and its distinct spherical tables are written by the host into one
// pinned, device-mapped block and copied into the context's device arena by a small kernel of the launch stream (render.hpp
// launch_upload_tables), as a cached record's tables are -- no host wait.  `uploaded` is recorded behind that kernel: the host
// rewrites a block only when the event has passed, and takes another block of the ring while it has not (FrameSlot::uploaded's
// rule, without its wait).  With every block of the ring in flight the host waits for the oldest.
struct ViewStage {
	double *h = nullptr, *h_dev = nullptr; // pinned memory and the same as the device sees it
	size_t cap = 0;                        // doubles
	hipEvent_t uploaded = nullptr;
	bool used = false; // `uploaded` has been recorded at least once
	uint64_t stamp = 0;
};
constexpr int kViewStages = 4;
// The bytes a batch may stage: n records and the distinct tables (hmrm.h HMRM_MAX_VIEWS_STAGING).
constexpr size_t kMaxViewStagingBytes = (size_t)256 << 20;
// A device arena that was outgrown while launches of its stream might still read it: freed once `after`, recorded on the stream
// when it was replaced, has passed -- looked at by the stream's next batch -- or with the context.
struct RetiredArena {
	void *ptr;
	hipEvent_t after;
};

// Everything a launch mutates, per HIP stream: launches on different streams of one scene never
// share a table or a counter (hmrm_render_rows_device takes the caller's stream).
struct StreamCtx {
	hipStream_t stream = nullptr;
	bool scene_owned = false; // the scene's own stream or one of its launch lanes: never recycled
	uint64_t stamp = 0;
	FrameSlot slots[kFrameSlots];
	// table storage of all slots: one device and one pinned allocation per context (a slot's first use would
	// otherwise cost a hipMalloc + hipHostMalloc, ~0.1 ms each, in the middle of a sequence of frames)
	double *d_arena = nullptr, *h_arena = nullptr;
	double *h_arena_dev = nullptr; // the pinned arena as the device sees it (the upload kernel reads it)
	// calibration records (allocated with the first measured launch): the device buffer of the ONE measured launch a
	// context has in flight at a time, and per slot kMaxMeasRows x {start, longest wave} in pinned memory
	unsigned long long *d_meas = nullptr, *h_meas = nullptr, *h_meas_dev = nullptr;
	FrameSlot *meas_owner = nullptr; // the slot whose measured launch uses d_meas (until its event is done)
	size_t arena_n = 0; // doubles per slot
	// [0] steps [1] hits [2] capped rays (cumulative, never reset) [4..7] traversal diagnostics; [8..15] the same for the
	// second launch of a shadow probe (its rays must not be counted twice)
	unsigned long long *d_counters = nullptr;
	bool probe_in_flight = false; // the scene's shadow probe uses this context's calibration records
	unsigned long long capped_seen = 0; // value of [2] the host has already reported
	// view batches: the ring of staging blocks and the device arena (records, then column tables, then row tables); both only grow.
	// Stream order puts a batch's upload behind the previous batch's kernel, so one arena serves every batch of the stream
	ViewStage view_stages[kViewStages];
	double *d_views = nullptr;
	size_t d_views_cap = 0; // doubles
	std::vector<RetiredArena> retired_views;
};

// One slot of the asynchronous read-back ring (hmrm_render_begin/_wait/_release): a device frame
// the kernel writes, a pinned host frame the copy engine fills while the next kernel runs, and the
// events that order the two streams.
struct RingFrame {
	StreamCtx *ctx = nullptr;   // launch state of the lane the frame's kernel ran on (its capped-ray counter)
	DeviceScratch d_frame;      // width x height uint32 RGBA, rows packed
	PinnedScratch h_frame;      // the same bytes
	unsigned long long *h_capped = nullptr; // pinned: the stream's cumulative capped-ray counter after this frame
	int32_t width = 0, height = 0;
	hipEvent_t kernel_done = nullptr, copy_done = nullptr;
	bool busy = false;
	// What acquire_ticket (api_frames.cpp) asks of a ticket kind: complete() makes a fresh slot usable -- its events and its pinned
	// counter word; the frame buffers grow with the first frame -- and teardown() frees whatever a slot holds, half-made or used.
	hipError_t complete() {
		hipError_t e = hipEventCreateWithFlags(&kernel_done, hipEventDisableTiming);
		if (e == hipSuccess) e = hipEventCreateWithFlags(&copy_done, hipEventDisableTiming);
		if (e == hipSuccess) e = hipHostMalloc((void **)&h_capped, sizeof(unsigned long long), hipHostMallocDefault);
		return e;
	}
	void teardown() {
		d_frame.release();
		h_frame.release();
		if (h_capped) (void)hipHostFree(h_capped);
		if (kernel_done) (void)hipEventDestroy(kernel_done);
		if (copy_done) (void)hipEventDestroy(copy_done);
	}
};
constexpr int kMaxRing = 64; // slots of either ticket pool
// Launch lanes: the ticketed entry points (hmrm_render_begin, hmrm_render_device_begin) send consecutive frames to
// kLanes scene-owned streams in turn, so that one launch's tail (a few long waves) overlaps the next launch's start
// without the caller managing streams -- what bench.py's `frames_in_flight` block does by hand (C2: 0.064 -> 0.045 ms per
// frame, profiles/r03_experiments.txt section 6).
constexpr int kLanes = 3;
// A frame rendered into the caller's DEVICE memory through a lane (hmrm_render_device_begin / _wait).
struct DevTicket {
	StreamCtx *ctx = nullptr;
	hipEvent_t done = nullptr;
	unsigned long long *h_capped = nullptr; // pinned: the lane's cumulative capped-ray counter after this frame
	bool busy = false;
	hipError_t complete() { // (as RingFrame's)
		hipError_t e = hipEventCreateWithFlags(&done, hipEventDisableTiming);
		if (e == hipSuccess) e = hipHostMalloc((void **)&h_capped, sizeof(unsigned long long), hipHostMallocDefault);
		return e;
	}
	void teardown() {
		if (done) (void)hipEventDestroy(done);
		if (h_capped) (void)hipHostFree(h_capped);
	}
};

struct hmrm_scene {
	int device = 0;
	int32_t map_w = 0, map_h = 0;
	hmrm_scene_params params{};
	Knobs knobs;
	uint8_t *d_rgb = nullptr;   // W*H*3  base_heightmap_buf (hmap.cpp:51)
	uint32_t *d_cmap = nullptr; // W*H    colormap_buf as packed RGBA (hmap.cpp:59)
	double *d_thr = nullptr;    // W*H    heightmap_buf[i] + min_height
	float *d_thr32 = nullptr;   // W*H    the same rounded to float, right behind d_thr in the same allocation: the "float heights"
	                            //        mode reads it; rebuilt with every update (never lazily beside frames in flight)
	double thr_max = 0.0;
	double thr_max_bil = 0.0; // whole-map bound of the interpolated thresholds (bilinear mode)
	bool bil_valid = false;
	bool records_valid = false; // d_records describes the current heights (ensure_records)
	float *d_mipbuf_bil = nullptr; // the same over the 3x3-dilated table (bilinear quality mode)
	float *d_mipbuf = nullptr; // window maxima over d_thr: 4/8/../256-cell windows every 2/4/../128 cells
	hmrm::WindowRecord *d_records = nullptr; // frame.hpp: the 16-cell windows' maxima without their 8 highest cells, and those cells (null: map too tall for the build's grid)
	int32_t mip_w[hmrm::kMipLevels] = {}, mip_h[hmrm::kMipLevels] = {};
	int32_t mip_row = 0, mip_plane_shift = 0; // plane layout of both pyramids, see DevFrame
	size_t mip_floats() const { return (size_t)(hmrm::kMipLevels + 1) << mip_plane_shift; }
	float *plane(float *buf, int l) const { return buf + ((size_t)l << mip_plane_shift); }
	hipStream_t stream = nullptr; // the scene's own stream (hmrm_render, updates)
	hipStream_t copy_stream = nullptr; // device-to-host copies of the asynchronous ring
	hipStream_t lanes[kLanes] = {};    // launch lanes of the ticketed entry points (created on first use)
	uint32_t lane_next = 0;
	std::vector<RingFrame *> ring;
	std::vector<DevTicket *> dev_tickets;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	unsigned long long *d_maxkey = nullptr; // UpdateHeightmap's max(thr) reduction
	// scratch of the host-memory entry points (one caller at a time, s->mu held): each grown on demand by the entry point that knows
	// the size, all released by hmrm_scene_destroy
	DeviceScratch d_frame;   // hmrm_render*'s pixels (uint32 RGBA, rows packed); hmrm_render_multi's strip; hmrm_render_lit_sum's pixels
	PinnedScratch h_stage;   // pinned staging strip of hmrm_render_multi (pageable destination frames)
	DeviceScratch d_steps;   // hmrm_render_stats' per-pixel steps (uint32) ...
	DeviceScratch d_entry;   // ... and entry distances (double).  hmrm_pick and hmrm_debug_ray borrow it for their probe's seven or
	                         // eight doubles, hmrm_pick also for a spherical camera's tables at + 8: 8 + 2W + 2H doubles
	DeviceScratch d_rays;    // hmrm_trace_rays / hmrm_trace_segments: host rays in (hmrm::BatchRay) ...
	DeviceScratch d_hits;    // ... and host records out (hmrm::BatchHit); hmrm_pick's one record
	DeviceScratch d_limits;  // hmrm_trace_segments' per-ray limits (uint32)
	DeviceScratch d_cells;   // hmrm_cell_map's rect of bytes, hmrm_cell_map_sum's rect of 16-bit words: rows packed
	DeviceScratch d_targets; // hmrm_cell_map_sum's targets and hmrm_render_lit_sum's directions: three doubles each; hmrm_render_haze's table
	DeviceScratch d_geom;    // hmrm_render_geometry's planes: the wanted ones back to back, slope first, rows packed
	DeviceScratch d_light;   // hmrm_render_lit_sum's light plane (uint16), rows packed
	// The scene's baked light plane (hmrm_scene_set_light, hmrm_scene_bake_light): map_w x map_h uint16, rows packed, read by the
	// baked frames' kernels; null / 0: none.  Changed only with s->mu held and every stream of the scene drained.
	uint16_t *d_baked = nullptr;
	uint32_t baked_scale = 0; // the plane's full scale D, 1 .. 65535
	// launch state per stream; `mu` guards the list and the slot choice (launches themselves are
	// asynchronous), so that threads driving different streams of one scene do not collide
	std::mutex mu;
	std::vector<StreamCtx *> ctxs;
	uint64_t clock = 0;
	// launch orders already settled by some stream's calibration, by camera: a record built for the same camera on
	// another stream (frames in flight) adopts the result instead of measuring again
	struct SettledOrder {
		hmrm_camera cam;
		hmrm_scene_params params;
		uint64_t thr_max_bits;
		hmrm::OrderTrial order;
	};
	// Which kernel suits the scene's content (launch_order.hpp KernelChoice): probed ONCE per scene and height update, by
	// the first camera that gets calibrated (two launches of the plain groups cost 3-6 ms on a 4K frame where leaps pay: too
	// much to spend per camera); every other camera -- a moving one is never calibrated -- renders with that verdict.
	hmrm::KernelChoice choice;
	// ... and a scene whose cameras never repeat (a moving camera: nothing is ever calibrated) is probed on its
	// kProbeAfterFrames-th full frame instead: that frame is launched twice into the same buffer -- production kernel,
	// then plain groups; same pixels -- both measured like a calibration launch, and the verdict is read when the second
	// has finished (any later launch looks).  One 3-6 ms hiccup per scene on a 4K frame; a caller that cannot have it
	// passes HMRM_NO_PROBE with its ticketed frames (hmrm.h).
	bool probe_pending = false;
	uint32_t probe_epoch = 0, probe_epoch_launched = 0; // (a height update or a knob reload voids a probe in flight)
	int probe_rows = 0;
	StreamCtx *probe_ctx = nullptr;
	hipEvent_t probe_done = nullptr;
	unsigned long long *h_probe = nullptr, *h_probe_dev = nullptr; // pinned: 2 x (2 x kMaxMeasRows) words
	// A measured launch (calibration trial or probe) wants the chip to itself: it is issued only when the scene's other
	// streams are idle, and launches on those streams wait for it (overlapping lanes inflated or deflated trials).
	hipEvent_t measure_fence = nullptr;
	StreamCtx *measure_fence_ctx = nullptr;
	std::vector<SettledOrder> settled;
};

// ---- what an entry point asks of a frame launch ----
// A frame with a sun (hmrm_render_lit, hmrm_render_shaded and their antialiased and ticketed forms).
struct LitFrame {
	hmrm::SunRules sun;
	bool primary_interior; // HMRM_TRACE_INTERIOR: the primary rays under the interior rule too
	uint32_t shade_flags;  // hmrm_render_shaded's HMRM_SHADE_*; 0: hmrm_render_lit's frame, by its kernels
	// hmrm_render_lit_sum's frame: the list of directions (device memory: pointer and count), the flags once more and the device
	// light plane (frame.hpp LightSum; the request's d_out may be null then: no colour plane); null: one sun, sun.dir
	const hmrm::LightSum *sum = nullptr;
};

// hmrm_render_interior's frame.  Perspective and spherical rays all start at the camera, so the host decides the rule once per
// frame: a camera that is not strictly inside the box gets the ordinary kernels, hmrm_render's frame (kHostSawNone) -- launched
// the way an interior frame is all the same; orthographic origins differ per pixel, the kernels built with the rule test each.
enum class Interior { kNot, kHostSawNone, kByKernels };
struct FrameRequest {
	uint32_t *d_out; // the target: uint32 RGBA per pixel, out_stride_px pixels per local row
	int64_t out_stride_px;
	uint32_t *d_steps; // per-pixel outputs of an instrumented frame (null: not wanted)
	double *d_entry;
	bool stats;    // instrumented: steps, hits and traversal diagnostics are counted
	bool no_probe; // the caller cannot have this frame launched twice (HMRM_NO_PROBE)
	Interior interior;
	const LitFrame *lit; // null: no sun
	// hmrm_render_geometry's frame: the device planes the launch stores beside the pixel (d_out may be null then); null: none.
	// Its primary rays are under the interior rule when `interior` is not kNot -- the geometry kernels test each origin.
	const hmrm::GeomPlanes *geom = nullptr;
	// hmrm_render_baked's frame: the scene's light plane, whose weight the launch applies to the hit pixels; null: none.  Its
	// primary rays are under the interior rule when `interior` is not kNot, as a geometry frame's are.
	const hmrm::BakedLight *baked = nullptr;
	// hmrm_render_water's frame: the water level, the mirror march and the blend; null: none.  Its primary rays are under the
	// interior rule when `interior` is not kNot, as a geometry frame's are.  With `baked` too (hmrm_render_water_aa with
	// HMRM_WATER_BAKED): the water frame under the light plane.
	const hmrm::WaterRules *water = nullptr;
	// hmrm_render_water_lit's frame: `water` (with the shade flags in its flags word, frame.hpp kWaterSun*) and this sun; null: none.
	const hmrm::SunRules *water_sun = nullptr;
	// hmrm_render_haze's frame: the table (device memory), the index arithmetic and the colour; null: none.  Its primary rays are
	// under the interior rule when `interior` is not kNot, as a geometry frame's are.
	const hmrm::HazeRules *haze = nullptr;
	// Frames under the interior rule, with a sun, with geometry planes, with baked light, with water or with haze run kernels of their own,
	// with the scene's current kernel kind (HMRM_KERNEL or the probe's verdict, read only).
	bool own_kernels() const {
		return interior != Interior::kNot || lit != nullptr || geom != nullptr || baked != nullptr || water != nullptr || haze != nullptr;
	}
	// Special frames -- those and instrumented ones -- are launched in the plain rotation order: never measured, never a probe,
	// not counted towards the probe.
	bool special() const { return stats || own_kernels(); }
};

// ---- the functions that cross files (comments at their definitions) ----
namespace hmrm {
// api_scene.cpp.  ctx_for, ensure_*, drain_scene_streams, drop_light_plane: s->mu held.
int ctx_for(hmrm_scene *s, hipStream_t stream, StreamCtx **out);
int ensure_records(hmrm_scene *s);
int ensure_bilinear_pyramid(hmrm_scene *s);
int drain_scene_streams(hmrm_scene *s, bool own_too);
int ensure_light_plane(hmrm_scene *s);
void drop_light_plane(hmrm_scene *s);
// api_launch.cpp.  prepare_frame, wait_for_measure_fence, launch_frame, pick_views_kernel, acquire_view_stage, launch_views, new_capped,
// take_capped, finish_host_call: s->mu held.
int check_camera(const hmrm_camera *cam);
void to_host_camera(const hmrm_camera *cam, hmrm::HostCamera *hc);
int prepare_frame(hmrm_scene *s, StreamCtx *c, const hmrm_camera *cam, hmrm::DevFrame *f, FrameSlot **slot_out);
int wait_for_measure_fence(hmrm_scene *s, StreamCtx *c);
int launch_frame(hmrm_scene *s, StreamCtx *c, const hmrm::DevFrame &f, FrameSlot *slot, const hmrm::RowMap &rows, const FrameRequest &req);
void finish_frame_record(const hmrm_scene *s, int sampling, hmrm::DevFrame *fr);
void apply_scene_knobs(const hmrm_scene *s, hmrm::DevFrame *f);
struct ViewsKernel {
	bool literal;
	hmrm::FastKernel kind;
};
int pick_views_kernel(hmrm_scene *s, StreamCtx *c, int sampling, ViewsKernel *out);
int acquire_view_stage(StreamCtx *c, size_t doubles, uint64_t stamp, ViewStage **out);
int launch_views(hmrm_scene *s, StreamCtx *c, const ViewsKernel &k, const hmrm::DevFrame &f0, const hmrm::DevFrame *d_frames, int32_t n,
                 bool interior, uint32_t *d_out, int64_t out_stride_px, int64_t view_stride_px);
unsigned long long new_capped(StreamCtx *c, unsigned long long now);
int take_capped(StreamCtx *c, unsigned long long *out);
int finish_host_call(hmrm_scene *s, StreamCtx *c, unsigned long long *capped_out = nullptr);
int noterm(unsigned long long capped);
} // namespace hmrm
#pragma GCC visibility pop
