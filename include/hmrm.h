/*
 * hmrm.h -- C ABI of libhmrm.so, the MI355X-native (gfx950) heightmap ray
 * marcher.  This is the drop-in boundary for the reference's hot path.
 *
 * The reference (Costava/heightmap-ray-marcher) has no FFI/plugin boundary: the
 * path is inline in main() and talks through file-scope globals
 * (main/hmap.cpp:28-112).  The contract a replacement has to honour is
 *     config text in  ->  RGBA8 framebuffer / PNG out.
 * Each entry point below names the reference interface it replaces.  All
 * pointers are plain host pointers unless the name says "device"; no torch, HIP
 * or C++ types appear in any signature.  All functions returning int return
 * HMRM_OK (0) or a negative HMRM_E_* code; hmrm_last_error() then holds the
 * message the reference would have printed to stderr before exit(1).
 *
 * There is NO CPU fallback: entry points that render fail with HMRM_E_DEVICE
 * when no gfx950 device / HIP runtime is usable.
 *
 * Threading (the reference's loop is an OpenMP region over read-only globals, hmap.cpp:978): a scene may
 * be used from several host threads.  Everything a launch mutates -- spherical tables, counters, the
 * cache of per-frame records -- is kept per HIP stream, so hmrm_render_rows_device calls on different
 * streams run concurrently on the device (a scene keeps that state for the 32 most recently used streams;
 * driving it from more makes every launch that takes over another stream's state wait for the DEVICE -- nothing is
 * recorded behind a frame on a caller's stream, so recycling a stream's state waits for all work on the device); the host-side
 * set-up of a call is serialised per scene.  The
 * entry points that return pixels in host memory (hmrm_render, _stats, _cycle, _multi) use the scene's own
 * stream and scratch frame: one such call at a time per scene.  hmrm_render_begin may be called while
 * other tickets are in flight.  hmrm_scene_update waits for every frame in flight on the scene's OWN streams
 * (tickets of hmrm_render_begin / hmrm_render_device_begin included: they finish with the old heights) before it
 * rewrites the tables; it and hmrm_scene_destroy require that no launch of that scene is in flight on a
 * CALLER's stream (hmrm_render_rows_device).  hmrm_last_error() is per thread.
 */
#ifndef HMRM_H
#define HMRM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMRM_ABI_VERSION 1

enum {
	HMRM_OK          =  0,
	HMRM_E_ARG       = -1,  /* bad argument / inconsistent sizes                       */
	HMRM_E_IO        = -2,  /* file cannot be opened / written (hmap.cpp:537-540,162)   */
	HMRM_E_IMAGE     = -3,  /* image cannot be decoded (hmap.cpp:324-329,345-350)       */
	HMRM_E_CONFIG    = -4,  /* config validation failed (hmap.cpp:493-515)              */
	HMRM_E_DEVICE    = -5,  /* HIP error / no device                                    */
	HMRM_E_NOTERM    = -6   /* a ray hit the step cap: the reference loop would not end */
};

/* main/hmap.cpp:104-106 IMAGEPLANE_* */
enum {
	HMRM_PERSPECTIVE  = 1,
	HMRM_SPHERICAL    = 2,
	HMRM_ORTHOGRAPHIC = 3
};

/* Height / colour sampling.  The reference samples the nearest cell with C truncation
 * (hmap.cpp:1001-1004,1013-1018): HMRM_NEAREST is the bit-exact drop-in.  HMRM_BILINEAR is a
 * build-side quality mode (north_star: "bilinear height/colour sampling"), not in the reference:
 * cell values sit at cell centres, thresholds and R,G,B are interpolated bilinearly in fp64
 * (definition: oracle/hmrm_oracle.c "bilinear quality mode"); additive config key
 * `sampling nearest|bilinear`.  HMRM_NEAREST_F32 (north_star: "float heights") keeps the reference's
 * loop and fp64 positions but compares against (float)(heightmap_buf[i] + min_height): a 4-byte
 * threshold table; a ray's hit step can move where z is within half a float ulp of the threshold
 * (tests bound it); additive config key `heights f64|f32`.  Bit-exactness (each mode against its
 * definition) is tested for worlds whose lengths -- grid_width, heights, camera position, step_dist,
 * ortho_width -- lie between 2^-900 and 2^900 times a unit-scale scene's (spherical and orthographic;
 * perspective 2^-900 .. 2^24, whose image plane cam_pos + look degenerates beyond, and one all-NaN frame at
 * 2^60), decimal scales 1e-12 .. 1e12 in every projection and a camera up to 1e10 away (perspective 1e8)
 * included (tests/world_scale.py); beyond, where an intermediate of the reference's loop is subnormal or
 * overflows, nothing is tested. */
enum {
	HMRM_NEAREST     = 0,
	HMRM_BILINEAR    = 1,
	HMRM_NEAREST_F32 = 2   /* nearest cell, hit thresholds kept as float (half the table); not parity */
};

/* The globals UpdateHeightmap() and the box corners read:
 * main/hmap.cpp:38-47 (min/max_height, lum_*), :65 (grid_width). */
typedef struct hmrm_scene_params {
	double min_height;   /* default 0.0   */
	double max_height;   /* default 10.0  */
	double lum_r;        /* default 0.299 */
	double lum_g;        /* default 0.587 */
	double lum_b;        /* default 0.114 */
	double grid_width;   /* default 0.05  */
} hmrm_scene_params;

/* The globals the per-frame set-up and the pixel loop read:
 * main/hmap.cpp:31-35 (resolution, hfov), :68 (step_dist), :75-85 (pos, hang,
 * vang), :98 (ortho_width), :107 (image_plane), :110-112 (bg).  Angles are in
 * RADIANS here (the config file holds degrees, hmap.cpp:131-133,367-384). */
typedef struct hmrm_camera {
	int32_t  width;        /* screen_width  */
	int32_t  height;       /* screen_height */
	int32_t  projection;   /* HMRM_PERSPECTIVE | HMRM_SPHERICAL | HMRM_ORTHOGRAPHIC */
	uint8_t  bg_r, bg_g, bg_b;
	uint8_t  sampling;     /* HMRM_NEAREST (0, the reference) | HMRM_BILINEAR (1) | HMRM_NEAREST_F32 (2) */
	double   hfov;
	double   hang;
	double   vang;
	double   pos[3];
	double   ortho_width;
	double   step_dist;
} hmrm_camera;

/* Per-render statistics (build-side addition; BASELINE.md metric definitions). */
typedef struct hmrm_stats {
	uint64_t rays;        /* pixels rendered                                          */
	uint64_t steps;       /* height loads the reference loop executes (hmap.cpp:1013) */
	uint64_t hits;        /* rays that end on terrain (hmap.cpp:1016)                 */
	uint64_t capped;      /* rays stopped by the step cap (reference: endless loop)   */
	/* traversal diagnostics of the production kernel (0 for HMRM_KERNEL=simple)      */
	uint64_t leap_attempts; /* pyramid look-ups tried                                 */
	uint64_t leaps;         /* ... that ended in an exact jump                        */
	uint64_t groups;        /* speculative groups executed (4 positions each; 6 in the plain-groups kernel) */
	uint64_t leaped_steps;  /* ray-steps covered by jumps (part of `steps`)           */
} hmrm_stats;

typedef struct hmrm_scene hmrm_scene;    /* device-resident height + colour maps */
typedef struct hmrm_config hmrm_config;  /* parsed config state                  */

/* ------------------------------------------------------------------ general */
int         hmrm_abi_version(void);
const char *hmrm_last_error(void);              /* thread-local, never NULL */
int         hmrm_device_count(void);            /* <0 on HIP error          */
int         hmrm_set_device(int device);

/* -------------------------------------------------------------------- scene */
/* Replaces the stbi_load results + UpdateHeightmap (hmap.cpp:314-353,171-191):
 * height_rgb is W*H*3 RGB8 (stbi_load req_comp 3), color_rgba W*H*4 RGBA8
 * (req_comp 4), both row-major top-left origin.  Uploads both once; heights are
 * converted on the device with the reference's exact operation order. */
int  hmrm_scene_create(const uint8_t *height_rgb, const uint8_t *color_rgba,
                       int32_t map_w, int32_t map_h,
                       const hmrm_scene_params *params, hmrm_scene **out);
/* Re-run UpdateHeightmap after min/max_height, lum_* (or grid_width) changed
 * (hmap.cpp:401-440,517-519). */
int  hmrm_scene_update(hmrm_scene *scene, const hmrm_scene_params *params);
void hmrm_scene_destroy(hmrm_scene *scene);
/* Copies the device height buffer (heightmap_buf, hmap.cpp:53,187) to `out`
 * (map_w*map_h doubles) -- test hook for UpdateHeightmap parity. */
int  hmrm_scene_read_heights(const hmrm_scene *scene, double *out);

/* ------------------------------------------------------------------- render */
/* Replaces one pass of the pixel loop main/hmap.cpp:978-1058 at `cycle 1` plus
 * the per-frame set-up :661-672,:952-974.  Writes every pixel of the
 * width x height RGBA8 frame (bytes R,G,B,A=255, top-left origin,
 * hmap.cpp:139-154) to host memory; stride_bytes >= width*4. */
int hmrm_render(const hmrm_scene *scene, const hmrm_camera *cam,
                uint8_t *rgba, size_t stride_bytes);

/* The same frame rendered by several scenes at once -- one per GPU, each created after
 * hmrm_set_device(i) with the same maps (BASELINE config C4's sharding of main/hmap.cpp:978-983's
 * independent pixels): scene i renders the cyclic 16-row bands i, i+n, ... and copies them to their
 * rows of `rgba` over its own PCIe link; no exchange between devices.  All kernels are launched before any
 * copy is enqueued and no device waits for another one's copy: into pinned `rgba` (hipHostMalloc /
 * hipHostRegister by the caller) the bands are copied directly, into pageable memory through a pinned
 * staging strip per scene and a host copy.  Same pixels and return codes as hmrm_render. */
int hmrm_render_multi(hmrm_scene *const *scenes, int32_t n_scenes, const hmrm_camera *cam,
                      uint8_t *rgba, size_t stride_bytes);

/* The same frame without blocking: hmrm_render_begin enqueues the kernel and the device-to-host
 * copy into a pinned frame owned by the scene and returns a ticket; hmrm_render_wait blocks until
 * that frame is in host memory and lends it out (*rgba, valid until hmrm_render_release; returns
 * HMRM_E_NOTERM like hmrm_render, the frame is still valid then).  Rays stopped by the step cap are counted per launch
 * stream, not per ticket: they are reported -- once, with their number -- by a wait (hmrm_render_wait or
 * hmrm_render_device_wait) on a ticket of that launch stream: at the latest by the wait for the frame's own ticket; a
 * ticket of the same stream that is waited for earlier may have seen them already and reports them instead (the k-th
 * ticket of a scene, host and device tickets counted together, uses stream k mod 3).  Copies run on their own
 * stream, so with two or more frames in flight kernel k+1 overlaps the PCIe transfer of frame k
 * (replaces the per-frame blit SDL_UpdateTexture, hmap.cpp:1082).  Up to 64 frames in flight per
 * scene; the ring grows on demand and is freed with the scene.
 * Consecutive frames go to three scene-owned launch streams in turn: with two or more tickets in flight the
 * tail of one launch (a few long waves) also overlaps the start of the next (small frames: 1080p over a 1024^2 map
 * 0.064 -> 0.042 ms of GPU time per frame, profiles/r04_lanes.txt) -- the caller manages no stream. */
int  hmrm_render_begin(const hmrm_scene *scene, const hmrm_camera *cam, int32_t *ticket);
/* Per-frame flags of the ticketed entry points.  HMRM_NO_PROBE: never spend this frame on the scene's one-time kernel probe (a scene
 * whose cameras never repeat launches its sixth full frame twice, production kernel and plain groups, to measure which suits
 * its content: a 3-6 ms hiccup on a 4K frame) -- for a caller that counts on every frame's latency.  The probe
 * then waits for a frame without the flag (or the calibration of a repeated camera). */
#define HMRM_NO_PROBE 1u
/* HMRM_AA(n): the frame antialiased with factor n (hmrm_render_aa below), in bits 8..11 of the flags; HMRM_AA(0) and
 * HMRM_AA(1) mean off.  Tickets with different factors may be in flight on one scene at once.  A flags word with a factor
 * outside {0, 1, 2, 4, 8}, a super frame over the limit or any bit other than these is refused with HMRM_E_ARG. */
#define HMRM_AA(n) (((uint32_t)(n) & 15u) << 8)
#define HMRM_AA_MASK HMRM_AA(15)
int  hmrm_render_begin_flags(const hmrm_scene *scene, const hmrm_camera *cam, uint32_t flags, int32_t *ticket);
int  hmrm_render_wait(const hmrm_scene *scene, int32_t ticket, const uint8_t **rgba, size_t *stride_bytes);
void hmrm_render_release(const hmrm_scene *scene, int32_t ticket);

/* The same pass of main/hmap.cpp:978-1058 for a frame that stays on the GPU (a sequence of frames consumed there -- an
 * encoder, a compositor, a collective -- in place of the blit at hmap.cpp:1082): hmrm_render_device_begin launches the frame into the caller's DEVICE memory d_rgba (width x height
 * RGBA8, stride_bytes a multiple of 4) on the next of the scene's launch streams and returns a ticket;
 * hmrm_render_device_wait blocks until that frame is complete (HMRM_E_NOTERM like hmrm_render; the ticket is
 * free again either way).  Frames in flight must not share memory.  Up to 64 in flight per scene. */
int  hmrm_render_device_begin(const hmrm_scene *scene, const hmrm_camera *cam, void *d_rgba, size_t stride_bytes,
                              int32_t *ticket);
int  hmrm_render_device_begin_flags(const hmrm_scene *scene, const hmrm_camera *cam, void *d_rgba, size_t stride_bytes,
                                    uint32_t flags, int32_t *ticket);
int  hmrm_render_device_wait(const hmrm_scene *scene, int32_t ticket);

/* The reference's progressive frame driver (hmap.cpp:976-983, `cycle n` key, default 47):
 * rewrites only pixels p = cycle, cycle + cycle_period, ... (p = x + y*width) of `rgba`
 * and leaves the others as they are; cycle_period consecutive calls with cycle = 0 ..
 * cycle_period-1 and a static camera give the full frame.  (The reference advances
 * `cycle = (cycle + 1) % cycle_period` before each frame, hmap.cpp:976.) */
int hmrm_render_cycle(const hmrm_scene *scene, const hmrm_camera *cam,
                      uint8_t *rgba, size_t stride_bytes, int32_t cycle, int32_t cycle_period);

/* Same pass restricted to rows [row_begin,row_end) of the frame, written to a
 * DEVICE buffer that holds only those rows (row row_begin at d_rgba), enqueued
 * on `hip_stream` (a hipStream_t, NULL = default stream) without a host sync.
 * stride_bytes: a multiple of 4, at least width*4, below 2^33.
 * This is the multi-GPU row-strip entry point. `band_rows`>0 selects cyclic
 * banding: the strip holds bands band_index, band_index+band_count, ... of
 * band_rows rows each, packed back to back (row_begin/row_end then ignored). */
int hmrm_render_rows_device(const hmrm_scene *scene, const hmrm_camera *cam,
                            void *d_rgba, size_t stride_bytes,
                            int32_t row_begin, int32_t row_end,
                            int32_t band_rows, int32_t band_index, int32_t band_count,
                            void *hip_stream);

/* hmrm_render_rows_device does not wait for its launch, so it cannot report rays stopped by the
 * step cap (HMRM_E_NOTERM of hmrm_render; the reference's loop would not terminate for them,
 * hmap.cpp:1000).  This call waits for `hip_stream`, stores in *capped how many rays of the launches
 * enqueued on it through this scene reached the cap since the last call, and returns
 * HMRM_E_NOTERM when that is not zero. */
int hmrm_scene_take_capped(const hmrm_scene *scene, void *hip_stream, uint64_t *capped);

/* Rows the strip buffer of one rank must hold in cyclic-band mode (full bands). */
int32_t hmrm_band_local_rows(int32_t height, int32_t band_rows, int32_t band_index, int32_t band_count);

/* As hmrm_render, plus per-render statistics and optional per-pixel outputs
 * (host pointers, width*height entries each, may be NULL): the step count of
 * each ray and the slab-entry distance returned by distance() (AABB.cpp:49-77).
 * Uses the instrumented kernel variant; pixels are identical. */
int hmrm_render_stats(const hmrm_scene *scene, const hmrm_camera *cam,
                      uint8_t *rgba, size_t stride_bytes,
                      hmrm_stats *stats, uint32_t *steps_per_pixel, double *entry_d);

/* Antialiased frame (build-side quality mode, not in the reference): the width x height frame is the frame the reference
 * would render at (n*width) x (n*height) -- same camera and scene, exactly the rays GetRay(x/(n*width-1), y/(n*height-1))
 * of that "super frame" -- box-filtered over n x n blocks: for c in R, G, B, out[y][x].c = (S + n*n/2) >> (2*log2 n),
 * S = the integer sum of channel c over the samples (n*x+i, n*y+j), 0 <= i, j < n (rounds half up); out.A = 255.
 * factor n is 1, 2, 4 or 8; n = 1 is hmrm_render byte for byte.  The super frame must itself be a frame the reference can
 * index (at most 2^29 pixels; 3840 x 2160 at n = 8 fits).  Every sampling mode and projection works, with the scene's own
 * kernel choice.  The samples are marched and reduced inside the kernel: no buffer of n*n*width*height pixels exists.
 * stats (may be NULL: the production kernel; else the instrumented one) count samples: rays = n*n*width*height, steps /
 * hits / capped summed over the samples; HMRM_E_NOTERM when any sample hits the step cap.  A bad factor or an oversized
 * super frame is refused with HMRM_E_ARG before the scene is looked at. */
int hmrm_render_aa(const hmrm_scene *scene, const hmrm_camera *cam, int32_t factor, uint8_t *rgba, size_t stride_bytes,
                   hmrm_stats *stats);

/* ------------------------------------------------------------- ray queries */
/* The march without a camera (build-side addition; the reference has no such entry, but its loop never looks at the
 * camera either: hmap.cpp:989-1057 takes a Ray {pos, dir} and the scene).  A ray is the reference's `Ray`: `dir` is used as
 * given and NOT normalised (the loop does not need unit length; the perspective plane normalises before the loop,
 * Perspective.cpp:27); zero, infinite and NaN components behave as the reference's arithmetic does on them -- (int)NaN
 * fails the range test of hmap.cpp:1006, so such a ray misses -- and no input faults the kernel.
 * Each ray runs exactly the body of hmap.cpp:989-1057: intersection() (AABB.cpp:33-44) sees a miss for d == inf or d < 0, so
 * a ray whose origin lies inside the box misses, as in the reference (hmrm_trace_segments below lifts that); the entry point is nudged by grid_width * 0.01 * dir
 * (:998); then step_dist * dir is added step by step (:1037) until a cell's height is above the ray (:1016) or the ray
 * leaves the grid (:1006).  There is no segment limit here (the reference's loop has none): hmrm_trace_segments has one. */
typedef struct hmrm_ray { double pos[3]; double dir[3]; } hmrm_ray;          /* 48 bytes */

enum { HMRM_RAY_MISS = 0, HMRM_RAY_HIT = 1, HMRM_RAY_CAPPED = 2 };

typedef struct hmrm_ray_hit {                                                /* 56 bytes */
	double   point[3];   /* HIT: int_point when hmap.cpp:1016 fires, the reference's bits; else 0,0,0 */
	double   entry_d;    /* distance(ray, c0, c1), AABB.cpp:49-77, bit for bit (inf, negative and NaN included) */
	uint32_t steps;      /* height loads the reference loop executes for this ray (hmap.cpp:1013), the hitting one included;
	                      * CAPPED: the step cap */
	int32_t  cell_x, cell_y; /* HIT: gridx, gridy of hmap.cpp:1001-1004; else -1, -1 */
	uint8_t  rgba[4];    /* the pixel the reference would write for this ray (hit colour :1018-1031, alpha-0 rule :1020, sky
	                      * and background :1041-1057; CAPPED: as a miss); A = 255 */
	uint32_t status;     /* HMRM_RAY_*; CAPPED: stopped by the step cap (HMRM_STEP_CAP), the reference would not return */
	uint32_t reserved;   /* written as 0 */
} hmrm_ray_hit;

typedef struct hmrm_trace_params {
	double  step_dist;   /* hmap.cpp:68, in units of |dir| */
	uint8_t bg_r, bg_g, bg_b;
	uint8_t sampling;    /* HMRM_NEAREST | HMRM_BILINEAR | HMRM_NEAREST_F32 */
} hmrm_trace_params;

/* Traces rays[0 .. n) (host memory) and writes hits[0 .. n) (host memory).  Synchronous, on the scene's own stream: one such
 * call at a time per scene, like hmrm_render.  Returns HMRM_E_NOTERM when any ray was stopped by the step cap; all n records
 * are valid then.  stats (may be NULL) receives rays = n and steps / hits / capped summed over the batch; the traversal
 * diagnostics are 0.  n == 0 returns HMRM_OK and launches nothing.  A NULL p, rays or hits with n > 0, n < 0, n > 2^29 or a
 * sampling outside the enum is refused with HMRM_E_ARG before the scene is looked at.
 * A batch is not a frame: it never triggers or counts towards the launch-order calibration, the scene's kernel probe or the
 * cache of per-frame records, and leaves hmrm_debug_kernel_choice and every later frame as they would have been.  It does run
 * the scene's current kernel (the probe's verdict or HMRM_KERNEL; the window records apply to HMRM_NEAREST, the other
 * sampling modes keep the production kernel, as frames do); every kernel writes the same records. */
int hmrm_trace_rays(const hmrm_scene *scene, const hmrm_trace_params *p, const hmrm_ray *rays, int64_t n,
                    hmrm_ray_hit *hits, hmrm_stats *stats /* may be NULL */);
/* The same for rays and records in DEVICE memory (n * 48 and n * 56 bytes, 8-byte aligned), enqueued on `hip_stream` (a
 * hipStream_t, NULL = default stream) without a host sync, under the contract of hmrm_render_rows_device: rays stopped by
 * the step cap are reported by hmrm_scene_take_capped for that stream. */
int hmrm_trace_rays_device(const hmrm_scene *scene, const hmrm_trace_params *p, const void *d_rays, int64_t n,
                           void *d_hits, void *hip_stream);
/* ------------------------------------------------ segments and interior origins */
/* Two rules the reference does not have (build-side additions), both exact and both off unless asked for.
 * Box: c0 = (0, 0, min_height), c1 = (map_w * grid_width, -map_h * grid_width, max_height) (hmap.cpp:968-974).
 * INTERIOR RULE (HMRM_TRACE_INTERIOR; hmrm_render_interior): a ray is interior when its origin lies strictly inside the box --
 * c0.x < pos.x < c1.x, c1.y < pos.y < c0.y, c0.z < pos.z < c1.z, all six true; NaN fails them.  The reference turns such a ray
 * into a miss (AABB.cpp:37-39: distance() is negative, -inf or NaN there).  Under the rule it runs the body of
 * hmap.cpp:989-1057 as if distance() had returned +0.0: int_point = pos + 0.0 * dir, then the nudge (:998), then the loop,
 * unchanged; non-finite dir components go through that arithmetic as written.  Every other ray -- origins exactly on a face
 * included -- is untouched.  In a record entry_d stays distance()'s own value bit for bit, not the d that was used.
 * STEP LIMIT: a ray has an effective limit L (0 = none) and ends after L height loads (hmap.cpp:1013) when the L-th did not
 * hit.  Order within a trip as for the step cap: the range test (:1006), then the budget, then the load -- a ray that leaves
 * the grid after exactly L loads is a MISS; one still inside it gets HMRM_RAY_END with steps = L, the miss shade, point 0 and
 * cell -1.  The budget is min(HMRM_STEP_CAP, L); running out of it is END when L != 0 && L < step cap, else CAPPED as before.
 * END rays are not capped rays: they never cause HMRM_E_NOTERM and never show up in hmrm_scene_take_capped.  The limit is
 * in loads, which is exact; with dir = (B - A) / N, step_dist = 1 and L = N a ray is the segment from A to B. */
#define HMRM_TRACE_INTERIOR 1u
enum { HMRM_RAY_END = 3 };   /* hmrm_ray_hit.status of hmrm_trace_segments: ended by the ray's own step limit, inside the grid */
typedef struct hmrm_segment_params {      /* 24 bytes */
	double  step_dist;   /* as hmrm_trace_params */
	uint8_t bg_r, bg_g, bg_b;
	uint8_t sampling;
	uint32_t flags;      /* HMRM_TRACE_INTERIOR; any other bit: HMRM_E_ARG */
	uint32_t max_steps;  /* limit for every ray, 0 = none */
	uint32_t reserved;   /* must be 0 */
} hmrm_segment_params;
/* hmrm_trace_rays under the two rules.  max_steps (n entries, may be NULL; 0 = none) holds per-ray limits: ray i's L is the
 * smaller of the non-zero values among p->max_steps and max_steps[i].  With flags = 0, p->max_steps = 0 and max_steps NULL
 * the records are hmrm_trace_rays', byte for byte.  Contracts are those of hmrm_trace_rays / _device: refusals (a flag bit
 * that is not defined, reserved != 0, a bad sampling, NULL p / rays / hits with n > 0, n < 0, n > 2^29) come before the scene
 * is looked at; a batch is not a frame (no calibration, no probe, the camera cache untouched); stats->capped counts CAPPED
 * rays only, and only they make the call return HMRM_E_NOTERM. */
int hmrm_trace_segments(const hmrm_scene *scene, const hmrm_segment_params *p, const hmrm_ray *rays,
                        const uint32_t *max_steps /* per ray, may be NULL */, int64_t n, hmrm_ray_hit *hits,
                        hmrm_stats *stats /* may be NULL */);
/* ... for rays, limits (n * 4 bytes, 4-byte aligned, may be NULL) and records in DEVICE memory, as hmrm_trace_rays_device. */
int hmrm_trace_segments_device(const hmrm_scene *scene, const hmrm_segment_params *p, const void *d_rays,
                               const void *d_max_steps /* may be NULL */, int64_t n, void *d_hits, void *hip_stream);
/* hmrm_render under the interior rule: a camera below max_height -- a walker, a low fly-through -- sees the terrain around it
 * instead of sky.  Synchronous, on the scene's stream, all three projections and sampling modes, with the scene's current
 * kernel (HMRM_KERNEL or the probe's verdict).  Launched the way an instrumented frame is: never measured, never the scene's
 * probe, not counted towards it.  A perspective or spherical camera that is not strictly inside the box gives hmrm_render's
 * frame byte for byte (the ordinary kernel runs); orthographic origins are tested per pixel.  HMRM_E_NOTERM as hmrm_render:
 * an interior ray with dir.x = dir.y = 0 that never hits (straight up) never leaves the grid and runs to the step cap.
 * Not antialiased, no tickets, strips or recording by itself: hmrm_render_shaded_aa, hmrm_render_shaded_begin and
 * hmrm_record_orbit_shaded with HMRM_SHADE_NO_SHADOWS and HMRM_TRACE_INTERIOR give this frame all of those; or trace a batch. */
int hmrm_render_interior(const hmrm_scene *scene, const hmrm_camera *cam, uint8_t *rgba, size_t stride_bytes);

/* ------------------------------------------------------------- sun shadows */
/* hmrm_render with hard sun shadows (build-side addition), exact: every pixel first gets hmrm_render's value -- with
 * HMRM_TRACE_INTERIOR in `flags` hmrm_render_interior's; the primary march is unchanged -- and every pixel whose primary ray
 * HIT (hmap.cpp:1016 fired; a hit cell with alpha 0, which shows the background, :1020, counts) then casts one shadow ray.
 * Misses, sky and primary rays stopped by the step cap cast none.
 * The shadow ray is an hmrm_trace_segments ray: pos = (P.x, P.y, t), dir = sun->dir as given, sun->step_dist, sun->max_steps,
 * the camera's sampling mode, HMRM_TRACE_INTERIOR always on.  P is the reference's int_point at the hit (hmrm_ray_hit.point),
 * t the threshold the hitting load compared z with: heightmap_buf[c] + min_height (HMRM_NEAREST), the float entry of that
 * table widened to double (HMRM_NEAREST_F32), the interpolated threshold at P (HMRM_BILINEAR) -- the ray starts on the
 * surface above the hit point (P itself lies below it, z < t).  Nothing is special-cased: an origin with t >= max_height is
 * not strictly inside and goes through distance() as written; a sun below the horizon, zero, infinite and NaN components and
 * step_dist = 0 go through the same arithmetic.
 * A pixel is SHADOWED when its shadow ray's status is HMRM_RAY_HIT; MISS, END and CAPPED leave it lit.  R, G and B of a
 * shadowed pixel become (c * ambient + 127) / 255 in integers, A stays 255; ambient = 255 reproduces the frame without
 * shadows (the shadow rays are marched all the same).
 * Capped primary rays and capped shadow rays are counted together; either kind makes the call return HMRM_E_NOTERM with a
 * valid frame.  END rays are never counted.  dir = (0, 0, 1) without max_steps never leaves the grid and runs to the cap.
 * Refusals (HMRM_E_ARG) come before the scene is looked at: NULL sun, an undefined flag bit, reserved != 0.  Synchronous, on
 * the scene's stream, launched the way hmrm_render_interior is: one launch renders the frame, never measured, never the
 * scene's probe and not counted towards it, with the scene's current kernel (HMRM_KERNEL or the probe's verdict; the window
 * records apply to HMRM_NEAREST).  All three projections and sampling modes.  Antialiased, ticketed and recorded lit
 * frames: hmrm_render_shaded_aa, hmrm_render_shaded_begin, hmrm_render_shaded_device_begin and hmrm_record_orbit_shaded below
 * with shade_flags = 0.  Still no row strips or bands, no multi-GPU single frame, no cycle, no statistics. */
typedef struct hmrm_sun {        /* 48 bytes */
	double   dir[3];     /* towards the sun; used as given, NOT normalised (like hmrm_ray.dir) */
	double   step_dist;  /* of the shadow march, in units of |dir| */
	uint32_t max_steps;  /* step limit L of every shadow ray, 0 = none (hmrm_trace_segments' rule) */
	uint32_t flags;      /* HMRM_TRACE_INTERIOR: primary rays under the interior rule too; any other bit: HMRM_E_ARG */
	uint8_t  ambient;    /* 0..255: what a shadowed pixel keeps; 255 = shadows change nothing */
	uint8_t  reserved[7];/* must be 0 */
} hmrm_sun;
int hmrm_render_lit(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_sun *sun, uint8_t *rgba, size_t stride_bytes);

/* ------------------------------------------------------- diffuse sun shading */
/* hmrm_render_lit with diffuse (hill) shading, with or without the shadow rays (build-side addition), exact.
 * Every pixel first gets hmrm_render's value (hmrm_render_interior's with HMRM_TRACE_INTERIOR in sun->flags; the primary
 * march is unchanged).  Every pixel whose primary ray HIT (alpha-0 cells count, as in hmrm_render_lit) gets a weight w in
 * 0..255, and its R, G and B become (c * w + 127) / 255 in integers; A stays 255.  Misses, sky and capped primary rays are
 * untouched.
 * Without HMRM_SHADE_NO_SHADOWS every hit pixel casts exactly hmrm_render_lit's shadow ray -- origin (P.x, P.y, t), dir =
 * sun->dir, sun->step_dist, sun->max_steps, the interior rule always on -- and a pixel whose shadow ray's status is
 * HMRM_RAY_HIT is SHADOWED: w = ambient.  With it no shadow ray is marched, no pixel is shadowed, and step_dist and
 * max_steps are not looked at.
 * A pixel that is not shadowed has w = 255 without HMRM_SHADE_DIFFUSE, and with it
 *   w = ambient + ((255 - ambient) * q + 127) / 255   in integers,
 * q in 0..255 the diffuse level of the hit: q = 255 gives the texel back, q = 0 what a shadowed pixel gets.
 * THE LEVEL q.  Plain IEEE double operations in this order, no contraction.  T is the threshold table of the camera's
 * sampling mode (heightmap_buf[i] + min_height for HMRM_NEAREST, its float entry widened to double for HMRM_NEAREST_F32),
 * gw = grid_width, s = sun->dir as given, W x H the map.
 *   HMRM_NEAREST, HMRM_NEAREST_F32: (cx, cy) = the hit's cell_x, cell_y (hmrm_ray_hit);
 *     xm = max(cx - 1, 0), xp = min(cx + 1, W - 1), ym = max(cy - 1, 0), yp = min(cy + 1, H - 1);
 *     gx = xp > xm ? (T[xp, cy] - T[xm, cy]) / ((double)(xp - xm) * gw) : 0.0;
 *     gy = yp > ym ? (T[cx, yp] - T[cx, ym]) / ((double)(yp - ym) * gw) : 0.0.
 *   HMRM_BILINEAR: the gradient of the interpolated surface at P: the four cells c00, c10, c01, c11 and the weights tx, ty of
 *     the bilinear mode at ((P.x - c0.x) / gw, -(P.y - c0.y) / gw);
 *     a = T[c10] - T[c00], b = T[c11] - T[c01], gx = (a + ty * (b - a)) / gw;
 *     c = T[c01] - T[c00], d = T[c11] - T[c10], gy = (c + tx * (d - c)) / gw.
 *   n = (-gx, gy, 1)  (rows grow towards decreasing world y: gy is minus the y slope);
 *   dot = (n.x * s.x + n.y * s.y) + s.z;
 *   len = sqrt(((n.x * n.x + n.y * n.y) + 1.0) * ((s.x * s.x + s.y * s.y) + s.z * s.z)), correctly rounded;
 *   k = dot / len;  k = k > 0 ? (k < 1 ? k : 1) : 0  (NaN gives 0);  q = (uint32_t)(k * 255.0 + 0.5).
 * Nothing is special-cased: a zero, infinite or NaN sun gives q = 0 through this arithmetic; a sun below the horizon lights
 * the slopes that face it.
 * Consequences: shade_flags = 0 is hmrm_render_lit byte for byte (its kernels run); HMRM_SHADE_NO_SHADOWS alone is
 * hmrm_render / hmrm_render_interior byte for byte; ambient = 255 is the frame without shading under any flags.
 * Refusals (HMRM_E_ARG) come before the scene is looked at: hmrm_render_lit's three (NULL sun, an undefined bit in
 * sun->flags, reserved != 0) and an undefined bit in shade_flags.  Capped rays are counted and reported as in
 * hmrm_render_lit; with HMRM_SHADE_NO_SHADOWS only primary rays can be capped.  Synchronous, on the scene's stream, launched
 * the way a lit frame is: one launch, never measured, never the scene's probe and not counted towards it, with the scene's
 * current kernel (HMRM_KERNEL or the probe's verdict; the window records apply to HMRM_NEAREST).  All three projections and
 * sampling modes.  Antialiased, ticketed and recorded: the entry points below.  Still no row strips or bands
 * (hmrm_render_rows_device), no hmrm_render_multi, no hmrm_render_cycle, no statistics.  The shading arithmetic is tested bit for bit across
 * world scales (tests/test_world_scale_families_gpu.py): every length times 2^-900 .. 2^900 and decimal scales, grid widths an ulp off a
 * power of two, relief on top of 1e9, and suns of magnitude 2^-600 .. 2^600.  Two consequences of the arithmetic as written, not
 * limits of the kernels: a shadow ray starts (0.01 * grid_width) * dir past its origin, so it leaves the grid before its
 * first load, and shadows nothing, once 0.01 * |dir| exceeds the grid's extent in grid widths (keep |dir| near 1); and q is 0
 * where s.s or (n.n) * (s.s) overflows, and 0 or 255 where s.s underflows to zero. */
#define HMRM_SHADE_DIFFUSE    1u
#define HMRM_SHADE_NO_SHADOWS 2u
int hmrm_render_shaded(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_sun *sun,
                       uint32_t shade_flags, uint8_t *rgba, size_t stride_bytes);

/* -------------------------------------- antialiased, ticketed and recorded sun-lit frames */
/* THE ANTIALIASED LIT FRAME with factor n (1, 2, 4, 8) of a W x H camera is the frame hmrm_render_shaded returns for the super
 * camera (n*W) x (n*H) -- hmrm_render_aa's super frame -- with the same sun and shade_flags: every sample is shaded and
 * shadowed on its own.  That frame is then box-filtered with hmrm_render_aa's formula: per channel (S + n*n/2) >> (2 log2 n),
 * A = 255.  The samples are marched, lit and reduced inside one launch: no buffer of n*n*W*H pixels exists.
 * Consequences, all byte for byte: factor 1 is hmrm_render_shaded (its kernels run); HMRM_SHADE_NO_SHADOWS alone is
 * hmrm_render_aa's frame -- with HMRM_TRACE_INTERIOR and a camera inside the box the box-filtered hmrm_render_interior frame,
 * which is how an unlit interior fly-through reaches tickets and recording; ambient = 255 is hmrm_render_aa's frame under any
 * flags; shade_flags = 0 is the antialiased hmrm_render_lit frame.
 * Capped samples (primary and shadow rays together) are counted as in hmrm_render_lit and make the call -- or the wait --
 * return HMRM_E_NOTERM with a valid frame; END rays never do.
 * Refusals (HMRM_E_ARG) come before the scene is looked at, in this order: NULL sun, an undefined bit in sun->flags, reserved
 * != 0, an undefined bit in shade_flags; then those of hmrm_render_aa (hmrm_render_begin_flags for the tickets): the camera,
 * the flag bits, the factor, the super frame's size.
 * hmrm_render_shaded_aa is synchronous, on the scene's stream, launched the way a lit frame is. */
int hmrm_render_shaded_aa(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_sun *sun, uint32_t shade_flags,
                          int32_t factor, uint8_t *rgba, size_t stride_bytes);
/* Lit tickets: hmrm_render_begin_flags / hmrm_render_device_begin_flags for the lit frame above.  flags: HMRM_AA(n), and
 * HMRM_NO_PROBE, which is accepted and has no effect -- a lit frame is never the scene's probe, never measured and not counted
 * towards the probe; hmrm_debug_kernel_choice and every later plain frame are as they would have been without it.  The
 * tickets come from the same rings as plain ones and are waited for and released with hmrm_render_wait, hmrm_render_release
 * and hmrm_render_device_wait; the lane rotation and the per-lane accounting of capped rays are the same; plain and lit
 * tickets with different factors may be in flight together on one scene; hmrm_scene_update waits for them as for any ticket
 * (they finish with the old heights).  *sun is copied into the launch: it need not outlive the call. */
int hmrm_render_shaded_begin(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_sun *sun, uint32_t shade_flags,
                             uint32_t flags, int32_t *ticket);
int hmrm_render_shaded_device_begin(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_sun *sun,
                                    uint32_t shade_flags, void *d_rgba, size_t stride_bytes, uint32_t flags, int32_t *ticket);

/* ---------------------------------------------------------------- cell maps */
/* The lighting model asked of the terrain itself (build-side addition), exact: one byte per map cell -- which cells a sun
 * reaches and how bright each one is (a light map, a hillshade map, baked lighting), which cells see a point (a viewshed).  It is
 * the terrain-space counterpart of hmrm_render_lit / hmrm_render_shaded: every cell casts ONE segment ray, made on the device
 * from the cell index and the threshold table; no ray is read from memory and no record is written.
 * THE RAY OF CELL (cx, cy), 0 <= cx < W, 0 <= cy < H, gw = grid_width, T the threshold table of p->sampling
 * (heightmap_buf[i] + min_height for HMRM_NEAREST and HMRM_BILINEAR, the float entry of that table widened to double for
 * HMRM_NEAREST_F32).  Plain IEEE double operations in this order, no contraction:
 *   pos.x = ((double)cx + 0.5) * gw
 *   pos.y = -(((double)cy + 0.5) * gw)
 *   pos.z = T[cx, cy] + lift
 *   dir = target                                                      (direction mode)
 *   dir = (target.x - pos.x, target.y - pos.y, target.z - pos.z)      (HMRM_MAP_TOWARDS_POINT)
 * The ray is an hmrm_trace_segments ray: step_dist and max_steps from the struct, the struct's sampling mode,
 * HMRM_TRACE_INTERIOR always on.  Its `status` is the cell's status s.  Nothing is special-cased, as in hmrm_render_lit: a cell
 * whose origin is not strictly inside the box (T + lift >= max_height, or T + lift <= min_height: a zero-height cell with lift
 * 0) goes through distance() as written; a sun below the horizon, a zero, infinite or NaN target and step_dist = 0 go through
 * the same arithmetic.  With lift 0 a ray may hit its own cell's neighbourhood in its first loads: the slope shadowing itself.
 * THE BYTE OF A CELL.  Without HMRM_MAP_WEIGHT: s, one of HMRM_RAY_MISS, HIT, CAPPED, END.  (Point mode with step_dist = 1/N and
 * max_steps = N: the ray ends at about O; HIT means hidden from O, END and MISS mean visible.)  With HMRM_MAP_WEIGHT: the
 * weight w of hmrm_render_shaded.  A cell is SHADOWED when s == HIT -- never with HMRM_MAP_NO_SHADOWS, and then no ray is
 * marched and step_dist and max_steps are not looked at, nor is lift in direction mode -- and gets w = ambient.  A cell that is not shadowed gets
 * w = 255 without HMRM_MAP_DIFFUSE, and with it w = ambient + ((255 - ambient) * q + 127) / 255, q the diffuse level above
 * ("THE LEVEL q"), operation for operation, with s = the cell's `dir` (in point mode the cell's own direction as made above, lift
 * included); nearest modes: (cx, cy) is the cell; HMRM_BILINEAR: the gradient of the interpolated surface at P = pos.
 * out[(cy - y0) * stride_bytes + (cx - x0)] is the byte; bytes between rows are not touched.
 * Refusals (HMRM_E_ARG) before the scene is looked at, in this order: NULL p, an undefined flag bit, reserved != 0, a sampling
 * outside the enum, DIFFUSE or NO_SHADOWS without WEIGHT, NULL out.  Then: a NULL scene, a rect that is empty, negative or not
 * inside the map, stride_bytes below the rect's width, a map with a side of 2^24 cells or more with a sampling other than
 * nearest (as for ray batches).
 * Capped rays make hmrm_cell_map return HMRM_E_NOTERM with a valid map; END rays never do.  hmrm_cell_map_device reports them
 * through hmrm_scene_take_capped for its stream -- hmrm_trace_rays_device's contract: no host sync; d_out needs no alignment.
 * hmrm_cell_map is synchronous on the scene's stream, one such call at a time per scene.  A cell map is not a frame: no
 * calibration, no probe, not counted towards the probe; hmrm_debug_kernel_choice and every later frame are as they would have
 * been.  It runs the scene's current kernel (HMRM_KERNEL or the probe's verdict; the window records apply to HMRM_NEAREST);
 * every kernel writes the same bytes, the literal loop too (HMRM_KERNEL=simple, maps with a side >= 2^24).  Rays, statuses
 * and weights are tested bit for bit across world scales, as for hmrm_render_shaded (tests/test_world_scale_families_gpu.py).
 * SUPPORTED RANGE OF POINT MODE: grid_width < 100.  There `dir` = O - pos is a length, so the first position,
 * pos + (0.01 * grid_width) * dir, lies the FRACTION 0.01 * grid_width of the way from the cell to O, whatever the distance.
 * While that fraction is small the map is the viewshed described above; it thins out as the fraction grows (the test scene hides
 * 1818 of 3072 cells at grid_width 1, 1505 at 16, 1039 at 32, 96 at 64); from grid_width = 100 the ray STARTS AT OR BEYOND O and
 * marches on away from it, so no cell is ever reported hidden, and a few thousand grid widths further every ray has left the
 * grid before its first load (all MISS).  A world in metres with cells of 100 m or more needs its lengths divided by a constant
 * before they go in (grid_width, heights, O, lift; step_dist is a fraction of |dir| and stays).  The bytes are the arithmetic
 * above on both sides of the limit, and are tested there (grid_width 32 and 128); the nudge is the reference's entry nudge,
 * kept for every ray family alike (DESIGN.md 5.6.4 has the trade-off). */
#define HMRM_MAP_TOWARDS_POINT 1u  /* target is a point O, not a direction: a viewshed, a point light */
#define HMRM_MAP_WEIGHT        2u  /* write the light weight w (0..255) instead of the ray's status */
#define HMRM_MAP_DIFFUSE       4u  /* with WEIGHT: an unshadowed cell gets its diffuse level */
#define HMRM_MAP_NO_SHADOWS    8u  /* with WEIGHT: march no ray, no cell is shadowed (pure hillshade) */
typedef struct hmrm_cell_map_params {   /* 56 bytes */
	double   target[3];  /* direction towards the sun, used as given, NOT normalised; TOWARDS_POINT: the point O */
	double   step_dist;  /* in units of |dir| */
	double   lift;       /* the ray starts this far above the cell's surface (an observer's eye height; 0 = on it) */
	uint32_t max_steps;  /* step limit L of every ray, 0 = none (hmrm_trace_segments' rule) */
	uint32_t flags;
	uint8_t  sampling;   /* HMRM_NEAREST | HMRM_BILINEAR | HMRM_NEAREST_F32 */
	uint8_t  ambient;    /* as hmrm_sun.ambient */
	uint8_t  reserved[6];/* must be 0 */
} hmrm_cell_map_params;
typedef struct hmrm_cell_rect { int32_t x0, y0, w, h; } hmrm_cell_rect;  /* cells [x0, x0+w) x [y0, y0+h) */
int hmrm_cell_map(const hmrm_scene *scene, const hmrm_cell_map_params *p, const hmrm_cell_rect *rect /* NULL: the map */,
                  uint8_t *out, size_t stride_bytes);
int hmrm_cell_map_device(const hmrm_scene *scene, const hmrm_cell_map_params *p, const hmrm_cell_rect *rect,
                         void *d_out, size_t stride_bytes, void *hip_stream);

/* ACCUMULATED CELL MAPS: many suns, sky directions or observers in one launch (sun hours, a sky-view factor / ambient
 * occlusion, a soft shadow from samples on the sun's disc, a cumulative viewshed).  For target k, 0 <= k < n_targets, the ray
 * of cell (cx, cy) is hmrm_cell_map's ray above with p->target replaced by targets[3k .. 3k+2]; p->flags (HMRM_MAP_TOWARDS_POINT
 * applies to every target), step_dist, lift, max_steps, sampling and ambient are p's, the interior rule stays always on and
 * nothing is special-cased (a NaN, infinite or zero target goes through the same arithmetic).  p->target itself is not looked at.
 * THE VALUE v_k, s_k the ray's status: with HMRM_MAP_WEIGHT exactly the byte hmrm_cell_map would write for target k (ambient
 * for a shadowed cell, else 255 or HMRM_MAP_DIFFUSE's weight of the level under THIS target's direction, in point mode the
 * cell's own direction with lift; HMRM_MAP_NO_SHADOWS marches no ray); without it v_k = 1 when s_k != HMRM_RAY_HIT, else 0 --
 * MISS, END and CAPPED count as reached / visible, the rule that decides SHADOWED everywhere else.
 * THE WORD OF A CELL: the native uint16 sum of v_0 .. v_{K-1}, K = n_targets in 1 .. 256 (at most 256 * 255 = 65280), at
 * (char *)out + (cy - y0) * stride_bytes + 2 * (cx - x0); bytes between rows are not touched.  Byte for byte: K = 1 with WEIGHT
 * is hmrm_cell_map's map widened to 16 bits, any K is the integer sum of K hmrm_cell_map maps, the order of the targets does
 * not matter.
 * Refusals (HMRM_E_ARG) before the scene is looked at, in this order: hmrm_cell_map's own, in its order, with `out` for its
 * out; NULL targets; n_targets outside 1 .. 256.  Then: a NULL scene, the rect, stride_bytes below 2 * w or odd, an odd d_out
 * address (device entry), the 2^24-side rule.
 * Capped rays are counted per RAY, so a cell can contribute up to K of them: hmrm_cell_map_sum returns HMRM_E_NOTERM with a
 * valid map, hmrm_cell_map_sum_device reports them through hmrm_scene_take_capped; END rays never count.  Not a frame:
 * everything hmrm_cell_map says about the probe, the calibration, the camera cache and hmrm_debug_kernel_choice holds.  The host
 * entry is synchronous on the scene's stream and stages the targets and the map through scene-owned device buffers that grow
 * on demand; the device entry does no host sync and reads d_targets on hip_stream. */
int hmrm_cell_map_sum(const hmrm_scene *scene, const hmrm_cell_map_params *p,
                      const double *targets /* n_targets x 3, host */, int32_t n_targets,
                      const hmrm_cell_rect *rect /* NULL: the map */,
                      uint16_t *out, size_t stride_bytes);
int hmrm_cell_map_sum_device(const hmrm_scene *scene, const hmrm_cell_map_params *p,
                             const void *d_targets /* n_targets x 24 bytes, DEVICE, 8-byte aligned */, int32_t n_targets,
                             const hmrm_cell_rect *rect, void *d_out /* 2-byte aligned */, size_t stride_bytes,
                             void *hip_stream);
/* Host only, no GPU: rings * per_ring (1 .. 256 in total) directions of the upper hemisphere, cosine-weighted, so that a plain
 * count over them (status mode) is a sky-view factor.  Ring i, slot j: u = (i + 0.5) / rings, z = sqrt(u), r = sqrt(1.0 - u),
 * a = 2 pi (j + 0.5 * (i & 1)) / per_ring, out_xyz[3 * (i * per_ring + j) ..] = (r cos a, r sin a, z), libm's functions.
 * Returns the count, or HMRM_E_ARG (NULL out_xyz, a count below 1 or a product outside 1 .. 256). */
int hmrm_sky_directions(int32_t rings, int32_t per_ring, double *out_xyz);

/* ---------------------------------------------------------- geometry frames */
/* The geometry behind the picture (build-side addition), exact: a depth plane to composite a caller's own objects over the
 * terrain (distance fog alone needs no plane: haze frames, below), an ID plane to pick any pixel without a second call, a slope plane to relight a still frame
 * under a moving sun without marching again (INTEGRATION.md 2a has the three recipes).  It is the screen-space counterpart of
 * the cell maps: the march already knows all of it for every pixel, and an epilogue of the same launch stores it -- no ray is
 * read from memory and no record is written.
 * A GEOMETRY FRAME of a camera is hmrm_render's frame plus up to three more planes; with HMRM_TRACE_INTERIOR in `flags` it is
 * hmrm_render_interior's frame instead.  Each plane is optional, and all of them come from the SAME launch.
 * Let R(x, y) be the hmrm_ray_hit record hmrm_trace_rays writes for the ray GetRay makes for pixel (x, y) -- the pos and dir
 * hmrm_debug_ray returns; with the interior flag the record hmrm_trace_segments writes for it with HMRM_TRACE_INTERIOR and no
 * limits -- under the camera's step_dist, background and sampling.  O is that ray's pos, W x H the map.
 *   rgba,  uint32 per pixel: R.rgba -- byte for byte the frame of hmrm_render / hmrm_render_interior.
 *   cell,  int32 per pixel:  R.cell_y * W + R.cell_x when R.status == HMRM_RAY_HIT (a map has at most 2^29 cells), else -1.
 *   range, float per pixel:  for a hit ex = P.x - O.x, ey = P.y - O.y, ez = P.z - O.z with P = R.point,
 *                            r = sqrt((ex * ex + ey * ey) + ez * ez) in plain IEEE doubles in this order, no contraction, the
 *                            sqrt correctly rounded, and the plane holds (float)r, rounded to nearest even; else +inf (bits
 *                            0x7f800000).  The Euclidean distance from the ray's origin to int_point: not the entry distance,
 *                            not a step count; view-space z is range times the pixel's direction along the view axis.
 *   slope, two floats per pixel: for a hit ((float)gx, (float)gy), gx and gy the doubles of THE LEVEL q above
 *                            (hmrm_render_shaded) for the camera's sampling mode -- nearest modes: central differences of the
 *                            threshold table around the hit cell; HMRM_BILINEAR: the gradient of the interpolated surface at P
 *                            -- the normal is (-gx, gy, 1); else (+0.0f, +0.0f).
 * Nothing is special-cased: alpha-0 hit cells are hits, as in hmrm_render_lit.  Capped rays are non-hits in all planes and are
 * counted as in hmrm_render_interior: hmrm_render_geometry returns HMRM_E_NOTERM with valid planes; END cannot occur (no limit).
 * Like the shading arithmetic, range and slope are tested bit for bit across world scales (tests/test_world_scale_families_gpu.py): ex * ex
 * is denormal below about 2^-515 (r loses bits, and is 0 from about 2^-540 down) and infinite from about 2^508; the float is +inf
 * from 2^128, a float denormal below 2^-126 and 0 below 2^-150 -- the casts round to nearest even and keep denormals.
 * Every pointer of the struct may be NULL: that plane is not written, and nothing is fetched for it (no colour without rgba).
 * Rows are `stride` bytes apart; bytes between rows are not touched.
 * Refusals (HMRM_E_ARG, with a message) before the scene is looked at, in this order: NULL planes; an undefined flag bit;
 * reserved != 0; all four pointers NULL; a bad stride or alignment of a non-NULL plane (rgba, cell, range: stride >= 4 * width,
 * a multiple of 4; slope: >= 8 * width, a multiple of 8, the pointer 8-byte aligned; device planes are aligned to their
 * element).  Then the camera checks of hmrm_render, then a NULL scene, then the 2^24-side rule of frames.
 * hmrm_render_geometry is synchronous on the scene's stream, one such call at a time per scene; it stages the planes through
 * scene-owned device buffers that grow on demand.  hmrm_render_geometry_device takes DEVICE pointers, launches on hip_stream,
 * does no host sync and reports capped rays through hmrm_scene_take_capped for its stream -- hmrm_trace_rays_device's contract.
 * A geometry frame is launched the way an interior frame is: one launch, never measured, never the scene's probe and not
 * counted towards it; hmrm_debug_kernel_choice and every later frame are as they would have been.  It runs the scene's current
 * kernel (HMRM_KERNEL or the probe's verdict; the window records apply to HMRM_NEAREST); every kernel writes the same bytes, the
 * literal loop too (HMRM_KERNEL=simple, maps with a side >= 2^24: nearest sampling only).  All three projections, grid modes
 * and sampling modes.
 * OUT OF SCOPE: antialiasing (a filtered depth is not defined); tickets and lanes; row strips or bands; hmrm_render_multi,
 * hmrm_render_cycle, recording and statistics; a sun -- the slope plane is what a caller relights from. */
typedef struct hmrm_geometry_planes {   /* every pointer may be NULL: that plane is not written */
	void    *rgba;   size_t rgba_stride;    /* bytes per row, >= 4 * width, multiple of 4 */
	int32_t *cell;   size_t cell_stride;    /* >= 4 * width, multiple of 4 */
	float   *range;  size_t range_stride;   /* >= 4 * width, multiple of 4 */
	float   *slope;  size_t slope_stride;   /* >= 8 * width, multiple of 8; pointer 8-byte aligned */
	uint32_t flags;                          /* HMRM_TRACE_INTERIOR; any other bit: HMRM_E_ARG */
	uint32_t reserved;                       /* must be 0 */
} hmrm_geometry_planes;
int hmrm_render_geometry(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_geometry_planes *host_planes);
int hmrm_render_geometry_device(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_geometry_planes *device_planes,
                                void *hip_stream);

/* ------------------------------------------------------ accumulated lit frames */
/* Many suns or sky directions per pixel in one launch (build-side addition), exact: a soft shadow from K samples on the sun's
 * disc, an ambient-occlusion (sky-view) term, or sun plus sky composited from two light planes (INTEGRATION.md 2a has the three
 * recipes).  It is the screen-space counterpart of hmrm_cell_map_sum: the primary rays are marched ONCE, then every pixel whose
 * primary ray hit casts one shadow ray per direction, and the weights are summed per pixel before anything is quantised.
 * THE PRIMARY RAY.  Every pixel first gets hmrm_render's value; with HMRM_TRACE_INTERIOR in sun->flags hmrm_render_interior's.
 * K = n_dirs, in 1 .. 256.
 * THE VALUE PER DIRECTION.  For a pixel whose primary ray HIT (alpha-0 hit cells count, as in hmrm_render_lit) and direction k
 * let w_k be exactly the weight hmrm_render_shaded defines for that pixel when sun->dir is replaced by dirs[3k .. 3k+2] and
 * shade_flags is the one given: without HMRM_SHADE_NO_SHADOWS the pixel casts hmrm_render_lit's shadow ray towards direction k
 * -- origin (P.x, P.y, t), dir as given and NOT normalised, sun->step_dist, sun->max_steps, the camera's sampling, the interior
 * rule always on -- and a shadow ray whose status is HIT gives w_k = ambient; a pixel that is not shadowed gets 255 or,
 * HMRM_SHADE_DIFFUSE, the weight of THE LEVEL q under direction k.  Nothing is special-cased: NaN, infinite, zero and
 * below-horizon directions go through the same arithmetic.  sun->dir itself is not looked at.
 * THE SUM AND THE PLANES.  S = w_0 + .. + w_{K-1}, at most 65280.
 *   rgba,  uint32 per pixel: for a hit R, G and B become (c * S + (255 * K) / 2) / (255 * K) in integers, A stays 255; the other
 *          pixels -- misses, sky, capped primary rays -- keep the primary ray's value.
 *   light, native uint16 per pixel: S for a hit, 0xFFFF otherwise.
 * Either pointer may be NULL: that plane is not written, and no colour is fetched without rgba.  Rows are `stride` bytes apart;
 * bytes between rows are not touched.
 * Consequences, byte for byte: K = 1 is hmrm_render_shaded with sun->dir = dirs[0], under all four shade_flags; K copies of one
 * direction give that direction's K = 1 frame with light = K * w (the rounding term (255 * K) / 2 was chosen for that); the order
 * of the directions does not matter; HMRM_SHADE_NO_SHADOWS alone, or ambient = 255 without HMRM_SHADE_DIFFUSE, is hmrm_render /
 * hmrm_render_interior.
 * CAPPED RAYS.  A capped primary ray counts once; shadow rays count per RAY, up to K per pixel, as in hmrm_cell_map_sum; a capped
 * shadow ray leaves its direction lit, as in hmrm_render_lit.  hmrm_render_lit_sum returns HMRM_E_NOTERM with valid planes; the
 * device entry reports through hmrm_scene_take_capped for its stream, with no host sync -- hmrm_render_geometry_device's
 * contract.  END rays never count.
 * Refusals (HMRM_E_ARG, with a message) before the scene is looked at, in this order: hmrm_render_shaded's four; NULL dirs;
 * n_dirs outside 1 .. 256; NULL planes; reserved not 0; both pointers NULL; a bad stride or alignment of a non-NULL plane (rgba:
 * stride >= 4 * width, a multiple of 4; light: >= 2 * width, even; device pointers are aligned to their element, d_dirs to 8).
 * Then the camera checks of hmrm_render, then a NULL scene, then the 2^24-side rule of frames.
 * hmrm_render_lit_sum is synchronous on the scene's stream, one such call at a time per scene; it stages the directions, the
 * pixels and the light plane through scene-owned device buffers that grow on demand.  hmrm_render_lit_sum_device takes DEVICE
 * pointers (d_dirs: n_dirs x 3 doubles, read when the launch runs) and launches on hip_stream.
 * Launched the way a lit frame is: one launch, never measured, never the scene's probe and not counted towards it;
 * hmrm_debug_kernel_choice and every later frame are as they would have been.  It runs the scene's current kernel (HMRM_KERNEL or
 * the probe's verdict; the window records apply to HMRM_NEAREST); every kernel writes the same bytes, the literal loop too
 * (HMRM_KERNEL=simple, maps with a side >= 2^24: nearest sampling only).  All three projections, grid modes and sampling modes.
 * The work is bounded: every ray has its own budget of at most the step cap, and a pixel marches at most 1 + K rays.
 * OUT OF SCOPE: antialiasing; tickets and lanes; row strips or bands; hmrm_render_multi, hmrm_render_cycle, recording and
 * statistics; per-direction weights or colours; a baked per-cell light map read by the frame kernels (since built:
 * hmrm_render_baked below). */
typedef struct hmrm_light_planes {      /* either pointer may be NULL: that plane is not written */
	void     *rgba;  size_t rgba_stride;   /* bytes per row, >= 4 * width, multiple of 4 */
	uint16_t *light; size_t light_stride;  /* bytes per row, >= 2 * width, even */
	uint32_t  reserved[2];                 /* must be 0 */
} hmrm_light_planes;
int hmrm_render_lit_sum(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_sun *sun,
                        const double *dirs /* n_dirs x 3, host */, int32_t n_dirs, uint32_t shade_flags,
                        const hmrm_light_planes *host_planes);
int hmrm_render_lit_sum_device(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_sun *sun,
                               const void *d_dirs /* n_dirs x 24 bytes, DEVICE, 8-byte aligned */, int32_t n_dirs,
                               uint32_t shade_flags, const hmrm_light_planes *device_planes, void *hip_stream);

/* ------------------------------------------------------ baked-light frames */
/* A per-cell light plane the frame kernels read (build-side addition): the light of a static terrain under a fixed sun or sky
 * does not depend on the camera, so it is baked once -- hmrm_scene_bake_light, or any plane of the caller's: a painted light
 * map, a cumulative viewshed, a radiosity solution -- and every later frame costs a plain frame plus a small epilogue
 * (INTEGRATION.md 2a has three recipes).
 * THE SCENE'S LIGHT PLANE.  A scene owns at most one: map_w x map_h native uint16 in device memory, rows packed like the threshold
 * table, and its full scale D in 1 .. 65535: a cell whose light equals D gives the texel back.
 *   hmrm_scene_set_light         copies a HOST plane of map_w x map_h values, rows stride_bytes apart; format HMRM_LIGHT_U8 (bytes,
 *                                widened to 16 bits) or HMRM_LIGHT_U16 (native uint16).
 *   hmrm_scene_set_light_device  the same from DEVICE memory: d_plane is read on hip_stream, behind whatever the caller enqueued
 *                                there -- the output of hmrm_cell_map_sum_device goes in without a trip over the host -- and the
 *                                call returns only after the copy has finished.
 *   hmrm_scene_bake_light        the launch of hmrm_cell_map_sum over the whole map with `p` and the K = n_targets targets (host
 *                                memory), written straight into the scene's plane: byte for byte the words hmrm_cell_map_sum
 *                                writes.  D = 255 * K with HMRM_MAP_WEIGHT, else D = K (status mode: a count);
 *                                HMRM_MAP_TOWARDS_POINT is allowed.  Capped rays: HMRM_E_NOTERM with a valid plane, as there.
 *   hmrm_scene_clear_light       drops the plane.
 *   hmrm_scene_light             reads the plane back: *full_scale = D, or 0 when the scene has no plane; `out` may be NULL, else
 *                                it takes map_w x map_h native uint16, rows stride_bytes (>= 2 * map_w, even) apart.
 * Every call that changes the plane first drains the scene's own streams and its copy stream, as hmrm_scene_update does: a ticket
 * begun before the call finishes with the old plane.  Callers' own streams are the caller's business, as there.
 * hmrm_scene_update leaves the plane as it is: the light is the caller's data, and stale light is the caller's to bake again.
 * hmrm_scene_destroy frees it.
 * Refusals of hmrm_scene_set_light and hmrm_scene_set_light_device (HMRM_E_ARG, with a message), in this order: a NULL scene; a
 * NULL plane; a format outside the enum; full_scale outside 1 .. 65535; a stride below a row, or an odd stride for
 * HMRM_LIGHT_U16; for the device entry a HMRM_LIGHT_U16 pointer that is not 2-byte aligned.  Of hmrm_scene_bake_light: those of
 * hmrm_cell_map_sum, in its order and without its `out`, then a NULL scene.  After a refusal the old plane stays; if a HIP call
 * fails half-way the scene has no plane.
 * THE BAKED FRAME.  Every pixel first gets hmrm_render's value; with HMRM_TRACE_INTERIOR in baked_flags hmrm_render_interior's.
 * The primary march is unchanged.  Every pixel whose primary ray HIT (alpha-0 hit cells count, as in hmrm_render_lit) is then
 * reweighted: for each of R, G and B, c' = min(255, (c * L + D / 2) / D) in unsigned 32-bit integers; A stays 255.  Misses, sky
 * and capped primary rays are untouched.
 *   L, HMRM_NEAREST and HMRM_NEAREST_F32: plane[cell_y * map_w + cell_x] of the hit cell (hmrm_ray_hit's).
 *   L, HMRM_BILINEAR: interpolated like the colour -- the four cells c00, c10, c01, c11 and the weights tx, ty of the bilinear
 *      mode at P (the ones THE LEVEL q names), the four words read as doubles f00 .. f11, a = f00 + tx * (f10 - f00),
 *      c = f01 + tx * (f11 - f01), m = a + ty * (c - a) as plain IEEE operations in this order, no contraction; v = m + 0.5
 *      clamped to [0, 65535], L = (uint32_t)floor(v).
 * Nothing else is special-cased: L > D over-brightens and saturates at 255; L = D everywhere is hmrm_render /
 * hmrm_render_interior, byte for byte.
 * ANTIALIASING.  factor is 1, 2, 4 or 8: the baked frame of hmrm_render_aa's super camera, box-filtered with its formula inside
 * the launch; every sample is weighted on its own.  Factor 1 is the plain baked frame.
 * CAPPED RAYS are counted and reported as in hmrm_render_interior: HMRM_E_NOTERM with a valid frame.
 * TICKETS.  hmrm_render_baked_begin and hmrm_render_baked_device_begin issue tickets from the same rings and lanes as the plain
 * and lit tickets, waited for and released with the existing calls; `flags` takes HMRM_AA(n) and HMRM_NO_PROBE, which is accepted
 * and has no effect.  hmrm_record_orbit_baked (below, with the recorders) is hmrm_record_orbit_flags whose frames are baked
 * tickets.
 * Refusals (HMRM_E_ARG, with a message), in this order: an undefined bit in baked_flags; those of hmrm_render_aa (tickets: those
 * of hmrm_render_begin_flags) in their order; a NULL scene; "the scene has no light plane"; the 2^24-side rule of frames.
 * Launched the way a lit frame is: one launch, never measured, never the scene's probe and not counted towards it;
 * hmrm_debug_kernel_choice and every later frame are as they would have been.  It runs the scene's current kernel (HMRM_KERNEL or
 * the probe's verdict; the window records apply to HMRM_NEAREST); every kernel writes the same bytes, the literal loop too
 * (HMRM_KERNEL=simple, maps with a side >= 2^24: nearest sampling only).  All three projections, grid modes and sampling modes.
 * OUT OF SCOPE: row strips and bands; hmrm_render_multi, hmrm_render_cycle and statistics; several planes or coloured light; light
 * for geometry frames; a plane smaller than the map. */
enum { HMRM_LIGHT_U8 = 0, HMRM_LIGHT_U16 = 1 };
int hmrm_scene_set_light(hmrm_scene *scene, const void *plane, size_t stride_bytes, int32_t format, uint32_t full_scale);
int hmrm_scene_set_light_device(hmrm_scene *scene, const void *d_plane, size_t stride_bytes, int32_t format, uint32_t full_scale,
                                void *hip_stream);
int hmrm_scene_bake_light(hmrm_scene *scene, const hmrm_cell_map_params *p, const double *targets /* n_targets x 3, host */,
                          int32_t n_targets);
int hmrm_scene_clear_light(hmrm_scene *scene);
int hmrm_scene_light(const hmrm_scene *scene, uint16_t *out /* may be NULL */, size_t stride_bytes, uint32_t *full_scale);
int hmrm_render_baked(const hmrm_scene *scene, const hmrm_camera *cam, uint32_t baked_flags, int32_t factor, uint8_t *rgba,
                      size_t stride_bytes);
int hmrm_render_baked_begin(const hmrm_scene *scene, const hmrm_camera *cam, uint32_t baked_flags, uint32_t flags, int32_t *ticket);
int hmrm_render_baked_device_begin(const hmrm_scene *scene, const hmrm_camera *cam, uint32_t baked_flags, void *d_rgba,
                                   size_t stride_bytes, uint32_t flags, int32_t *ticket);

/* ------------------------------------------------------------ water frames */
/* hmrm_render with mirror reflections on flat water (build-side addition), exact: lakes and sea are cells at one height, and a
 * pixel that shows one mirrors the far shore and the sky.  One launch; nothing per pixel goes through memory.
 * PRIMARY PIXEL.  Every pixel first gets hmrm_render's value -- with HMRM_TRACE_INTERIOR in `flags` hmrm_render_interior's; the
 * primary march is unchanged.
 * WATER PIXEL.  A pixel whose primary ray HIT (hmap.cpp:1016 fired; an alpha-0 hit cell counts, as in hmrm_render_lit) has t,
 * exactly hmrm_render_lit's t: the threshold the hitting load compared z with -- heightmap_buf[c] + min_height (HMRM_NEAREST), the
 * float entry of that table widened to double (HMRM_NEAREST_F32), the interpolated threshold at P (HMRM_BILINEAR).  The pixel is
 * WATER when t <= level, compared as doubles, as given: a NaN level gives no water, a level of +inf makes every hit water.
 * Misses, sky, primary rays stopped by the step cap and hits above the level are untouched and cast nothing.
 * THE MIRROR RAY.  A water pixel casts one mirror ray, an hmrm_trace_segments ray: pos = (P.x, P.y, t), P the reference's int_point
 * at the hit; dir = (d.x, d.y, -d.z), d the primary ray's direction as the loop used it -- the reflection off a horizontal plane,
 * exact in IEEE arithmetic, no normal and no normalisation; water->step_dist, water->max_steps, the camera's sampling mode,
 * HMRM_TRACE_INTERIOR always on.  Nothing is special-cased: an origin with t >= max_height is not strictly inside and goes through
 * distance() as written; zero, infinite and NaN components and step_dist = 0 go through the same arithmetic.
 * THE MIRROR PIXEL m is the mirror ray's pixel as hmrm_ray_hit.rgba defines it: a HIT gives the hit cell's colour (the background
 * for an alpha-0 cell; HMRM_BILINEAR: interpolated at the mirror ray's hit point); MISS, END and CAPPED give the miss shade of the
 * mirror ray's own dir.z -- the sky gradient for a ray that rises.
 * THE STORED PIXEL.  b is the primary pixel, or `color` with HMRM_WATER_OWN_COLOR.  Each of R, G and B becomes
 * (b * (255 - r) + m * r + 127) / 255 in integers, r = reflectivity; A stays 255.  So r = 0 without HMRM_WATER_OWN_COLOR is
 * hmrm_render byte for byte (the mirror rays are marched all the same), r = 255 is the pure mirror image, and a level below
 * every threshold is hmrm_render.
 * CAPPED RAYS.  Capped primary rays and capped mirror rays are counted together; either kind makes the call return HMRM_E_NOTERM
 * with a valid frame.  END rays are never counted.  A camera looking straight down casts mirror rays straight up: without
 * max_steps they never leave the grid and run to the cap.
 * FLOODING IS THE CALLER'S JOB.  The map is not changed and no cell is made flat: clamp the height image from below at the lake's
 * luminance L, max(pixel, L), before it goes into the scene, and pass the threshold of L -- heightmap_buf's value of L plus
 * min_height -- as `level`; add a margin below the next luminance step for HMRM_NEAREST_F32, whose t is a rounded float, and for
 * HMRM_BILINEAR, whose t is interpolated (INTEGRATION.md 2a has the recipe).  Like the shading arithmetic, `t <= level`, the mirror
 * rays and the blend are tested bit for bit across world scales (tests/test_world_scale_families_gpu.py).
 * Refusals (HMRM_E_ARG, with a message) before the scene is looked at, in this order: NULL water; an undefined flag bit;
 * reserved != 0.  Then the camera checks of hmrm_render, then a NULL scene or target, then the stride (hmrm_render_water:
 * stride_bytes < width * 4; hmrm_render_water_device: hmrm_render_rows_device's rule -- >= width * 4, a multiple of 4, below 2^33),
 * then the 2^24-side rule of frames.
 * hmrm_render_water is synchronous on the scene's stream.  hmrm_render_water_device takes a DEVICE pointer, launches on
 * hip_stream, does no host sync and reports capped rays through hmrm_scene_take_capped for its stream -- hmrm_trace_rays_device's
 * contract.  Both are launched like a lit frame: one launch, never measured, never the scene's probe and not counted towards it,
 * with the scene's current kernel (HMRM_KERNEL or the probe's verdict; the window records apply to HMRM_NEAREST); every kernel
 * writes the same bytes, the literal loop too (HMRM_KERNEL=simple, maps with a side >= 2^24: nearest sampling only).  All three
 * projections, grid modes and sampling modes.
 * OUT OF SCOPE: strip and multi-GPU water frames (hmrm_render_multi), statistics and geometry planes of a water frame;
 * refraction, Fresnel terms, waves; a second bounce.  Antialiased, ticketed and recorded water frames, and water under the scene's
 * baked light: below.  Water combined with shadow rays and diffuse shading: hmrm_render_water_lit, below those. */
#define HMRM_WATER_OWN_COLOR 2u      /* the water's own colour is `color`, not the primary pixel */
typedef struct hmrm_water {          /* 32 bytes */
	double   level;        /* a hit is WATER when t <= level; compared as doubles, as given */
	double   step_dist;    /* of the mirror march, in units of |dir| */
	uint32_t max_steps;    /* step limit L of every mirror ray, 0 = none (hmrm_trace_segments' rule) */
	uint32_t flags;        /* HMRM_TRACE_INTERIOR (primary rays under the interior rule), HMRM_WATER_OWN_COLOR; any other bit: HMRM_E_ARG */
	uint8_t  reflectivity; /* r, 0..255 */
	uint8_t  color[3];     /* R, G, B with HMRM_WATER_OWN_COLOR */
	uint8_t  reserved[4];  /* must be 0 */
} hmrm_water;
int hmrm_render_water(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_water *water, uint8_t *rgba, size_t stride_bytes);
int hmrm_render_water_device(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_water *water, void *d_rgba,
                             size_t stride_bytes, void *hip_stream);
/* The water frame's second step: antialiased, ticketed, recorded, and under the scene's light plane.  `water_mode` is an argument
 * of its own, not a bit of hmrm_water.flags, whose undefined bits stay refused; hmrm_render_water and hmrm_render_water_device do
 * not change.
 * THE BAKED WATER FRAME (water_mode & HMRM_WATER_BAKED) composes hmrm_render_water and hmrm_render_baked and adds nothing.  L of a
 * hit is hmrm_render_baked's L of that hit: for the nearest modes the plane's word of the hit cell, for HMRM_BILINEAR the
 * interpolated word at the hit point, in that definition's operation order; weight(c, L) is its min(255, (c * L + D / 2) / D) per
 * channel.  Every pixel whose primary ray HIT, wet or dry, has b' = weight(b, L of the primary hit), b the primary pixel or, for a
 * WATER pixel with HMRM_WATER_OWN_COLOR, the water's `color`; an alpha-0 hit cell's background is weighted too.  A water pixel's
 * mirror pixel is m' = weight(m, L of the mirror ray's hit) when the mirror ray's status is HIT; for MISS, END and CAPPED m' is that
 * ray's miss shade, untouched.  The stored pixel is hmrm_render_water's blend of b' and m'; a dry pixel stores b'; misses and capped
 * primary rays are untouched.  So L = D everywhere is hmrm_render_water byte for byte, a level below every threshold is
 * hmrm_render_baked, r = 0 without HMRM_WATER_OWN_COLOR is hmrm_render_baked, and water_mode 0 with factor 1 is hmrm_render_water.
 * ANTIALIASING.  factor is 1, 2, 4 or 8: the result is the water frame (baked or not) of hmrm_render_aa's super camera, box-filtered
 * with its formula inside the launch.  Every sample decides "water" on its own, casts its own mirror ray and is weighted and blended
 * on its own before the filter.
 * TICKETS (hmrm_render_water_begin, hmrm_render_water_device_begin) come from the same rings, lanes and device-ticket pool as the
 * plain, lit and baked tickets and are waited for and released with the same calls.  `flags` takes HMRM_AA(n), and HMRM_NO_PROBE,
 * which is accepted and has no effect.  *water is copied at begin.  The light plane is looked up under the scene's lock at begin: a
 * ticket begun before hmrm_scene_set_light finishes with the old plane.
 * THE RECORDER (hmrm_record_orbit_water) is hmrm_record_orbit_flags whose frames are water tickets; it checks the water, the mode
 * and every scene's plane before any frame and writes no file on refusal.
 * CAPPED RAYS.  Primary and mirror rays are counted together, per sample, as in hmrm_render_water, and reported the way the
 * corresponding baked entry reports them.
 * Refusals (HMRM_E_ARG, with a message), in this order: hmrm_render_water's three of the water; an undefined bit in water_mode;
 * those of hmrm_render_aa (tickets: those of hmrm_render_begin_flags) in their order; a NULL scene; with HMRM_WATER_BAKED "the scene
 * has no light plane"; the 2^24-side rule.
 * Launched like every water frame: one launch, never measured, never the probe and not counted towards it, with the scene's
 * current kernel; every kernel writes the same bytes, the literal loop too (nearest sampling only). */
#define HMRM_WATER_BAKED 1u          /* water_mode: the frame under the scene's light plane */
int hmrm_render_water_aa(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_water *water, uint32_t water_mode,
                         int32_t factor, uint8_t *rgba, size_t stride_bytes);
int hmrm_render_water_begin(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_water *water, uint32_t water_mode,
                            uint32_t flags, int32_t *ticket);
int hmrm_render_water_device_begin(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_water *water, uint32_t water_mode,
                                   void *d_rgba, size_t stride_bytes, uint32_t flags, int32_t *ticket);
int hmrm_record_orbit_water(hmrm_scene *const *scenes, int32_t n_scenes, const hmrm_camera *base, double centre_x,
                            double centre_y, double radius, double hang0, int32_t frames, const char *dir, long long id,
                            int32_t encoder_threads, int32_t verbose, uint32_t flags, const hmrm_water *water,
                            uint32_t water_mode);

/* THE SUN-LIT WATER FRAME composes hmrm_render_water and hmrm_render_shaded and adds nothing.  It follows the pattern of the baked
 * water frame, with hmrm_render_shaded's weight in place of the plane's.
 * Inputs: a camera, an hmrm_water, an hmrm_sun, and shade_flags, with HMRM_SHADE_DIFFUSE and HMRM_SHADE_NO_SHADOWS as today.  The
 * primary rays run under the interior rule when water->flags or sun->flags carries HMRM_TRACE_INTERIOR.
 * 1. PRIMARY PIXEL, t, WATER.  These are exactly hmrm_render_water's: the same primary march, the same threshold t, the same
 *    t <= level comparison.
 * 2. WEIGHT OF A HIT.  w(hit) is hmrm_render_shaded's w for that hit under sun and shade_flags:
 *    - Without HMRM_SHADE_NO_SHADOWS, the hit casts hmrm_render_lit's shadow ray.  Its origin is (H.x, H.y, t_H), with H the hit's
 *      int_point and t_H the threshold its hitting load compared z with.  It uses sun->dir, sun->step_dist and sun->max_steps, with
 *      the interior rule on.  A shadow ray whose status is HIT gives w = ambient.
 *    - Otherwise w = 255 without HMRM_SHADE_DIFFUSE.  With it, w = ambient + ((255 - ambient) * q + 127) / 255.  q is the level of
 *      that hit from the existing arithmetic: the hit's cell for the nearest modes, the hit's point for bilinear.
 *    - weight(c, w) = (c * w + 127) / 255 per channel.
 * 3. BASE.  Every pixel whose primary ray HIT, wet or dry, has b' = weight(b, w(primary hit)).  b is the primary pixel, or for a
 *    WATER pixel with HMRM_WATER_OWN_COLOR the water's color.  An alpha-0 cell's background is weighted too, as in
 *    hmrm_render_shaded.
 * 4. MIRROR PIXEL.  A WATER pixel casts hmrm_render_water's mirror ray, unchanged.
 *    - If that ray's status is HIT, m' = weight(m, w(mirror hit)).  Its own shadow ray starts at the mirror ray's int_point and the
 *      threshold of the mirror ray's hitting load.  Its own diffuse level is taken at the mirror hit's cell or point.
 *    - For MISS, END and CAPPED, m' is the mirror ray's miss shade, untouched.
 * 5. STORED PIXEL.  A WATER pixel stores hmrm_render_water's blend of b' and m'.  A dry hit stores b'.  Misses and capped primary
 *    rays are untouched.
 * 6. CAPPED RAYS.  All four kinds are counted together: primary rays, primary shadow rays, mirror rays and mirror shadow rays.  END
 *    rays are never counted.  Either kind returns HMRM_E_NOTERM with a valid frame.
 * Consequences, each byte for byte: a level below every threshold, or a NaN level, gives hmrm_render_shaded; r = 0 without own
 * colour gives hmrm_render_shaded; HMRM_SHADE_NO_SHADOWS alone gives hmrm_render_water; ambient = 255 gives hmrm_render_water under
 * any flags (the shadow rays are marched all the same).
 * Refusals are HMRM_E_ARG with a message and come before the scene is looked at, in this order: hmrm_render_water's three of the
 * water; hmrm_render_shaded's four of the sun and shade_flags; then as hmrm_render_water / hmrm_render_water_device.
 * hmrm_render_water_lit is synchronous on the scene's stream; hmrm_render_water_lit_device is hmrm_render_water_device's form.
 * Launched like every water frame: one launch, never measured, never the probe and not counted towards it, with the scene's
 * current kernel; every kernel writes the same bytes, the literal loop too (nearest sampling only).  A wave marches up to four
 * times in that launch; nothing per pixel goes through memory.
 * OUT OF SCOPE: antialiased, ticketed and recorded lit water frames; lit water under the baked plane; several suns; strips and
 * multi-GPU. */
int hmrm_render_water_lit(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_water *water, const hmrm_sun *sun,
                          uint32_t shade_flags, uint8_t *rgba, size_t stride_bytes);
int hmrm_render_water_lit_device(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_water *water, const hmrm_sun *sun,
                                 uint32_t shade_flags, void *d_rgba, size_t stride_bytes, void *hip_stream);

/* -------------------------------------------------------------- haze frames */
/* hmrm_render with distance fog (build-side addition), exact: a far ridge fades towards one haze colour, blended by the kernel
 * before the pixel is stored -- and before the box filter of an antialiased frame.  One launch; no range plane and no second
 * kernel.  (A caller who composites objects of their own still takes the range plane of hmrm_render_geometry: INTEGRATION.md 2a.)
 * A HAZE FRAME is hmrm_render's frame; with HMRM_TRACE_INTERIOR in haze->flags it is hmrm_render_interior's frame; with `factor` 2,
 * 4 or 8 it is hmrm_render_aa's frame (of either kind of primary ray).  In each case every pixel, or every sample of the super
 * camera, is blended towards haze->color by an amount read from the caller's table at the pixel's range.
 * RANGE.  r is the geometry frame's range BEFORE its rounding to float: e = int_point - the ray's origin,
 * r = sqrt((ex * ex + ey * ey) + ez * ez) in plain IEEE doubles in this order, no contraction, the sqrt correctly rounded.
 * INDEX.  u = (r - start) * scale: one double subtract, then one double multiply.  i = n - 1 if u >= (double)(n - 1); else
 * i = (int)u, the truncation, if u > 0; else i = 0 -- a NaN u takes index 0.  start and scale are used as given: NaN, infinite,
 * zero and negative values go through the same arithmetic and are not refused.
 * AMOUNT.  f = table[i], a byte; n is 1 .. 4096.
 * THE STORED PIXEL OF A HIT (hmap.cpp:1016 fired; an alpha-0 hit cell counts, as in hmrm_render_lit, and its background colour is
 * hazed too): each of R, G and B becomes (c * (255 - f) + h * f + 127) / 255 in integers, h = haze->color; A stays 255 -- the water
 * frame's blend.
 * NON-HITS -- the miss shade, and rays stopped by the step cap -- are untouched; with HMRM_HAZE_SKY they are blended at
 * f = table[n - 1]: the sky is as hazy as the farthest terrain.
 * ANTIALIASING.  Every sample is hazed on its own, then hmrm_render_aa's box filter runs.
 * CAPPED RAYS are counted and reported as in hmrm_render_interior / hmrm_render_aa: hmrm_render_haze returns HMRM_E_NOTERM with a
 * valid frame, hmrm_render_haze_device reports through hmrm_scene_take_capped for its stream.
 * Consequences, each byte for byte: a table of zeros gives hmrm_render / hmrm_render_interior / hmrm_render_aa; a table of 255s
 * with HMRM_HAZE_SKY gives a frame of the haze colour; without HMRM_HAZE_SKY the non-hit pixels are hmrm_render's; the order of the
 * entries matters only through i.  The kernel evaluates no transcendental -- the law is the table's -- which is why the frame is
 * bit-exact.  Like the shading arithmetic, the range and the index are tested bit for bit across world scales
 * (tests/test_world_scale_families_gpu.py), r = 0, denormal and +inf included: from about 2^508 every hit sits on the last entry.
 * hmrm_haze_table (host only) fills out[i] = min(255, (int)(255 * (1 - T) + 0.5)), x = (i + 0.5) / n, with T = 1 - x
 * (HMRM_HAZE_LINEAR), T = exp(-density * x) (HMRM_HAZE_EXP) or T = exp(-(density * x) * (density * x)) (HMRM_HAZE_EXP2), exp the
 * host's libm; HMRM_E_ARG for another law, n outside 1 .. 4096 or NULL out.
 * Refusals (HMRM_E_ARG, with a message) before the scene is looked at, in this order: NULL haze; an undefined flag bit;
 * reserved != 0; n outside 1 .. 4096; NULL table; a factor that is not 1, 2, 4 or 8; the camera checks of hmrm_render, and behind
 * them hmrm_render_aa's limit on the super frame, which needs the camera; a NULL scene or target; the stride (hmrm_render_haze:
 * stride_bytes < width * 4; hmrm_render_haze_device: hmrm_render_rows_device's rule -- >= width * 4, a multiple of 4, below 2^33);
 * the 2^24-side rule of frames.
 * hmrm_render_haze is synchronous on the scene's stream and stages the n bytes of the table through a scene-owned device buffer.
 * hmrm_render_haze_device takes a DEVICE table of n bytes and a DEVICE target, launches on hip_stream and does no host sync --
 * hmrm_trace_rays_device's contract.  Both are launched like an interior frame: one launch, never measured, never the scene's
 * probe and not counted towards it, with the scene's current kernel (HMRM_KERNEL or the probe's verdict; the window records apply
 * to HMRM_NEAREST); every kernel writes the same bytes, the literal loop too (HMRM_KERNEL=simple, maps with a side >= 2^24: nearest
 * sampling only).  All three projections, grid modes and sampling modes.
 * OUT OF SCOPE: tickets and lanes; the recorder; row strips, bands and hmrm_render_multi; statistics; haze combined with a sun,
 * the scene's light plane or water; height-dependent fog. */
#define HMRM_HAZE_SKY 2u             /* the pixels that did not hit are blended at table[n - 1] */
#define HMRM_HAZE_LINEAR 0
#define HMRM_HAZE_EXP    1
#define HMRM_HAZE_EXP2   2
typedef struct hmrm_haze {           /* 32 bytes */
	double   start;        /* range at which entry 0 ends being the only entry */
	double   scale;        /* entries per unit of range */
	uint32_t n;            /* table length, 1 .. 4096 */
	uint32_t flags;        /* HMRM_TRACE_INTERIOR, HMRM_HAZE_SKY; any other bit: HMRM_E_ARG */
	uint8_t  color[3];     /* R, G, B of the haze */
	uint8_t  reserved[5];  /* must be 0 */
} hmrm_haze;
int hmrm_render_haze(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_haze *haze, const uint8_t *table, int32_t factor,
                     uint8_t *rgba, size_t stride_bytes);
int hmrm_render_haze_device(const hmrm_scene *scene, const hmrm_camera *cam, const hmrm_haze *haze, const void *d_table,
                            int32_t factor, void *d_rgba, size_t stride_bytes, void *hip_stream);
int hmrm_haze_table(int32_t law, double density, int32_t n, uint8_t *out);   /* host only */

/* -------------------------------------------------------------- view batches */
/* Many cameras of one scene in ONE launch (build-side addition): the six faces of an environment probe, a stereo pair, a strip of
 * thumbnails, a few hundred small views for agents.  Below about a megapixel a frame's time is launch cost and the tail of a short
 * grid; a batch pays both once.
 * VIEW k OF A BATCH is, byte for byte, hmrm_render's frame of cams[k]; with HMRM_TRACE_INTERIOR in `flags` it is
 * hmrm_render_interior's frame of cams[k].  Nothing is shared between views except the scene.
 * BATCH SIZE.  n is 1 .. HMRM_MAX_VIEWS.
 * UNIFORM FIELDS.  All cameras share width, height, projection and sampling: what the launch dispatches on and what fixes its grid.
 * FREE FIELDS.  Everything else may differ per view: pos, hang, vang, hfov, ortho_width, step_dist, the background.
 * TARGET LAYOUT.  View k starts at byte k * view_stride_bytes of the target; its rows are stride_bytes apart.  Bytes between rows
 * and between views are not written.
 * REFUSALS (HMRM_E_ARG, with a message) before the scene is looked at, in this order:
 *   1. NULL cams;
 *   2. n outside 1 .. HMRM_MAX_VIEWS;
 *   3. an undefined flag bit (defined: HMRM_TRACE_INTERIOR);
 *   4. a camera that differs from cams[0] in one of the four uniform fields -- the message names the first such view and the field
 *      -- and then cams[0] itself where hmrm_render's camera checks refuse it (they look at those four fields only);
 *   5. a NULL scene or target;
 *   6. the stride.  hmrm_render_views: stride_bytes < width * 4.  hmrm_render_views_device: hmrm_render_rows_device's rule -- >=
 *      width * 4, a multiple of 4, below 2^33;
 *   7. view_stride_bytes < height * stride_bytes; hmrm_render_views_device only: it must also be a multiple of 4;
 *   8. a batch whose last byte, (n - 1) * view_stride_bytes + (height - 1) * stride_bytes + width * 4 - 1, lies at or beyond 2^40;
 *   9. a batch of more than 65535 * 32768 tile rows, n * ceil(height / 16): the launch's grid does not hold them;
 *  10. a batch whose frame records (352 bytes per view) and DISTINCT spherical tables exceed HMRM_MAX_VIEWS_STAGING bytes: it is
 *      refused, not truncated.  Spherical views that agree bit for bit in (hang, hfov, width) share one pair of column tables, 16 *
 *      width bytes; views that agree in (vang, hfov, width, height) share one pair of row tables, 16 * height bytes: a cube of
 *      agents looking the same way, or an orbit at one vang, costs one row table.
 * Behind them the 2^24-side rule of frames.
 * CAPPED RAYS.  hmrm_render_views returns HMRM_E_NOTERM with valid frames when a ray of any view reached the step cap, as
 * hmrm_render_interior does; hmrm_render_views_device reports through hmrm_scene_take_capped for its stream.  The count is the
 * batch's, not per view.
 * SYNCHRONY.  hmrm_render_views is synchronous on the scene's stream, renders into a scene-owned device buffer and reads the frames
 * back.  hmrm_render_views_device takes a DEVICE target, launches on hip_stream and does no host wait -- not for the upload of its
 * frame records and tables either: they travel through pinned memory the stream's launch state owns and are copied in stream
 * order; an event guards the reuse of each of its four staging blocks, so batches on one stream may follow each other at once (a
 * fifth batch while four uploads are still in flight waits for the oldest).  The first call on a stream, and a call that needs
 * larger blocks than any before it, allocate.
 * KERNELS.  One launch, never measured, never the scene's probe and not counted towards it, with the scene's current kernel
 * (HMRM_KERNEL or the probe's verdict; the window records apply to HMRM_NEAREST); every kernel writes the same bytes, the literal
 * loop too (HMRM_KERNEL=simple, maps with a side >= 2^24: nearest sampling only).  All three projections, grid modes and sampling
 * modes.
 * OUT OF SCOPE: antialiasing; tickets and lanes; the recorder; row strips, bands and hmrm_render_multi; statistics; launch-order
 * calibration and the probe; every other family (sun, water, baked light, haze, geometry planes). */
#define HMRM_MAX_VIEWS 65536
#define HMRM_MAX_VIEWS_STAGING (256u << 20)
int hmrm_render_views(const hmrm_scene *scene, const hmrm_camera *cams, int32_t n, uint32_t flags,
                      uint8_t *rgba, size_t stride_bytes, size_t view_stride_bytes);
int hmrm_render_views_device(const hmrm_scene *scene, const hmrm_camera *cams, int32_t n, uint32_t flags,
                             void *d_rgba, size_t stride_bytes, size_t view_stride_bytes, void *hip_stream);
/* Host only, for tests: which pair of column tables and which pair of row tables each view of such a batch uses -- tables numbered
 * from 0 in the order of their first view; -1 for every view of a batch that is not spherical.  Looks at nothing but n (1 ..
 * HMRM_MAX_VIEWS) and the cameras. */
int hmrm_debug_views_tables(const hmrm_camera *cams, int32_t n, int32_t *out_col_index, int32_t *out_row_index);

/* Picking: the ray of pixel (px, py) of `cam` (ImagePlane::GetRay on the device, as hmrm_debug_ray) traced with the camera's
 * step_dist, background and sampling.  hit->rgba is that pixel of hmrm_render.  A convenience (two small launches and a
 * host sync), not a hot path: trace a batch for many pixels.  HMRM_E_NOTERM when the ray was stopped by the step cap. */
int hmrm_pick(const hmrm_scene *scene, const hmrm_camera *cam, int32_t px, int32_t py, hmrm_ray_hit *hit);

/* Device-side ImagePlane::GetRay (ImagePlane.hpp:10) and distance()
 * (AABB.hpp:12) for one pixel -- per-ray parity hooks. */
int hmrm_debug_ray(const hmrm_scene *scene, const hmrm_camera *cam,
                   int32_t px, int32_t py, double pos[3], double dir[3], double *entry_d);

/* Host-only (no GPU needed): the per-frame record the kernel receives for this
 * camera -- the reference's per-frame set-up, main/hmap.cpp:661-672,:952-974.
 * out25 = cam[3], upper_left[3], plane_right[3], plane_down[3], look[3], c0[3],
 * c1[3], nudge, step_dist, grid_pow2, inv_grid_width.  `tables` (may be NULL;
 * used for HMRM_SPHERICAL) receives 2*width + 2*height doubles: cos(ha) and
 * sin(ha) per column, then sin(va) and cos(va) per row (Spherical.cpp:18-25). */
int hmrm_debug_frame(const hmrm_camera *cam, const hmrm_scene_params *params,
                     int32_t map_w, int32_t map_h, double *out25, double *tables);

/* Host-only test hook (no GPU needed, no reference counterpart: the reference's OpenMP loop has no launch order).
 * The library hands a frame's 16-row tile rows to the GPU in an order calibrated from one measured launch per
 * cached camera: records[2 t] = start of tile row t's first workgroup, records[2 t + 1] = duration of its longest
 * wave (10 ns ticks), measured under the plain rotation that starts at tile row `rot`.  Returns the number of
 * contiguous pieces (0..3; 0 = the rotation stays) the plan starts first, in order, in pieces_begin / pieces_count,
 * and, when tile_row_of_grid_row is not NULL (tile_rows entries), the resulting permutation: which tile row the
 * grid's row j renders.  Scheduling only -- no order changes a pixel.  Negative = HMRM_E_ARG. */
int hmrm_debug_plan_order(const uint64_t *records, int32_t tile_rows, int32_t rot, int32_t pieces_begin[3],
                          int32_t pieces_count[3], int32_t *tile_row_of_grid_row);

/* Host-only test hook (no GPU, no reference counterpart): the state machine behind that calibration and the scene's kernel
 * probe, driven through `launches` full-frame launches of one camera.  records holds, per launch, tile_rows x {start,
 * longest wave} as above: what a measured launch would report (read only for the launches the machine decides to measure; the
 * report arrives before the next launch).  can_measure[i] (NULL = always): the caller has free record buffers and the scene's
 * other streams are idle.  Out, per launch: the trial whose order it uses (0 = the rotation), whether it is measured, whether it
 * runs the plain-groups kernel; then the number of trials made, the settled one (-1: none yet), the scene's verdict
 * (1 = plain groups) and the launch whose report settled the calibration (-1: not settled). */
int hmrm_debug_calibrate(const uint64_t *records, int32_t launches, int32_t tile_rows, int32_t rot, int32_t may_probe,
                         int32_t scene_already_probed, const uint8_t *can_measure, int32_t *trial_used, int32_t *measured,
                         int32_t *group_kernel, int32_t *n_trials, int32_t *best, int32_t *scene_use_group,
                         int32_t *settled_at_launch);

/* Host-only test hook (no GPU, no reference counterpart): what the march kernels read of pyramid level `level` (0 .. levels - 1,
 * or `levels` = the whole map), unpacked from the per-level byte they fetch it from, and where the level policy moves from
 * there for a ray that is `young` (non-zero: it moves two levels at a time) in a frame whose finest level is min_level.
 * out: [0] log2 of the window stride in cells, [1] strides a ray steps back when its cell index falls (strides per window
 * - 1), [2] window size in cells, [3] levels per move, [4] the level a move up goes to, [5] the level a move down goes to,
 * [6] 1 when level == min_level, [7] the byte itself.  Returns the number of pyramid levels; negative = HMRM_E_ARG. */
int hmrm_debug_level_state(int32_t level, int32_t young, int32_t min_level, int32_t out[8]);

/* Accuracy of the hardware reciprocal v_rcp_f64 on the current device (test hook; no reference counterpart:
 * the reference divides, AABB.cpp:62-63, and the kernel's one-division shortcut through distance() must prove
 * from approximate quotients which exact quotient is the result).  mode 0: the leading 32 mantissa bits
 * exhaustively for exponent exp_lo (count = 2^32 covers them; trailing 20 bits 0 / all ones / hashed by
 * seed & 3); mode 1: hashed mantissa, sign and exponent in [exp_lo, exp_hi]; mode 2: n * rcp(d) against the
 * correctly rounded n / d for box-like n (exponent in [exp_lo, exp_hi]) and direction-like d (2^-40..1).
 * *max_rel_err = largest relative error seen; hist64 (may be NULL) = 64 counters, [k] = samples with an
 * error in [2^-k, 2^-(k-1)), [63] also holds the exact ones. */
int hmrm_debug_rcp_error(int32_t mode, uint64_t count, uint64_t seed, int32_t exp_lo, int32_t exp_hi,
                         double *max_rel_err, uint64_t *hist64);

/* Test hook, needs no GPU: the window-maximum pyramid layout hmrm_scene_create chooses for a map_w x map_h map
 * (row pitch in windows, log2 of the plane pitch, number of levels).  Returns 1 when 32-bit BYTE offsets would cover
 * every plane, 0 when only 64-bit ones do (very oblong maps near the 2^29-cell limit, e.g. 16385 x 32766).  The
 * production kernel forms the offsets in 64 bits since round 5, so both kinds of map render with it (round 4 sent the
 * second kind through the literal loop, main/hmap.cpp:1000-1038 as written, 85 x slower).  Negative = HMRM_E_ARG. */
int hmrm_debug_mip_layout(int32_t map_w, int32_t map_h, int32_t *mip_row, int32_t *plane_shift, int32_t *levels);

/* Which kernel full frames of this scene are rendered with: 0 = the production kernel (speculative groups + exact
 * leaps over the window-maximum pyramid), 1 = the speculative groups alone, 2 = the literal loop, 3 = the speculative
 * groups with leaps over window records (a 16-cell window's maximum without its 8 highest cells, and where those stand:
 * nearest-sampling frames; frames of the other sampling modes keep the production kernel then).  1 or 3 without
 * HMRM_KERNEL=group / rec means the scene's one-time probe (part of the launch-order calibration of the first camera
 * that is rendered repeatedly, or -- for cameras that never repeat -- the scene's sixth full frame launched twice)
 * measured that kernel at least 3 % faster on this content -- maps on which rays cannot jump over whole windows: needles
 * on a plateau, white noise. */
int hmrm_debug_kernel_choice(const hmrm_scene *scene);

/* Test hook: the scene's window records -- one 32-byte record per 16 x 16-cell window of the map, a window every 4 cells,
 * ceil(map_w / 4) per row and ceil(map_h / 4) rows: { float max2; uint32 spare; uint8 xs[8]; uint8 ys[8]; uint32 spare[2] },
 * max2 = the window's maximum hit threshold without its 8 highest cells (rounded up to float), xs / ys = where the cells
 * strictly above it stand inside the window (255: slot unused) -- and the threshold table they were built from
 * (heightmap_buf[i] + min_height, main/hmap.cpp:1013-1016; map_w x map_h doubles), copied to the host.  Either pointer
 * may be NULL.  The record kernel (hmrm_debug_kernel_choice 3) leaps across a window when the ray stays at or above max2
 * and its path misses the recorded cells; no counterpart in the reference, which samples every step. */
int hmrm_debug_read_records(const hmrm_scene *scene, void *records_out, double *thr_out);

/* Test hook (no GPU): which kernel a frame is launched with -- returns 0 the plain groups, 1 the production kernel, 2 the
 * record kernel -- given HMRM_KERNEL (`forced`: 0 none, 1 group, 3 rec), whether the launch plan or the scene's verdict
 * asks for the other kernel, whether this frame could run the record kernel (nearest sampling), and the scene's probe
 * state (verdict for the other kernel; obtained with the record kernel or with the plain groups).  A verdict holds for
 * the frames that would run what was measured.  *with_records_after: what the scene remembers afterwards (a probe's own
 * launch notes what it measures). */
int hmrm_debug_pick_kernel(int32_t forced, int32_t use_other, int32_t records_ok, int32_t scene_verdict, int32_t scene_with_records,
                           int32_t *with_records_after);

/* The environment knobs (HMRM_KERNEL, HMRM_STEP_CAP, ...) are read once, when a
 * scene is created; this re-reads them for a live scene (tests and tools switch kernel variants).  Launch orders
 * calibrated so far are forgotten (they were measured on the old kernel variant). */
int hmrm_debug_reload_env(hmrm_scene *scene);

/* Time of the most recent render kernel launch on this thread, measured with
 * HIP events on the launch stream (ms); <0 if none. Only valid after
 * hmrm_render / hmrm_render_stats, which synchronise. */
double hmrm_last_kernel_ms(void);

/* Launches the render kernel `iters` times back to back into a device scratch
 * frame (no D2H) and returns the mean kernel duration in ms measured with HIP
 * events on the launch stream; <0 on error.  Bench hook. */
double hmrm_bench_kernel_ms(const hmrm_scene *scene, const hmrm_camera *cam, int32_t iters);

/* ---------------------------------------------------------------- recording */
/* Programmatic animation for the reference's recording mode (hmap.cpp:869-900,
 * :916-926 is an empty "alter this block and recompile" stub, :1131-1144 saves
 * frames).  The sweep is the orbit of BASELINE config C5: camera of frame k of
 * `frames` on a horizontal circle of `radius` around (centre_x, centre_y), looking at
 * the centre: hang_k = hang0 + 2*pi*k/frames, pos_k = centre - radius*(cos, sin)(hang_k);
 * everything else from `base`. */
void hmrm_orbit_camera(const hmrm_camera *base, double centre_x, double centre_y, double radius,
                       double hang0, int32_t frame, int32_t frames, hmrm_camera *out);
/* Renders `frames` orbit frames and saves them as <dir>/hmap_<id>_<n>.png
 * (hmap.cpp:1132-1134) with a pool of PNG encoder threads (0 = one per host core).
 * verbose != 0 prints the reference's "Saved screenshot at ..." / "Done recording." lines. */
int hmrm_record_orbit(const hmrm_scene *scene, const hmrm_camera *base, double centre_x, double centre_y,
                      double radius, double hang0, int32_t frames, const char *dir, long long id,
                      int32_t encoder_threads, int32_t verbose);
/* The same sweep sharded over several scenes -- one per GPU, each created after hmrm_set_device
 * with the same maps (BASELINE config C5): frame k is rendered by scenes[k mod n_scenes]
 * (hmrm_orbit_frame_owner), no exchange between devices, one shared pool of encoder threads.
 * Files and bytes are those of hmrm_record_orbit. */
int hmrm_record_orbit_multi(hmrm_scene *const *scenes, int32_t n_scenes, const hmrm_camera *base,
                            double centre_x, double centre_y, double radius, double hang0, int32_t frames,
                            const char *dir, long long id, int32_t encoder_threads, int32_t verbose);
/* hmrm_record_orbit_multi with per-frame flags for its ticketed renders (hmrm_render_begin_flags: HMRM_AA(n) records an
 * antialiased sweep, HMRM_NO_PROBE).  flags = 0 writes the files of hmrm_record_orbit_multi, which calls it so. */
int hmrm_record_orbit_flags(hmrm_scene *const *scenes, int32_t n_scenes, const hmrm_camera *base,
                            double centre_x, double centre_y, double radius, double hang0, int32_t frames,
                            const char *dir, long long id, int32_t encoder_threads, int32_t verbose, uint32_t flags);
/* hmrm_record_orbit_flags whose frames are lit tickets (hmrm_render_shaded_begin with `sun`, `shade_flags` and `flags`): a
 * shaded, shadowed, antialiased orbit as PNGs.  sun = NULL with shade_flags = 0 is hmrm_record_orbit_flags, which calls it so:
 * the same ticketed renders, the same files; sun = NULL with shade_flags != 0 is HMRM_E_ARG, and so is a sun or a shade_flags
 * word that hmrm_render_shaded_begin refuses -- before any scene is looked at.  *sun is copied. */
int hmrm_record_orbit_shaded(hmrm_scene *const *scenes, int32_t n_scenes, const hmrm_camera *base,
                             double centre_x, double centre_y, double radius, double hang0, int32_t frames,
                             const char *dir, long long id, int32_t encoder_threads, int32_t verbose, uint32_t flags,
                             const hmrm_sun *sun, uint32_t shade_flags);
/* hmrm_record_orbit_flags whose frames are baked tickets (hmrm_render_baked_begin with `baked_flags` and `flags`): a flight
 * through baked light as PNGs.  Every scene must have a light plane, else HMRM_E_ARG before any frame; an undefined bit in
 * baked_flags is refused before anything else. */
int hmrm_record_orbit_baked(hmrm_scene *const *scenes, int32_t n_scenes, const hmrm_camera *base,
                            double centre_x, double centre_y, double radius, double hang0, int32_t frames,
                            const char *dir, long long id, int32_t encoder_threads, int32_t verbose, uint32_t flags,
                            uint32_t baked_flags);
int32_t hmrm_orbit_frame_owner(int32_t frame, int32_t n_devices);

/* ------------------------------------------------------------------- config */
/* Replaces ConsumeConfigStream (main/hmap.cpp:309-520) and the globals'
 * defaults (:31-112).  Same whitespace token grammar, same 27 keys, same echo of
 * every option to `echo_fd`-style sinks: echo text is appended to an internal
 * log retrievable with hmrm_config_log().  Additive keys (not in the reference,
 * named by north_star): `projection perspective|spherical|orthographic|1|2|3`,
 * `output <path.png|.ppm>`, `record orbit|off`, `devices n`, `sampling nearest|bilinear`, `heights f64|f32`,
 * `antialias 1|2|4|8` (hmrm_render_aa's factor; another value warns "WARNING: Unknown antialias: v" and keeps the old one),
 * `interior on|off|1|0` (default off; the CLI renders its single frame with hmrm_render_interior; another value warns
 * "WARNING: Unknown interior: v" and keeps the old one),
 * `shadows on|off|1|0` (default off; the CLI renders its single frame with hmrm_render_lit; another value warns "WARNING:
 * Unknown shadows: v" and keeps the old one), `sun_dir x y z` (default 0.5 0.5 0.7071..., used as given), `shadow_ambient n`
 * (0..255, default 128; another value warns "WARNING: shadow_ambient must be 0..255" and keeps the old one),
 * `shadow_step_dist v` (absent: the camera's step_dist), `shadow_max_steps n` (default 0 = none; a value outside
 * 0..4294967295 warns and keeps the old one), `shading on|off|1|0` (default off; the CLI renders its single frame with
 * hmrm_render_shaded, HMRM_SHADE_DIFFUSE, plus HMRM_SHADE_NO_SHADOWS unless `shadows on`; another value warns "WARNING:
 * Unknown shading: v" and keeps the old one), `sun_scope single|all` (default single: shadows / shading apply to the plain
 * single frame only, as before; all: they also apply with `antialias n` > 1 -- hmrm_render_shaded_aa -- and to `record orbit`
 * -- hmrm_record_orbit_shaded; another value warns "WARNING: Unknown sun_scope: v" and keeps the old one),
 * `sun_map <path.png>` (echoed like `output`; after its frames the CLI writes the whole map's HMRM_MAP_WEIGHT cell map as a
 * one-component PNG: the config's sun, the camera's sampling, HMRM_MAP_DIFFUSE with `shading on`, HMRM_MAP_NO_SHADOWS only for
 * `shading on` without `shadows on`), `sun_map_lift v` (default 0: hmrm_cell_map_params.lift of that map),
 * `sky_map <path.png>` (echoed like `output`; after its frames and an optional sun_map the CLI writes the whole map's sky-view
 * map as a one-component PNG: hmrm_cell_map_sum in status mode over hmrm_sky_directions(r, n), K = r * n, with
 * shadow_step_dist, shadow_max_steps, sun_map_lift and the camera's sampling; byte = (c * 255 + K / 2) / K for count c),
 * `sky_map_rings r n` (default 4 16; a product outside 1 .. 256 warns "WARNING: sky_map_rings must give 1..256 directions" and
 * keeps the old value),
 * `sky_light on|off|1|0` (default off; the CLI renders its single frame with hmrm_render_lit_sum over those same directions --
 * shadow rays always on, HMRM_SHADE_DIFFUSE with `shading on`, shadow_ambient, shadow_step_dist, shadow_max_steps and interior
 * as for `shadows`, sun_dir not used; ignored, with a warning, with `antialias n` > 1, `devices n` > 1 or `record orbit`,
 * whatever sun_scope says; another value warns "WARNING: Unknown sky_light: v" and keeps the old one),
 * `baked_light off|sun|sky` (default off; before its frames the CLI bakes the scene's light plane once with
 * hmrm_scene_bake_light -- sun: one target, sun_dir, with exactly the flags, sun_map_lift, shadow_ambient, shadow_step_dist,
 * shadow_max_steps and sampling of `sun_map`; sky: status mode over hmrm_sky_directions(sky_map_rings), as `sky_map` -- prints
 * "baked light: K direction(s), full scale D", and renders the single frame, the `antialias n` frame and `record orbit` as
 * baked frames, hmrm_render_baked / hmrm_record_orbit_baked, with HMRM_TRACE_INTERIOR for `interior on`; `shadows` and
 * `shading` then only choose what is baked; `sky_light on` is ignored with "WARNING: sky_light is ignored with baked_light";
 * `devices n` > 1 ignores the key with "WARNING: baked_light is ignored with devices > 1"; another value warns "WARNING:
 * Unknown baked_light: v" and keeps the old one),
 * `water on|off|1|0` (default off; the CLI renders its single frame with hmrm_render_water under hmrm_config_get_water's water;
 * ignored, with "WARNING: water is ignored with <what>", beside `antialias n` > 1, `devices n` > 1, `record orbit`, `shadows`,
 * `shading` and `baked_light`; `sky_light on` beside it is ignored with "WARNING: sky_light is ignored with water"; another value
 * warns "WARNING: Unknown water: v" and keeps the old one), `water_level v`, `water_reflectivity n` (default 128; outside 0..255:
 * "WARNING: water_reflectivity must be 0..255", the old value stays), `water_color r g b` (sets HMRM_WATER_OWN_COLOR; a component
 * outside 0..255: "WARNING: water_color must be three values 0..255"), `water_step_dist v` (absent: step_dist),
 * `water_max_steps n` (default 0 = none; outside 0..4294967295: "WARNING: water_max_steps must be 0..4294967295"),
 * `water_scope frame|all` (default frame: everything above; with `all`, `water on` goes through `antialias n`
 * (hmrm_render_water_aa) and `record orbit` (hmrm_record_orbit_water), and `baked_light sun|sky` bakes as described and then
 * renders those with HMRM_WATER_BAKED; beside `devices n` > 1, `shadows` and `shading` without `baked_light`, and `sky_light` the
 * key is still ignored with its warnings; another value warns "WARNING: Unknown water_scope: v" and keeps the old one),
 * `range_map <path.pfm>` (echoed like `output`; after its frames and before an optional sun_map the CLI writes the range plane
 * of the configured camera -- hmrm_render_geometry with that plane alone, under the interior rule with `interior on` -- as a
 * one-component portable float map, hmrm_write_pfm),
 * `haze on|off|1|0` (default off; the CLI renders its single frame with hmrm_render_haze under hmrm_config_get_haze's haze and
 * table, with `antialias n` for the factor and HMRM_TRACE_INTERIOR for `interior on`; ignored, with "WARNING: haze is ignored with
 * <what>", beside `shadows`, `shading`, `water`, `baked_light`, `sky_light`, `record orbit` and `devices n` > 1; another value
 * warns "WARNING: Unknown haze: v" and keeps the old one), `haze_start v` (default 0), `haze_far v` (default 1000: scale = n / (far - start)),
 * `haze_law linear|exp|exp2` (default exp; another value warns "WARNING: Unknown haze_law: v"), `haze_density v` (default 3),
 * `haze_color r g b` (default 200 210 220; a component outside 0..255: "WARNING: haze_color must be three values 0..255"),
 * `haze_sky on|off|1|0` (default off: HMRM_HAZE_SKY; another value warns "WARNING: Unknown haze_sky: v"), `haze_entries n`
 * (default 256; outside 1..4096: "WARNING: haze_entries must be 1..4096", the old value stays),
 * `view x y z hang vang` (repeatable, at most 64 lines: one more camera of the CLI's view batch, hmrm_render_views -- position and
 * the two angles, in the unit the `hang` and `vang` keys take; everything else comes from the main camera as it stands when the
 * views are asked for; echoed like `pos` and the angles; a 65th line warns "WARNING: too many views" and is dropped),
 * `views_output <prefix>` (echoed like `output`; with at least one `view` the CLI renders the views with ONE hmrm_render_views call
 * after its frames, HMRM_TRACE_INTERIOR for `interior on`, and writes <prefix>000.png, <prefix>001.png, ...; one key without the
 * other warns "WARNING: view is ignored without views_output" / "WARNING: views_output is ignored without a view").
 * Unknown key -> "WARNING: Unknown identifier: k". */
hmrm_config *hmrm_config_create(void);
void         hmrm_config_destroy(hmrm_config *cfg);
/* Consume a whole stream; loads heightmap/colormap images when those keys
 * appear; runs the end-of-stream validation (maps present, equal dimensions). */
int          hmrm_config_consume_file(hmrm_config *cfg, const char *path);
int          hmrm_config_consume_string(hmrm_config *cfg, const char *text);
const char  *hmrm_config_log(const hmrm_config *cfg);      /* stdout echo so far   */
const char  *hmrm_config_warnings(const hmrm_config *cfg); /* stderr text so far   */
void         hmrm_config_get_camera(const hmrm_config *cfg, hmrm_camera *out);
void         hmrm_config_get_scene_params(const hmrm_config *cfg, hmrm_scene_params *out);
int32_t      hmrm_config_cycle(const hmrm_config *cfg);
int32_t      hmrm_config_recording_frame_count(const hmrm_config *cfg);
const char  *hmrm_config_heightmap_path(const hmrm_config *cfg);
const char  *hmrm_config_colormap_path(const hmrm_config *cfg);
const char  *hmrm_config_output_path(const hmrm_config *cfg);
int32_t      hmrm_config_record_mode(const hmrm_config *cfg);   /* additive `record orbit|off`: 1|0 */
int32_t      hmrm_config_devices(const hmrm_config *cfg);       /* additive `devices n`: GPUs for recording, 0 = all */
int32_t      hmrm_config_antialias(const hmrm_config *cfg);     /* additive `antialias n`: 1 (default, off), 2, 4 or 8 */
int32_t      hmrm_config_interior(const hmrm_config *cfg);      /* additive `interior on|off`: 1|0 */
int32_t      hmrm_config_shadows(const hmrm_config *cfg);       /* additive `shadows on|off`: 1|0 */
int32_t      hmrm_config_shading(const hmrm_config *cfg);       /* additive `shading on|off`: 1|0 */
int32_t      hmrm_config_sky_light(const hmrm_config *cfg);     /* additive `sky_light on|off`: 1|0 */
int32_t      hmrm_config_baked_light(const hmrm_config *cfg);   /* additive `baked_light off|sun|sky`: 0|1|2 */
int32_t      hmrm_config_sun_scope(const hmrm_config *cfg);     /* additive `sun_scope single|all`: 0|1 */
const char  *hmrm_config_sun_map_path(const hmrm_config *cfg);  /* additive `sun_map <path.png>`: "" = none */
double       hmrm_config_sun_map_lift(const hmrm_config *cfg);  /* additive `sun_map_lift v` */
const char  *hmrm_config_sky_map_path(const hmrm_config *cfg);  /* additive `sky_map <path.png>`: "" = none */
void         hmrm_config_sky_map_rings(const hmrm_config *cfg, int32_t *rings, int32_t *per_ring); /* additive `sky_map_rings r n` */
const char  *hmrm_config_range_map_path(const hmrm_config *cfg); /* additive `range_map <path.pfm>`: "" = none */
/* The sun of the additive keys: sun_dir, shadow_step_dist (the config's step_dist when the key was absent),
 * shadow_max_steps, shadow_ambient; flags = HMRM_TRACE_INTERIOR when `interior on`. */
void         hmrm_config_get_sun(const hmrm_config *cfg, hmrm_sun *out);
int32_t      hmrm_config_water(const hmrm_config *cfg);         /* additive `water on|off`: 1|0 */
/* The water of the additive keys: water_level (default 0), water_step_dist (the config's step_dist when the key was absent),
 * water_max_steps (default 0 = none; a value outside 0..4294967295 is warned about and ignored), water_reflectivity (default 128;
 * outside 0..255 likewise), water_color r g b (sets HMRM_WATER_OWN_COLOR; a component outside 0..255 likewise);
 * flags |= HMRM_TRACE_INTERIOR when `interior on`.  `hmap` renders its single frame with hmrm_render_water when `water on`; the key
 * is ignored, with a warning, beside `antialias` > 1, `devices` > 1, `record orbit`, `shadows`, `shading` and `baked_light`
 * (`water_scope all` and `water_light sun`, below, lift some of these). */
void         hmrm_config_get_water(const hmrm_config *cfg, hmrm_water *out);
int32_t      hmrm_config_water_scope(const hmrm_config *cfg);   /* additive `water_scope frame|all`: 0|1 */
/* Additive `water_light off|sun` (default off; another value warns "WARNING: Unknown water_light: v" and keeps the old one): 0|1.
 * With `sun`, `hmap` renders `water on` beside `shadows on` and / or `shading on` with hmrm_render_water_lit -- the sun and the
 * shade flags the shaded single frame would get -- when there is no `baked_light`, one device and `antialias 1`, under either
 * `water_scope`; beside `antialias` > 1, `devices` > 1, `record orbit` or `baked_light` the existing warnings stand.  With `off`
 * nothing changes. */
int32_t      hmrm_config_water_light(const hmrm_config *cfg);
int32_t      hmrm_config_haze(const hmrm_config *cfg);          /* additive `haze on|off`: 1|0 */
/* The haze of the additive keys: start = haze_start, scale = haze_entries / (haze_far - haze_start) in doubles, n = haze_entries,
 * color = haze_color, flags = HMRM_HAZE_SKY for `haze_sky on` | HMRM_TRACE_INTERIOR for `interior on`; and, when `table` is not
 * NULL, its n bytes (room for 4096 always suffices): hmrm_haze_table(haze_law, haze_density, n).  `out` may be NULL. */
void         hmrm_config_get_haze(const hmrm_config *cfg, hmrm_haze *out, uint8_t *table);
int32_t      hmrm_config_haze_law(const hmrm_config *cfg);      /* additive `haze_law linear|exp|exp2`: HMRM_HAZE_* */
double       hmrm_config_haze_density(const hmrm_config *cfg);  /* additive `haze_density v` */
double       hmrm_config_haze_far(const hmrm_config *cfg);      /* additive `haze_far v` */
int32_t      hmrm_config_view_count(const hmrm_config *cfg);    /* additive `view x y z hang vang`: lines kept, 0 .. 64 */
/* The cameras of those lines, hmrm_config_view_count of them: hmrm_config_get_camera's camera with the line's pos, hang and vang. */
void         hmrm_config_get_views(const hmrm_config *cfg, hmrm_camera *out);
const char  *hmrm_config_views_output(const hmrm_config *cfg);  /* additive `views_output <prefix>`: "" = none */
/* Loaded maps (owned by cfg): RGB8 / RGBA8; NULL until the key was consumed. */
const uint8_t *hmrm_config_height_rgb(const hmrm_config *cfg, int32_t *w, int32_t *h);
const uint8_t *hmrm_config_color_rgba(const hmrm_config *cfg, int32_t *w, int32_t *h);
/* 1 if heights need recomputing since the last call (should_update_heightmap). */
int          hmrm_config_take_heightmap_dirty(hmrm_config *cfg);
/* Scene from the loaded maps + params (= hmrm_scene_create on the above). */
int          hmrm_config_create_scene(const hmrm_config *cfg, hmrm_scene **out);

/* ----------------------------------------------------------------- image IO */
/* Replaces stbi_load(path,&w,&h,&n,req_comp) (hmap.cpp:320-321,341-342) for the formats decoded
 * natively: PNG (all colour types / bit depths, interlaced too), JPEG (baseline, extended and
 * progressive Huffman, 8-bit; grey, YCbCr, RGB, CMYK/YCCK), BMP (1/4/8-bit palette, 16/24/32-bit,
 * bit fields), TGA (types 1/2/3/9/10/11) and binary PNM (P5/P6).  Pixels equal stb_image v2.27's
 * for every req_comp (16-bit -> 8 by >>8; grey -> RGB replicate; missing alpha = 255).  The other
 * formats the reference's stb reads (README.md:75) are decoded too, with stb's pixels: GIF (first frame),
 * PSD (8/16-bit RGB, raw or RLE), Softimage PIC and Radiance HDR (stb's float -> 8-bit tone curve).
 * *out is malloc'ed; free with hmrm_image_free. */
int  hmrm_image_load(const char *path, int32_t req_comp,
                     uint8_t **out, int32_t *w, int32_t *h, int32_t *comp_in_file);
int  hmrm_image_load_memory(const uint8_t *bytes, size_t len, int32_t req_comp,
                            uint8_t **out, int32_t *w, int32_t *h, int32_t *comp_in_file);
void hmrm_image_free(void *p);
/* Replaces SavePNG / stbi_write_png(path,w,h,comp,data,stride)
 * (hmap.cpp:157-160): same filter choice and the same deflate as
 * stb_image_write v1.16, so equal pixels give equal files. */
int  hmrm_write_png(const char *path, int32_t w, int32_t h, int32_t comp,
                    const uint8_t *data, size_t stride_bytes);
int  hmrm_write_png_memory(int32_t w, int32_t h, int32_t comp, const uint8_t *data,
                           size_t stride_bytes, uint8_t **out, size_t *out_len);
/* Binary PPM (P6), alpha dropped -- build-side addition named by north_star. */
int  hmrm_write_ppm(const char *path, int32_t w, int32_t h, int32_t comp,
                    const uint8_t *data, size_t stride_bytes);
/* Portable float map (build-side addition, for the float planes of hmrm_render_geometry): header "Pf" (comp 1) or "PF"
 * (comp 3), "w h", the scale "-1.0" (negative: little-endian), then the rows BOTTOM TO TOP, w * comp IEEE floats each, bit
 * for bit (+inf included).  HMRM_E_ARG for a NULL argument, a size below 1, another comp or a stride below one row. */
int  hmrm_write_pfm(const char *path, int32_t w, int32_t h, int32_t comp /* 1 or 3 */,
                    const float *data, size_t stride_bytes);

#ifdef __cplusplus
}
#endif
#endif /* HMRM_H */
