// api_launch.cpp -- the frame launch path behind the entry points of api_frames.cpp: the per-frame host set-up with its cached
// records, the launch-order calibration and the kernel probe (the HIP side of launch_order.hpp), and the kernel launch.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "api_internal.hpp"
#include "host_pool.hpp"

// cached records and settled launch orders are looked up with memcmp on these two: no padding bytes allowed
static_assert(sizeof(hmrm_sun) == 48, "hmrm_sun has padding");
static_assert(sizeof(hmrm_camera) == 3 * sizeof(int32_t) + 4 + 8 * sizeof(double), "hmrm_camera has padding");
static_assert(sizeof(hmrm_scene_params) == 6 * sizeof(double), "hmrm_scene_params has padding");
static_assert(HMRM_SHADE_DIFFUSE == hmrm::kShadeDiffuse && HMRM_SHADE_NO_SHADOWS == hmrm::kShadeNoShadows, "route_frame's flag bits");

namespace {

// The calibration records of a context: the device buffer of the ONE measured launch it has in flight at a time and, per
// cached record, kMaxMeasRows x {start, longest wave} in pinned memory (allocated with the first measured launch).
int ensure_meas(StreamCtx *c) {
	if (!c->d_meas) HIP_TRY(hipMalloc((void **)&c->d_meas, (size_t)kMaxMeasRows * hmrm::kMeasureStride * sizeof(unsigned long long)));
	if (!c->h_meas) {
		const size_t n = (size_t)kFrameSlots * 2 * kMaxMeasRows * sizeof(unsigned long long);
		HIP_TRY(hipHostMalloc((void **)&c->h_meas, n, hipHostMallocMapped));
		HIP_TRY(hipHostGetDevicePointer((void **)&c->h_meas_dev, c->h_meas, 0));
	}
	return HMRM_OK;
}

// ---- measured launches: the HIP side of launch_order.hpp's calibration ----
// Is nothing of the scene running on another of its own streams?  (A measured launch wants the chip to itself.)
// The scene owns those streams, so it asks them directly: nothing has to be recorded behind a frame for this.
bool others_idle(hmrm_scene *s, StreamCtx *c) {
	for (StreamCtx *o : s->ctxs) {
		if (o == c || !o->scene_owned) continue;
		const hipError_t e = hipStreamQuery(o->stream);
		if (e == hipSuccess) continue;
		if (e == hipErrorNotReady) (void)hipGetLastError(); // (busy is no error: not left behind for the caller's next check)
		return false;
	}
	return true;
}

int raise_measure_fence(hmrm_scene *s, StreamCtx *c) {
	if (!s->measure_fence) HIP_TRY(hipEventCreateWithFlags(&s->measure_fence, hipEventDisableTiming));
	HIP_TRY(hipEventRecord(s->measure_fence, c->stream));
	s->measure_fence_ctx = c;
	return HMRM_OK;
}

// A finished measured launch of this record is folded into its calibration; a calibration that settles is published.
void poll_measured(hmrm_scene *s, StreamCtx *c, FrameSlot *slot, int tiles_y, int rot) {
	if (slot->cal.in_flight >= 0 && slot->meas_rows == tiles_y && hipEventQuery(slot->measured) == hipSuccess) {
		const int trial = slot->cal.in_flight;
		const unsigned long long *h_rec = c->h_meas + (size_t)(slot - c->slots) * 2 * kMaxMeasRows;
		const bool settled = slot->cal.on_measured(h_rec, tiles_y, rot, s->knobs.kernel == 0 && s->knobs.try_group, s->choice);
		if (s->knobs.order_verbose) {
			const hmrm::OrderTrial &t = slot->cal.trials[trial];
			fprintf(stderr, "hmrm order: trial %d of %d tile rows measured, makespan %.1f us:", trial, tiles_y, t.makespan / 100.0);
			for (int k = 0; k < t.n; ++k) fprintf(stderr, " [%d,%d)", t.b[k], t.b[k] + t.c[k]);
			fprintf(stderr, "%s\n", t.group ? " plain groups, rotation" : (t.n ? "" : " rotation"));
			if (settled) fprintf(stderr, "hmrm order: settled on trial %d\n", slot->cal.best);
		}
		if (settled) {
			if (s->settled.size() >= 256) s->settled.erase(s->settled.begin());
			s->settled.push_back(hmrm_scene::SettledOrder{slot->cam, slot->params, slot->thr_max_bits, slot->cal.trials[slot->cal.best]});
		}
	}
	// (one measured launch per context at a time: they share the device records)
	if (c->meas_owner && (c->meas_owner->cal.in_flight < 0 || hipEventQuery(c->meas_owner->measured) == hipSuccess)) c->meas_owner = nullptr;
}

// The verdict of a shadow probe in flight, once both of its launches have finished.
void poll_shadow_probe(hmrm_scene *s) {
	if (!s->probe_pending || hipEventQuery(s->probe_done) != hipSuccess) return;
	s->probe_pending = false;
	if (s->probe_ctx) s->probe_ctx->probe_in_flight = false;
	if (s->probe_epoch_launched != s->probe_epoch) return; // (the heights or the knobs changed meanwhile)
	hmrm::fold_shadow_probe(s->choice, s->h_probe, s->h_probe + 2 * kMaxMeasRows, s->probe_rows);
	if (s->knobs.order_verbose)
		fprintf(stderr, "hmrm probe: production kernel %.1f us, the other kernel %.1f us -> %s\n", hmrm::measured_makespan(s->h_probe, s->probe_rows) / 100.0,
		        hmrm::measured_makespan(s->h_probe + 2 * kMaxMeasRows, s->probe_rows) / 100.0, s->choice.use_group ? (s->choice.with_records ? "groups + window records" : "plain groups") : "production kernel");
}

// The launch of `req` on the context's stream, for the plain family (launch_kernel sets another).
hmrm::FrameLaunch frame_launch(const hmrm_scene *s, const StreamCtx *c, const hmrm::DevFrame &f, const hmrm::RowMap &rows, const FrameRequest &req) {
	return hmrm::FrameLaunch{s->d_thr, s->d_thr32, s->d_cmap, s->d_records, req.d_out, req.out_stride_px, c->d_counters, req.d_steps,
	                         req.d_entry, req.stats, f, rows, hmrm::kFramePlain, hmrm::SunRules{}, false, hmrm::GeomPlanes{}, c->stream};
}

// The shadow probe: this frame twice into the same buffer -- production kernel, then the other kernel (launch_kernel: the
// plain groups, with window records for nearest-sampling frames); same pixels, the
// second launch's capped rays counted apart -- both measured like a calibration launch.
int launch_shadow_probe(hmrm_scene *s, StreamCtx *c, const hmrm::DevFrame &f, const hmrm::RowMap &rows_in_order, int tiles_y,
                        const FrameRequest &req) {
	if (!s->h_probe) {
		HIP_TRY(hipHostMalloc((void **)&s->h_probe, (size_t)4 * kMaxMeasRows * sizeof(unsigned long long), hipHostMallocMapped));
		HIP_TRY(hipHostGetDevicePointer((void **)&s->h_probe_dev, s->h_probe, 0));
		HIP_TRY(hipEventCreateWithFlags(&s->probe_done, hipEventDisableTiming));
	}
	const int rc_m = ensure_meas(c);
	if (rc_m) return rc_m;
	hmrm::RowMap measured = rows_in_order;
	measured.measure = c->d_meas;
	const bool records_ok = f.sampling == 0 && s->d_records; // (the other kernel of this frame: launch_kernel)
	s->choice.with_records = records_ok;
	if (records_ok) {
		const int rc_r = ensure_records(s);
		if (rc_r) return rc_r;
	}
	hmrm::FrameLaunch l = frame_launch(s, c, f, measured, req); // (a frame that may probe: the plain family, no per-pixel outputs)
	for (int pass = 0; pass < 2; ++pass) {
		HIP_TRY(hmrm::launch_measure_init(measured.measure, tiles_y, c->stream));
		l.d_counters = c->d_counters + (pass ? 8 : 0);
		HIP_TRY(hmrm::launch_frame_march(l, pass == 0 ? hmrm::kLeaps : (records_ok ? hmrm::kRecords : hmrm::kPlainGroups)));
		HIP_TRY(hmrm::launch_measure_readback(measured.measure, s->h_probe_dev + (size_t)pass * 2 * kMaxMeasRows, tiles_y, c->stream));
	}
	HIP_TRY(hipEventRecord(s->probe_done, c->stream));
	s->probe_pending = true;
	s->choice.probed = true;
	s->probe_rows = tiles_y;
	s->probe_epoch_launched = s->probe_epoch;
	s->probe_ctx = c;
	c->probe_in_flight = true;
	return raise_measure_fence(s, c);
}

// The render kernel itself (march_dispatch.hpp route_frame): the literal loop, else the production kernel or the other one (the
// plain groups, with leaps over window records where the frame's sampling allows them), of the family the request asks for:
// hmrm_render's, the kernels built with the interior rule, or the ones that march the shadow rays or shade too.
int launch_kernel(hmrm_scene *s, StreamCtx *c, const hmrm::DevFrame &f, const hmrm::RowMap &rows_in_order, const FrameRequest &req,
                  bool use_group) {
	const bool huge_side = s->map_w >= (1 << 24) || s->map_h >= (1 << 24);
	const LitFrame *lit = req.lit;
	const hmrm::FrameRoute route = hmrm::route_frame(s->knobs.kernel, huge_side, f.sampling, f.aa_shift != 0, req.interior == Interior::kByKernels,
	                                                 lit != nullptr, lit ? lit->shade_flags : 0u, lit && lit->sum);
	if (route.refused) return fail(HMRM_E_ARG, "maps with a side of 2^24 cells or more support nearest sampling only");
	hmrm::FrameLaunch l = frame_launch(s, c, f, rows_in_order, req);
	l.family = route.family;
	if (lit) {
		l.sun = lit->sun;
		if (route.ambient_sun) l.sun.ambient = 255u;
		l.primary_interior = lit->primary_interior;
		if (lit->sum) l.lsum = *lit->sum;
	}
	if (req.geom) { // (the literal-or-march decision is the plain frame's: route_frame knows no geometry family)
		l.family = hmrm::kFrameGeometry;
		l.geo = *req.geom;
		l.primary_interior = req.interior != Interior::kNot;
	}
	if (req.baked) { // (likewise)
		l.family = hmrm::kFrameBaked;
		l.baked = *req.baked;
		l.primary_interior = req.interior != Interior::kNot;
	}
	if (req.water) { // (likewise; with the light plane and / or a factor: one of the water family's three other kinds)
		const bool aa = f.aa_shift != 0;
		if (req.baked) l.family = aa ? hmrm::kFrameWaterBakedAA : hmrm::kFrameWaterBaked;
		else l.family = aa ? hmrm::kFrameWaterAA : hmrm::kFrameWater;
		l.water = *req.water;
		l.primary_interior = req.interior != Interior::kNot;
		if (req.water_sun) { // (the sun-lit water frame: neither a factor nor the plane reaches here with it)
			l.family = hmrm::kFrameWaterLit;
			l.sun = *req.water_sun;
		}
	}
	if (req.haze) { // (likewise; a factor picks the family's antialiased kernels in its launchers)
		l.family = hmrm::kFrameHaze;
		l.haze = *req.haze;
		l.primary_interior = req.interior != Interior::kNot;
	}
	if (route.literal) {
		HIP_TRY(hmrm::launch_frame_literal(l));
		return HMRM_OK;
	}
	// (the records bound the nearest cell's double thresholds: launch_order.hpp pick_fast_kernel)
	const hmrm::FastKernel k = (hmrm::FastKernel)hmrm::pick_fast_kernel(s->knobs.kernel, use_group, f.sampling == 0 && s->d_records, s->choice);
	if (k == hmrm::kRecords) {
		const int rc_r = ensure_records(s);
		if (rc_r) return rc_r;
	}
	HIP_TRY(hmrm::launch_frame_march(l, k));
	return HMRM_OK;
}

// The kernel launch -- bracketed, when it is a measured one, by the set-up of the records in front of it and their read-back,
// the record's event and the scene's fence behind it.
int launch_maybe_measured(hmrm_scene *s, StreamCtx *c, const hmrm::DevFrame &f, FrameSlot *slot, hmrm::RowMap &rows_in_order, int tiles_y,
                          bool measure_now, const FrameRequest &req, bool use_group) {
	if (measure_now) {
		const int rc_m = ensure_meas(c);
		if (rc_m) return rc_m;
		if (!slot->measured) HIP_TRY(hipEventCreateWithFlags(&slot->measured, hipEventDisableTiming));
		rows_in_order.measure = c->d_meas;
		HIP_TRY(hmrm::launch_measure_init(rows_in_order.measure, tiles_y, c->stream));
	}
	const int rc_k = launch_kernel(s, c, f, rows_in_order, req, use_group);
	if (rc_k || !measure_now) return rc_k;
	const size_t idx = (size_t)(slot - c->slots);
	HIP_TRY(hmrm::launch_measure_readback(rows_in_order.measure, c->h_meas_dev + idx * 2 * kMaxMeasRows, tiles_y, c->stream));
	HIP_TRY(hipEventRecord(slot->measured, c->stream));
	slot->meas_rows = tiles_y;
	c->meas_owner = slot;
	return raise_measure_fence(s, c);
}

} // namespace

namespace hmrm {

int check_camera(const hmrm_camera *cam) {
	if (!cam) return fail(HMRM_E_ARG, "camera is NULL");
	if (cam->width <= 0 || cam->height <= 0) return fail(HMRM_E_ARG, "resolution must be positive");
	if ((int64_t)cam->width * cam->height > ((int64_t)1 << 31) / 4)
		return fail(HMRM_E_ARG, "resolution too large (the reference indexes the framebuffer with int)");
	if (cam->projection < 1 || cam->projection > 3) return fail(HMRM_E_ARG, "projection must be 1, 2 or 3");
	if (cam->sampling > HMRM_NEAREST_F32) return fail(HMRM_E_ARG, "sampling must be 0 (nearest), 1 (bilinear) or 2 (nearest, float heights)");
	return HMRM_OK;
}

void to_host_camera(const hmrm_camera *cam, hmrm::HostCamera *hc) {
	*hc = hmrm::HostCamera{};
	hc->width = cam->width;
	hc->height = cam->height;
	hc->projection = cam->projection;
	hc->bg_r = cam->bg_r;
	hc->bg_g = cam->bg_g;
	hc->bg_b = cam->bg_b;
	hc->sampling = cam->sampling;
	hc->hfov = cam->hfov;
	hc->hang = cam->hang;
	hc->vang = cam->vang;
	hc->pos[0] = cam->pos[0];
	hc->pos[1] = cam->pos[1];
	hc->pos[2] = cam->pos[2];
	hc->ortho_width = cam->ortho_width;
	hc->step_dist = cam->step_dist;
}

// Host set-up for one frame (the reference rebuilds its ImagePlane every frame, hmap.cpp:952-965;
// same values): finds the stream's cached record for this camera or builds it into the least
// recently used slot; for spherical cameras the table upload is enqueued on the launch stream, in
// front of the kernel that reads it.  *slot_out stays valid until the next call on this context.
int prepare_frame(hmrm_scene *s, StreamCtx *c, const hmrm_camera *cam, hmrm::DevFrame *f, FrameSlot **slot_out) {
	const uint64_t thr_bits = *(const uint64_t *)&s->thr_max;
	FrameSlot *slot = nullptr;
	for (FrameSlot &sl : c->slots)
		if (sl.valid && memcmp(&sl.cam, cam, sizeof *cam) == 0 && memcmp(&sl.params, &s->params, sizeof s->params) == 0 &&
		    sl.thr_max_bits == thr_bits)
			slot = &sl;
	if (!slot) {
		slot = &c->slots[0];
		for (FrameSlot &sl : c->slots)
			if (!sl.valid || sl.stamp < slot->stamp) {
				slot = &sl;
				if (!sl.valid) break;
			}
		slot->valid = false;
		if (slot->cal.in_flight >= 0) HIP_TRY(hipEventSynchronize(slot->measured)); // (its records are about to be reused)
		slot->cal.reset();
		hmrm::HostCamera hc;
		to_host_camera(cam, &hc);
		double *cc = nullptr, *cs = nullptr, *rs = nullptr, *rc = nullptr;
		const size_t W = (size_t)cam->width, H = (size_t)cam->height;
		if (cam->projection == HMRM_SPHERICAL) {
			const size_t n = 2 * W + 2 * H;
			if (n > c->arena_n) {
				// (kernels of this stream may still read the old tables; every cached spherical record of the context
				// loses its tables with the old arena)
				HIP_TRY(hipStreamSynchronize(c->stream));
				if (c->d_arena) (void)hipFree(c->d_arena);
				if (c->h_arena) (void)hipHostFree(c->h_arena);
				c->d_arena = c->h_arena = nullptr;
				c->arena_n = 0;
				for (FrameSlot &sl : c->slots) {
					if (sl.cam.projection == HMRM_SPHERICAL) sl.valid = false;
					sl.d_tables = sl.h_tables = nullptr;
				}
				const size_t per = (n + 31) & ~(size_t)31; // (slots start on 256-byte boundaries)
				HIP_TRY(hipMalloc((void **)&c->d_arena, per * kFrameSlots * sizeof(double)));
				HIP_TRY(hipHostMalloc((void **)&c->h_arena, per * kFrameSlots * sizeof(double), hipHostMallocMapped));
				HIP_TRY(hipHostGetDevicePointer((void **)&c->h_arena_dev, c->h_arena, 0));
				c->arena_n = per;
			}
			const size_t idx = (size_t)(slot - c->slots);
			slot->d_tables = c->d_arena + idx * c->arena_n;
			slot->h_tables = c->h_arena + idx * c->arena_n;
			if (!slot->uploaded) HIP_TRY(hipEventCreateWithFlags(&slot->uploaded, hipEventDisableTiming));
			else HIP_TRY(hipEventSynchronize(slot->uploaded)); // the previous upload out of h_tables is done
			cc = slot->h_tables;
			cs = cc + W;
			rs = cs + W;
			rc = rs + H;
		}
		hmrm::DevFrame &fr = slot->frame;
		hmrm::build_frame(hc, s->map_w, s->map_h, s->params.min_height, s->params.max_height, s->params.grid_width,
		                  &fr, nullptr, nullptr, nullptr, nullptr);
		if (cam->projection == HMRM_SPHERICAL) {
			// A moving camera seldom changes everything: the row tables (sin / cos of va) depend on vang, hfov and
			// the resolution only -- they survive any orbit or translation -- and the column tables on hang, hfov
			// and the width.  A half some cached record of this stream already holds is copied from its staging
			// memory; what is left is filled by the host pool (glibc sin / cos, ~15 ns per call: 12 000 calls for
			// a fresh 4K camera would otherwise cost more host time than the kernel takes on the GPU).
			const FrameSlot *row_donor = nullptr, *col_donor = nullptr;
			for (const FrameSlot &o : c->slots) {
				if (!o.valid || &o == slot || o.cam.projection != HMRM_SPHERICAL || !o.h_tables) continue;
				if (o.cam.width != cam->width || o.cam.hfov != cam->hfov) continue;
				if (!col_donor && o.cam.hang == cam->hang) col_donor = &o;
				if (!row_donor && o.cam.height == cam->height && o.cam.vang == cam->vang) row_donor = &o;
			}
			if (col_donor) memcpy(cc, col_donor->h_tables, 2 * W * sizeof(double));
			if (row_donor) memcpy(rs, row_donor->h_tables + 2 * (size_t)row_donor->cam.width, 2 * H * sizeof(double));
			const int nc = col_donor ? 0 : cam->width, nr = row_donor ? 0 : cam->height;
			if (nc + nr > 0)
				hmrm::parallel_ranges(nc + nr, 1024, [&](int b, int e) {
					// items [0, nc) are columns, [nc, nc + nr) rows
					if (b < nc) hmrm::fill_col_tables(hc, b, std::min(e, nc), cc, cs);
					if (e > nc) hmrm::fill_row_tables(hc, std::max(b, nc) - nc, e - nc, rs, rc);
				});
		}
		slot->row_cost.assign(((size_t)cam->height + kCostRows - 1) / kCostRows, 0.0f);
		hmrm::estimate_row_costs(fr, cc, cs, rs, rc, kCostRows, slot->row_cost.data());
		if (cam->projection == HMRM_SPHERICAL) {
			// stream order puts the upload (a small kernel reading the pinned staging memory) behind every earlier
			// kernel of this stream that read the slot's device tables and in front of the one about to be launched
			HIP_TRY(hmrm::launch_upload_tables(c->h_arena_dev + (slot->h_tables - c->h_arena), slot->d_tables, 2 * W + 2 * H, c->stream));
			HIP_TRY(hipEventRecord(slot->uploaded, c->stream));
			fr.col_cos_ha = slot->d_tables;
			fr.col_sin_ha = slot->d_tables + W;
			fr.row_sin_va = slot->d_tables + 2 * W;
			fr.row_cos_va = slot->d_tables + 2 * W + H;
		}
		if (cam->sampling == HMRM_BILINEAR) {
			const int rc2 = ensure_bilinear_pyramid(s);
			if (rc2 != HMRM_OK) return rc2;
		}
		finish_frame_record(s, cam->sampling, &fr);
		slot->cam = *cam;
		slot->params = s->params;
		slot->thr_max_bits = thr_bits;
		slot->valid = true;
		for (size_t k = s->settled.size(); k-- > 0;) { // (newest first)
			const hmrm_scene::SettledOrder &so = s->settled[k];
			if (memcmp(&so.cam, cam, sizeof *cam) != 0 || memcmp(&so.params, &s->params, sizeof s->params) != 0 || so.thr_max_bits != thr_bits) continue;
			slot->cal.adopt(so.order);
			break;
		}
	}
	slot->stamp = ++s->clock;
	*f = slot->frame;
	apply_scene_knobs(s, f);
	if (slot_out) *slot_out = slot;
	return HMRM_OK;
}

// What a frame record takes from the scene once build_frame (camera.cpp) has made it from the camera: the part of the cached
// record that is the scene's.  (A bilinear record's pyramid exists: ensure_bilinear_pyramid is its caller's matter.)
void finish_frame_record(const hmrm_scene *s, int sampling, hmrm::DevFrame *fr) {
	// (informational: the kernel reads the whole-map bound from the pyramid's top plane, rounded up to
	// float like every window maximum -- which also bounds the float copy of a threshold)
	fr->thr_max = sampling == HMRM_BILINEAR ? s->thr_max_bil : s->thr_max;
	// the finest level whose windows have at least min_window cells (camera.cpp's hint)
	fr->min_level = 0;
	while (fr->min_level < hmrm::kMipLevels - 1 && hmrm::win_cells(fr->min_level) < fr->min_window)
		++fr->min_level;
	fr->mipbuf = s->d_mipbuf;
	fr->mipbuf_bil = s->d_mipbuf_bil;
	fr->mip_row = s->mip_row;
	fr->mip_plane_shift = s->mip_plane_shift;
}

// ... and the per-scene settings, which are not part of the cached record.
void apply_scene_knobs(const hmrm_scene *s, hmrm::DevFrame *f) {
	f->step_cap = s->knobs.step_cap;
	f->diag_mode = s->knobs.diag_mode;
	if (s->knobs.min_level >= 0) f->min_level = s->knobs.min_level;
	if (s->knobs.finest_pause >= 0) f->finest_pause = s->knobs.finest_pause;
}

// ---- view batches (hmrm_render_views): the launch path of api_frames.cpp render_views_common ----
// Which kernel renders a batch: the literal loop (HMRM_KERNEL=simple, a huge side) or a march kernel of the scene's standing
// verdict, as a frame with kernels of its own gets it (launch_frame): never a probe, never a measured launch, and behind the
// scene's measure fence like every launch.  Decided before the records are built: the record kernel finds its table in them.
int pick_views_kernel(hmrm_scene *s, StreamCtx *c, int sampling, ViewsKernel *out) {
	const bool huge_side = s->map_w >= (1 << 24) || s->map_h >= (1 << 24);
	const hmrm::FrameRoute route = hmrm::route_frame(s->knobs.kernel, huge_side, sampling, false, true, false, 0u);
	if (route.refused) return fail(HMRM_E_ARG, "maps with a side of 2^24 cells or more support nearest sampling only");
	int rc = wait_for_measure_fence(s, c);
	if (rc) return rc;
	poll_shadow_probe(s);
	const bool use_group = s->knobs.kernel == 0 && s->knobs.try_group && s->choice.use_group;
	out->literal = route.literal;
	out->kind = (hmrm::FastKernel)hmrm::pick_fast_kernel(s->knobs.kernel, use_group, sampling == 0 && s->d_records, s->choice);
	if (!route.literal && out->kind == hmrm::kRecords && (rc = ensure_records(s))) return rc;
	return HMRM_OK;
}

// A staging block of at least `doubles` that no upload still reads, without a host wait while the ring has one; blocks only grow
// (a block that is too small and free is replaced by one twice its size at least).
int acquire_view_stage(StreamCtx *c, size_t doubles, uint64_t stamp, ViewStage **out) {
	ViewStage *pick = nullptr, *oldest = &c->view_stages[0];
	for (ViewStage &v : c->view_stages) {
		if (v.stamp < oldest->stamp) oldest = &v;
		bool free_now = !v.used;
		if (!free_now) {
			const hipError_t e = hipEventQuery(v.uploaded);
			if (e == hipErrorNotReady) (void)hipGetLastError(); // (busy is no error: not left behind for the caller's next check)
			free_now = e == hipSuccess;
		}
		if (!free_now) continue;
		if (!pick || (pick->cap < doubles && v.cap > pick->cap)) pick = &v; // (the first free block, or a larger one where that is too small)
	}
	if (!pick) { // (every block's upload is still in flight: the one host wait of this path)
		HIP_TRY(hipEventSynchronize(oldest->uploaded));
		pick = oldest;
	}
	if (pick->cap < doubles) {
		if (pick->h) (void)hipHostFree(pick->h);
		pick->h = pick->h_dev = nullptr;
		const size_t cap = std::max(doubles, 2 * pick->cap);
		pick->cap = 0;
		HIP_TRY(hipHostMalloc((void **)&pick->h, cap * sizeof(double), hipHostMallocMapped));
		HIP_TRY(hipHostGetDevicePointer((void **)&pick->h_dev, pick->h, 0));
		pick->cap = cap;
	}
	if (!pick->uploaded) HIP_TRY(hipEventCreateWithFlags(&pick->uploaded, hipEventDisableTiming));
	pick->stamp = stamp;
	*out = pick;
	return HMRM_OK;
}

// The one launch of a batch whose records lie at d_frames (f0: view 0's, on the host).
int launch_views(hmrm_scene *s, StreamCtx *c, const ViewsKernel &k, const hmrm::DevFrame &f0, const hmrm::DevFrame *d_frames, int32_t n,
                 bool interior, uint32_t *d_out, int64_t out_stride_px, int64_t view_stride_px) {
	const hmrm::RowMap rows{0, f0.screen_h, 0, 0, 1, {0x7fffffff, 0x7fffffff, 0x7fffffff}, {0, 0, 0, 0}, nullptr};
	hmrm::FrameLaunch l{s->d_thr, s->d_thr32, s->d_cmap, s->d_records, d_out, out_stride_px, c->d_counters, nullptr, nullptr, false, f0, rows,
	                    hmrm::kFrameViews, hmrm::SunRules{}, interior, hmrm::GeomPlanes{}, c->stream};
	l.d_frames = d_frames;
	l.n_views = n;
	l.view_stride_px = view_stride_px;
	if (k.literal) HIP_TRY(hmrm::launch_frame_literal(l));
	else HIP_TRY(hmrm::launch_frame_march(l, k.kind));
	return HMRM_OK;
}

// A measured launch of another context is still running: this context's launch waits for it (stream order, no host wait).
int wait_for_measure_fence(hmrm_scene *s, StreamCtx *c) {
	if (!s->measure_fence_ctx || s->measure_fence_ctx == c) return HMRM_OK;
	if (hipEventQuery(s->measure_fence) == hipSuccess) s->measure_fence_ctx = nullptr;
	else HIP_TRY(hipStreamWaitEvent(c->stream, s->measure_fence, 0));
	return HMRM_OK;
}

// One frame (or row strip) on the context's stream.  Kernel variant: "leap" (default; speculative
// groups + exact leaps), "group" (speculative groups only), "simple" (the literal
// one-step-at-a-time loop, kept for A/B runs and as an in-library cross-check).  All produce
// identical pixels and counts.  What the request's fields change: FrameRequest.  (s->mu held.)
int launch_frame(hmrm_scene *s, StreamCtx *c, const hmrm::DevFrame &f, FrameSlot *slot, const hmrm::RowMap &rows, const FrameRequest &req) {
	hmrm::RowMap rows_in_order = rows;
	int tile_w = 1, tile_h = 1;
	hmrm::render_tile_shape(&tile_w, &tile_h);
	const int tiles_y = (rows.local_rows + tile_h - 1) / tile_h;
	const bool pieces = s->knobs.seg_n > 0 && rows.band_rows == 0 && rows.row_begin == 0; // (HMRM_TILE_SEGMENTS: an explicit order)
	const int rot = hmrm::choose_tile_rot(s->knobs.tile_order, slot->row_cost, rows, tile_h);
	const bool other_kernel_allowed = s->knobs.kernel == 0 && s->knobs.try_group;
	const bool may_probe = !req.special() && other_kernel_allowed;
	// calibration (launch_order.hpp): full frames of the fast kernels only
	const bool eligible = !pieces && !req.special() && s->knobs.tile_order && s->knobs.order_mode == 2 && s->knobs.kernel != 2 &&
	                      rows.band_rows == 0 && rows.row_begin == 0 && rows.local_rows == f.screen_h && tiles_y >= 12 &&
	                      tiles_y <= kMaxMeasRows && s->map_w < (1 << 24) && s->map_h < (1 << 24);
	int rc = wait_for_measure_fence(s, c);
	if (rc) return rc;
	poll_shadow_probe(s);
	hmrm::OrderTrial order; // (the rotation)
	if (pieces) {
		order.n = s->knobs.seg_n;
		for (int k = 0; k < 3; ++k) { order.b[k] = s->knobs.seg_b[k]; order.c[k] = s->knobs.seg_c[k]; }
	}
	// strips, bands, small frames, and frames with kernels of their own: the scene's verdict (never a probe); an instrumented
	// frame: the production kernel
	bool use_group = (may_probe || (req.own_kernels() && other_kernel_allowed)) && s->choice.use_group;
	bool measure_now = false;
	if (eligible) {
		poll_measured(s, c, slot, tiles_y, rot);
		// (whether a measurement may run is only looked up -- event queries on the scene's other streams -- while one is wanted)
		const bool probe_open = may_probe && !req.no_probe && !s->choice.probed && !s->probe_pending;
		const bool quiet = (slot->cal.wants_measure() || probe_open) && c->meas_owner == nullptr && !c->probe_in_flight && others_idle(s, c);
		const hmrm::LaunchPlan p = slot->cal.plan(quiet, s->choice);
		order = slot->cal.trials[p.trial];
		use_group = p.use_group;
		measure_now = p.measure;
		if (!measure_now && probe_open && quiet && slot->cal.in_flight < 0 && ++s->choice.unprobed_frames >= (unsigned)kProbeAfterFrames) {
			hmrm::set_tile_order(&rows_in_order, tiles_y, rot, order.n, order.b, order.c);
			return launch_shadow_probe(s, c, f, rows_in_order, tiles_y, req);
		}
	}
	hmrm::set_tile_order(&rows_in_order, tiles_y, rot, order.n, order.b, order.c);
	// (a measured launch that cannot be issued or reported must not stay "in flight" in the record: nothing would ever
	// report it, and the record's next reuse would wait for an event that was never recorded)
	if ((rc = launch_maybe_measured(s, c, f, slot, rows_in_order, tiles_y, measure_now, req, use_group))) {
		if (measure_now) slot->cal.drop_in_flight();
		return rc;
	}
	return HMRM_OK;
}

// Rays of this context that reached the step cap since the host last asked, given the value `now` of its counter: cumulative
// over the stream's launches, so a value read behind an earlier launch than the last one asked about brings nothing new (the
// ticket waits: a capped ray is reported with the first frame of the lane waited for after it happened).  (s->mu held.)
unsigned long long new_capped(StreamCtx *c, unsigned long long now) {
	if (now <= c->capped_seen) return 0;
	const unsigned long long n = now - c->capped_seen;
	c->capped_seen = now;
	return n;
}

// ... read from the device (the stream must be idle).
int take_capped(StreamCtx *c, unsigned long long *out) {
	unsigned long long now = 0;
	HIP_TRY(hipMemcpy(&now, c->d_counters + 2, sizeof now, hipMemcpyDeviceToHost));
	*out = new_capped(c, now);
	return HMRM_OK;
}

// The tail of a host-memory entry point that launched on the scene's own stream (c: its context) and has enqueued its copies
// to the caller's memory there: the stream's capped-ray count comes back behind them, the stream is drained -- the caller's
// memory is filled then, and the scene's scratch is free for the next call -- and the call's result is noterm() of the new
// capped rays (*capped_out: how many, for a caller that reports them in its stats).  (s->mu held.)
int finish_host_call(hmrm_scene *s, StreamCtx *c, unsigned long long *capped_out) {
	unsigned long long capped_now = 0;
	HIP_TRY(hipMemcpyAsync(&capped_now, c->d_counters + 2, sizeof capped_now, hipMemcpyDeviceToHost, s->stream));
	HIP_TRY(hipStreamSynchronize(s->stream));
	const unsigned long long capped = new_capped(c, capped_now);
	if (capped_out) *capped_out = capped;
	return noterm(capped);
}

// What a call returns for `capped` rays at the step cap: HMRM_OK for none.
int noterm(unsigned long long capped) {
	if (!capped) return HMRM_OK;
	char buf[160];
	snprintf(buf, sizeof buf, "%llu ray(s) reached the step cap; the reference's loop would not terminate for them",
	         capped);
	return fail(HMRM_E_NOTERM, buf);
}

} // namespace hmrm
