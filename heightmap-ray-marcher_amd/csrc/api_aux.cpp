// api_aux.cpp -- the C ABI declared in include/hmrm.h beside the renderer: config, image IO, and the debug hooks of the tests
// and tools.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <new>
#include <sstream>

#include "api_internal.hpp"
#include "config.hpp"
#include "host_pool.hpp"
#include "image_io.hpp"

struct hmrm_config {
	hmrm::Config cfg;
	std::string log_cache, warn_cache;
};

extern "C" {

int hmrm_debug_kernel_choice(const hmrm_scene *s) {
	if (!s) return fail(HMRM_E_ARG, "NULL argument");
	std::lock_guard<std::mutex> lk(const_cast<hmrm_scene *>(s)->mu);
	if (s->knobs.kernel != 0) return s->knobs.kernel; // forced by HMRM_KERNEL: 1 group, 2 simple, 3 rec
	return s->choice.use_group ? (s->choice.with_records ? 3 : 1) : 0;
}

// ------------------------------------------------------------------ config --
hmrm_config *hmrm_config_create(void) { return new (std::nothrow) hmrm_config(); }
void hmrm_config_destroy(hmrm_config *c) { delete c; }

int hmrm_config_consume_file(hmrm_config *c, const char *path) {
	if (!c || !path) return fail(HMRM_E_ARG, "NULL argument");
	std::ifstream in(path);
	if (!in.is_open()) return fail(HMRM_E_IO, std::string("Failed to open input file: ") + path); // hmap.cpp:537-540
	std::string fatal;
	if (!c->cfg.consume(in, &fatal)) {
		bool img = fatal.compare(0, 14, "Failed to load") == 0;
		return fail(img ? HMRM_E_IMAGE : HMRM_E_CONFIG, fatal);
	}
	return HMRM_OK;
}

int hmrm_config_consume_string(hmrm_config *c, const char *text) {
	if (!c || !text) return fail(HMRM_E_ARG, "NULL argument");
	std::istringstream in(text);
	std::string fatal;
	if (!c->cfg.consume(in, &fatal)) {
		bool img = fatal.compare(0, 14, "Failed to load") == 0;
		return fail(img ? HMRM_E_IMAGE : HMRM_E_CONFIG, fatal);
	}
	return HMRM_OK;
}

const char *hmrm_config_log(const hmrm_config *c) {
	hmrm_config *m = const_cast<hmrm_config *>(c);
	m->log_cache = m->cfg.log.str();
	return m->log_cache.c_str();
}
const char *hmrm_config_warnings(const hmrm_config *c) {
	hmrm_config *m = const_cast<hmrm_config *>(c);
	m->warn_cache = m->cfg.warn.str();
	return m->warn_cache.c_str();
}

void hmrm_config_get_camera(const hmrm_config *c, hmrm_camera *out) {
	const hmrm::Config &g = c->cfg;
	memset(out, 0, sizeof *out);
	out->width = g.screen_width;
	out->height = g.screen_height;
	out->projection = g.image_plane;
	out->bg_r = g.bg_r;
	out->bg_g = g.bg_g;
	out->bg_b = g.bg_b;
	out->sampling = (uint8_t)g.sampling;
	out->hfov = g.hfov;
	out->hang = g.hang;
	out->vang = g.vang;
	out->pos[0] = g.cam_pos[0];
	out->pos[1] = g.cam_pos[1];
	out->pos[2] = g.cam_pos[2];
	out->ortho_width = g.ortho_width;
	out->step_dist = g.step_dist;
}

void hmrm_config_get_scene_params(const hmrm_config *c, hmrm_scene_params *out) {
	const hmrm::Config &g = c->cfg;
	out->min_height = g.min_height;
	out->max_height = g.max_height;
	out->lum_r = g.lum_r;
	out->lum_g = g.lum_g;
	out->lum_b = g.lum_b;
	out->grid_width = g.grid_width;
}

int32_t hmrm_config_cycle(const hmrm_config *c) { return c->cfg.cycle_period; }
int32_t hmrm_config_recording_frame_count(const hmrm_config *c) { return c->cfg.recording_frame_count; }
const char *hmrm_config_heightmap_path(const hmrm_config *c) { return c->cfg.heightmap_path.c_str(); }
const char *hmrm_config_colormap_path(const hmrm_config *c) { return c->cfg.colormap_path.c_str(); }
const char *hmrm_config_output_path(const hmrm_config *c) { return c->cfg.output_path.c_str(); }
int32_t hmrm_config_record_mode(const hmrm_config *c) { return c->cfg.record_mode; }
int32_t hmrm_config_devices(const hmrm_config *c) { return c->cfg.devices; }
int32_t hmrm_config_antialias(const hmrm_config *c) { return c->cfg.antialias; }
int32_t hmrm_config_interior(const hmrm_config *c) { return c->cfg.interior; }
int32_t hmrm_config_shadows(const hmrm_config *c) { return c->cfg.shadows; }
int32_t hmrm_config_shading(const hmrm_config *c) { return c->cfg.shading; }
int32_t hmrm_config_sky_light(const hmrm_config *c) { return c->cfg.sky_light; }
int32_t hmrm_config_baked_light(const hmrm_config *c) { return c->cfg.baked_light; }
int32_t hmrm_config_sun_scope(const hmrm_config *c) { return c->cfg.sun_scope; }
int32_t hmrm_config_water_scope(const hmrm_config *c) { return c->cfg.water_scope; }
int32_t hmrm_config_water_light(const hmrm_config *c) { return c->cfg.water_light; }
const char *hmrm_config_sun_map_path(const hmrm_config *c) { return c->cfg.sun_map_path.c_str(); }
double hmrm_config_sun_map_lift(const hmrm_config *c) { return c->cfg.sun_map_lift; }
const char *hmrm_config_sky_map_path(const hmrm_config *c) { return c->cfg.sky_map_path.c_str(); }
const char *hmrm_config_range_map_path(const hmrm_config *c) { return c->cfg.range_map_path.c_str(); }
void hmrm_config_sky_map_rings(const hmrm_config *c, int32_t *rings, int32_t *per_ring) {
	if (rings) *rings = c->cfg.sky_map_rings;
	if (per_ring) *per_ring = c->cfg.sky_map_per_ring;
}
void hmrm_config_get_sun(const hmrm_config *c, hmrm_sun *out) {
	const hmrm::Config &g = c->cfg;
	memset(out, 0, sizeof *out);
	for (int k = 0; k < 3; ++k) out->dir[k] = g.sun_dir[k];
	out->step_dist = g.have_shadow_step_dist ? g.shadow_step_dist : g.step_dist;
	out->max_steps = (uint32_t)g.shadow_max_steps;
	out->flags = g.interior ? HMRM_TRACE_INTERIOR : 0u;
	out->ambient = (uint8_t)g.shadow_ambient;
}

int32_t hmrm_config_water(const hmrm_config *c) { return c->cfg.water; }
void hmrm_config_get_water(const hmrm_config *c, hmrm_water *out) {
	const hmrm::Config &g = c->cfg;
	memset(out, 0, sizeof *out);
	out->level = g.water_level;
	out->step_dist = g.have_water_step_dist ? g.water_step_dist : g.step_dist;
	out->max_steps = (uint32_t)g.water_max_steps;
	out->flags = (g.interior ? HMRM_TRACE_INTERIOR : 0u) | (g.have_water_color ? HMRM_WATER_OWN_COLOR : 0u);
	out->reflectivity = (uint8_t)g.water_reflectivity;
	for (int k = 0; k < 3; ++k) out->color[k] = (uint8_t)g.water_color[k];
}

int32_t hmrm_config_haze(const hmrm_config *c) { return c->cfg.haze; }
int32_t hmrm_config_haze_law(const hmrm_config *c) { return c->cfg.haze_law; }
double hmrm_config_haze_density(const hmrm_config *c) { return c->cfg.haze_density; }
double hmrm_config_haze_far(const hmrm_config *c) { return c->cfg.haze_far; }
void hmrm_config_get_haze(const hmrm_config *c, hmrm_haze *out, uint8_t *table) {
	const hmrm::Config &g = c->cfg;
	if (out) {
		memset(out, 0, sizeof *out);
		out->start = g.haze_start;
		out->scale = (double)g.haze_entries / (g.haze_far - g.haze_start);
		out->n = (uint32_t)g.haze_entries;
		out->flags = (g.interior ? HMRM_TRACE_INTERIOR : 0u) | (g.haze_sky ? HMRM_HAZE_SKY : 0u);
		for (int k = 0; k < 3; ++k) out->color[k] = (uint8_t)g.haze_color[k];
	}
	if (table) (void)hmrm::fill_haze_table(g.haze_law, g.haze_density, g.haze_entries, table);
}
int hmrm_haze_table(int32_t law, double density, int32_t n, uint8_t *out) {
	if (!hmrm::fill_haze_table(law, density, n, out))
		return fail(HMRM_E_ARG, "hmrm_haze_table: law must be HMRM_HAZE_LINEAR, _EXP or _EXP2, n 1 .. 4096 and out not NULL");
	return HMRM_OK;
}

int32_t hmrm_config_view_count(const hmrm_config *c) { return (int32_t)c->cfg.views.size(); }
const char *hmrm_config_views_output(const hmrm_config *c) { return c->cfg.views_output.c_str(); }
void hmrm_config_get_views(const hmrm_config *c, hmrm_camera *out) {
	if (!out) return;
	size_t k = 0;
	for (const hmrm::Config::View &v : c->cfg.views) {
		hmrm_camera &cam = out[k++];
		hmrm_config_get_camera(c, &cam);
		for (int a = 0; a < 3; ++a) cam.pos[a] = v.pos[a];
		cam.hang = v.hang;
		cam.vang = v.vang;
	}
}

const uint8_t *hmrm_config_height_rgb(const hmrm_config *c, int32_t *w, int32_t *h) {
	if (!c->cfg.have_heightmap) return nullptr;
	if (w) *w = c->cfg.heightmap.w;
	if (h) *h = c->cfg.heightmap.h;
	return c->cfg.heightmap.px.data();
}
const uint8_t *hmrm_config_color_rgba(const hmrm_config *c, int32_t *w, int32_t *h) {
	if (!c->cfg.have_colormap) return nullptr;
	if (w) *w = c->cfg.colormap.w;
	if (h) *h = c->cfg.colormap.h;
	return c->cfg.colormap.px.data();
}
int hmrm_config_take_heightmap_dirty(hmrm_config *c) {
	int d = c->cfg.heightmap_dirty ? 1 : 0;
	c->cfg.heightmap_dirty = false;
	return d;
}
int hmrm_config_create_scene(const hmrm_config *c, hmrm_scene **out) {
	if (!c || !out) return fail(HMRM_E_ARG, "NULL argument");
	if (!c->cfg.have_heightmap) return fail(HMRM_E_CONFIG, "Must specify heightmap in config");
	if (!c->cfg.have_colormap) return fail(HMRM_E_CONFIG, "Must specify colormap in config");
	hmrm_scene_params p;
	hmrm_config_get_scene_params(c, &p);
	return hmrm_scene_create(c->cfg.heightmap.px.data(), c->cfg.colormap.px.data(), c->cfg.heightmap.w,
	                         c->cfg.heightmap.h, &p, out);
}

// ---------------------------------------------------------------- image IO --
static int hand_out(hmrm::Image &img, uint8_t **out, int32_t *w, int32_t *h, int32_t *n) {
	uint8_t *p = (uint8_t *)malloc(img.px.size() ? img.px.size() : 1);
	if (!p) return fail(HMRM_E_ARG, "out of memory");
	memcpy(p, img.px.data(), img.px.size());
	*out = p;
	if (w) *w = img.w;
	if (h) *h = img.h;
	if (n) *n = img.comp_in_file;
	return HMRM_OK;
}

int hmrm_image_load(const char *path, int32_t req_comp, uint8_t **out, int32_t *w, int32_t *h,
                    int32_t *comp_in_file) {
	if (!path || !out) return fail(HMRM_E_ARG, "NULL argument");
	hmrm::Image img;
	std::string err;
	if (!hmrm::load_image_file(path, req_comp, &img, &err))
		return fail(err == "can't fopen" ? HMRM_E_IO : HMRM_E_IMAGE, err);
	return hand_out(img, out, w, h, comp_in_file);
}

int hmrm_image_load_memory(const uint8_t *bytes, size_t len, int32_t req_comp, uint8_t **out,
                           int32_t *w, int32_t *h, int32_t *comp_in_file) {
	if (!bytes || !out) return fail(HMRM_E_ARG, "NULL argument");
	hmrm::Image img;
	std::string err;
	if (!hmrm::decode_image(bytes, len, req_comp, &img, &err)) return fail(HMRM_E_IMAGE, err);
	return hand_out(img, out, w, h, comp_in_file);
}

void hmrm_image_free(void *p) { free(p); }

int hmrm_write_png_memory(int32_t w, int32_t h, int32_t comp, const uint8_t *data, size_t stride_bytes,
                          uint8_t **out, size_t *out_len) {
	if (!out || !out_len) return fail(HMRM_E_ARG, "NULL argument");
	std::vector<uint8_t> png;
	if (!hmrm::encode_png(w, h, comp, data, stride_bytes, &png)) return fail(HMRM_E_ARG, "bad image arguments");
	uint8_t *p = (uint8_t *)malloc(png.size());
	if (!p) return fail(HMRM_E_ARG, "out of memory");
	memcpy(p, png.data(), png.size());
	*out = p;
	*out_len = png.size();
	return HMRM_OK;
}

int hmrm_write_png(const char *path, int32_t w, int32_t h, int32_t comp, const uint8_t *data,
                   size_t stride_bytes) {
	if (!path) return fail(HMRM_E_ARG, "NULL argument");
	std::vector<uint8_t> png;
	if (!hmrm::encode_png(w, h, comp, data, stride_bytes, &png)) return fail(HMRM_E_ARG, "bad image arguments");
	if (!hmrm::write_file(path, png.data(), png.size()))
		return fail(HMRM_E_IO, std::string("Failed to write screenshot to ") + path); // hmap.cpp:162-164
	return HMRM_OK;
}

int hmrm_write_ppm(const char *path, int32_t w, int32_t h, int32_t comp, const uint8_t *data,
                   size_t stride_bytes) {
	if (!path) return fail(HMRM_E_ARG, "NULL argument");
	std::vector<uint8_t> pnm;
	if (!hmrm::encode_pnm(w, h, comp, data, stride_bytes, &pnm)) return fail(HMRM_E_ARG, "bad image arguments");
	if (!hmrm::write_file(path, pnm.data(), pnm.size()))
		return fail(HMRM_E_IO, std::string("Failed to write image to ") + path);
	return HMRM_OK;
}

// The portable float map: "Pf" (one component) or "PF" (three), width and height, the scale -1.0 -- negative: little-endian
// floats -- then the rows BOTTOM TO TOP, each w * comp floats as they are in memory.
int hmrm_write_pfm(const char *path, int32_t w, int32_t h, int32_t comp, const float *data, size_t stride_bytes) {
	if (!path || !data) return fail(HMRM_E_ARG, "NULL argument");
	if (w <= 0 || h <= 0 || (comp != 1 && comp != 3) || stride_bytes < (size_t)w * (size_t)comp * sizeof(float))
		return fail(HMRM_E_ARG, "bad image arguments");
	static_assert(sizeof(float) == 4, "PFM holds IEEE binary32");
	const uint16_t endian_probe = 1;
	if (*reinterpret_cast<const uint8_t *>(&endian_probe) != 1) return fail(HMRM_E_ARG, "hmrm_write_pfm: little-endian hosts only");
	const std::string head = std::string(comp == 1 ? "Pf\n" : "PF\n") + std::to_string(w) + " " + std::to_string(h) + "\n-1.0\n";
	const size_t row = (size_t)w * (size_t)comp * sizeof(float);
	std::vector<uint8_t> pfm(head.size() + row * (size_t)h);
	memcpy(pfm.data(), head.data(), head.size());
	for (int32_t y = 0; y < h; ++y)
		memcpy(pfm.data() + head.size() + (size_t)y * row, reinterpret_cast<const uint8_t *>(data) + (size_t)(h - 1 - y) * stride_bytes, row);
	if (!hmrm::write_file(path, pfm.data(), pfm.size())) return fail(HMRM_E_IO, std::string("Failed to write image to ") + path);
	return HMRM_OK;
}

// Device-side GetRay + distance() for one pixel (test hook).
int hmrm_debug_ray(const hmrm_scene *scene, const hmrm_camera *cam, int32_t px, int32_t py,
                   double pos[3], double dir[3], double *entry_d) {
	hmrm_scene *s = const_cast<hmrm_scene *>(scene);
	int rc = check_camera(cam);
	if (rc) return rc;
	if (!s || !pos || !dir || !entry_d) return fail(HMRM_E_ARG, "NULL argument");
	if (px < 0 || py < 0 || px >= cam->width || py >= cam->height) return fail(HMRM_E_ARG, "pixel out of range");
	HIP_TRY(hipSetDevice(s->device));
	std::lock_guard<std::mutex> lk(s->mu);
	if ((rc = s->d_entry.reserve(8 * sizeof(double)))) return rc; // (borrowed: the probe's seven doubles)
	StreamCtx *c = nullptr;
	if ((rc = ctx_for(s, s->stream, &c))) return rc;
	hmrm::DevFrame f;
	if ((rc = prepare_frame(s, c, cam, &f, nullptr))) return rc;
	HIP_TRY(hmrm::launch_probe(f, px, py, s->d_entry.as<double>(), s->stream));
	double host[7];
	HIP_TRY(hipMemcpyAsync(host, s->d_entry.ptr, sizeof host, hipMemcpyDeviceToHost, s->stream));
	HIP_TRY(hipStreamSynchronize(s->stream));
	for (int i = 0; i < 3; ++i) { pos[i] = host[i]; dir[i] = host[3 + i]; }
	*entry_d = host[6];
	return HMRM_OK;
}

// Host-only test hook for the launch-order calibration: the plan api_launch.cpp derives from the records of a measured launch
// (tile_rows x {start of the row's first workgroup, longest wave of the row}, 10 ns ticks, measured under the plain
// rotation by `rot`), and the grid-row -> tile-row map the kernel would apply for it.
int hmrm_debug_plan_order(const uint64_t *records, int32_t tile_rows, int32_t rot, int32_t pieces_begin[3],
                          int32_t pieces_count[3], int32_t *tile_row_of_grid_row) {
	if (!records || !pieces_begin || !pieces_count || tile_rows <= 0 || rot < 0 || rot >= tile_rows) return fail(HMRM_E_ARG, "bad argument");
	int b[3] = {0, 0, 0}, c[3] = {0, 0, 0};
	const int n = hmrm::plan_order_from_measurement((const unsigned long long *)records, tile_rows, rot, b, c);
	for (int k = 0; k < 3; ++k) {
		pieces_begin[k] = k < n ? b[k] : 0;
		pieces_count[k] = k < n ? c[k] : 0;
	}
	if (tile_row_of_grid_row) {
		hmrm::RowMap r{};
		hmrm::set_tile_order(&r, tile_rows, rot, n, b, c);
		for (int gy = 0; gy < tile_rows; ++gy) { // device_common.hpp pixel_of_lane, restated
			int delta = r.seg_delta[0];
			for (int k = 1; k < hmrm::kOrderSegs; ++k) delta = (unsigned)gy >= (unsigned)r.seg_first[k - 1] ? r.seg_delta[k] : delta;
			unsigned ty = (unsigned)gy + (unsigned)delta;
			if (ty >= (unsigned)tile_rows) ty -= (unsigned)tile_rows;
			tile_row_of_grid_row[gy] = (int32_t)ty;
		}
	}
	return n;
}

// v_rcp_f64 accuracy on this device (render.hip k_rcp_error): the premise of slab_classify's margins.
int hmrm_debug_rcp_error(int32_t mode, uint64_t count, uint64_t seed, int32_t exp_lo, int32_t exp_hi,
                         double *max_rel_err, uint64_t *hist64) {
	if (!max_rel_err) return fail(HMRM_E_ARG, "NULL argument");
	if (mode < 0 || mode > 2 || count == 0 || count > ((uint64_t)1 << 40) || exp_lo > exp_hi || exp_lo < -1000 || exp_hi > 1000)
		return fail(HMRM_E_ARG, "hmrm_debug_rcp_error: bad mode, count or exponent range");
	unsigned long long *d = nullptr, host[65] = {};
	HIP_TRY(hipMalloc((void **)&d, sizeof host));
	hipError_t e = hipMemset(d, 0, sizeof host);
	if (e == hipSuccess) e = hmrm::launch_rcp_error(mode, count, seed, exp_lo, exp_hi, d, nullptr);
	if (e == hipSuccess) e = hipMemcpy(host, d, sizeof host, hipMemcpyDeviceToHost);
	(void)hipFree(d);
	if (e != hipSuccess) return fail(HMRM_E_DEVICE, std::string("rcp probe: ") + hipGetErrorString(e));
	memcpy(max_rel_err, &host[0], sizeof(double));
	if (hist64)
		for (int i = 0; i < 64; ++i) hist64[i] = host[1 + i];
	return HMRM_OK;
}

int hmrm_debug_frame(const hmrm_camera *cam, const hmrm_scene_params *params, int32_t map_w,
                     int32_t map_h, double *out25, double *tables) {
	int rc = check_camera(cam);
	if (rc) return rc;
	if (!params || !out25) return fail(HMRM_E_ARG, "NULL argument");
	if (cam->projection == HMRM_SPHERICAL && !tables) return fail(HMRM_E_ARG, "tables required for spherical");
	hmrm::HostCamera hc;
	to_host_camera(cam, &hc);
	const size_t W = (size_t)cam->width, H = (size_t)cam->height;
	hmrm::DevFrame f;
	hmrm::build_frame(hc, map_w, map_h, params->min_height, params->max_height, params->grid_width, &f, nullptr, nullptr,
	                  nullptr, nullptr);
	if (cam->projection == HMRM_SPHERICAL) {
		// the tables exactly as a launch fills them: in pieces, on the host pool (prepare_frame)
		double *cc = tables, *cs = tables + W, *rs = tables + 2 * W, *rc2 = tables + 2 * W + H;
		const int nc = cam->width, nr = cam->height;
		hmrm::parallel_ranges(nc + nr, 1024, [&](int b, int e) {
			if (b < nc) hmrm::fill_col_tables(hc, b, std::min(e, nc), cc, cs);
			if (e > nc) hmrm::fill_row_tables(hc, std::max(b, nc) - nc, e - nc, rs, rc2);
		});
	}
	double *o = out25;
	for (int i = 0; i < 3; ++i) *o++ = f.cam[i];
	for (int i = 0; i < 3; ++i) *o++ = f.upper_left[i];
	for (int i = 0; i < 3; ++i) *o++ = f.plane_right[i];
	for (int i = 0; i < 3; ++i) *o++ = f.plane_down[i];
	for (int i = 0; i < 3; ++i) *o++ = f.look[i];
	for (int i = 0; i < 3; ++i) *o++ = f.c0[i];
	for (int i = 0; i < 3; ++i) *o++ = f.c1[i];
	*o++ = f.nudge;
	*o++ = f.step_dist;
	*o++ = (double)f.grid_pow2;
	*o++ = f.inv_grid_width;
	return HMRM_OK;
}

// Test hook (no GPU): launch_order.hpp pick_fast_kernel for a scene whose probe state is (scene_verdict, scene_with_records).
int hmrm_debug_pick_kernel(int32_t forced, int32_t use_other, int32_t records_ok, int32_t scene_verdict, int32_t scene_with_records,
                           int32_t *with_records_after) {
	hmrm::KernelChoice choice;
	choice.use_group = scene_verdict != 0;
	choice.probed = choice.use_group;
	choice.with_records = scene_with_records != 0;
	const int k = hmrm::pick_fast_kernel(forced, use_other != 0, records_ok != 0, choice);
	if (with_records_after) *with_records_after = choice.with_records ? 1 : 0;
	return k;
}

// Test hook (no GPU): the level state byte of frame.hpp unpacked, and the policy's level moves from that level.
int hmrm_debug_level_state(int32_t level, int32_t young, int32_t min_level, int32_t out[8]) {
	if (!out || level < 0 || level > hmrm::kMipLevels || min_level < 0 || min_level >= hmrm::kMipLevels)
		return fail(HMRM_E_ARG, "hmrm_debug_level_state: bad argument");
	const uint32_t b = (uint32_t)(hmrm::level_state_table() >> (8 * level)) & 0xffu;
	const int hs = (int)(b & 31u), back = (int)(b >> 5);
	const int lstep = hmrm::level_step(young ? 0 : -1);
	out[0] = hs;
	out[1] = back;
	out[2] = (back + 1) << hs;
	out[3] = lstep;
	out[4] = hmrm::level_coarser(level, lstep);
	out[5] = hmrm::level_finer(level, lstep, min_level);
	out[6] = level == min_level ? 1 : 0;
	out[7] = (int32_t)b;
	return hmrm::kMipLevels;
}

// Test hook (no GPU): the calibration's state machine (launch_order.hpp OrderCalibration / KernelChoice) driven through a
// sequence of full-frame launches of one camera; the measurement of a launch arrives before the next launch.
int hmrm_debug_calibrate(const uint64_t *records, int32_t launches, int32_t tile_rows, int32_t rot, int32_t may_probe,
                         int32_t scene_already_probed, const uint8_t *can_measure, int32_t *trial_used, int32_t *measured,
                         int32_t *group_kernel, int32_t *n_trials, int32_t *best, int32_t *scene_use_group, int32_t *settled_at_launch) {
	if (!records || launches <= 0 || tile_rows <= 0 || tile_rows > kMaxMeasRows || rot < 0 || rot >= tile_rows)
		return fail(HMRM_E_ARG, "hmrm_debug_calibrate: bad argument");
	hmrm::OrderCalibration cal;
	hmrm::KernelChoice choice;
	choice.probed = scene_already_probed != 0;
	int settled_at = -1;
	for (int32_t i = 0; i < launches; ++i) {
		const hmrm::LaunchPlan p = cal.plan(!can_measure || can_measure[i] != 0, choice);
		if (trial_used) trial_used[i] = p.trial;
		if (measured) measured[i] = p.measure ? 1 : 0;
		if (group_kernel) group_kernel[i] = p.use_group ? 1 : 0;
		if (p.measure && cal.on_measured((const unsigned long long *)records + (size_t)i * 2 * (size_t)tile_rows, tile_rows, rot, may_probe != 0, choice))
			settled_at = i;
	}
	if (n_trials) *n_trials = cal.n_trials;
	if (best) *best = cal.best;
	if (scene_use_group) *scene_use_group = choice.use_group ? 1 : 0;
	if (settled_at_launch) *settled_at_launch = settled_at;
	return HMRM_OK;
}

} // extern "C"
