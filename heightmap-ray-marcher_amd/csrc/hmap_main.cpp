// hmap -- headless command line front end over libhmrm's C ABI.
//
// Same argv contract as the reference (main/hmap.cpp:526-544): exactly one
// argument, the config file; "USAGE" + exit 1 otherwise; every parsed option is
// echoed to stdout; warnings/errors go to stderr; fatal conditions exit 1.
// Instead of opening an SDL window (hmap.cpp:546-649, out of scope) it renders
// ONE full frame (`cycle 1` semantics) on the GPU and saves it the way F12 does
// (hmap.cpp:828-850 -> SavePNG :157-168): to the config's `output` path if
// given (.ppm selects binary PPM), else screenshots/hmap_<epoch>.png.  `antialias n` renders (and records)
// n x n box-filtered samples per pixel (hmrm_render_aa).  `interior on` renders the single frame under the interior rule
// (hmrm_render_interior: a camera inside the box sees the terrain); it is ignored, with a warning, together with
// `antialias` > 1, `devices` > 1 or `record orbit`.  `shadows on` renders the single frame with sun shadows (hmrm_render_lit;
// under the interior rule too when `interior on`), and is ignored, with a warning, in the same three cases.  `shading on`
// renders it with diffuse sun shading (hmrm_render_shaded with HMRM_SHADE_DIFFUSE, and HMRM_SHADE_NO_SHADOWS unless
// `shadows on`; the sun is the same), and is ignored, with a warning, in those three cases too.  `sun_scope all` lifts two of
// the three for shadows and shading: with `antialias n` > 1 the single frame is the antialiased lit frame
// (hmrm_render_shaded_aa), and `record orbit` records lit frames (hmrm_record_orbit_shaded, antialiased with `antialias n`,
// over `devices n`); `interior on` then reaches those frames as the sun's HMRM_TRACE_INTERIOR.  A single frame over
// `devices` > 1 stays plain.  `sun_map <path.png>`: after its frames the whole map's light map (hmrm_cell_map with HMRM_MAP_WEIGHT:
// one byte per cell under the config's sun, the camera's sampling, `sun_map_lift` above the surface; diffuse levels with
// `shading on`, shadow rays unless `shading on` stands without `shadows on`) is written there as a one-component PNG.
// `sky_map <path.png>`: after that, the whole map's sky-view map (hmrm_cell_map_sum over `sky_map_rings r n` sky directions).
// `range_map <path.pfm>`: after the frames and before the sun map, the range plane of the configured camera (hmrm_render_geometry).
// `view x y z hang vang` (up to 64 lines) with `views_output <prefix>`: after the frames and before the range map, those cameras --
// everything else from the configured one -- as ONE view batch (hmrm_render_views), written to <prefix>000.png, <prefix>001.png, ...
// `water on`: the single frame with mirror reflections at or below `water_level` (hmrm_render_water; under the interior rule too
// when `interior on`); ignored, with a warning, beside `antialias` > 1, `devices` > 1, `record orbit`, `shadows`, `shading` and
// `baked_light`.  `water_scope all` lifts three of them: with `antialias n` > 1 the single frame is the antialiased water frame
// (hmrm_render_water_aa), `record orbit` records water frames (hmrm_record_orbit_water, antialiased with `antialias n`), and
// `baked_light sun|sky` bakes as usual and then renders those under the plane (HMRM_WATER_BAKED).  `water_light sun`: `water on`
// beside `shadows on` and / or `shading on` is the sun-lit water frame (hmrm_render_water_lit, with the shaded single frame's
// flags) -- one device, `antialias 1`, no `baked_light`, either `water_scope`; elsewhere the warnings above stand.
#include <sys/stat.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/hmrm.h"

// `devices n` (0 = all visible).  HMRM_OVERSUBSCRIBE_DEVICES=1 (tests on a one-GPU box) keeps n above the
// number of visible GPUs and deals the scenes out round-robin over the devices there are.
static int wanted_devices(hmrm_config *cfg, int *visible_out) {
	int n = hmrm_config_devices(cfg);
	const int visible = hmrm_device_count() > 0 ? hmrm_device_count() : 1;
	const char *over = std::getenv("HMRM_OVERSUBSCRIBE_DEVICES");
	if (n <= 0) n = visible;
	if (n > visible && !(over && over[0] == '1')) n = visible;
	*visible_out = visible;
	return n;
}

static bool ends_with(const std::string &s, const char *suffix) {
	const size_t n = strlen(suffix);
	return s.size() >= n && s.compare(s.size() - n, n, suffix) == 0;
}

// `range_map <path.pfm>`: the range plane of the configured camera's geometry frame (hmrm_render_geometry; under the interior rule
// with `interior on`) as a one-component portable float map.  Returns false when it could not be made or written.
static bool write_range_map(hmrm_config *cfg, hmrm_scene *scene, const hmrm_camera &cam, bool interior) {
	const std::string path = hmrm_config_range_map_path(cfg);
	if (path.empty()) return true;
	std::vector<float> range((size_t)cam.width * cam.height);
	hmrm_geometry_planes planes;
	memset(&planes, 0, sizeof planes);
	planes.range = range.data();
	planes.range_stride = (size_t)cam.width * sizeof(float);
	planes.flags = interior ? HMRM_TRACE_INTERIOR : 0u;
	const int rc = hmrm_render_geometry(scene, &cam, &planes);
	if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
		std::cerr << hmrm_last_error() << "\n";
		return false;
	}
	if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
	if (hmrm_write_pfm(path.c_str(), cam.width, cam.height, 1, range.data(), planes.range_stride) != HMRM_OK) {
		std::cerr << "Failed to write range map to " << path << "\n";
		return false;
	}
	std::cout << "Saved range map at " << path << "\n";
	return true;
}

// `view x y z hang vang` lines with `views_output <prefix>`: those cameras as one view batch (hmrm_render_views; under the interior
// rule with `interior on`), written to <prefix>000.png, <prefix>001.png, ...  One key without the other warns and does nothing.
// Returns false when the batch could not be rendered or a file not written.
static bool write_views(hmrm_config *cfg, hmrm_scene *scene, bool interior) {
	const int32_t n = hmrm_config_view_count(cfg);
	const std::string prefix = hmrm_config_views_output(cfg);
	if (n == 0 && prefix.empty()) return true;
	if (n == 0 || prefix.empty()) {
		std::cerr << (n == 0 ? "WARNING: views_output is ignored without a view\n" : "WARNING: view is ignored without views_output\n");
		return true;
	}
	std::vector<hmrm_camera> cams((size_t)n);
	hmrm_config_get_views(cfg, cams.data());
	const size_t stride = (size_t)cams[0].width * 4, view = stride * (size_t)cams[0].height;
	std::vector<uint8_t> frames(view * (size_t)n);
	const int rc = hmrm_render_views(scene, cams.data(), n, interior ? HMRM_TRACE_INTERIOR : 0u, frames.data(), stride, view);
	if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
		std::cerr << hmrm_last_error() << "\n";
		return false;
	}
	if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
	std::cout << "rendered " << n << " views in " << hmrm_last_kernel_ms() << " ms (kernel)\n";
	for (int32_t k = 0; k < n; ++k) {
		char num[16];
		snprintf(num, sizeof num, "%03d", (int)k);
		const std::string path = prefix + num + ".png";
		if (hmrm_write_png(path.c_str(), cams[0].width, cams[0].height, 4, frames.data() + view * (size_t)k, stride) != HMRM_OK) {
			std::cerr << "Failed to write view to " << path << "\n";
			return false;
		}
		std::cout << "Saved view at " << path << "\n";
	}
	return true;
}

// `sun_map <path>`: the whole map's light map, one byte per cell.  Returns false when it could not be made or written.
static bool write_sun_map(hmrm_config *cfg, hmrm_scene *scene, const hmrm_camera &cam, bool shading, bool shadows) {
	const std::string path = hmrm_config_sun_map_path(cfg);
	if (path.empty()) return true;
	int32_t mw = 0, mh = 0;
	hmrm_config_height_rgb(cfg, &mw, &mh);
	hmrm_sun sun;
	hmrm_config_get_sun(cfg, &sun);
	hmrm_cell_map_params p;
	memset(&p, 0, sizeof p);
	for (int k = 0; k < 3; ++k) p.target[k] = sun.dir[k];
	p.step_dist = sun.step_dist;
	p.lift = hmrm_config_sun_map_lift(cfg);
	p.max_steps = sun.max_steps;
	p.flags = HMRM_MAP_WEIGHT | (shading ? HMRM_MAP_DIFFUSE : 0u) | (shading && !shadows ? HMRM_MAP_NO_SHADOWS : 0u);
	p.sampling = cam.sampling;
	p.ambient = sun.ambient;
	std::vector<uint8_t> map((size_t)mw * mh);
	const int rc = hmrm_cell_map(scene, &p, NULL, map.data(), (size_t)mw);
	if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
		std::cerr << hmrm_last_error() << "\n";
		return false;
	}
	if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
	if (hmrm_write_png(path.c_str(), mw, mh, 1, map.data(), (size_t)mw) != HMRM_OK) {
		std::cerr << "Failed to write sun map to " << path << "\n";
		return false;
	}
	std::cout << "Saved sun map at " << path << "\n";
	return true;
}

// `sky_map <path>`: the whole map's sky-view map -- how many of the K = r * n cosine-weighted sky directions of `sky_map_rings`
// are open above each cell (hmrm_cell_map_sum in status mode), scaled to a byte.  Returns false when it could not be made or written.
static bool write_sky_map(hmrm_config *cfg, hmrm_scene *scene, const hmrm_camera &cam) {
	const std::string path = hmrm_config_sky_map_path(cfg);
	if (path.empty()) return true;
	int32_t mw = 0, mh = 0, rings = 0, per_ring = 0;
	hmrm_config_height_rgb(cfg, &mw, &mh);
	hmrm_config_sky_map_rings(cfg, &rings, &per_ring);
	std::vector<double> dirs((size_t)3 * rings * per_ring);
	const int K = hmrm_sky_directions(rings, per_ring, dirs.data());
	if (K < 1) {
		std::cerr << hmrm_last_error() << "\n";
		return false;
	}
	hmrm_sun sun;
	hmrm_config_get_sun(cfg, &sun);
	hmrm_cell_map_params p;
	memset(&p, 0, sizeof p);
	p.step_dist = sun.step_dist;
	p.lift = hmrm_config_sun_map_lift(cfg);
	p.max_steps = sun.max_steps;
	p.sampling = cam.sampling;
	p.ambient = sun.ambient;
	std::vector<uint16_t> counts((size_t)mw * mh);
	const int rc = hmrm_cell_map_sum(scene, &p, dirs.data(), K, NULL, counts.data(), 2 * (size_t)mw);
	if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
		std::cerr << hmrm_last_error() << "\n";
		return false;
	}
	if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
	std::vector<uint8_t> map(counts.size());
	for (size_t i = 0; i < counts.size(); ++i) map[i] = (uint8_t)(((uint32_t)counts[i] * 255u + (uint32_t)K / 2u) / (uint32_t)K);
	if (hmrm_write_png(path.c_str(), mw, mh, 1, map.data(), (size_t)mw) != HMRM_OK) {
		std::cerr << "Failed to write sky map to " << path << "\n";
		return false;
	}
	std::cout << "Saved sky map at " << path << "\n";
	return true;
}

// `baked_light sun|sky` (mode 1|2): the scene's light plane baked once, before the frames -- the light `sun_map` would write, under
// `sun_dir`, or the count `sky_map` would scale, over `sky_map_rings`.  Returns false when it could not be baked.
static bool bake_light(hmrm_config *cfg, hmrm_scene *scene, const hmrm_camera &cam, int mode, bool shading, bool shadows) {
	hmrm_sun sun;
	hmrm_config_get_sun(cfg, &sun);
	hmrm_cell_map_params p;
	memset(&p, 0, sizeof p);
	p.step_dist = sun.step_dist;
	p.lift = hmrm_config_sun_map_lift(cfg);
	p.max_steps = sun.max_steps;
	p.sampling = cam.sampling;
	p.ambient = sun.ambient;
	std::vector<double> dirs(sun.dir, sun.dir + 3);
	int K = 1;
	if (mode == 1) {
		p.flags = HMRM_MAP_WEIGHT | (shading ? HMRM_MAP_DIFFUSE : 0u) | (shading && !shadows ? HMRM_MAP_NO_SHADOWS : 0u);
	} else {
		int32_t rings = 0, per_ring = 0;
		hmrm_config_sky_map_rings(cfg, &rings, &per_ring);
		dirs.assign((size_t)3 * rings * per_ring, 0.0);
		K = hmrm_sky_directions(rings, per_ring, dirs.data());
		if (K < 1) {
			std::cerr << hmrm_last_error() << "\n";
			return false;
		}
	}
	const int rc = hmrm_scene_bake_light(scene, &p, dirs.data(), K);
	if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
		std::cerr << hmrm_last_error() << "\n";
		return false;
	}
	if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
	uint32_t full_scale = 0;
	(void)hmrm_scene_light(scene, NULL, 0, &full_scale);
	std::cout << "baked light: " << K << " direction(s), full scale " << full_scale << "\n";
	return true;
}

int main(int argc, char *argv[]) {
	if (argc != 2) {
		std::cerr << "USAGE: hmap.exe path/to/config.txt\n";
		return 1;
	}
	hmrm_config *cfg = hmrm_config_create();
	int rc = hmrm_config_consume_file(cfg, argv[1]);
	std::cout << hmrm_config_log(cfg);
	std::cerr << hmrm_config_warnings(cfg);
	if (rc != HMRM_OK) {
		if (rc == HMRM_E_IO) std::cerr << hmrm_last_error() << "\n";
		return 1;
	}

	hmrm_camera cam;
	hmrm_config_get_camera(cfg, &cam);
	// (the library applies the same test, check_camera; here it guards the framebuffer allocation below)
	if (cam.width <= 0 || cam.height <= 0 || (long long)cam.width * cam.height > (1LL << 31) / 4) {
		std::cerr << "resolution must be positive and at most 2^29 pixels (the reference indexes the framebuffer with int)\n";
		return 1;
	}
	const int32_t aa = hmrm_config_antialias(cfg);
	const bool interior = hmrm_config_interior(cfg) != 0;
	const bool shadows = hmrm_config_shadows(cfg) != 0;
	const bool shading = hmrm_config_shading(cfg) != 0;
	bool sky_light = hmrm_config_sky_light(cfg) != 0; // (the single frame under the sky's directions: hmrm_render_lit_sum)
	const int baked_mode = hmrm_config_baked_light(cfg); // (1 sun, 2 sky: the frames under a light plane baked once)
	// `sun_scope all`: shadows / shading also apply to antialiased and recorded frames
	const bool sun_all = hmrm_config_sun_scope(cfg) != 0 && (shadows || shading);
	const uint32_t shade_flags = shading ? (HMRM_SHADE_DIFFUSE | (shadows ? 0u : HMRM_SHADE_NO_SHADOWS)) : 0u;
	// `water_scope all`: water also applies to antialiased, recorded and baked-light frames
	const bool water_all = hmrm_config_water_scope(cfg) != 0 && hmrm_config_water(cfg) != 0;
	hmrm_scene *scene = NULL;
	if (hmrm_config_create_scene(cfg, &scene) != HMRM_OK) {
		std::cerr << hmrm_last_error() << "\n";
		return 1;
	}

	if (hmrm_config_record_mode(cfg) == 1) {
		int visible_rec = 1;
		bool baked = baked_mode != 0;
		if (baked && wanted_devices(cfg, &visible_rec) > 1) {
			std::cerr << "WARNING: baked_light is ignored with devices > 1\n";
			baked = false;
		}
		if (baked && sky_light) {
			std::cerr << "WARNING: sky_light is ignored with baked_light\n";
			sky_light = false;
		}
		// (`water_scope all`: the orbit's frames are water frames -- on one device, and beside shadows or shading only under baked light)
		bool water_orbit = water_all;
		if (water_orbit) {
			const char *beside = wanted_devices(cfg, &visible_rec) > 1 ? "devices > 1"
			                     : baked ? nullptr : shadows ? "shadows" : shading ? "shading" : nullptr;
			if (beside) {
				std::cerr << "WARNING: water is ignored with " << beside << "\n";
				water_orbit = false;
			}
		}
		if (!sun_all && !baked && !water_orbit) {
			if (interior) std::cerr << "WARNING: interior is ignored with record orbit\n";
			if (shadows) std::cerr << "WARNING: shadows is ignored with record orbit\n";
			if (shading) std::cerr << "WARNING: shading is ignored with record orbit\n";
		}
		if (sky_light) std::cerr << "WARNING: sky_light is ignored with record orbit\n";
		if (hmrm_config_water(cfg) != 0 && !water_all) std::cerr << "WARNING: water is ignored with record orbit\n";
		if (hmrm_config_haze(cfg) != 0) std::cerr << "WARNING: haze is ignored with record orbit\n";
		// `record orbit`: recording_frame_count frames on a circle around the map centre through
		// the configured camera position, always looking at the centre;
		// files screenshots/hmap_<epoch>_<n>.png as hmap.cpp:1131-1144.
		hmrm_scene_params sp;
		hmrm_config_get_scene_params(cfg, &sp);
		int32_t mw = 0, mh = 0;
		hmrm_config_height_rgb(cfg, &mw, &mh);
		const double cx = mw * sp.grid_width / 2.0, cy = -(mh * sp.grid_width) / 2.0;
		const double dx = cx - cam.pos[0], dy = cy - cam.pos[1];
		const double radius = std::sqrt(dx * dx + dy * dy);
		const double hang0 = std::atan2(dy, dx);
		std::time_t id = std::time(NULL);
		if (id == (std::time_t)(-1)) {
			std::cerr << "Failed to get time for recording. Recording NOT started.\n"; // hmap.cpp:886-892
			return 1;
		}
		std::string dir = hmrm_config_output_path(cfg);
		if (dir.empty()) dir = "screenshots";
		mkdir(dir.c_str(), 0777);
		// `devices n`: one scene per GPU, frame k on device k mod n (BASELINE config C5); the scene
		// created above lives on device 0
		int visible = 1;
		const int ndev = wanted_devices(cfg, &visible);
		std::vector<hmrm_scene *> scenes(1, scene);
		for (int d = 1; d < ndev && rc == HMRM_OK; ++d) {
			hmrm_scene *extra = NULL;
			rc = hmrm_set_device(d % visible);
			if (rc == HMRM_OK) rc = hmrm_config_create_scene(cfg, &extra);
			if (rc == HMRM_OK) scenes.push_back(extra);
		}
		if (rc == HMRM_OK && water_orbit) {
			hmrm_water w;
			hmrm_config_get_water(cfg, &w);
			if (baked && !bake_light(cfg, scene, cam, baked_mode, shading, shadows)) rc = HMRM_E_DEVICE;
			else
				rc = hmrm_record_orbit_water(scenes.data(), (int32_t)scenes.size(), &cam, cx, cy, radius, hang0,
				                             hmrm_config_recording_frame_count(cfg), dir.c_str(), (long long)id, 0, 1,
				                             aa > 1 ? HMRM_AA(aa) : 0u, &w, baked ? HMRM_WATER_BAKED : 0u);
		} else if (rc == HMRM_OK && baked) {
			if (!bake_light(cfg, scene, cam, baked_mode, shading, shadows)) rc = HMRM_E_DEVICE;
			else
				rc = hmrm_record_orbit_baked(scenes.data(), (int32_t)scenes.size(), &cam, cx, cy, radius, hang0,
				                             hmrm_config_recording_frame_count(cfg), dir.c_str(), (long long)id, 0, 1,
				                             aa > 1 ? HMRM_AA(aa) : 0u, interior ? HMRM_TRACE_INTERIOR : 0u);
		} else if (rc == HMRM_OK && sun_all) {
			hmrm_sun sun;
			hmrm_config_get_sun(cfg, &sun);
			rc = hmrm_record_orbit_shaded(scenes.data(), (int32_t)scenes.size(), &cam, cx, cy, radius, hang0,
			                              hmrm_config_recording_frame_count(cfg), dir.c_str(), (long long)id, 0, 1,
			                              aa > 1 ? HMRM_AA(aa) : 0u, &sun, shade_flags);
		} else if (rc == HMRM_OK)
			rc = hmrm_record_orbit_flags(scenes.data(), (int32_t)scenes.size(), &cam, cx, cy, radius, hang0,
			                             hmrm_config_recording_frame_count(cfg), dir.c_str(), (long long)id, 0, 1,
			                             aa > 1 ? HMRM_AA(aa) : 0u);
		if (rc != HMRM_OK) std::cerr << hmrm_last_error() << "\n";
		for (size_t i = 1; i < scenes.size(); ++i) hmrm_scene_destroy(scenes[i]);
		if (rc == HMRM_OK && !write_views(cfg, scene, interior)) rc = HMRM_E_IO;
		if (rc == HMRM_OK && !write_range_map(cfg, scene, cam, interior)) rc = HMRM_E_IO;
		if (rc == HMRM_OK && !write_sun_map(cfg, scene, cam, shading, shadows)) rc = HMRM_E_IO;
		if (rc == HMRM_OK && !write_sky_map(cfg, scene, cam)) rc = HMRM_E_IO;
		hmrm_scene_destroy(scene);
		hmrm_config_destroy(cfg);
		return rc == HMRM_OK ? 0 : 1;
	}

	std::vector<uint8_t> framebuf((size_t)cam.width * cam.height * 4);
	int visible_dev = 1;
	const int want_dev = wanted_devices(cfg, &visible_dev);
	if (want_dev > 1 && aa > 1)
		std::cerr << "WARNING: antialias " << aa << " renders the single frame on one device (devices " << want_dev << " ignored)\n";
	const bool baked = baked_mode != 0 && want_dev <= 1;
	if (baked_mode != 0 && !baked) std::cerr << "WARNING: baked_light is ignored with devices > 1\n";
	if (baked && sky_light) {
		std::cerr << "WARNING: sky_light is ignored with baked_light\n";
		sky_light = false;
	}
	// (`water_scope all`: the single frame is a water frame whatever the factor, under the baked plane too -- on one device, and
	// beside shadows or shading only under baked light)
	const bool water_wide = water_all && want_dev <= 1 && (baked || (!shadows && !shading));
	const bool lit_aa = sun_all && want_dev <= 1 && aa > 1 && !baked; // (the antialiased lit single frame)
	// `haze on`: the single frame with distance fog (hmrm_render_haze), antialiased with `antialias n`, under the interior rule with
	// `interior on` -- on one device, and with neither a sun, nor water, nor a light plane
	bool haze = hmrm_config_haze(cfg) != 0;
	if (haze) {
		const char *beside = shadows ? "shadows" : shading ? "shading" : hmrm_config_water(cfg) != 0 ? "water" : baked_mode != 0 ? "baked_light"
		                     : sky_light ? "sky_light" : want_dev > 1 ? "devices > 1" : nullptr;
		if (beside) {
			std::cerr << "WARNING: haze is ignored with " << beside << "\n";
			haze = false;
		}
	}
	if (interior && !lit_aa && !baked && !water_wide && !haze && (want_dev > 1 || aa > 1))
		std::cerr << "WARNING: interior is ignored with " << (aa > 1 ? "antialias > 1" : "devices > 1") << "\n";
	if (shadows && !lit_aa && !baked && (want_dev > 1 || aa > 1))
		std::cerr << "WARNING: shadows is ignored with " << (aa > 1 ? "antialias > 1" : "devices > 1") << "\n";
	if (shading && !lit_aa && !baked && (want_dev > 1 || aa > 1))
		std::cerr << "WARNING: shading is ignored with " << (aa > 1 ? "antialias > 1" : "devices > 1") << "\n";
	if (sky_light && (want_dev > 1 || aa > 1)) // (whatever sun_scope says: there is no antialiased accumulated frame)
		std::cerr << "WARNING: sky_light is ignored with " << (aa > 1 ? "antialias > 1" : "devices > 1") << "\n";
	// `water on`: the single frame with mirror reflections at or below `water_level` (hmrm_render_water) -- the plain frame's only
	bool water = hmrm_config_water(cfg) != 0;
	// `water_light sun`: beside shadows and / or shading that frame is the sun-lit water frame (hmrm_render_water_lit)
	const bool water_lit = water && hmrm_config_water_light(cfg) != 0 && (shadows || shading) && baked_mode == 0 && want_dev <= 1 && aa == 1;
	if (water && water_all) {
		const char *beside = want_dev > 1 ? "devices > 1" : (baked || water_lit) ? nullptr : shadows ? "shadows" : shading ? "shading" : nullptr;
		if (beside) {
			std::cerr << "WARNING: water is ignored with " << beside << "\n";
			water = false;
		}
	} else
	if (water) {
		const char *beside = water_lit ? nullptr : aa > 1 ? "antialias > 1" : want_dev > 1 ? "devices > 1" : shadows ? "shadows" : shading ? "shading"
		                     : baked_mode != 0 ? "baked_light" : nullptr;
		if (beside) {
			std::cerr << "WARNING: water is ignored with " << beside << "\n";
			water = false;
		}
	}
	if (water && sky_light) {
		std::cerr << "WARNING: sky_light is ignored with water\n";
		sky_light = false;
	}
	if (haze) {
		hmrm_haze hz;
		std::vector<uint8_t> table(4096);
		hmrm_config_get_haze(cfg, &hz, table.data());
		rc = hmrm_render_haze(scene, &cam, &hz, table.data(), aa, framebuf.data(), (size_t)cam.width * 4);
		if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
			std::cerr << hmrm_last_error() << "\n";
			return 1;
		}
		if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
		std::cout << "rendered " << (long long)cam.width * cam.height * aa * aa << " rays with haze from " << hz.start << " to "
		          << hmrm_config_haze_far(cfg) << (aa > 1 ? " at antialias " + std::to_string(aa) : std::string())
		          << (interior ? " under the interior rule" : "") << " in " << hmrm_last_kernel_ms() << " ms (kernel)\n";
	} else if (water && water_lit) {
		hmrm_water w;
		hmrm_config_get_water(cfg, &w);
		hmrm_sun sun;
		hmrm_config_get_sun(cfg, &sun);
		rc = hmrm_render_water_lit(scene, &cam, &w, &sun, shade_flags, framebuf.data(), (size_t)cam.width * 4);
		if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
			std::cerr << hmrm_last_error() << "\n";
			return 1;
		}
		if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
		std::cout << "rendered " << (long long)cam.width * cam.height << " rays with water at level " << w.level
		          << (shading ? (shadows ? " with sun shading and sun shadows" : " with sun shading") : " with sun shadows")
		          << (interior ? " under the interior rule" : "") << "\n";
	} else if (water && water_all) {
		// the single frame, antialiased or not, under the light plane baked here or under none
		hmrm_water w;
		hmrm_config_get_water(cfg, &w);
		if (baked && !bake_light(cfg, scene, cam, baked_mode, shading, shadows)) return 1;
		rc = hmrm_render_water_aa(scene, &cam, &w, baked ? HMRM_WATER_BAKED : 0u, aa, framebuf.data(), (size_t)cam.width * 4);
		if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
			std::cerr << hmrm_last_error() << "\n";
			return 1;
		}
		if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
		std::cout << "rendered " << (long long)cam.width * cam.height * aa * aa << " rays with water at level " << w.level
		          << (aa > 1 ? " at antialias " + std::to_string(aa) : std::string()) << (baked ? " under baked light" : "")
		          << (interior ? " under the interior rule" : "") << "\n";
	} else if (water) {
		hmrm_water w;
		hmrm_config_get_water(cfg, &w);
		rc = hmrm_render_water(scene, &cam, &w, framebuf.data(), (size_t)cam.width * 4);
		if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
			std::cerr << hmrm_last_error() << "\n";
			return 1;
		}
		if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
		std::cout << "rendered " << (long long)cam.width * cam.height << " rays with water at level " << w.level
		          << (interior ? " under the interior rule" : "") << "\n";
	} else if (baked) {
		// the single frame, antialiased or not, under the light plane baked here: `shadows` and `shading` only chose what was baked
		if (!bake_light(cfg, scene, cam, baked_mode, shading, shadows)) return 1;
		rc = hmrm_render_baked(scene, &cam, interior ? HMRM_TRACE_INTERIOR : 0u, aa, framebuf.data(), (size_t)cam.width * 4);
		if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
			std::cerr << hmrm_last_error() << "\n";
			return 1;
		}
		if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
		std::cout << "rendered " << (long long)cam.width * cam.height * aa * aa << " rays under baked light"
		          << (interior ? " under the interior rule" : "") << " in " << hmrm_last_kernel_ms() << " ms (kernel)\n";
	} else if (sky_light && want_dev <= 1 && aa == 1) {
		// every hit pixel under the K = r * n cosine-weighted sky directions of `sky_map_rings`, shadow rays always on, the diffuse
		// level per direction with `shading on`; ambient, step and limit are the sun's keys, sun_dir is not used
		int32_t rings = 0, per_ring = 0;
		hmrm_config_sky_map_rings(cfg, &rings, &per_ring);
		std::vector<double> dirs((size_t)3 * rings * per_ring);
		const int K = hmrm_sky_directions(rings, per_ring, dirs.data());
		if (K < 1) {
			std::cerr << hmrm_last_error() << "\n";
			return 1;
		}
		hmrm_sun sun;
		hmrm_config_get_sun(cfg, &sun);
		hmrm_light_planes planes;
		memset(&planes, 0, sizeof planes);
		planes.rgba = framebuf.data();
		planes.rgba_stride = (size_t)cam.width * 4;
		rc = hmrm_render_lit_sum(scene, &cam, &sun, dirs.data(), K, shading ? HMRM_SHADE_DIFFUSE : 0u, &planes);
		if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
			std::cerr << hmrm_last_error() << "\n";
			return 1;
		}
		if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
		std::cout << "rendered " << (long long)cam.width * cam.height << " rays with sky light from " << K << " directions"
		          << (shading ? " and sun shading" : "") << (interior ? " under the interior rule" : "") << "\n";
	} else if (lit_aa) {
		hmrm_sun sun;
		hmrm_config_get_sun(cfg, &sun);
		rc = hmrm_render_shaded_aa(scene, &cam, &sun, shade_flags, aa, framebuf.data(), (size_t)cam.width * 4);
		if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
			std::cerr << hmrm_last_error() << "\n";
			return 1;
		}
		if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
		std::cout << "rendered " << (long long)cam.width * cam.height * aa * aa << " rays at antialias " << aa
		          << (shading ? (shadows ? " with sun shading and sun shadows" : " with sun shading") : " with sun shadows")
		          << (interior ? " under the interior rule" : "") << " in " << hmrm_last_kernel_ms() << " ms (kernel)\n";
	} else if (shading && want_dev <= 1 && aa == 1) {
		hmrm_sun sun;
		hmrm_config_get_sun(cfg, &sun);
		rc = hmrm_render_shaded(scene, &cam, &sun, HMRM_SHADE_DIFFUSE | (shadows ? 0u : HMRM_SHADE_NO_SHADOWS), framebuf.data(),
		                        (size_t)cam.width * 4);
		if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
			std::cerr << hmrm_last_error() << "\n";
			return 1;
		}
		if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
		std::cout << "rendered " << (long long)cam.width * cam.height << " rays with sun shading" << (shadows ? " and sun shadows" : "")
		          << (interior ? " under the interior rule" : "") << " in " << hmrm_last_kernel_ms() << " ms (kernel)\n";
	} else if (shadows && want_dev <= 1 && aa == 1) {
		hmrm_sun sun;
		hmrm_config_get_sun(cfg, &sun);
		rc = hmrm_render_lit(scene, &cam, &sun, framebuf.data(), (size_t)cam.width * 4);
		if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
			std::cerr << hmrm_last_error() << "\n";
			return 1;
		}
		if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
		std::cout << "rendered " << (long long)cam.width * cam.height << " rays with sun shadows" << (interior ? " under the interior rule" : "")
		          << " in " << hmrm_last_kernel_ms() << " ms (kernel)\n";
	} else if (interior && want_dev <= 1 && aa == 1) {
		rc = hmrm_render_interior(scene, &cam, framebuf.data(), (size_t)cam.width * 4);
		if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
			std::cerr << hmrm_last_error() << "\n";
			return 1;
		}
		if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
		std::cout << "rendered " << (long long)cam.width * cam.height << " rays under the interior rule in " << hmrm_last_kernel_ms()
		          << " ms (kernel)\n";
	} else if (want_dev > 1 && aa == 1) {
		// `devices n`: the frame's 16-row bands are dealt out over n GPUs (BASELINE config C4)
		std::vector<hmrm_scene *> scenes(1, scene);
		for (int d = 1; d < want_dev && rc == HMRM_OK; ++d) {
			hmrm_scene *extra = NULL;
			rc = hmrm_set_device(d % visible_dev);
			if (rc == HMRM_OK) rc = hmrm_config_create_scene(cfg, &extra);
			if (rc == HMRM_OK) scenes.push_back(extra);
		}
		if (rc == HMRM_OK) rc = hmrm_render_multi(scenes.data(), (int32_t)scenes.size(), &cam, framebuf.data(), (size_t)cam.width * 4);
		for (size_t i = 1; i < scenes.size(); ++i) hmrm_scene_destroy(scenes[i]);
		if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
			std::cerr << hmrm_last_error() << "\n";
			return 1;
		}
		if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
		std::cout << "rendered " << (long long)cam.width * cam.height << " rays on " << want_dev << " devices\n";
	} else {
		hmrm_stats stats;
		rc = hmrm_render_aa(scene, &cam, aa, framebuf.data(), (size_t)cam.width * 4, &stats);
		if (rc != HMRM_OK && rc != HMRM_E_NOTERM) {
			std::cerr << hmrm_last_error() << "\n";
			return 1;
		}
		if (rc == HMRM_E_NOTERM) std::cerr << "WARNING: " << hmrm_last_error() << "\n";
		std::cout << "rendered " << stats.rays << " rays, " << stats.steps << " ray-steps, " << stats.hits
		          << " hits in " << hmrm_last_kernel_ms() << " ms (kernel)\n";
	}

	std::string path = hmrm_config_output_path(cfg);
	if (path.empty()) {
		std::time_t seconds = std::time(NULL);
		if (seconds == (std::time_t)(-1)) {
			std::cerr << "Failed to get time for screenshot. Screenshot NOT saved.\n";
			return 1;
		}
		mkdir("screenshots", 0777);
		std::stringstream ss;
		ss << "screenshots/hmap_" << seconds << ".png";
		path = ss.str();
	}
	int wrc;
	if (ends_with(path, ".ppm") || ends_with(path, ".pnm"))
		wrc = hmrm_write_ppm(path.c_str(), cam.width, cam.height, 4, framebuf.data(), (size_t)cam.width * 4);
	else
		wrc = hmrm_write_png(path.c_str(), cam.width, cam.height, 4, framebuf.data(), (size_t)cam.width * 4);
	if (wrc != HMRM_OK)
		std::cerr << "Failed to write screenshot to " << path << "\n";
	else
		std::cout << "Saved screenshot at " << path << "\n";
	if (wrc == HMRM_OK && !write_views(cfg, scene, interior)) wrc = HMRM_E_IO;
	if (wrc == HMRM_OK && !write_range_map(cfg, scene, cam, interior)) wrc = HMRM_E_IO;
	if (wrc == HMRM_OK && !write_sun_map(cfg, scene, cam, shading, shadows)) wrc = HMRM_E_IO;
	if (wrc == HMRM_OK && !write_sky_map(cfg, scene, cam)) wrc = HMRM_E_IO;

	hmrm_scene_destroy(scene);
	hmrm_config_destroy(cfg);
	return wrc == HMRM_OK ? 0 : 1;
}
