// config.hpp -- the reference's config-file interface (main/hmap.cpp:28-112
// globals + :309-520 ConsumeConfigStream), as an object instead of globals.
#pragma once
#include <cstdint>
#include <istream>
#include <sstream>
#include <string>
#include <vector>

#include "image_io.hpp"

namespace hmrm {

struct Config {
	// defaults = the initialisers at main/hmap.cpp:31-112
	int screen_width = 800, screen_height = 600;
	double hfov; // M_PI / 2.0, set in the constructor with hang (-M_PI/4) and vang (M_PI/2)
	double min_height = 0.0, max_height = 10.0;
	double lum_r = 0.299, lum_g = 0.587, lum_b = 0.114;
	std::string heightmap_path, colormap_path;
	Image heightmap; // RGB8  (stbi_load req_comp 3)
	Image colormap;  // RGBA8 (stbi_load req_comp 4)
	bool have_heightmap = false, have_colormap = false;
	double grid_width = 0.05;
	double step_dist = 5.0 * 0.05;
	int cycle_period = 47;
	double cam_pos[3] = {-5.0, 5.0, 0.0};
	double hang, vang;
	double mouse_sens = 1.0, scroll_sens = 1.0, move_speed = 0.05;
	double ortho_width = 2.0 * 0.05;
	int recording_frame_count = 200;
	int image_plane = 1; // IMAGEPLANE_PERSPECTIVE
	uint8_t bg_r = 0, bg_g = 0, bg_b = 0;
	// additive (north_star): output file; empty = caller decides
	std::string output_path;
	// additive: `record orbit` renders recording_frame_count frames of an orbit sweep
	int record_mode = 0;
	// additive: `devices n` -- GPUs the recording is sharded over, frame k on device k mod n (0 = all visible)
	int devices = 1;
	// additive: `sampling nearest|bilinear` (nearest = the reference's truncating lookup), `heights f32` (= 2)
	int sampling = 0;
	// additive: `antialias n` -- hmrm_render_aa's factor (1 = off, 2, 4, 8)
	int antialias = 1;
	// additive: `interior on|off|1|0` -- the CLI's single frame under the interior rule (hmrm_render_interior)
	int interior = 0;
	// additive: sun shadows of the CLI's single frame (hmrm_render_lit): `shadows on|off|1|0`, `sun_dir x y z` (towards the sun,
	// used as given), `shadow_ambient 0..255`, `shadow_step_dist v` (absent: the camera's step_dist), `shadow_max_steps n`
	int shadows = 0;
	// additive: `shading on|off|1|0` -- diffuse sun shading of that frame (hmrm_render_shaded), with the shadow rays when
	// `shadows on`; the sun is the same
	int shading = 0;
	// additive: `sky_light on|off|1|0` -- that frame lit by the sky instead of the sun (hmrm_render_lit_sum over the directions of
	// `sky_map_rings`), diffuse with `shading on`; the shadow march's keys are the sun's, `sun_dir` is not used
	int sky_light = 0;
	// additive: `baked_light off|sun|sky` -- 0, 1, 2: the CLI bakes the scene's light plane once before its frames (hmrm_scene_bake_light:
	// the sun_map's light under `sun_dir`, or the sky_map's count over `sky_map_rings`) and renders them as baked frames (hmrm_render_baked)
	int baked_light = 0;
	// additive: water of the CLI's single frame (hmrm_render_water): `water on|off|1|0`, `water_level v` (a hit at or below it
	// mirrors), `water_reflectivity 0..255`, `water_color r g b` (the water's own colour: sets HMRM_WATER_OWN_COLOR),
	// `water_step_dist v` (absent: the camera's step_dist), `water_max_steps n`
	int water = 0;
	double water_level = 0.0;
	int water_reflectivity = 128;
	int water_color[3] = {0, 0, 0};
	bool have_water_color = false;
	double water_step_dist = 0.0;
	bool have_water_step_dist = false;
	long long water_max_steps = 0;
	// additive: `water_scope frame|all` -- 0: water applies to the plain single frame only; 1: also with `antialias n` > 1
	// (hmrm_render_water_aa), to `record orbit` (hmrm_record_orbit_water) and under `baked_light` (HMRM_WATER_BAKED)
	int water_scope = 0;
	// additive: `water_light off|sun` -- 0: `water on` beside `shadows` / `shading` is ignored; 1: that single frame is the sun-lit
	// water frame (hmrm_render_water_lit) -- one device, `antialias 1`, no `baked_light`
	int water_light = 0;
	// additive: `sun_scope single|all` -- 0: shadows / shading apply to the plain single frame only; 1: also with `antialias n` > 1
	// (hmrm_render_shaded_aa) and to `record orbit` (hmrm_record_orbit_shaded)
	int sun_scope = 0;
	double sun_dir[3] = {0.5, 0.5, 0.70710678118654757};
	int shadow_ambient = 128;
	double shadow_step_dist = 0.0;
	bool have_shadow_step_dist = false;
	long long shadow_max_steps = 0;
	// additive: `sun_map <path.png>` -- the CLI also writes the whole map's light map (hmrm_cell_map with HMRM_MAP_WEIGHT under the
	// same sun) there, one byte per cell; `sun_map_lift v` -- how far above the surface its rays start
	std::string sun_map_path;
	double sun_map_lift = 0.0;
	// additive: `sky_map <path.png>` -- the CLI also writes the whole map's sky-view map there (hmrm_cell_map_sum in status mode
	// over hmrm_sky_directions(r, n), scaled to a byte); `sky_map_rings r n` -- the directions, r * n in 1 .. 256
	std::string sky_map_path;
	int sky_map_rings = 4, sky_map_per_ring = 16;
	// additive: `range_map <path.pfm>` -- the CLI also writes the range plane of the configured camera's geometry frame
	// (hmrm_render_geometry; under the interior rule with `interior on`) there as a one-component portable float map
	std::string range_map_path;
	// additive: haze of the CLI's single frame (hmrm_render_haze): `haze on|off|1|0`, `haze_start v` and `haze_far v` (the ranges
	// of the table's first and last entry: scale = entries / (far - start)), `haze_law linear|exp|exp2` and `haze_density v`
	// (hmrm_haze_table's), `haze_color r g b`, `haze_sky on|off|1|0` (HMRM_HAZE_SKY), `haze_entries n` (1 .. 4096)
	int haze = 0;
	double haze_start = 0.0, haze_far = 1000.0;
	int haze_law = 1;
	double haze_density = 3.0;
	int haze_color[3] = {200, 210, 220};
	int haze_sky = 0;
	int haze_entries = 256;
	// additive: `view x y z hang vang` (repeatable, at most kMaxConfigViews lines; angles in the unit of the `hang` and `vang` keys,
	// degrees, kept in radians) -- one more camera of the CLI's view batch (hmrm_render_views), everything else from the main
	// camera; a line beyond the limit warns "WARNING: too many views" and is dropped -- and `views_output <prefix>`, echoed like
	// `output`: the batch's frames go to <prefix>000.png, <prefix>001.png, ...
	struct View { double pos[3], hang, vang; };
	std::vector<View> views;
	std::string views_output;

	bool heightmap_dirty = false; // should_update_heightmap, sticky until taken
	std::ostringstream log;       // what the reference prints to stdout
	std::ostringstream warn;      // what the reference prints to stderr

	Config();

	// Returns true on success; on a condition where the reference calls
	// std::exit(1) returns false with the stderr text in *fatal (also appended
	// to `warn`).
	bool consume(std::istream &input, std::string *fatal);

};

constexpr int kMaxConfigViews = 64;

// hmrm_haze_table (hmrm.h): out[i] = min(255, (int)(255 * (1 - T) + 0.5)), x = (i + 0.5) / n, T by `law` with libm's exp.
// False for an unknown law, n outside 1 .. 4096 or a null `out`.
bool fill_haze_table(int law, double density, int n, unsigned char *out);

} // namespace hmrm
