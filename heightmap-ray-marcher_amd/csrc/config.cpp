// config.cpp -- whitespace-token config grammar of the reference
// (main/hmap.cpp:309-520).  The stream is consumed with the same
// `input >> value` extractions, so malformed numbers behave as there: the
// stream's failbit ends the token loop and validation runs on what was read.
// Every option is echoed (Print* functions, :197-302) into `log`; unknown keys
// give the reference's WARNING line (:487) in `warn`.
//
// The grammar is data here: one table row per key -- what it reads, what it
// touches, how it is echoed -- instead of a chain of comparisons.
//
// Additive keys, not in the reference (it switches projection with the 1/2/3
// keys at run time, :851-868, and only ever writes PNG):
//   projection perspective|spherical|orthographic   (or 1|2|3)
//   output <path>                                   (.png or .ppm)
//   record orbit|off, devices n, sampling nearest|bilinear, heights f64|f32, antialias 1|2|4|8, interior on|off,
//   shadows on|off, sun_dir x y z, shadow_ambient n, shadow_step_dist v, shadow_max_steps n
//   shading on|off, sun_scope single|all, sky_light on|off, baked_light off|sun|sky
//   water on|off, water_level v, water_reflectivity n, water_color r g b, water_step_dist v, water_max_steps n,
//   water_scope frame|all, water_light off|sun
//   haze on|off, haze_start v, haze_far v, haze_law linear|exp|exp2, haze_density v, haze_color r g b, haze_sky on|off,
//   haze_entries n
//   view x y z hang vang (repeatable, at most 64), views_output <prefix>   (the CLI's view batch, hmrm_render_views)
//   sun_map <path.png>, sun_map_lift v                (the whole map's light map, hmrm_cell_map, written by the CLI)
//   sky_map <path.png>, sky_map_rings r n             (the whole map's sky-view map, hmrm_cell_map_sum, written by the CLI)
//   range_map <path.pfm>                              (the camera's range plane, hmrm_render_geometry, written by the CLI)
#include "config.hpp"

#include <cmath>
#include <cstring>

namespace hmrm {

namespace {

// main/hmap.cpp:131-137
double degrees_to_rads(double degrees) { return (degrees / 180.0) * M_PI; }
double rads_to_degrees(double rads) { return (rads / M_PI) * 180.0; }

// What a key's handler may report: nothing, or the message the reference prints before std::exit(1).
using Handler = void (*)(Config &c, std::istream &in, const char *key, std::string *die);

// ---- generic rows ----
template <auto Member>
void scalar(Config &c, std::istream &in, const char *key, std::string *) {
	in >> c.*Member;
	c.log << key << " " << c.*Member << "\n";
}
// ... that also invalidate the converted heights (should_update_heightmap, :401-440)
template <auto Member>
void height_scalar(Config &c, std::istream &in, const char *key, std::string *die) {
	scalar<Member>(c, in, key, die);
	c.heightmap_dirty = true;
}
// angles are given in degrees and kept in radians; the echo converts back (:367-384)
template <auto Member>
void angle(Config &c, std::istream &in, const char *key, std::string *) {
	double deg = 0.0; // (a key at the very end of a stream extracts nothing: the reference reads an uninitialised local there)
	in >> deg;
	c.*Member = degrees_to_rads(deg);
	c.log << key << " " << rads_to_degrees(c.*Member) << "\n";
}
template <int Axis>
void position_axis(Config &c, std::istream &in, const char *key, std::string *) {
	in >> c.cam_pos[Axis];
	c.log << key << " " << c.cam_pos[Axis] << "\n";
}
// a word out of a short list -> an integer setting; an unknown word warns and leaves the setting alone
struct Word { const char *text; int value; };
template <size_t N>
bool pick(std::istream &in, const Word (&words)[N], int *out, std::string *seen) {
	in >> *seen;
	for (const Word &w : words)
		if (*seen == w.text) {
			*out = w.value;
			return true;
		}
	return false;
}

// ---- the rows that do more ----
void echo_lum(Config &c) { c.log << "lum " << c.lum_r << " " << c.lum_g << " " << c.lum_b << "\n"; }

template <int Comp>
void map_image(Config &c, std::istream &in, const char *key, std::string *die) {
	std::string &path = Comp == 3 ? c.heightmap_path : c.colormap_path;
	bool &have = Comp == 3 ? c.have_heightmap : c.have_colormap;
	in >> path;
	std::string err;
	Image img;
	if (!load_image_file(path.c_str(), Comp, &img, &err)) { // stbi_load(path, .., req_comp), :320-329 / :341-350
		have = false;
		*die = std::string("Failed to load image for ") + key + " from " + path + " (" + err + ")";
		return;
	}
	(Comp == 3 ? c.heightmap : c.colormap) = std::move(img);
	have = true;
	if (Comp == 3) c.heightmap_dirty = true;
	c.log << key << " " << path << "\n";
}

void print_all(Config &c, std::istream &, const char *key, std::string *) { // PrintAllOptions, :282-302
	c.log << key << "\n"
	      << "heightmap " << c.heightmap_path << "\n"
	      << "colormap " << c.colormap_path << "\n"
	      << "resolution " << c.screen_width << " " << c.screen_height << "\n"
	      << "hfov " << rads_to_degrees(c.hfov) << "\n"
	      << "hang " << rads_to_degrees(c.hang) << "\n"
	      << "vang " << rads_to_degrees(c.vang) << "\n"
	      << "pos " << c.cam_pos[0] << " " << c.cam_pos[1] << " " << c.cam_pos[2] << "\n"
	      << "min_height " << c.min_height << "\n"
	      << "max_height " << c.max_height << "\n";
	echo_lum(c);
	c.log << "grid_width " << c.grid_width << "\n"
	      << "ortho_width " << c.ortho_width << "\n"
	      << "step_dist " << c.step_dist << "\n"
	      << "bg_color " << (int)c.bg_r << " " << (int)c.bg_g << " " << (int)c.bg_b << "\n"
	      << "cycle " << c.cycle_period << "\n"
	      << "mouse_sens " << c.mouse_sens << "\n"
	      << "scroll_sens " << c.scroll_sens << "\n"
	      << "move " << c.move_speed << "\n"
	      << "recording_frame_count " << c.recording_frame_count << "\n";
}

void resolution(Config &c, std::istream &in, const char *key, std::string *) {
	in >> c.screen_width >> c.screen_height;
	c.log << key << " " << c.screen_width << " " << c.screen_height << "\n";
}

void position(Config &c, std::istream &in, const char *key, std::string *) {
	in >> c.cam_pos[0] >> c.cam_pos[1] >> c.cam_pos[2];
	c.log << key << " " << c.cam_pos[0] << " " << c.cam_pos[1] << " " << c.cam_pos[2] << "\n";
}

template <bool Normalise>
void lum_weights(Config &c, std::istream &in, const char *, std::string *) {
	double w[3] = {0.0, 0.0, 0.0};
	in >> w[0] >> w[1] >> w[2];
	const double total = Normalise ? w[0] + w[1] + w[2] : 1.0; // lum_norm divides by the sum (:417-427)
	c.lum_r = Normalise ? w[0] / total : w[0];
	c.lum_g = Normalise ? w[1] / total : w[1];
	c.lum_b = Normalise ? w[2] / total : w[2];
	c.heightmap_dirty = true;
	echo_lum(c);
}

void background(Config &c, std::istream &in, const char *key, std::string *) {
	int v[3] = {0, 0, 0}; // read as ints, then narrowed (:456-461)
	in >> v[0] >> v[1] >> v[2];
	c.bg_r = (uint8_t)v[0];
	c.bg_g = (uint8_t)v[1];
	c.bg_b = (uint8_t)v[2];
	c.log << key << " " << (int)c.bg_r << " " << (int)c.bg_g << " " << (int)c.bg_b << "\n";
}

// -- additive keys --
void projection(Config &c, std::istream &in, const char *key, std::string *) {
	static const Word words[] = {{"perspective", 1}, {"1", 1}, {"spherical", 2}, {"2", 2}, {"orthographic", 3}, {"3", 3}};
	static const char *const names[] = {"", "perspective", "spherical", "orthographic"};
	std::string seen;
	if (!pick(in, words, &c.image_plane, &seen)) c.warn << "WARNING: Unknown projection: " << seen << "\n";
	c.log << key << " " << names[c.image_plane] << "\n";
}

void sampling_mode(Config &c, std::istream &in, const char *key, std::string *) { // quality mode; hmap.cpp always samples the nearest cell
	static const Word words[] = {{"nearest", 0}, {"bilinear", 1}};
	std::string seen;
	if (!pick(in, words, &c.sampling, &seen)) c.warn << "WARNING: Unknown sampling: " << seen << "\n";
	c.log << key << " " << (c.sampling == 1 ? "bilinear" : "nearest") << "\n";
}

void heights_type(Config &c, std::istream &in, const char *key, std::string *) { // float thresholds for the nearest-cell lookup (not parity)
	static const Word words[] = {{"f64", 0}, {"f32", 1}};
	std::string seen;
	int f32 = 0;
	if (!pick(in, words, &f32, &seen)) c.warn << "WARNING: Unknown heights type: " << seen << "\n";
	else if (f32) c.sampling = 2;
	else if (c.sampling == 2) c.sampling = 0;
	c.log << key << " " << (c.sampling == 2 ? "f32" : "f64") << "\n";
}

void device_count_key(Config &c, std::istream &in, const char *key, std::string *) { // multi-GPU recording (BASELINE config C5)
	in >> c.devices;
	if (c.devices < 0) c.devices = 1;
	c.log << key << " " << c.devices << "\n";
}

void record_mode_key(Config &c, std::istream &in, const char *key, std::string *) { // programmatic animation (hmap.cpp:907-926 is a stub)
	static const Word words[] = {{"off", 0}, {"orbit", 1}};
	std::string seen;
	if (!pick(in, words, &c.record_mode, &seen)) c.warn << "WARNING: Unknown record mode: " << seen << "\n";
	c.log << key << " " << (c.record_mode == 1 ? "orbit" : "off") << "\n";
}

void antialias_key(Config &c, std::istream &in, const char *key, std::string *) { // n x n box-filtered samples per pixel
	static const Word words[] = {{"1", 1}, {"2", 2}, {"4", 4}, {"8", 8}};
	std::string seen;
	if (!pick(in, words, &c.antialias, &seen)) c.warn << "WARNING: Unknown antialias: " << seen << "\n";
	c.log << key << " " << c.antialias << "\n";
}

void interior_key(Config &c, std::istream &in, const char *key, std::string *) { // a camera inside the box sees the terrain (hmrm_render_interior)
	static const Word words[] = {{"on", 1}, {"1", 1}, {"off", 0}, {"0", 0}};
	std::string seen;
	if (!pick(in, words, &c.interior, &seen)) c.warn << "WARNING: Unknown interior: " << seen << "\n";
	c.log << key << " " << (c.interior ? "on" : "off") << "\n";
}

// sun shadows of the single frame (hmrm_render_lit)
void shadows_key(Config &c, std::istream &in, const char *key, std::string *) {
	static const Word words[] = {{"on", 1}, {"1", 1}, {"off", 0}, {"0", 0}};
	std::string seen;
	if (!pick(in, words, &c.shadows, &seen)) c.warn << "WARNING: Unknown shadows: " << seen << "\n";
	c.log << key << " " << (c.shadows ? "on" : "off") << "\n";
}

// diffuse sun shading of the single frame (hmrm_render_shaded)
void shading_key(Config &c, std::istream &in, const char *key, std::string *) {
	static const Word words[] = {{"on", 1}, {"1", 1}, {"off", 0}, {"0", 0}};
	std::string seen;
	if (!pick(in, words, &c.shading, &seen)) c.warn << "WARNING: Unknown shading: " << seen << "\n";
	c.log << key << " " << (c.shading ? "on" : "off") << "\n";
}

// the single frame lit by the sky directions of sky_map_rings (hmrm_render_lit_sum)
void sky_light_key(Config &c, std::istream &in, const char *key, std::string *) {
	static const Word words[] = {{"on", 1}, {"1", 1}, {"off", 0}, {"0", 0}};
	std::string seen;
	if (!pick(in, words, &c.sky_light, &seen)) c.warn << "WARNING: Unknown sky_light: " << seen << "\n";
	c.log << key << " " << (c.sky_light ? "on" : "off") << "\n";
}

// the frames under a light plane baked once (hmrm_scene_bake_light, hmrm_render_baked)
void baked_light_key(Config &c, std::istream &in, const char *key, std::string *) {
	static const Word words[] = {{"off", 0}, {"sun", 1}, {"sky", 2}};
	std::string seen;
	if (!pick(in, words, &c.baked_light, &seen)) c.warn << "WARNING: Unknown baked_light: " << seen << "\n";
	c.log << key << " " << (c.baked_light == 1 ? "sun" : c.baked_light == 2 ? "sky" : "off") << "\n";
}

// mirror reflections on flat water in the single frame (hmrm_render_water)
void water_key(Config &c, std::istream &in, const char *key, std::string *) {
	static const Word words[] = {{"on", 1}, {"1", 1}, {"off", 0}, {"0", 0}};
	std::string seen;
	if (!pick(in, words, &c.water, &seen)) c.warn << "WARNING: Unknown water: " << seen << "\n";
	c.log << key << " " << (c.water ? "on" : "off") << "\n";
}

void water_reflectivity_key(Config &c, std::istream &in, const char *key, std::string *) { // the mirror pixel's share, of 255
	long long v = -1;
	in >> v;
	if (!in || v < 0 || v > 255) c.warn << "WARNING: water_reflectivity must be 0..255\n";
	else c.water_reflectivity = (int)v;
	c.log << key << " " << c.water_reflectivity << "\n";
}

void water_color_key(Config &c, std::istream &in, const char *key, std::string *) { // the water's own colour instead of the primary pixel
	long long v[3] = {-1, -1, -1};
	in >> v[0] >> v[1] >> v[2];
	if (!in || v[0] < 0 || v[0] > 255 || v[1] < 0 || v[1] > 255 || v[2] < 0 || v[2] > 255) c.warn << "WARNING: water_color must be three values 0..255\n";
	else {
		for (int k = 0; k < 3; ++k) c.water_color[k] = (int)v[k];
		c.have_water_color = true;
	}
	c.log << key << " " << c.water_color[0] << " " << c.water_color[1] << " " << c.water_color[2] << "\n";
}

void water_step_dist_key(Config &c, std::istream &in, const char *key, std::string *) {
	in >> c.water_step_dist;
	c.have_water_step_dist = true;
	c.log << key << " " << c.water_step_dist << "\n";
}

void water_max_steps_key(Config &c, std::istream &in, const char *key, std::string *) { // 0 = no limit
	long long v = -1;
	in >> v;
	if (!in || v < 0 || v > 0xffffffffll) c.warn << "WARNING: water_max_steps must be 0..4294967295\n";
	else c.water_max_steps = v;
	c.log << key << " " << c.water_max_steps << "\n";
}

// which frames water applies to: the plain single frame, or antialiased, recorded and baked-light ones too
void water_scope_key(Config &c, std::istream &in, const char *key, std::string *) {
	static const Word words[] = {{"frame", 0}, {"all", 1}};
	std::string seen;
	if (!pick(in, words, &c.water_scope, &seen)) c.warn << "WARNING: Unknown water_scope: " << seen << "\n";
	c.log << key << " " << (c.water_scope ? "all" : "frame") << "\n";
}

// what lights a water frame beside `shadows` / `shading`: nothing (water is ignored there), or the sun (hmrm_render_water_lit)
void water_light_key(Config &c, std::istream &in, const char *key, std::string *) {
	static const Word words[] = {{"off", 0}, {"sun", 1}};
	std::string seen;
	if (!pick(in, words, &c.water_light, &seen)) c.warn << "WARNING: Unknown water_light: " << seen << "\n";
	c.log << key << " " << (c.water_light ? "sun" : "off") << "\n";
}

// distance fog in the single frame (hmrm_render_haze)
void haze_key(Config &c, std::istream &in, const char *key, std::string *) {
	static const Word words[] = {{"on", 1}, {"1", 1}, {"off", 0}, {"0", 0}};
	std::string seen;
	if (!pick(in, words, &c.haze, &seen)) c.warn << "WARNING: Unknown haze: " << seen << "\n";
	c.log << key << " " << (c.haze ? "on" : "off") << "\n";
}

void haze_sky_key(Config &c, std::istream &in, const char *key, std::string *) { // the pixels that did not hit at the table's last entry
	static const Word words[] = {{"on", 1}, {"1", 1}, {"off", 0}, {"0", 0}};
	std::string seen;
	if (!pick(in, words, &c.haze_sky, &seen)) c.warn << "WARNING: Unknown haze_sky: " << seen << "\n";
	c.log << key << " " << (c.haze_sky ? "on" : "off") << "\n";
}

void haze_law_key(Config &c, std::istream &in, const char *key, std::string *) { // the table's law, hmrm_haze_table's
	static const Word words[] = {{"linear", 0}, {"exp", 1}, {"exp2", 2}};
	std::string seen;
	if (!pick(in, words, &c.haze_law, &seen)) c.warn << "WARNING: Unknown haze_law: " << seen << "\n";
	c.log << key << " " << words[c.haze_law].text << "\n";
}

void haze_color_key(Config &c, std::istream &in, const char *key, std::string *) {
	long long v[3] = {-1, -1, -1};
	in >> v[0] >> v[1] >> v[2];
	if (!in || v[0] < 0 || v[0] > 255 || v[1] < 0 || v[1] > 255 || v[2] < 0 || v[2] > 255) c.warn << "WARNING: haze_color must be three values 0..255\n";
	else
		for (int k = 0; k < 3; ++k) c.haze_color[k] = (int)v[k];
	c.log << key << " " << c.haze_color[0] << " " << c.haze_color[1] << " " << c.haze_color[2] << "\n";
}

void haze_entries_key(Config &c, std::istream &in, const char *key, std::string *) { // the table's length
	long long v = -1;
	in >> v;
	if (!in || v < 1 || v > 4096) c.warn << "WARNING: haze_entries must be 1..4096\n";
	else c.haze_entries = (int)v;
	c.log << key << " " << c.haze_entries << "\n";
}

// one more camera of the CLI's view batch (hmrm_render_views): position and the two angles, in the `hang` / `vang` keys' unit
void view_key(Config &c, std::istream &in, const char *key, std::string *) {
	double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
	in >> v[0] >> v[1] >> v[2] >> v[3] >> v[4];
	if ((int)c.views.size() >= kMaxConfigViews) {
		c.warn << "WARNING: too many views\n";
		return;
	}
	c.views.push_back(Config::View{{v[0], v[1], v[2]}, degrees_to_rads(v[3]), degrees_to_rads(v[4])});
	const Config::View &w = c.views.back();
	c.log << key << " " << w.pos[0] << " " << w.pos[1] << " " << w.pos[2] << " " << rads_to_degrees(w.hang) << " " << rads_to_degrees(w.vang) << "\n";
}

// which frames shadows / shading apply to: the plain single frame, or antialiased and recorded ones too
void sun_scope_key(Config &c, std::istream &in, const char *key, std::string *) {
	static const Word words[] = {{"single", 0}, {"all", 1}};
	std::string seen;
	if (!pick(in, words, &c.sun_scope, &seen)) c.warn << "WARNING: Unknown sun_scope: " << seen << "\n";
	c.log << key << " " << (c.sun_scope ? "all" : "single") << "\n";
}

void sun_dir_key(Config &c, std::istream &in, const char *key, std::string *) { // towards the sun, used as given
	in >> c.sun_dir[0] >> c.sun_dir[1] >> c.sun_dir[2];
	c.log << key << " " << c.sun_dir[0] << " " << c.sun_dir[1] << " " << c.sun_dir[2] << "\n";
}

void shadow_ambient_key(Config &c, std::istream &in, const char *key, std::string *) { // what a shadowed pixel keeps, of 255
	long long v = -1;
	in >> v;
	if (!in || v < 0 || v > 255) c.warn << "WARNING: shadow_ambient must be 0..255\n";
	else c.shadow_ambient = (int)v;
	c.log << key << " " << c.shadow_ambient << "\n";
}

void shadow_step_dist_key(Config &c, std::istream &in, const char *key, std::string *) {
	in >> c.shadow_step_dist;
	c.have_shadow_step_dist = true;
	c.log << key << " " << c.shadow_step_dist << "\n";
}

void shadow_max_steps_key(Config &c, std::istream &in, const char *key, std::string *) { // 0 = no limit
	long long v = -1;
	in >> v;
	if (!in || v < 0 || v > 0xffffffffll) c.warn << "WARNING: shadow_max_steps must be 0..4294967295\n";
	else c.shadow_max_steps = v;
	c.log << key << " " << c.shadow_max_steps << "\n";
}

void sky_map_rings_key(Config &c, std::istream &in, const char *key, std::string *) { // rings x directions per ring of the sky map
	long long r = 0, n = 0;
	in >> r >> n;
	if (!in || r < 1 || n < 1 || r > 256 || n > 256 || r * n > 256) c.warn << "WARNING: sky_map_rings must give 1..256 directions\n";
	else {
		c.sky_map_rings = (int)r;
		c.sky_map_per_ring = (int)n;
	}
	c.log << key << " " << c.sky_map_rings << " " << c.sky_map_per_ring << "\n";
}

struct Row { const char *key; Handler apply; };
const Row kGrammar[] = {
	// the reference's 27 keys (main/hmap.cpp:314-488)
	{"heightmap", map_image<3>},
	{"colormap", map_image<4>},
	{"print", print_all},
	{"resolution", resolution},
	{"hfov", angle<&Config::hfov>},
	{"hang", angle<&Config::hang>},
	{"vang", angle<&Config::vang>},
	{"pos", position},
	{"pos_x", position_axis<0>},
	{"pos_y", position_axis<1>},
	{"pos_z", position_axis<2>},
	{"min_height", height_scalar<&Config::min_height>},
	{"max_height", height_scalar<&Config::max_height>},
	{"lum", lum_weights<false>},
	{"lum_norm", lum_weights<true>},
	{"lum_r", height_scalar<&Config::lum_r>},
	{"lum_g", height_scalar<&Config::lum_g>},
	{"lum_b", height_scalar<&Config::lum_b>},
	{"grid_width", scalar<&Config::grid_width>},
	{"ortho_width", scalar<&Config::ortho_width>},
	{"step_dist", scalar<&Config::step_dist>},
	{"bg_color", background},
	{"cycle", scalar<&Config::cycle_period>},
	{"mouse_sens", scalar<&Config::mouse_sens>},
	{"scroll_sens", scalar<&Config::scroll_sens>},
	{"move", scalar<&Config::move_speed>},
	{"recording_frame_count", scalar<&Config::recording_frame_count>},
	// additive
	{"projection", projection},
	{"output", scalar<&Config::output_path>},
	{"sampling", sampling_mode},
	{"heights", heights_type},
	{"devices", device_count_key},
	{"record", record_mode_key},
	{"antialias", antialias_key},
	{"interior", interior_key},
	{"shadows", shadows_key},
	{"shading", shading_key},
	{"sky_light", sky_light_key},
	{"baked_light", baked_light_key},
	{"sun_scope", sun_scope_key},
	{"sun_dir", sun_dir_key},
	{"shadow_ambient", shadow_ambient_key},
	{"shadow_step_dist", shadow_step_dist_key},
	{"shadow_max_steps", shadow_max_steps_key},
	{"sun_map", scalar<&Config::sun_map_path>},
	{"sun_map_lift", scalar<&Config::sun_map_lift>},
	{"sky_map", scalar<&Config::sky_map_path>},
	{"sky_map_rings", sky_map_rings_key},
	{"range_map", scalar<&Config::range_map_path>},
	{"water", water_key},
	{"water_scope", water_scope_key},
	{"water_light", water_light_key},
	{"water_level", scalar<&Config::water_level>},
	{"water_reflectivity", water_reflectivity_key},
	{"water_color", water_color_key},
	{"water_step_dist", water_step_dist_key},
	{"water_max_steps", water_max_steps_key},
	{"haze", haze_key},
	{"haze_start", scalar<&Config::haze_start>},
	{"haze_far", scalar<&Config::haze_far>},
	{"haze_law", haze_law_key},
	{"haze_density", scalar<&Config::haze_density>},
	{"haze_color", haze_color_key},
	{"haze_sky", haze_sky_key},
	{"haze_entries", haze_entries_key},
	{"view", view_key},
	{"views_output", scalar<&Config::views_output>},
};

} // namespace

Config::Config() {
	hfov = M_PI / 2.0;  // :35
	hang = -M_PI / 4.0; // :80
	vang = M_PI / 2.0;  // :85
}

bool Config::consume(std::istream &input, std::string *fatal) {
	auto die = [&](const std::string &msg) {
		warn << msg << "\n";
		if (fatal) *fatal = msg;
		return false;
	};
	std::string token;
	while (input >> token) {
		const Row *row = nullptr;
		for (const Row &r : kGrammar)
			if (token == r.key) row = &r;
		if (!row) {
			warn << "WARNING: Unknown identifier: " << token << "\n"; // :487
			continue;
		}
		std::string fatal_msg;
		row->apply(*this, input, row->key, &fatal_msg);
		if (!fatal_msg.empty()) return die(fatal_msg);
	}
	// end of stream: both maps present and of one size (:493-515)
	if (!have_heightmap) return die("Must specify heightmap in config");
	if (!have_colormap) return die("Must specify colormap in config");
	if (heightmap.w != colormap.w || heightmap.h != colormap.h) {
		std::ostringstream m;
		m << "heightmap dimensions (" << heightmap.w << "x" << heightmap.h
		  << ") must match colormap dimensions (" << colormap.w << "x" << colormap.h << ")";
		return die(m.str());
	}
	return true;
}

bool fill_haze_table(int law, double density, int n, unsigned char *out) {
	if (law < 0 || law > 2 || n < 1 || n > 4096 || !out) return false;
	for (int i = 0; i < n; ++i) {
		const double x = ((double)i + 0.5) / (double)n;
		const double dx = density * x;
		const double t = law == 0 ? 1.0 - x : (law == 1 ? std::exp(-density * x) : std::exp(-(dx * dx)));
		const int v = (int)(255.0 * (1.0 - t) + 0.5);
		out[i] = (unsigned char)(v > 255 ? 255 : v);
	}
	return true;
}

} // namespace hmrm
