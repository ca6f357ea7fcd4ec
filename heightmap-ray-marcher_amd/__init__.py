"""heightmap-ray-marcher_amd -- MI355X-native (gfx950) heightmap ray marcher.

Host-side mirror of the reference's interface for the hot path only
(config text in -> RGBA8 framebuffer / PNG out) over the C ABI of libhmrm.so
(include/hmrm.h).  Import with importlib (the directory name has hyphens):

    hmrm = importlib.import_module("heightmap-ray-marcher_amd")
"""
from .lib import (  # noqa: F401
    Camera, Config, HmrmError, Scene, SceneParams, Stats,
    Ray, RayHit, TraceParams, SegmentParams, Sun, Water, CellMapParams, CellRect, GeometryPlanes, LightPlanes, MAP_TOWARDS_POINT, MAP_WEIGHT, MAP_DIFFUSE, MAP_NO_SHADOWS, RAY_END, TRACE_INTERIOR, SHADE_DIFFUSE, SHADE_NO_SHADOWS, RAY_DTYPE, RAY_HIT_DTYPE, RAY_MISS, RAY_HIT, RAY_CAPPED, MAX_RAYS, as_rays,
    PERSPECTIVE, SPHERICAL, ORTHOGRAPHIC, NEAREST, BILINEAR, NEAREST_F32,
    HMRM_OK, HMRM_E_ARG, HMRM_E_IO, HMRM_E_IMAGE, HMRM_E_CONFIG, HMRM_E_DEVICE, HMRM_E_NOTERM,
    EXPORTED_SYMBOLS, LIB_PATH, NO_PROBE, AA_FACTORS, aa_flags,
    band_local_rows, debug_frame, degrees_to_rads, device_count, image_load, image_load_memory, kernel_src_sha,
    last_error, mip_layout, level_state, calibrate, pick_kernel, plan_order, rcp_error, orbit_camera, orbit_frame_owner, png_encode, record_orbit, record_orbit_multi, record_orbit_shaded, record_orbit_baked, record_orbit_water, LIGHT_U8, LIGHT_U16, WATER_OWN_COLOR, WATER_BAKED, Haze, HAZE_SKY, HAZE_LINEAR, HAZE_EXP, HAZE_EXP2, MAX_HAZE_ENTRIES, haze_table, MAX_VIEWS, camera_array, views_tables, shade_flags, map_flags, sky_directions, render_multi, set_device, write_png, write_ppm, write_pfm,
)
from . import synth  # noqa: F401
