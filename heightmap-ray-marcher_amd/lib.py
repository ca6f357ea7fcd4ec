"""ctypes binding of libhmrm.so (C ABI: include/hmrm.h).

This module is plumbing only: it loads the in-tree shared library built from
csrc/ and exposes thin wrappers.  There is NO Python or CPU fallback for the hot
path -- if the library is missing, import fails loudly; if no GPU is usable, the
render calls raise HmrmError(HMRM_E_DEVICE).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhmrm.so")

HMRM_OK = 0
HMRM_E_ARG, HMRM_E_IO, HMRM_E_IMAGE, HMRM_E_CONFIG, HMRM_E_DEVICE, HMRM_E_NOTERM = -1, -2, -3, -4, -5, -6
PERSPECTIVE, SPHERICAL, ORTHOGRAPHIC = 1, 2, 3
NEAREST, BILINEAR, NEAREST_F32 = 0, 1, 2
_PROJ_NAMES = {"perspective": 1, "spherical": 2, "orthographic": 3}


NO_PROBE = 1  # HMRM_NO_PROBE (hmrm.h)
AA_FACTORS = (1, 2, 4, 8)  # hmrm_render_aa's factors


def aa_flags(n: int) -> int:
    """HMRM_AA(n) (hmrm.h): the antialias factor field of the ticketed calls' flags (0 and 1 mean off)."""
    return (int(n) & 15) << 8


class HmrmError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"hmrm error {code}: {msg}")
        self.code = code
        self.message = msg


class SceneParams(C.Structure):
    """hmrm_scene_params -- defaults are main/hmap.cpp:38-47,65."""
    _fields_ = [("min_height", C.c_double), ("max_height", C.c_double),
                ("lum_r", C.c_double), ("lum_g", C.c_double), ("lum_b", C.c_double),
                ("grid_width", C.c_double)]

    @classmethod
    def make(cls, min_height=0.0, max_height=10.0, lum=(0.299, 0.587, 0.114), grid_width=0.05):
        return cls(min_height, max_height, lum[0], lum[1], lum[2], grid_width)


class Camera(C.Structure):
    """hmrm_camera -- angles in radians; defaults are main/hmap.cpp:31-35,68,75-85,98,107,110-112."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("projection", C.c_int32),
                ("bg_r", C.c_uint8), ("bg_g", C.c_uint8), ("bg_b", C.c_uint8), ("sampling", C.c_uint8),
                ("hfov", C.c_double), ("hang", C.c_double), ("vang", C.c_double),
                ("pos", C.c_double * 3), ("ortho_width", C.c_double), ("step_dist", C.c_double)]

    @classmethod
    def make(cls, width=800, height=600, projection=PERSPECTIVE, hfov=np.pi / 2.0, hang=-np.pi / 4.0,
             vang=np.pi / 2.0, pos=(-5.0, 5.0, 0.0), ortho_width=0.1, step_dist=0.25, bg=(0, 0, 0), sampling=0):
        if isinstance(projection, str):
            projection = _PROJ_NAMES[projection]
        c = cls()
        c.width, c.height, c.projection = int(width), int(height), int(projection)
        c.bg_r, c.bg_g, c.bg_b = (int(v) & 255 for v in bg)
        c.hfov, c.hang, c.vang = float(hfov), float(hang), float(vang)
        c.pos[0], c.pos[1], c.pos[2] = (float(v) for v in pos)
        c.ortho_width, c.step_dist = float(ortho_width), float(step_dist)
        c.sampling = int(sampling)
        return c


class Stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("steps", C.c_uint64), ("hits", C.c_uint64), ("capped", C.c_uint64),
                ("leap_attempts", C.c_uint64), ("leaps", C.c_uint64), ("groups", C.c_uint64),
                ("leaped_steps", C.c_uint64)]


RAY_MISS, RAY_HIT, RAY_CAPPED = 0, 1, 2  # hmrm_ray_hit.status (HMRM_RAY_*)
RAY_END = 3  # ... of hmrm_trace_segments: ended by the ray's own step limit, inside the grid
TRACE_INTERIOR = 1  # hmrm_segment_params.flags (HMRM_TRACE_INTERIOR)
SHADE_DIFFUSE, SHADE_NO_SHADOWS = 1, 2  # hmrm_render_shaded's shade_flags (HMRM_SHADE_*)
LIGHT_U8, LIGHT_U16 = 0, 1  # hmrm_scene_set_light's format (HMRM_LIGHT_*)
MAX_RAYS = 1 << 29  # rays per batch


class Ray(C.Structure):
    """hmrm_ray -- the reference's Ray {pos, dir}; dir is used as given, not normalised."""
    _fields_ = [("pos", C.c_double * 3), ("dir", C.c_double * 3)]


class RayHit(C.Structure):
    """hmrm_ray_hit -- one record per traced ray (hmrm.h)."""
    _fields_ = [("point", C.c_double * 3), ("entry_d", C.c_double), ("steps", C.c_uint32),
                ("cell_x", C.c_int32), ("cell_y", C.c_int32), ("rgba", C.c_uint8 * 4),
                ("status", C.c_uint32), ("reserved", C.c_uint32)]


class TraceParams(C.Structure):
    """hmrm_trace_params"""
    _fields_ = [("step_dist", C.c_double), ("bg_r", C.c_uint8), ("bg_g", C.c_uint8), ("bg_b", C.c_uint8),
                ("sampling", C.c_uint8)]

    @classmethod
    def make(cls, step_dist, bg=(0, 0, 0), sampling=NEAREST):
        return cls(float(step_dist), int(bg[0]) & 255, int(bg[1]) & 255, int(bg[2]) & 255, int(sampling))


class SegmentParams(C.Structure):
    """hmrm_segment_params (24 bytes)"""
    _fields_ = [("step_dist", C.c_double), ("bg_r", C.c_uint8), ("bg_g", C.c_uint8), ("bg_b", C.c_uint8),
                ("sampling", C.c_uint8), ("flags", C.c_uint32), ("max_steps", C.c_uint32), ("reserved", C.c_uint32)]

    @classmethod
    def make(cls, step_dist, bg=(0, 0, 0), sampling=NEAREST, interior=False, max_steps=0):
        return cls(float(step_dist), int(bg[0]) & 255, int(bg[1]) & 255, int(bg[2]) & 255, int(sampling),
                   TRACE_INTERIOR if interior else 0, int(max_steps), 0)


class Sun(C.Structure):
    """hmrm_sun (48 bytes): the sun of Scene.render_lit"""
    _fields_ = [("dir", C.c_double * 3), ("step_dist", C.c_double), ("max_steps", C.c_uint32), ("flags", C.c_uint32),
                ("ambient", C.c_uint8), ("reserved", C.c_uint8 * 7)]

    @classmethod
    def make(cls, dir, step_dist, max_steps=0, ambient=128, interior=False):
        """dir: towards the sun, used as given (not normalised); step_dist in units of |dir|; max_steps: limit of every shadow
        ray (0 = none); ambient 0..255: what a shadowed pixel keeps; interior: the primary rays under the interior rule too."""
        if not 0 <= int(ambient) <= 255:
            raise ValueError("ambient must be 0..255")
        return cls((C.c_double * 3)(*(float(v) for v in dir)), float(step_dist), int(max_steps),
                   TRACE_INTERIOR if interior else 0, int(ambient), (C.c_uint8 * 7)())


assert C.sizeof(Sun) == 48

WATER_OWN_COLOR = 2  # hmrm_water.flags (HMRM_WATER_OWN_COLOR)
WATER_BAKED = 1  # water_mode (HMRM_WATER_BAKED): the water frame under the scene's light plane


class Water(C.Structure):
    """hmrm_water (32 bytes): the water of Scene.render_water"""
    _fields_ = [("level", C.c_double), ("step_dist", C.c_double), ("max_steps", C.c_uint32), ("flags", C.c_uint32),
                ("reflectivity", C.c_uint8), ("color", C.c_uint8 * 3), ("reserved", C.c_uint8 * 4)]

    @classmethod
    def make(cls, level, step_dist, max_steps=0, reflectivity=128, color=None, interior=False):
        """level: a hit whose threshold t <= level is water; step_dist of the mirror march, in units of |dir|; max_steps: limit of
        every mirror ray (0 = none); reflectivity 0..255: the mirror pixel's share; color (r, g, b): the water's own colour
        instead of the primary pixel (HMRM_WATER_OWN_COLOR); interior: the primary rays under the interior rule."""
        if not 0 <= int(reflectivity) <= 255:
            raise ValueError("reflectivity must be 0..255")
        if color is not None and not all(0 <= int(v) <= 255 for v in color):
            raise ValueError("color components must be 0..255")
        rgb = (C.c_uint8 * 3)(*(int(v) for v in color)) if color is not None else (C.c_uint8 * 3)()
        return cls(float(level), float(step_dist), int(max_steps),
                   (TRACE_INTERIOR if interior else 0) | (WATER_OWN_COLOR if color is not None else 0), int(reflectivity), rgb,
                   (C.c_uint8 * 4)())


assert C.sizeof(Water) == 32

HAZE_SKY = 2  # hmrm_haze.flags (HMRM_HAZE_SKY): the pixels that did not hit are blended at the table's last entry
HAZE_LINEAR, HAZE_EXP, HAZE_EXP2 = 0, 1, 2  # hmrm_haze_table's laws (HMRM_HAZE_*)
MAX_HAZE_ENTRIES = 4096


class Haze(C.Structure):
    """hmrm_haze (32 bytes): the haze of Scene.render_haze"""
    _fields_ = [("start", C.c_double), ("scale", C.c_double), ("n", C.c_uint32), ("flags", C.c_uint32),
                ("color", C.c_uint8 * 3), ("reserved", C.c_uint8 * 5)]

    @classmethod
    def make(cls, start, far, n, color, sky=False, interior=False):
        """start, far: the ranges at which the table's first entry ends and its last begins -- scale = n / (far - start), in
        doubles; n: the table's length; color (r, g, b): what a pixel is blended towards; sky: HMRM_HAZE_SKY; interior: the
        primary rays under the interior rule."""
        if not all(0 <= int(v) <= 255 for v in color):
            raise ValueError("color components must be 0..255")
        h = cls.raw(float(start), float(n) / (float(far) - float(start)), n, color,
                    (TRACE_INTERIOR if interior else 0) | (HAZE_SKY if sky else 0))
        return h

    @classmethod
    def raw(cls, start, scale, n, color, flags=0):
        """The struct from `start` and `scale` as given (NaN, infinite, zero and negative values are legal)."""
        return cls(float(start), float(scale), int(n), int(flags), (C.c_uint8 * 3)(*(int(v) for v in color)), (C.c_uint8 * 5)())


assert C.sizeof(Haze) == 32


def haze_table(law: int, density: float, n: int) -> np.ndarray:
    """hmrm_haze_table: n bytes of HAZE_LINEAR, HAZE_EXP or HAZE_EXP2 at `density` (host arithmetic, libm's exp)."""
    if not 1 <= int(n) <= MAX_HAZE_ENTRIES:
        raise HmrmError(HMRM_E_ARG, "hmrm_haze_table: n must be 1 .. 4096")
    out = np.zeros(int(n), dtype=np.uint8)
    rc = lib.hmrm_haze_table(int(law), float(density), int(n), out.ctypes.data)
    if rc != HMRM_OK:
        raise HmrmError(rc, lib.hmrm_last_error().decode(errors="replace"))
    return out

MAP_TOWARDS_POINT, MAP_WEIGHT, MAP_DIFFUSE, MAP_NO_SHADOWS = 1, 2, 4, 8  # hmrm_cell_map_params.flags (HMRM_MAP_*)


class CellMapParams(C.Structure):
    """hmrm_cell_map_params (56 bytes): the rays and the byte of Scene.cell_map"""
    _fields_ = [("target", C.c_double * 3), ("step_dist", C.c_double), ("lift", C.c_double), ("max_steps", C.c_uint32),
                ("flags", C.c_uint32), ("sampling", C.c_uint8), ("ambient", C.c_uint8), ("reserved", C.c_uint8 * 6)]

    @classmethod
    def make(cls, target, step_dist, lift=0.0, max_steps=0, flags=0, sampling=NEAREST, ambient=128):
        """target: the direction towards the sun, used as given -- with MAP_TOWARDS_POINT in flags the point O; step_dist in
        units of |dir|; lift: how far above its cell's surface a ray starts; max_steps: limit of every ray (0 = none); flags:
        MAP_*; ambient 0..255: the weight of a shadowed cell."""
        if not 0 <= int(ambient) <= 255:
            raise ValueError("ambient must be 0..255")
        return cls((C.c_double * 3)(*(float(v) for v in target)), float(step_dist), float(lift), int(max_steps), int(flags),
                   int(sampling), int(ambient), (C.c_uint8 * 6)())


class CellRect(C.Structure):
    """hmrm_cell_rect: cells [x0, x0 + w) x [y0, y0 + h)"""
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32)]


assert C.sizeof(CellMapParams) == 56 and C.sizeof(CellRect) == 16


class GeometryPlanes(C.Structure):
    """hmrm_geometry_planes (72 bytes): where Scene.render_geometry's planes go -- host or device addresses, each with its row
    stride in bytes; a null address: that plane is not written"""
    _fields_ = [("rgba", C.c_void_p), ("rgba_stride", C.c_size_t), ("cell", C.c_void_p), ("cell_stride", C.c_size_t),
                ("range", C.c_void_p), ("range_stride", C.c_size_t), ("slope", C.c_void_p), ("slope_stride", C.c_size_t),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]

    @classmethod
    def make(cls, rgba=(0, 0), cell=(0, 0), range=(0, 0), slope=(0, 0), interior=False):
        """Each plane: (address, stride_bytes); address 0 = not wanted.  interior: HMRM_TRACE_INTERIOR."""
        flat = [int(v) or None if i % 2 == 0 else int(v) for i, v in enumerate((*rgba, *cell, *range, *slope))]
        return cls(*flat, TRACE_INTERIOR if interior else 0, 0)


assert C.sizeof(GeometryPlanes) == 72


class LightPlanes(C.Structure):
    """hmrm_light_planes (40 bytes): where Scene.render_lit_sum's planes go -- host or device addresses, each with its row stride
    in bytes; a null address: that plane is not written"""
    _fields_ = [("rgba", C.c_void_p), ("rgba_stride", C.c_size_t), ("light", C.c_void_p), ("light_stride", C.c_size_t),
                ("reserved", C.c_uint32 * 2)]

    @classmethod
    def make(cls, rgba=(0, 0), light=(0, 0)):
        """Each plane: (address, stride_bytes); address 0 = not wanted."""
        return cls(int(rgba[0]) or None, int(rgba[1]), int(light[0]) or None, int(light[1]), (C.c_uint32 * 2)())


assert C.sizeof(LightPlanes) == 40

# the same layouts as numpy structured dtypes (arrays of rays in, arrays of records out)
RAY_DTYPE = np.dtype([("pos", np.float64, 3), ("dir", np.float64, 3)])
RAY_HIT_DTYPE = np.dtype([("point", np.float64, 3), ("entry_d", np.float64), ("steps", np.uint32),
                          ("cell_x", np.int32), ("cell_y", np.int32), ("rgba", np.uint8, 4),
                          ("status", np.uint32), ("reserved", np.uint32)])
assert RAY_DTYPE.itemsize == C.sizeof(Ray) == 48 and RAY_HIT_DTYPE.itemsize == C.sizeof(RayHit) == 56


def as_rays(rays) -> np.ndarray:
    """An (n, 6) float64 array (pos, dir per row) or a RAY_DTYPE array -> contiguous RAY_DTYPE array of n rays."""
    a = np.asarray(rays)
    if a.dtype == RAY_DTYPE:
        return np.ascontiguousarray(a).reshape(-1)
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 6:
        raise ValueError("rays must be an (n, 6) float64 array (pos, dir) or an array of RAY_DTYPE")
    return a.view(RAY_DTYPE).reshape(-1)


def degrees_to_rads(deg: float) -> float:
    """DegreesToRads, main/hmap.cpp:131-133 (same two operations, same order)."""
    return (float(deg) / 180.0) * float(np.pi)


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C heightmap-ray-marcher_amd/csrc` (there is no fallback path)")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 and must be
    # the first to load it, otherwise torch later finds "No HIP GPUs" next to the system
    # runtime this library would pull in.  Loading torch first makes libhmrm.so resolve the
    # same, already-loaded runtime (same SONAME).  The C++ CLI uses the system runtime alone.
    if os.environ.get("HMRM_NO_TORCH_PRELOAD", "") == "":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(LIB_PATH)
    u8p, dp, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    vp, i32 = C.c_void_p, C.c_int32
    sig = {
        "hmrm_abi_version": (C.c_int, []),
        "hmrm_last_error": (C.c_char_p, []),
        "hmrm_device_count": (C.c_int, []),
        "hmrm_set_device": (C.c_int, [C.c_int]),
        "hmrm_scene_create": (C.c_int, [vp, vp, i32, i32, C.POINTER(SceneParams), C.POINTER(vp)]),
        "hmrm_scene_update": (C.c_int, [vp, C.POINTER(SceneParams)]),
        "hmrm_scene_destroy": (None, [vp]),
        "hmrm_scene_read_heights": (C.c_int, [vp, vp]),
        "hmrm_render": (C.c_int, [vp, C.POINTER(Camera), vp, C.c_size_t]),
        "hmrm_render_cycle": (C.c_int, [vp, C.POINTER(Camera), vp, C.c_size_t, i32, i32]),
        "hmrm_render_multi": (C.c_int, [C.POINTER(vp), i32, C.POINTER(Camera), vp, C.c_size_t]),
        "hmrm_render_rows_device": (C.c_int, [vp, C.POINTER(Camera), vp, C.c_size_t, i32, i32, i32, i32, i32, vp]),
        "hmrm_scene_take_capped": (C.c_int, [vp, vp, C.POINTER(C.c_uint64)]),
        "hmrm_debug_reload_env": (C.c_int, [vp]),
        "hmrm_debug_kernel_choice": (C.c_int, [vp]),
        "hmrm_debug_read_records": (C.c_int, [vp, vp, vp]),
        "hmrm_debug_pick_kernel": (C.c_int, [i32, i32, i32, i32, i32, C.POINTER(i32)]),
        "hmrm_debug_calibrate": (C.c_int, [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "hmrm_debug_mip_layout": (C.c_int, [i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "hmrm_debug_level_state": (C.c_int, [i32, i32, i32, C.POINTER(i32)]),
        "hmrm_band_local_rows": (i32, [i32, i32, i32, i32]),
        "hmrm_render_stats": (C.c_int, [vp, C.POINTER(Camera), vp, C.c_size_t, C.POINTER(Stats), vp, vp]),
        "hmrm_render_aa": (C.c_int, [vp, C.POINTER(Camera), i32, vp, C.c_size_t, C.POINTER(Stats)]),
        "hmrm_trace_rays": (C.c_int, [vp, C.POINTER(TraceParams), vp, C.c_int64, vp, C.POINTER(Stats)]),
        "hmrm_trace_rays_device": (C.c_int, [vp, C.POINTER(TraceParams), vp, C.c_int64, vp, vp]),
        "hmrm_trace_segments": (C.c_int, [vp, C.POINTER(SegmentParams), vp, vp, C.c_int64, vp, C.POINTER(Stats)]),
        "hmrm_trace_segments_device": (C.c_int, [vp, C.POINTER(SegmentParams), vp, vp, C.c_int64, vp, vp]),
        "hmrm_cell_map": (C.c_int, [vp, C.POINTER(CellMapParams), C.POINTER(CellRect), vp, C.c_size_t]),
        "hmrm_cell_map_device": (C.c_int, [vp, C.POINTER(CellMapParams), C.POINTER(CellRect), vp, C.c_size_t, vp]),
        "hmrm_cell_map_sum": (C.c_int, [vp, C.POINTER(CellMapParams), dp, i32, C.POINTER(CellRect), vp, C.c_size_t]),
        "hmrm_cell_map_sum_device": (C.c_int, [vp, C.POINTER(CellMapParams), vp, i32, C.POINTER(CellRect), vp, C.c_size_t, vp]),
        "hmrm_sky_directions": (C.c_int, [i32, i32, dp]),
        "hmrm_render_geometry": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(GeometryPlanes)]),
        "hmrm_render_geometry_device": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(GeometryPlanes), vp]),
        "hmrm_render_lit_sum": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(Sun), dp, i32, C.c_uint32, C.POINTER(LightPlanes)]),
        "hmrm_render_lit_sum_device": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(Sun), vp, i32, C.c_uint32, C.POINTER(LightPlanes), vp]),
        "hmrm_render_interior": (C.c_int, [vp, C.POINTER(Camera), vp, C.c_size_t]),
        "hmrm_render_lit": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(Sun), vp, C.c_size_t]),
        "hmrm_render_water": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(Water), vp, C.c_size_t]),
        "hmrm_render_water_device": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(Water), vp, C.c_size_t, vp]),
        "hmrm_render_water_lit": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(Water), C.POINTER(Sun), C.c_uint32, vp, C.c_size_t]),
        "hmrm_render_water_lit_device": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(Water), C.POINTER(Sun), C.c_uint32, vp, C.c_size_t, vp]),
        "hmrm_render_water_aa": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(Water), C.c_uint32, i32, vp, C.c_size_t]),
        "hmrm_render_water_begin": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(Water), C.c_uint32, C.c_uint32, C.POINTER(i32)]),
        "hmrm_render_water_device_begin": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(Water), C.c_uint32, vp, C.c_size_t, C.c_uint32,
                                                     C.POINTER(i32)]),
        "hmrm_record_orbit_water": (C.c_int, [C.POINTER(vp), i32, C.POINTER(Camera), C.c_double, C.c_double, C.c_double,
                                              C.c_double, i32, C.c_char_p, C.c_longlong, i32, i32, C.c_uint32, C.POINTER(Water),
                                              C.c_uint32]),
        "hmrm_config_water_scope": (i32, [vp]),
        "hmrm_config_water_light": (i32, [vp]),
        "hmrm_config_water": (i32, [vp]),
        "hmrm_config_get_water": (None, [vp, C.POINTER(Water)]),
        "hmrm_render_haze": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(Haze), vp, i32, vp, C.c_size_t]),
        "hmrm_render_haze_device": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(Haze), vp, i32, vp, C.c_size_t, vp]),
        "hmrm_haze_table": (C.c_int, [i32, C.c_double, i32, vp]),
        "hmrm_render_views": (C.c_int, [vp, vp, i32, C.c_uint32, vp, C.c_size_t, C.c_size_t]),
        "hmrm_render_views_device": (C.c_int, [vp, vp, i32, C.c_uint32, vp, C.c_size_t, C.c_size_t, vp]),
        "hmrm_debug_views_tables": (C.c_int, [vp, i32, vp, vp]),
        "hmrm_config_view_count": (i32, [vp]),
        "hmrm_config_get_views": (None, [vp, vp]),
        "hmrm_config_views_output": (C.c_char_p, [vp]),
        "hmrm_config_haze": (i32, [vp]),
        "hmrm_config_get_haze": (None, [vp, C.POINTER(Haze), vp]),
        "hmrm_config_haze_law": (i32, [vp]),
        "hmrm_config_haze_density": (C.c_double, [vp]),
        "hmrm_config_haze_far": (C.c_double, [vp]),
        "hmrm_render_shaded": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(Sun), C.c_uint32, vp, C.c_size_t]),
        "hmrm_render_shaded_aa": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(Sun), C.c_uint32, i32, vp, C.c_size_t]),
        "hmrm_render_shaded_begin": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(Sun), C.c_uint32, C.c_uint32, C.POINTER(i32)]),
        "hmrm_render_shaded_device_begin": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(Sun), C.c_uint32, vp, C.c_size_t, C.c_uint32,
                                                      C.POINTER(i32)]),
        "hmrm_scene_set_light": (C.c_int, [vp, vp, C.c_size_t, i32, C.c_uint32]),
        "hmrm_scene_set_light_device": (C.c_int, [vp, vp, C.c_size_t, i32, C.c_uint32, vp]),
        "hmrm_scene_bake_light": (C.c_int, [vp, C.POINTER(CellMapParams), dp, i32]),
        "hmrm_scene_clear_light": (C.c_int, [vp]),
        "hmrm_scene_light": (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_uint32)]),
        "hmrm_render_baked": (C.c_int, [vp, C.POINTER(Camera), C.c_uint32, i32, vp, C.c_size_t]),
        "hmrm_render_baked_begin": (C.c_int, [vp, C.POINTER(Camera), C.c_uint32, C.c_uint32, C.POINTER(i32)]),
        "hmrm_render_baked_device_begin": (C.c_int, [vp, C.POINTER(Camera), C.c_uint32, vp, C.c_size_t, C.c_uint32, C.POINTER(i32)]),
        "hmrm_record_orbit_baked": (C.c_int, [C.POINTER(vp), i32, C.POINTER(Camera), C.c_double, C.c_double, C.c_double,
                                              C.c_double, i32, C.c_char_p, C.c_longlong, i32, i32, C.c_uint32, C.c_uint32]),
        "hmrm_config_baked_light": (i32, [vp]),
        "hmrm_pick": (C.c_int, [vp, C.POINTER(Camera), i32, i32, C.POINTER(RayHit)]),
        "hmrm_debug_ray": (C.c_int, [vp, C.POINTER(Camera), i32, i32, dp, dp, dp]),
        "hmrm_debug_frame": (C.c_int, [C.POINTER(Camera), C.POINTER(SceneParams), i32, i32, vp, vp]),
        "hmrm_debug_plan_order": (C.c_int, [vp, i32, i32, C.POINTER(i32), C.POINTER(i32), vp]),
        "hmrm_debug_rcp_error": (C.c_int, [i32, C.c_uint64, C.c_uint64, i32, i32, dp, C.POINTER(C.c_uint64)]),
        "hmrm_last_kernel_ms": (C.c_double, []),
        "hmrm_bench_kernel_ms": (C.c_double, [vp, C.POINTER(Camera), i32]),
        "hmrm_orbit_camera": (None, [C.POINTER(Camera), C.c_double, C.c_double, C.c_double, C.c_double, i32, i32,
                                     C.POINTER(Camera)]),
        "hmrm_record_orbit": (C.c_int, [vp, C.POINTER(Camera), C.c_double, C.c_double, C.c_double, C.c_double, i32,
                                        C.c_char_p, C.c_longlong, i32, i32]),
        "hmrm_config_record_mode": (i32, [vp]),
        "hmrm_config_devices": (i32, [vp]),
        "hmrm_config_antialias": (i32, [vp]),
        "hmrm_config_interior": (i32, [vp]),
        "hmrm_config_shadows": (i32, [vp]),
        "hmrm_config_shading": (i32, [vp]),
        "hmrm_config_sky_light": (i32, [vp]),
        "hmrm_config_sun_scope": (i32, [vp]),
        "hmrm_config_sun_map_path": (C.c_char_p, [vp]),
        "hmrm_config_sun_map_lift": (C.c_double, [vp]),
        "hmrm_config_sky_map_path": (C.c_char_p, [vp]),
        "hmrm_config_sky_map_rings": (None, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "hmrm_config_range_map_path": (C.c_char_p, [vp]),
        "hmrm_config_get_sun": (None, [vp, C.POINTER(Sun)]),
        "hmrm_record_orbit_multi": (C.c_int, [C.POINTER(vp), i32, C.POINTER(Camera), C.c_double, C.c_double, C.c_double,
                                              C.c_double, i32, C.c_char_p, C.c_longlong, i32, i32]),
        "hmrm_record_orbit_flags": (C.c_int, [C.POINTER(vp), i32, C.POINTER(Camera), C.c_double, C.c_double, C.c_double,
                                              C.c_double, i32, C.c_char_p, C.c_longlong, i32, i32, C.c_uint32]),
        "hmrm_record_orbit_shaded": (C.c_int, [C.POINTER(vp), i32, C.POINTER(Camera), C.c_double, C.c_double, C.c_double,
                                               C.c_double, i32, C.c_char_p, C.c_longlong, i32, i32, C.c_uint32, C.POINTER(Sun),
                                               C.c_uint32]),
        "hmrm_orbit_frame_owner": (i32, [i32, i32]),
        "hmrm_render_begin": (C.c_int, [vp, C.POINTER(Camera), C.POINTER(i32)]),
        "hmrm_render_begin_flags": (C.c_int, [vp, C.POINTER(Camera), C.c_uint32, C.POINTER(i32)]),
        "hmrm_render_wait": (C.c_int, [vp, i32, C.POINTER(u8p), C.POINTER(C.c_size_t)]),
        "hmrm_render_release": (None, [vp, i32]),
        "hmrm_render_device_begin": (C.c_int, [vp, C.POINTER(Camera), vp, C.c_size_t, C.POINTER(i32)]),
        "hmrm_render_device_begin_flags": (C.c_int, [vp, C.POINTER(Camera), vp, C.c_size_t, C.c_uint32, C.POINTER(i32)]),
        "hmrm_render_device_wait": (C.c_int, [vp, i32]),
        "hmrm_config_create": (vp, []),
        "hmrm_config_destroy": (None, [vp]),
        "hmrm_config_consume_file": (C.c_int, [vp, C.c_char_p]),
        "hmrm_config_consume_string": (C.c_int, [vp, C.c_char_p]),
        "hmrm_config_log": (C.c_char_p, [vp]),
        "hmrm_config_warnings": (C.c_char_p, [vp]),
        "hmrm_config_get_camera": (None, [vp, C.POINTER(Camera)]),
        "hmrm_config_get_scene_params": (None, [vp, C.POINTER(SceneParams)]),
        "hmrm_config_cycle": (i32, [vp]),
        "hmrm_config_recording_frame_count": (i32, [vp]),
        "hmrm_config_heightmap_path": (C.c_char_p, [vp]),
        "hmrm_config_colormap_path": (C.c_char_p, [vp]),
        "hmrm_config_output_path": (C.c_char_p, [vp]),
        "hmrm_config_height_rgb": (u8p, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "hmrm_config_color_rgba": (u8p, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "hmrm_config_take_heightmap_dirty": (C.c_int, [vp]),
        "hmrm_config_create_scene": (C.c_int, [vp, C.POINTER(vp)]),
        "hmrm_image_load": (C.c_int, [C.c_char_p, i32, C.POINTER(u8p), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "hmrm_image_load_memory": (C.c_int, [vp, C.c_size_t, i32, C.POINTER(u8p), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "hmrm_image_free": (None, [vp]),
        "hmrm_write_png": (C.c_int, [C.c_char_p, i32, i32, i32, vp, C.c_size_t]),
        "hmrm_write_png_memory": (C.c_int, [i32, i32, i32, vp, C.c_size_t, C.POINTER(u8p), C.POINTER(C.c_size_t)]),
        "hmrm_write_ppm": (C.c_int, [C.c_char_p, i32, i32, i32, vp, C.c_size_t]),
        "hmrm_write_pfm": (C.c_int, [C.c_char_p, i32, i32, i32, vp, C.c_size_t]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError here = the ABI lost a symbol: fail loudly
        fn.restype = res
        fn.argtypes = args
    del u32p
    return lib, tuple(sig.keys())


lib, EXPORTED_SYMBOLS = _load()


# Device + launch sources: a PMC summary (profiles/traffic.json) is only valid for the kernel it was
# collected on, so it carries this hash and bench.py refuses one that does not match the tree.
KERNEL_SOURCES = ("render_fast.hip", "render_rays.hip", "leap_common.hpp", "leap_diag.hpp", "render.hip", "device_common.hpp", "frame.hpp",
                  "render.hpp", "api_internal.hpp", "api_launch.cpp", "api_frames.cpp", "launch_order.cpp", "launch_order.hpp", "camera.cpp", "Makefile",
                  "march.hpp", "march_family.hpp", "march_frame.hpp", "march_dispatch.hpp", "launch_common.hpp", "render_baked.hip", "render_baked_aa.hip",
                  "render_water.hip", "render_water_aa.hip", "render_water_baked.hip", "render_water_baked_aa.hip",
                  "render_water_lit.hip", "render_haze.hip", "render_haze_aa.hip", "render_views.hip")


MAX_VIEWS = 65536  # hmrm_render_views' largest batch (HMRM_MAX_VIEWS)
VIEWS_INTERIOR = 1  # its one flag (HMRM_TRACE_INTERIOR)


def camera_array(cams):
    """(ctypes array of Camera, n) of a sequence of Camera, or of such an array as it is."""
    if isinstance(cams, C.Array) and getattr(cams, "_type_", None) is Camera:
        return cams, len(cams)
    cams = list(cams)
    return (Camera * len(cams))(*cams), len(cams)


def views_tables(cams):
    """hmrm_debug_views_tables: which column tables and which row tables the views of a batch share -> (col_index, row_index),
    int32 arrays; -1 everywhere for a batch that is not spherical."""
    arr, n = camera_array(cams)
    col, row = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    _check(lib.hmrm_debug_views_tables(arr, n, _ptr(col), _ptr(row)))
    return col, row


def kernel_src_sha() -> str:
    import hashlib
    h = hashlib.sha256()
    for name in KERNEL_SOURCES:
        with open(os.path.join(_HERE, "csrc", name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def last_error() -> str:
    return (lib.hmrm_last_error() or b"").decode("utf-8", "replace")


def _check(rc: int, allow=()):
    if rc != HMRM_OK and rc not in allow:
        raise HmrmError(rc, last_error())
    return rc


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def device_count() -> int:
    n = lib.hmrm_device_count()
    if n < 0:
        raise HmrmError(n, last_error())
    return n


def set_device(i: int):
    _check(lib.hmrm_set_device(int(i)))


# The library reads its environment knobs once per scene.  Tests and tools flip them
# on live scenes, so the Python wrappers re-read them when one changed since the scene last looked.
_ENV_KNOBS = ("HMRM_KERNEL", "HMRM_STEP_CAP", "HMRM_TILE_ORDER", "HMRM_DIAG_ITERS", "HMRM_MIN_LEVEL", "HMRM_FINEST_PAUSE", "HMRM_TILE_SEGMENTS", "HMRM_ORDER_VERBOSE", "HMRM_TRY_GROUP")


def shade_flags(diffuse=True, shadows=True) -> int:
    """hmrm_render_shaded's shade_flags (HMRM_SHADE_*)."""
    return (SHADE_DIFFUSE if diffuse else 0) | (0 if shadows else SHADE_NO_SHADOWS)


def map_flags(point=False, weight=False, diffuse=False, shadows=True) -> int:
    """hmrm_cell_map_params.flags (HMRM_MAP_*)."""
    return ((MAP_TOWARDS_POINT if point else 0) | (MAP_WEIGHT if weight else 0) | (MAP_DIFFUSE if diffuse else 0)
            | (0 if shadows else MAP_NO_SHADOWS))


def sky_directions(rings: int, per_ring: int) -> np.ndarray:
    """hmrm_sky_directions: rings * per_ring (1 .. 256) cosine-weighted directions of the upper hemisphere -> (K, 3) float64.
    A plain count over them (Scene.cell_map_sum in status mode) is a sky-view factor.  Host only."""
    n = int(rings) * int(per_ring)
    out = np.zeros((max(min(n, 256), 1), 3), dtype=np.float64)
    rc = lib.hmrm_sky_directions(int(rings), int(per_ring), out.ctypes.data_as(C.POINTER(C.c_double)))
    if rc < 0:
        raise HmrmError(rc, last_error())
    return out[:rc]


def _as_rect(rect):
    if rect is None or isinstance(rect, CellRect):
        return rect
    x0, y0, w, h = (int(v) for v in rect)
    return CellRect(x0, y0, w, h)


def _env_snapshot():
    return tuple(os.environ.get(k) for k in _ENV_KNOBS)


class Scene:
    """Device-resident height + colour maps (replaces the globals filled at hmap.cpp:314-353)."""

    def __init__(self, height_rgb: np.ndarray, color_rgba: np.ndarray, params: SceneParams):
        h_rgb = np.ascontiguousarray(height_rgb, dtype=np.uint8)
        c_rgba = np.ascontiguousarray(color_rgba, dtype=np.uint8)
        if h_rgb.ndim != 3 or h_rgb.shape[2] != 3:
            raise ValueError("height_rgb must be HxWx3 uint8")
        if c_rgba.shape != (h_rgb.shape[0], h_rgb.shape[1], 4):
            # hmap.cpp:503-515
            raise ValueError(f"heightmap dimensions ({h_rgb.shape[1]}x{h_rgb.shape[0]}) must match colormap "
                             f"dimensions ({c_rgba.shape[1]}x{c_rgba.shape[0]})")
        self.map_h, self.map_w = int(h_rgb.shape[0]), int(h_rgb.shape[1])
        self.params = params
        self._h = C.c_void_p()
        self._env = _env_snapshot()
        _check(lib.hmrm_scene_create(_ptr(h_rgb), _ptr(c_rgba), self.map_w, self.map_h,
                                     C.byref(params), C.byref(self._h)))

    def _sync_env(self):
        now = _env_snapshot()
        if now != getattr(self, "_env", None):
            _check(lib.hmrm_debug_reload_env(self._h))
            self._env = now

    @classmethod
    def _adopt(cls, handle, map_w, map_h, params):
        s = cls.__new__(cls)
        s._h, s.map_w, s.map_h, s.params = handle, map_w, map_h, params
        s._env = _env_snapshot()
        return s

    def close(self):
        if getattr(self, "_h", None) and lib is not None:  # (lib is None during interpreter shutdown)
            lib.hmrm_scene_destroy(self._h)
            self._h = None

    __del__ = close

    def update(self, params: SceneParams):
        _check(lib.hmrm_scene_update(self._h, C.byref(params)))
        self.params = params

    def read_heights(self) -> np.ndarray:
        out = np.empty((self.map_h, self.map_w), dtype=np.float64)
        _check(lib.hmrm_scene_read_heights(self._h, _ptr(out)))
        return out

    def render(self, cam: Camera) -> np.ndarray:
        """One full frame (hmap.cpp:978-1058 at `cycle 1`) -> HxWx4 uint8."""
        self._sync_env()
        fb = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
        _check(lib.hmrm_render(self._h, C.byref(cam), _ptr(fb), cam.width * 4))
        return fb

    def render_interior(self, cam: Camera, allow_capped=False) -> np.ndarray:
        """One full frame under the interior rule (hmrm_render_interior): a camera strictly inside the box sees the terrain
        around it instead of sky -> HxWx4 uint8.  An interior ray that never leaves the grid (straight up) reaches the step
        cap: HMRM_E_NOTERM unless allow_capped."""
        self._sync_env()
        fb = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
        _check(lib.hmrm_render_interior(self._h, C.byref(cam), _ptr(fb), cam.width * 4),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return fb

    def render_lit(self, cam: Camera, sun: Sun, allow_capped=False, aa=1) -> np.ndarray:
        """One full frame with sun shadows (hmrm_render_lit): render()'s frame -- render_interior()'s with Sun.make(...,
        interior=True) -- in which every pixel whose shadow ray hits keeps ambient / 255 of its colour -> HxWx4 uint8.  Capped
        primary or shadow rays: HMRM_E_NOTERM unless allow_capped.  aa > 1: the antialiased lit frame (hmrm_render_shaded_aa
        with shade_flags = 0)."""
        if aa != 1:
            return self.render_shaded(cam, sun, diffuse=False, shadows=True, allow_capped=allow_capped, aa=aa)
        self._sync_env()
        fb = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
        _check(lib.hmrm_render_lit(self._h, C.byref(cam), C.byref(sun), _ptr(fb), cam.width * 4),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return fb

    def render_water(self, cam: Camera, water: Water, allow_capped=False) -> np.ndarray:
        """One full frame with mirror reflections on flat water (hmrm_render_water): render()'s frame -- render_interior()'s with
        Water.make(..., interior=True) -- in which every hit pixel at or below water.level takes its mirror ray's pixel blended
        in at water.reflectivity / 255 -> HxWx4 uint8.  Capped primary or mirror rays: HMRM_E_NOTERM unless allow_capped."""
        self._sync_env()
        fb = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
        _check(lib.hmrm_render_water(self._h, C.byref(cam), C.byref(water), _ptr(fb), cam.width * 4),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return fb

    def render_water_device(self, cam: Camera, water: Water, d_rgba: int, stride_bytes: int, stream: int = 0):
        """hmrm_render_water_device: the same frame into device memory at address d_rgba, rows stride_bytes apart, enqueued on
        `stream` without a host sync; take_capped(stream) reports the capped rays."""
        self._sync_env()
        _check(lib.hmrm_render_water_device(self._h, C.byref(cam), C.byref(water), C.c_void_p(d_rgba), int(stride_bytes),
                                            C.c_void_p(stream)))

    def render_water_lit(self, cam: Camera, water: Water, sun: Sun, diffuse=True, shadows=True, allow_capped=False) -> np.ndarray:
        """One full sun-lit water frame (hmrm_render_water_lit): render_water's and render_shaded's frames composed in one launch
        -- every hit pixel, wet or dry, at render_shaded's weight of its hit under `sun` (`diffuse`, `shadows` as there), a wet
        pixel's mirror pixel at the weight of the mirror ray's own hit, then render_water's blend -> HxWx4 uint8.  Capped primary,
        mirror or shadow rays: HMRM_E_NOTERM unless allow_capped."""
        self._sync_env()
        fb = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
        _check(lib.hmrm_render_water_lit(self._h, C.byref(cam), C.byref(water), C.byref(sun), shade_flags(diffuse, shadows), _ptr(fb),
                                         cam.width * 4),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return fb

    def render_water_lit_device(self, cam: Camera, water: Water, sun: Sun, d_rgba: int, stride_bytes: int, diffuse=True, shadows=True,
                                stream: int = 0):
        """hmrm_render_water_lit_device: the same frame into device memory at address d_rgba, rows stride_bytes apart, enqueued on
        `stream` without a host sync; take_capped(stream) reports the capped rays."""
        self._sync_env()
        _check(lib.hmrm_render_water_lit_device(self._h, C.byref(cam), C.byref(water), C.byref(sun), shade_flags(diffuse, shadows),
                                                C.c_void_p(d_rgba), int(stride_bytes), C.c_void_p(stream)))

    def render_water_aa(self, cam: Camera, water: Water, factor=1, baked=False, allow_capped=False) -> np.ndarray:
        """render_water's frame antialiased (factor 1, 2, 4 or 8: factor x factor box-filtered samples per pixel inside the
        launch, every sample deciding "water", casting its mirror ray and blended on its own) and / or, baked=True, under the
        scene's light plane (hmrm_render_water_aa with HMRM_WATER_BAKED: the primary pixel or the water's own colour at the weight
        of the primary hit's light, the mirror pixel at that of its own hit, then the blend) -> HxWx4 uint8."""
        self._sync_env()
        fb = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
        _check(lib.hmrm_render_water_aa(self._h, C.byref(cam), C.byref(water), WATER_BAKED if baked else 0, int(factor), _ptr(fb),
                                        cam.width * 4),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return fb

    def render_water_begin(self, cam: Camera, water: Water, baked=False, aa=1, no_probe=False) -> int:
        """render_begin for a water frame (hmrm_render_water_begin) -> ticket of the same ring: render_wait / render_release.
        The water is copied; no_probe is accepted and has no effect."""
        self._sync_env()
        t = C.c_int32()
        _check(lib.hmrm_render_water_begin(self._h, C.byref(cam), C.byref(water), WATER_BAKED if baked else 0,
                                           (NO_PROBE if no_probe else 0) | aa_flags(aa), C.byref(t)))
        return int(t.value)

    def render_water_device_begin(self, cam: Camera, water: Water, d_rgba: int, stride_bytes: int, baked=False, aa=1) -> int:
        """render_device_begin for a water frame (hmrm_render_water_device_begin) -> ticket for render_device_wait."""
        self._sync_env()
        t = C.c_int32()
        _check(lib.hmrm_render_water_device_begin(self._h, C.byref(cam), C.byref(water), WATER_BAKED if baked else 0,
                                                  C.c_void_p(d_rgba), int(stride_bytes), aa_flags(aa), C.byref(t)))
        return int(t.value)

    def render_haze(self, cam: Camera, haze: Haze, table, factor=1, allow_capped=False, pad_px=0) -> np.ndarray:
        """One full frame with distance fog (hmrm_render_haze): render()'s frame -- render_interior()'s for a haze made with
        interior=True; factor 2, 4 or 8: antialiased like render_aa, every sample hazed on its own -- whose hit pixels are blended
        towards haze.color by the byte of `table` (haze.n uint8) at their range, the others at its last entry with sky=True
        -> HxWx4 uint8.  pad_px: the rows are written pad_px pixels wider (returned whole, untouched bytes are 0xA5).  Capped
        rays: HMRM_E_NOTERM unless allow_capped."""
        self._sync_env()
        t = np.ascontiguousarray(table, dtype=np.uint8).reshape(-1)
        if t.size < int(haze.n):
            raise ValueError("render_haze: the table is shorter than haze.n")
        fb = np.full((cam.height, cam.width + int(pad_px), 4), 0xA5, dtype=np.uint8)
        _check(lib.hmrm_render_haze(self._h, C.byref(cam), C.byref(haze), _ptr(t), int(factor), _ptr(fb),
                                    (cam.width + int(pad_px)) * 4),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return fb

    def render_haze_device(self, cam: Camera, haze: Haze, d_table: int, d_rgba: int, stride_bytes: int, factor=1, stream: int = 0):
        """The same frame into DEVICE memory on a caller stream (hmrm_render_haze_device): d_table the device address of haze.n
        bytes, d_rgba that of the frame; no host sync, capped rays through take_capped(stream)."""
        self._sync_env()
        _check(lib.hmrm_render_haze_device(self._h, C.byref(cam), C.byref(haze), C.c_void_p(d_table), int(factor), C.c_void_p(d_rgba),
                                           int(stride_bytes), C.c_void_p(stream)))

    def render_views(self, cams, interior=False, allow_capped=False, pad_px=0, pad_rows=0) -> np.ndarray:
        """A view batch (hmrm_render_views): the frames of `cams` -- a sequence of Camera or a ctypes array of them, all of one
        width, height, projection and sampling -- in ONE launch; view k is render()'s frame of cams[k], render_interior()'s with
        interior=True -> (n, H, W, 4) uint8.  pad_px / pad_rows: the rows are written pad_px pixels wider and the views pad_rows
        rows apart (returned whole, (n, H + pad_rows, W + pad_px, 4); untouched bytes are 0xA5).  Capped rays: HMRM_E_NOTERM
        unless allow_capped."""
        self._sync_env()
        arr, n = camera_array(cams)
        w, h = (int(arr[0].width), int(arr[0].height)) if n else (0, 0)
        fb = np.full((max(n, 1), h + int(pad_rows), w + int(pad_px), 4), 0xA5, dtype=np.uint8)
        stride = (w + int(pad_px)) * 4
        _check(lib.hmrm_render_views(self._h, arr, n, VIEWS_INTERIOR if interior else 0, _ptr(fb), stride, stride * (h + int(pad_rows))),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return fb

    def render_views_device(self, cams, d_ptr: int, stride_bytes: int, view_stride_bytes: int, interior=False, stream: int = 0):
        """The same batch into DEVICE memory on a caller stream (hmrm_render_views_device): view k at d_ptr + k *
        view_stride_bytes, rows stride_bytes apart (e.g. an (n, H, W, 4) uint8 torch tensor: tensor.data_ptr(), W * 4, H * W * 4);
        no host wait, capped rays through take_capped(stream)."""
        self._sync_env()
        arr, n = camera_array(cams)
        _check(lib.hmrm_render_views_device(self._h, arr, n, VIEWS_INTERIOR if interior else 0, C.c_void_p(d_ptr), int(stride_bytes),
                                            int(view_stride_bytes), C.c_void_p(stream)))

    def render_shaded(self, cam: Camera, sun: Sun, diffuse=True, shadows=True, allow_capped=False, aa=1) -> np.ndarray:
        """One full frame with diffuse sun shading (hmrm_render_shaded): render_lit()'s frame in which every hit pixel that is
        not shadowed is weighted by the diffuse level of its hit (`diffuse`; include/hmrm.h has the arithmetic); shadows=False
        marches no shadow rays (HMRM_SHADE_NO_SHADOWS) -> HxWx4 uint8.  Capped rays: HMRM_E_NOTERM unless allow_capped.
        aa > 1: the antialiased lit frame (hmrm_render_shaded_aa): every sample of the aa x aa times larger frame is shaded and
        shadowed on its own, then box-filtered."""
        self._sync_env()
        fb = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
        flags = shade_flags(diffuse, shadows)
        if aa == 1:
            rc = lib.hmrm_render_shaded(self._h, C.byref(cam), C.byref(sun), flags, _ptr(fb), cam.width * 4)
        else:
            rc = lib.hmrm_render_shaded_aa(self._h, C.byref(cam), C.byref(sun), flags, int(aa), _ptr(fb), cam.width * 4)
        _check(rc, allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return fb

    def render_shaded_begin(self, cam: Camera, sun: Sun, diffuse=True, shadows=True, aa=1, no_probe=False) -> int:
        """render_begin for a lit frame (hmrm_render_shaded_begin) -> ticket of the same ring: render_wait / render_release.
        diffuse=False, shadows=True is render_lit's frame.  no_probe is accepted and has no effect."""
        self._sync_env()
        t = C.c_int32()
        _check(lib.hmrm_render_shaded_begin(self._h, C.byref(cam), C.byref(sun), shade_flags(diffuse, shadows),
                                            (NO_PROBE if no_probe else 0) | aa_flags(aa), C.byref(t)))
        return int(t.value)

    def render_shaded_device_begin(self, cam: Camera, sun: Sun, d_ptr: int, stride_bytes: int, diffuse=True, shadows=True, aa=1,
                                   no_probe=False) -> int:
        """render_device_begin for a lit frame (hmrm_render_shaded_device_begin) -> ticket for render_device_wait."""
        self._sync_env()
        t = C.c_int32()
        _check(lib.hmrm_render_shaded_device_begin(self._h, C.byref(cam), C.byref(sun), shade_flags(diffuse, shadows),
                                                   C.c_void_p(d_ptr), stride_bytes, (NO_PROBE if no_probe else 0) | aa_flags(aa),
                                                   C.byref(t)))
        return int(t.value)

    def render_cycle(self, cam: Camera, framebuf: np.ndarray, cycle: int, cycle_period: int):
        """Progressive refresh (hmap.cpp:976-983): rewrites pixels p = cycle (mod cycle_period) in place."""
        assert framebuf.dtype == np.uint8 and framebuf.shape == (cam.height, cam.width, 4) and framebuf.flags.c_contiguous
        self._sync_env()
        _check(lib.hmrm_render_cycle(self._h, C.byref(cam), _ptr(framebuf), cam.width * 4, cycle, cycle_period))

    def render_stats(self, cam: Camera, per_pixel=False, allow_capped=False):
        self._sync_env()
        fb = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
        st = Stats()
        steps = np.empty((cam.height, cam.width), dtype=np.uint32) if per_pixel else None
        entry = np.empty((cam.height, cam.width), dtype=np.float64) if per_pixel else None
        _check(lib.hmrm_render_stats(self._h, C.byref(cam), _ptr(fb), cam.width * 4, C.byref(st),
                                     _ptr(steps) if per_pixel else None, _ptr(entry) if per_pixel else None),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return fb, st, steps, entry

    def render_aa(self, cam: Camera, factor: int, stats=False, allow_capped=False):
        """The antialiased frame (hmrm_render_aa): the frame of factor x the resolution, box-filtered over factor x factor
        blocks -> HxWx4 uint8, or (frame, Stats counted over the samples) with stats=True (the instrumented kernel)."""
        self._sync_env()
        fb = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
        st = Stats() if stats else None
        _check(lib.hmrm_render_aa(self._h, C.byref(cam), int(factor), _ptr(fb), cam.width * 4, C.byref(st) if stats else None),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return (fb, st) if stats else fb

    def render_rows_device(self, cam: Camera, d_ptr: int, stride_bytes: int, row_begin=0, row_end=0,
                           band_rows=0, band_index=0, band_count=1, stream: int = 0):
        self._sync_env()
        _check(lib.hmrm_render_rows_device(self._h, C.byref(cam), C.c_void_p(d_ptr), stride_bytes,
                                           row_begin, row_end, band_rows, band_index, band_count,
                                           C.c_void_p(stream)))

    def render_begin(self, cam: Camera, no_probe: bool = False, aa: int = 1) -> int:
        """Enqueue a frame (kernel + copy into a pinned frame of the scene's ring) -> ticket.  no_probe = HMRM_NO_PROBE;
        aa = antialias factor (HMRM_AA, the frame stays cam.width x cam.height)."""
        self._sync_env()
        t = C.c_int32()
        _check(lib.hmrm_render_begin_flags(self._h, C.byref(cam), (NO_PROBE if no_probe else 0) | aa_flags(aa), C.byref(t)))
        return int(t.value)

    def render_wait(self, ticket: int, shape, allow_capped=False, copy=True) -> np.ndarray:
        """Wait for the frame of `ticket` -> HxWx4 uint8 (a copy, or with copy=False a view of the
        ring's pinned memory that is valid until render_release)."""
        p = C.POINTER(C.c_uint8)()
        stride = C.c_size_t()
        _check(lib.hmrm_render_wait(self._h, ticket, C.byref(p), C.byref(stride)),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        h, w = shape
        assert stride.value == w * 4
        a = np.ctypeslib.as_array(p, shape=(h, w, 4))
        return a.copy() if copy else a

    def render_release(self, ticket: int):
        lib.hmrm_render_release(self._h, ticket)

    def render_device_begin(self, cam: Camera, d_ptr: int, stride_bytes: int, no_probe: bool = False, aa: int = 1) -> int:
        """Launch a frame into device memory on the next of the scene's launch streams -> ticket.  no_probe = HMRM_NO_PROBE;
        aa = antialias factor (HMRM_AA)."""
        self._sync_env()
        t = C.c_int32()
        _check(lib.hmrm_render_device_begin_flags(self._h, C.byref(cam), C.c_void_p(d_ptr), stride_bytes,
                                                  (NO_PROBE if no_probe else 0) | aa_flags(aa), C.byref(t)))
        return int(t.value)

    def render_device_wait(self, ticket: int, allow_capped=False):
        _check(lib.hmrm_render_device_wait(self._h, ticket), allow=(HMRM_E_NOTERM,) if allow_capped else ())

    def take_capped(self, stream: int = 0, allow_capped=False) -> int:
        """Rays of the launches enqueued on `stream` that reached the step cap since the last call
        (waits for the stream); raises HMRM_E_NOTERM for a non-zero count unless allowed."""
        n = C.c_uint64()
        _check(lib.hmrm_scene_take_capped(self._h, C.c_void_p(stream), C.byref(n)),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return int(n.value)

    def trace_rays(self, rays, step_dist, bg=(0, 0, 0), sampling=NEAREST, stats=False, allow_capped=False):
        """Trace a batch of rays (hmrm_trace_rays): `rays` is an (n, 6) float64 array (pos, dir per row) or a RAY_DTYPE
        array -> RAY_HIT_DTYPE array of n records, or (records, Stats) with stats=True.  A ray stopped by the step cap
        raises HMRM_E_NOTERM unless allow_capped (its record has status RAY_CAPPED)."""
        self._sync_env()
        r = as_rays(rays)
        hits = np.zeros(r.shape[0], dtype=RAY_HIT_DTYPE)
        p = TraceParams.make(step_dist, bg, sampling)
        st = Stats() if stats else None
        _check(lib.hmrm_trace_rays(self._h, C.byref(p), _ptr(r), r.shape[0], _ptr(hits), C.byref(st) if stats else None),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return (hits, st) if stats else hits

    def trace_rays_device(self, d_rays_ptr: int, n: int, d_hits_ptr: int, step_dist, bg=(0, 0, 0), sampling=NEAREST,
                          stream: int = 0):
        """hmrm_trace_rays_device: n rays (48 bytes each) and n records (56 bytes each) in device memory, enqueued on
        `stream` without a host sync; take_capped(stream) reports rays stopped by the step cap."""
        self._sync_env()
        p = TraceParams.make(step_dist, bg, sampling)
        _check(lib.hmrm_trace_rays_device(self._h, C.byref(p), C.c_void_p(d_rays_ptr), int(n), C.c_void_p(d_hits_ptr),
                                          C.c_void_p(stream)))

    def trace_segments(self, rays, step_dist, bg=(0, 0, 0), sampling=NEAREST, interior=False, max_steps=0,
                       per_ray_max_steps=None, stats=False, allow_capped=False):
        """trace_rays under the two segment rules (hmrm_trace_segments): interior = rays that start strictly inside the box
        enter it at d = +0.0 instead of missing; max_steps / per_ray_max_steps (n uint32, 0 = none) = a ray ends after the
        smaller non-zero one of the two height loads (status RAY_END when still inside the grid).  RAY_END rays are not
        capped rays: only RAY_CAPPED ones raise HMRM_E_NOTERM (unless allow_capped)."""
        self._sync_env()
        r = as_rays(rays)
        hits = np.zeros(r.shape[0], dtype=RAY_HIT_DTYPE)
        lim = None
        if per_ray_max_steps is not None:
            lim = np.ascontiguousarray(per_ray_max_steps, dtype=np.uint32).reshape(-1)
            if lim.shape[0] != r.shape[0]:
                raise ValueError("per_ray_max_steps must hold one limit per ray")
        p = SegmentParams.make(step_dist, bg, sampling, interior, max_steps)
        st = Stats() if stats else None
        _check(lib.hmrm_trace_segments(self._h, C.byref(p), _ptr(r), _ptr(lim) if lim is not None else None, r.shape[0],
                                       _ptr(hits), C.byref(st) if stats else None),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return (hits, st) if stats else hits

    def trace_segments_device(self, d_rays_ptr: int, n: int, d_hits_ptr: int, step_dist, bg=(0, 0, 0), sampling=NEAREST,
                              interior=False, max_steps=0, d_max_steps_ptr: int = 0, stream: int = 0):
        """hmrm_trace_segments_device: as trace_rays_device, with the rules; d_max_steps_ptr (n uint32 in device memory)
        may be 0."""
        self._sync_env()
        p = SegmentParams.make(step_dist, bg, sampling, interior, max_steps)
        _check(lib.hmrm_trace_segments_device(self._h, C.byref(p), C.c_void_p(d_rays_ptr),
                                              C.c_void_p(d_max_steps_ptr) if d_max_steps_ptr else None, int(n),
                                              C.c_void_p(d_hits_ptr), C.c_void_p(stream)))

    def cell_map(self, target, step_dist, lift=0.0, max_steps=0, point=False, weight=False, diffuse=False, shadows=True,
                 sampling=NEAREST, ambient=128, rect=None, allow_capped=False, stride_bytes=None) -> np.ndarray:
        """One byte per map cell (hmrm_cell_map): every cell of `rect` ((x0, y0, w, h) or a CellRect; None = the whole map)
        casts one segment ray from `lift` above its surface towards `target` -- a direction used as given, or with point=True
        the point O -- and gets the ray's status (RAY_MISS / HIT / CAPPED / END) or, with weight=True, the light weight of
        render_shaded (diffuse: the diffuse level of an unshadowed cell; shadows=False: no ray is marched) -> (h, w) uint8.
        stride_bytes > w: the rows are written into a wider buffer (returned whole, untouched bytes are 0xA5).  Capped rays:
        HMRM_E_NOTERM unless allow_capped."""
        self._sync_env()
        p = CellMapParams.make(target, step_dist, lift, max_steps, map_flags(point, weight, diffuse, shadows), sampling, ambient)
        r = _as_rect(rect)
        w, h = (r.w, r.h) if r is not None else (self.map_w, self.map_h)
        stride = w if stride_bytes is None else int(stride_bytes)
        out = np.full((max(h, 0), max(stride, 0)), 0xA5, dtype=np.uint8)
        _check(lib.hmrm_cell_map(self._h, C.byref(p), C.byref(r) if r is not None else None, _ptr(out), stride),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return out

    def cell_map_device(self, d_ptr: int, stride_bytes: int, target, step_dist, lift=0.0, max_steps=0, point=False, weight=False,
                        diffuse=False, shadows=True, sampling=NEAREST, ambient=128, rect=None, stream: int = 0):
        """hmrm_cell_map_device: the same bytes into device memory (no alignment asked), enqueued on `stream` without a host
        sync; take_capped(stream) reports the capped rays."""
        self._sync_env()
        p = CellMapParams.make(target, step_dist, lift, max_steps, map_flags(point, weight, diffuse, shadows), sampling, ambient)
        r = _as_rect(rect)
        _check(lib.hmrm_cell_map_device(self._h, C.byref(p), C.byref(r) if r is not None else None, C.c_void_p(d_ptr),
                                        int(stride_bytes), C.c_void_p(stream)))

    def cell_map_sum(self, targets, step_dist, lift=0.0, max_steps=0, point=False, weight=False, diffuse=False, shadows=True,
                     sampling=NEAREST, ambient=128, rect=None, allow_capped=False, stride_bytes=None) -> np.ndarray:
        """One uint16 per map cell (hmrm_cell_map_sum): cell_map's ray towards each of the K = 1 .. 256 `targets` ((K, 3):
        directions, or with point=True points) in ONE launch, and the sum of the K values -- with weight=True the bytes
        cell_map would write, else 1 per target whose ray did not hit (reached by that sun / sky direction, seen by that
        observer) -> (h, w) uint16.  stride_bytes > 2 * w: the rows are written into a wider buffer (returned whole,
        untouched words are 0xA5A5).  Capped rays, counted per ray: HMRM_E_NOTERM unless allow_capped."""
        self._sync_env()
        t = np.ascontiguousarray(targets, dtype=np.float64).reshape(-1, 3)
        p = CellMapParams.make((0.0, 0.0, 0.0), step_dist, lift, max_steps, map_flags(point, weight, diffuse, shadows), sampling, ambient)
        r = _as_rect(rect)
        w, h = (r.w, r.h) if r is not None else (self.map_w, self.map_h)
        stride = 2 * w if stride_bytes is None else int(stride_bytes)
        out = np.full((max(h, 0), max((stride + 1) // 2, 0)), 0xA5A5, dtype=np.uint16)
        _check(lib.hmrm_cell_map_sum(self._h, C.byref(p), t.ctypes.data_as(C.POINTER(C.c_double)), len(t),
                                     C.byref(r) if r is not None else None, _ptr(out), stride),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return out

    def cell_map_sum_device(self, d_ptr: int, stride_bytes: int, d_targets: int, n_targets: int, step_dist, lift=0.0, max_steps=0,
                            point=False, weight=False, diffuse=False, shadows=True, sampling=NEAREST, ambient=128, rect=None,
                            stream: int = 0):
        """hmrm_cell_map_sum_device: the same words into device memory (2-byte aligned), the targets read from device memory
        (n_targets x 3 float64, 8-byte aligned), enqueued on `stream` without a host sync; take_capped(stream) reports the
        capped rays."""
        self._sync_env()
        p = CellMapParams.make((0.0, 0.0, 0.0), step_dist, lift, max_steps, map_flags(point, weight, diffuse, shadows), sampling, ambient)
        r = _as_rect(rect)
        _check(lib.hmrm_cell_map_sum_device(self._h, C.byref(p), C.c_void_p(d_targets), int(n_targets),
                                            C.byref(r) if r is not None else None, C.c_void_p(d_ptr), int(stride_bytes),
                                            C.c_void_p(stream)))

    def render_geometry(self, cam: Camera, rgba=True, cell=True, range=True, slope=True, interior=False, allow_capped=False,
                        pad_px=0) -> dict:
        """One geometry frame (hmrm_render_geometry): render()'s frame -- render_interior()'s with interior=True -- and, from
        the same launch, the planes asked for -> {"rgba": (H, W, 4) uint8, "cell": (H, W) int32 (hit cell y * map_w + x, -1: no
        hit), "range": (H, W) float32 (origin to hit point, +inf: no hit), "slope": (H, W, 2) float32 (gx, gy of the diffuse
        level's gradient; the normal is (-gx, gy, 1))}, only the keys that are True.  pad_px > 0: every plane's rows are that
        many pixels wider (returned whole; the padding keeps its poison bytes 0xA5).  Capped rays: HMRM_E_NOTERM unless
        allow_capped."""
        self._sync_env()
        w, h, wp = cam.width, cam.height, cam.width + int(pad_px)
        out = {}
        if rgba:
            out["rgba"] = np.full((h, wp, 4), 0xA5, dtype=np.uint8)
        if cell:
            out["cell"] = np.full((h, wp), 0xA5, dtype=np.uint8).repeat(4, axis=1).view(np.int32)
        if range:
            out["range"] = np.full((h, wp), 0xA5, dtype=np.uint8).repeat(4, axis=1).view(np.float32)
        if slope:
            out["slope"] = np.full((h, wp, 8), 0xA5, dtype=np.uint8).view(np.float32)
        at = lambda k, elem: (out[k].ctypes.data, wp * elem) if k in out else (0, 0)
        p = GeometryPlanes.make(at("rgba", 4), at("cell", 4), at("range", 4), at("slope", 8), interior)
        _check(lib.hmrm_render_geometry(self._h, C.byref(cam), C.byref(p)), allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return out

    def render_geometry_device(self, cam: Camera, rgba=(0, 0), cell=(0, 0), range=(0, 0), slope=(0, 0), interior=False,
                               stream: int = 0):
        """hmrm_render_geometry_device: the same planes into device memory -- each an (address, stride_bytes) pair, address 0 =
        not wanted; slope 8-byte aligned, the others 4-byte -- enqueued on `stream` without a host sync; take_capped(stream)
        reports the capped rays."""
        self._sync_env()
        p = GeometryPlanes.make(rgba, cell, range, slope, interior)
        _check(lib.hmrm_render_geometry_device(self._h, C.byref(cam), C.byref(p), C.c_void_p(stream)))

    def render_lit_sum(self, cam: Camera, sun: Sun, dirs, diffuse=False, shadows=True, light=False, allow_capped=False, rgba=True,
                       pad_px=0):
        """One accumulated lit frame (hmrm_render_lit_sum): render()'s frame -- render_interior()'s for a sun made with
        interior=True -- in which every hit pixel is weighted by the SUM of render_shaded()'s weights under each of the
        K = 1 .. 256 directions `dirs` ((K, 3): towards a sun or a patch of sky, used as given; sun.dir is not looked at), the
        primary rays marched once -> the (H, W, 4) uint8 frame; with light=True (frame, light), light the (H, W) uint16 sums
        (0xFFFF: no hit); with rgba=False the light plane alone.  pad_px > 0: every plane's rows are that many pixels wider
        (returned whole; the padding keeps its poison bytes 0xA5).  Capped rays: HMRM_E_NOTERM unless allow_capped."""
        self._sync_env()
        d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        if not rgba and not light:
            raise ValueError("render_lit_sum: no plane asked for")
        h, wp = cam.height, cam.width + int(pad_px)
        fb = np.full((h, wp, 4), 0xA5, dtype=np.uint8) if rgba else None
        lp = np.full((h, wp, 2), 0xA5, dtype=np.uint8).view(np.uint16).reshape(h, wp) if light else None
        p = LightPlanes.make((fb.ctypes.data, wp * 4) if rgba else (0, 0), (lp.ctypes.data, wp * 2) if light else (0, 0))
        _check(lib.hmrm_render_lit_sum(self._h, C.byref(cam), C.byref(sun), d.ctypes.data_as(C.POINTER(C.c_double)), len(d),
                                       shade_flags(diffuse, shadows), C.byref(p)), allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return (fb, lp) if rgba and light else (fb if rgba else lp)

    def render_lit_sum_device(self, cam: Camera, sun: Sun, d_dirs: int, n_dirs: int, rgba=(0, 0), light=(0, 0), diffuse=False,
                              shadows=True, stream: int = 0):
        """hmrm_render_lit_sum_device: the same planes into device memory -- each an (address, stride_bytes) pair, address 0 =
        not wanted; rgba 4-byte aligned, light 2-byte -- the directions read from device memory (n_dirs x 3 float64, 8-byte
        aligned), enqueued on `stream` without a host sync; take_capped(stream) reports the capped rays."""
        self._sync_env()
        p = LightPlanes.make(rgba, light)
        _check(lib.hmrm_render_lit_sum_device(self._h, C.byref(cam), C.byref(sun), C.c_void_p(d_dirs), int(n_dirs),
                                              shade_flags(diffuse, shadows), C.byref(p), C.c_void_p(stream)))

    def set_light(self, plane, full_scale: int, stride_bytes=None):
        """The scene's light plane from host memory (hmrm_scene_set_light): `plane` is (map_h, >= map_w) uint8 (HMRM_LIGHT_U8,
        widened) or uint16 (HMRM_LIGHT_U16), its row pitch the stride unless stride_bytes says otherwise; a cell whose light
        equals full_scale (1 .. 65535) gives the texel back.  Tickets in flight finish with the old plane."""
        a = np.asarray(plane)
        if a.dtype not in (np.uint8, np.uint16):
            raise TypeError("light plane: uint8 or uint16")
        a = np.ascontiguousarray(a)
        stride = a.strides[0] if stride_bytes is None else int(stride_bytes)
        _check(lib.hmrm_scene_set_light(self._h, _ptr(a), stride, LIGHT_U16 if a.dtype == np.uint16 else LIGHT_U8, int(full_scale)))

    def set_light_device(self, d_ptr: int, stride_bytes: int, full_scale: int, u16=True, stream: int = 0):
        """hmrm_scene_set_light_device: the plane from device memory, read on `stream` behind what the caller enqueued there
        (cell_map_sum_device's output goes in without a trip over the host); returns after the copy."""
        _check(lib.hmrm_scene_set_light_device(self._h, C.c_void_p(d_ptr), int(stride_bytes), LIGHT_U16 if u16 else LIGHT_U8,
                                               int(full_scale), C.c_void_p(stream)))

    def bake_light(self, targets, step_dist, lift=0.0, max_steps=0, point=False, weight=False, diffuse=False, shadows=True,
                   sampling=NEAREST, ambient=128, allow_capped=False):
        """cell_map_sum over the whole map written straight into the scene's light plane (hmrm_scene_bake_light): full scale
        255 * K with weight=True, else K (a count).  Capped rays: HMRM_E_NOTERM, with a valid plane, unless allow_capped."""
        self._sync_env()
        t = np.ascontiguousarray(targets, dtype=np.float64).reshape(-1, 3)
        p = CellMapParams.make((0.0, 0.0, 0.0), step_dist, lift, max_steps, map_flags(point, weight, diffuse, shadows), sampling, ambient)
        _check(lib.hmrm_scene_bake_light(self._h, C.byref(p), t.ctypes.data_as(C.POINTER(C.c_double)), len(t)),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())

    def clear_light(self):
        """Drops the scene's light plane (hmrm_scene_clear_light)."""
        _check(lib.hmrm_scene_clear_light(self._h))

    def light(self):
        """The scene's light plane read back (hmrm_scene_light) -> ((map_h, map_w) uint16, full_scale), or (None, 0) for a
        scene without one."""
        fs = C.c_uint32()
        _check(lib.hmrm_scene_light(self._h, None, 0, C.byref(fs)))
        if fs.value == 0:
            return None, 0
        out = np.empty((self.map_h, self.map_w), dtype=np.uint16)
        _check(lib.hmrm_scene_light(self._h, _ptr(out), 2 * self.map_w, C.byref(fs)))
        return out, int(fs.value)

    def render_baked(self, cam: Camera, interior=False, factor=1, pad_px=0, allow_capped=False) -> np.ndarray:
        """One full frame under the scene's baked light (hmrm_render_baked): render()'s frame -- render_interior()'s with
        interior=True -- whose hit pixels are weighted by the light plane; factor 2, 4 or 8: antialiased like render_aa, every
        sample weighted on its own -> HxWx4 uint8.  pad_px: the rows are written pad_px pixels apart wider (returned whole,
        untouched bytes are 0xA5).  Capped primary rays: HMRM_E_NOTERM unless allow_capped."""
        self._sync_env()
        fb = np.full((cam.height, cam.width + int(pad_px), 4), 0xA5, dtype=np.uint8)
        _check(lib.hmrm_render_baked(self._h, C.byref(cam), TRACE_INTERIOR if interior else 0, int(factor), _ptr(fb),
                                     (cam.width + int(pad_px)) * 4),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return fb

    def render_baked_begin(self, cam: Camera, interior=False, aa=1, no_probe=False) -> int:
        """render_begin for a baked-light frame (hmrm_render_baked_begin) -> ticket of the same ring: render_wait /
        render_release.  no_probe is accepted and has no effect."""
        self._sync_env()
        t = C.c_int32()
        _check(lib.hmrm_render_baked_begin(self._h, C.byref(cam), TRACE_INTERIOR if interior else 0,
                                           (NO_PROBE if no_probe else 0) | aa_flags(aa), C.byref(t)))
        return int(t.value)

    def render_baked_device_begin(self, cam: Camera, d_ptr: int, stride_bytes: int, interior=False, aa=1, no_probe=False) -> int:
        """render_device_begin for a baked-light frame (hmrm_render_baked_device_begin) -> ticket for render_device_wait."""
        self._sync_env()
        t = C.c_int32()
        _check(lib.hmrm_render_baked_device_begin(self._h, C.byref(cam), TRACE_INTERIOR if interior else 0, C.c_void_p(d_ptr),
                                                  stride_bytes, (NO_PROBE if no_probe else 0) | aa_flags(aa), C.byref(t)))
        return int(t.value)

    def pick(self, cam: Camera, px: int, py: int, allow_capped=False) -> np.ndarray:
        """hmrm_pick: the record (RAY_HIT_DTYPE scalar) of the ray of pixel (px, py) of `cam`."""
        self._sync_env()
        hit = np.zeros(1, dtype=RAY_HIT_DTYPE)
        _check(lib.hmrm_pick(self._h, C.byref(cam), int(px), int(py), hit.ctypes.data_as(C.POINTER(RayHit))),
               allow=(HMRM_E_NOTERM,) if allow_capped else ())
        return hit[0]

    def debug_ray(self, cam: Camera, px: int, py: int):
        pos, dirv, d = (C.c_double * 3)(), (C.c_double * 3)(), C.c_double()
        _check(lib.hmrm_debug_ray(self._h, C.byref(cam), px, py, pos, dirv, C.byref(d)))
        return np.array(pos[:]), np.array(dirv[:]), d.value

    def read_records(self):
        """(records, thr): the window records as a structured array of shape (ceil(map_h / 4), ceil(map_w / 4)) with fields
        max2 / xs / ys, and the threshold table (map_h x map_w doubles) they were built from."""
        rw, rh = (self.map_w + 3) // 4, (self.map_h + 3) // 4
        dt = np.dtype([("max2", np.float32), ("spare0", np.uint32), ("xs", np.uint8, 8), ("ys", np.uint8, 8), ("spare1", np.uint32, 2)])
        assert dt.itemsize == 32
        recs = np.empty((rh, rw), dtype=dt)
        thr = np.empty((self.map_h, self.map_w), dtype=np.float64)
        _check(lib.hmrm_debug_read_records(self._h, recs.ctypes.data_as(C.c_void_p), thr.ctypes.data_as(C.c_void_p)))
        return recs, thr

    def kernel_choice(self) -> int:
        """0 production kernel (leaps), 1 plain groups, 2 literal loop, 3 groups + window records (1 / 3: forced, or chosen by the scene's probe)."""
        return int(lib.hmrm_debug_kernel_choice(self._h))

    def bench_kernel_ms(self, cam: Camera, iters: int) -> float:
        self._sync_env()
        ms = lib.hmrm_bench_kernel_ms(self._h, C.byref(cam), int(iters))
        if ms < 0:
            raise HmrmError(HMRM_E_DEVICE, last_error())
        return ms


def debug_frame(cam: Camera, params: SceneParams, map_w: int, map_h: int):
    """Host-only per-frame record (no GPU): dict of the DevFrame fields + spherical tables."""
    out = np.empty(25, dtype=np.float64)
    tables = np.empty(2 * cam.width + 2 * cam.height, dtype=np.float64)
    _check(lib.hmrm_debug_frame(C.byref(cam), C.byref(params), map_w, map_h, _ptr(out), _ptr(tables)))
    W, H = cam.width, cam.height
    rec = {"cam": out[0:3], "upper_left": out[3:6], "plane_right": out[6:9], "plane_down": out[9:12],
           "look": out[12:15], "c0": out[15:18], "c1": out[18:21], "nudge": out[21], "step_dist": out[22],
           "grid_pow2": int(out[23]), "inv_grid_width": out[24]}
    if cam.projection == SPHERICAL:
        rec.update(col_cos_ha=tables[0:W], col_sin_ha=tables[W:2 * W],
                   row_sin_va=tables[2 * W:2 * W + H], row_cos_va=tables[2 * W + H:])
    return rec


def mip_layout(map_w: int, map_h: int):
    """Pyramid layout hmrm_scene_create would choose (no GPU needed) -> (row pitch, log2 plane pitch, levels,
    production kernel usable: its 32-bit look-up offsets cover every plane)."""
    row, shift, levels = C.c_int32(), C.c_int32(), C.c_int32()
    rc = lib.hmrm_debug_mip_layout(int(map_w), int(map_h), C.byref(row), C.byref(shift), C.byref(levels))
    if rc < 0:
        raise HmrmError(rc, last_error())
    return row.value, shift.value, levels.value, bool(rc)


def level_state(level: int, young: bool, min_level: int):
    """hmrm_debug_level_state (no GPU) -> (dict of the level's unpacked state and the policy's moves from it, pyramid levels)."""
    out = (C.c_int32 * 8)()
    rc = lib.hmrm_debug_level_state(int(level), int(bool(young)), int(min_level), out)
    if rc < 0:
        raise HmrmError(rc, last_error())
    keys = ("stride_shift", "back", "cells", "lstep", "coarser", "finer", "at_finest", "byte")
    return dict(zip(keys, (int(v) for v in out))), int(rc)


def pick_kernel(forced=0, use_other=False, records_ok=True, verdict=False, verdict_with_records=False):
    """launch_order.hpp pick_fast_kernel (no GPU) -> (kernel: 0 plain groups, 1 production, 2 records; what the scene remembers
    as the probe's alternative afterwards)."""
    after = C.c_int32()
    k = lib.hmrm_debug_pick_kernel(int(forced), int(use_other), int(records_ok), int(verdict), int(verdict_with_records), C.byref(after))
    return int(k), bool(after.value)


def calibrate(records: np.ndarray, rot: int, may_probe=True, scene_already_probed=False, can_measure=None):
    """hmrm_debug_calibrate: records (launches, tile_rows, 2) uint64 -> dict of the per-launch decisions and the outcome."""
    rec = np.ascontiguousarray(records, dtype=np.uint64)
    n, rows = int(rec.shape[0]), int(rec.shape[1])
    used, meas, grp = (np.zeros(n, dtype=np.int32) for _ in range(3))
    cm = None if can_measure is None else np.ascontiguousarray(can_measure, dtype=np.uint8)
    nt, best, verdict, at = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    _check(lib.hmrm_debug_calibrate(_ptr(rec), n, rows, int(rot), int(bool(may_probe)), int(bool(scene_already_probed)),
                                    _ptr(cm) if cm is not None else None, _ptr(used), _ptr(meas), _ptr(grp), C.byref(nt), C.byref(best),
                                    C.byref(verdict), C.byref(at)))
    return {"settled_at": int(at.value), "trial": used.tolist(), "measured": meas.tolist(), "group": grp.tolist(), "n_trials": int(nt.value),
            "best": int(best.value), "scene_use_group": bool(verdict.value)}


def plan_order(records: np.ndarray, rot: int):
    """The launch-order plan for measured records ((tile_rows, 2) uint64: start, longest wave) -> (pieces, permutation)."""
    rec = np.ascontiguousarray(records, dtype=np.uint64)
    n_rows = rec.shape[0]
    b, c = (C.c_int32 * 3)(), (C.c_int32 * 3)()
    perm = np.empty(n_rows, dtype=np.int32)
    n = lib.hmrm_debug_plan_order(_ptr(rec), n_rows, rot, b, c, _ptr(perm))
    if n < 0:
        raise HmrmError(n, last_error())
    return [(b[k], c[k]) for k in range(n)], perm


def rcp_error(mode: int, count: int, seed: int = 0, exp_lo: int = 0, exp_hi: int = 0):
    """Largest relative error of v_rcp_f64 over a sample (hmrm_debug_rcp_error) -> (max_rel_err, hist[64])."""
    m = C.c_double()
    hist = (C.c_uint64 * 64)()
    _check(lib.hmrm_debug_rcp_error(mode, count, seed, exp_lo, exp_hi, C.byref(m), hist))
    return m.value, np.array(hist[:], dtype=np.uint64)


def orbit_camera(base: Camera, centre_x: float, centre_y: float, radius: float, hang0: float,
                 frame: int, frames: int) -> Camera:
    """Frame `frame` of an orbit sweep (BASELINE config C5); see hmrm_orbit_camera."""
    out = Camera()
    lib.hmrm_orbit_camera(C.byref(base), centre_x, centre_y, radius, hang0, frame, frames, C.byref(out))
    return out


def record_orbit(scene: "Scene", base: Camera, centre_x, centre_y, radius, hang0, frames, directory, rec_id,
                 encoder_threads=0, verbose=False, aa=1):
    """aa: antialias factor of every frame (HMRM_AA through hmrm_record_orbit_flags)."""
    if aa == 1:
        _check(lib.hmrm_record_orbit(scene._h, C.byref(base), centre_x, centre_y, radius, hang0, frames,
                                     os.fsencode(directory), rec_id, encoder_threads, int(verbose)),
               allow=(HMRM_E_NOTERM,))
    else:
        record_orbit_multi([scene], base, centre_x, centre_y, radius, hang0, frames, directory, rec_id,
                           encoder_threads, verbose, aa=aa)


def record_orbit_multi(scenes, base: Camera, centre_x, centre_y, radius, hang0, frames, directory, rec_id,
                       encoder_threads=0, verbose=False, aa=1):
    """The sweep sharded over several scenes (one per GPU): frame k on scenes[k mod len(scenes)].  aa: antialias factor."""
    arr = (C.c_void_p * len(scenes))(*[s._h for s in scenes])
    if aa == 1:
        _check(lib.hmrm_record_orbit_multi(arr, len(scenes), C.byref(base), centre_x, centre_y, radius, hang0, frames,
                                           os.fsencode(directory), rec_id, encoder_threads, int(verbose)),
               allow=(HMRM_E_NOTERM,))
    else:
        _check(lib.hmrm_record_orbit_flags(arr, len(scenes), C.byref(base), centre_x, centre_y, radius, hang0, frames,
                                           os.fsencode(directory), rec_id, encoder_threads, int(verbose), aa_flags(aa)),
               allow=(HMRM_E_NOTERM,))


def record_orbit_shaded(scenes, base: Camera, centre_x, centre_y, radius, hang0, frames, directory, rec_id, sun,
                        diffuse=True, shadows=True, aa=1, encoder_threads=0, verbose=False):
    """record_orbit_multi whose frames are lit ones (hmrm_record_orbit_shaded): `sun` with diffuse / shadows as in
    Scene.render_shaded, aa the antialias factor.  sun=None records plain frames (diffuse and shadows are not looked at)."""
    for s in scenes:
        s._sync_env()
    arr = (C.c_void_p * len(scenes))(*[s._h for s in scenes])
    _check(lib.hmrm_record_orbit_shaded(arr, len(scenes), C.byref(base), centre_x, centre_y, radius, hang0, frames,
                                        os.fsencode(directory), rec_id, encoder_threads, int(verbose), aa_flags(aa),
                                        C.byref(sun) if sun is not None else None,
                                        shade_flags(diffuse, shadows) if sun is not None else 0),
           allow=(HMRM_E_NOTERM,))


def record_orbit_water(scenes, base: Camera, centre_x, centre_y, radius, hang0, frames, directory, rec_id, water: Water, baked=False,
                       aa=1, encoder_threads=0, verbose=False):
    """record_orbit_multi whose frames are water ones (hmrm_record_orbit_water); baked=True: under the light plane, which every
    scene then needs."""
    for s in scenes:
        s._sync_env()
    arr = (C.c_void_p * len(scenes))(*[s._h for s in scenes])
    _check(lib.hmrm_record_orbit_water(arr, len(scenes), C.byref(base), centre_x, centre_y, radius, hang0, frames,
                                       os.fsencode(directory), rec_id, encoder_threads, int(verbose), aa_flags(aa),
                                       C.byref(water), WATER_BAKED if baked else 0),
           allow=(HMRM_E_NOTERM,))


def record_orbit_baked(scenes, base: Camera, centre_x, centre_y, radius, hang0, frames, directory, rec_id, interior=False, aa=1,
                       encoder_threads=0, verbose=False):
    """record_orbit_multi whose frames are baked-light ones (hmrm_record_orbit_baked): every scene needs a light plane."""
    for s in scenes:
        s._sync_env()
    arr = (C.c_void_p * len(scenes))(*[s._h for s in scenes])
    _check(lib.hmrm_record_orbit_baked(arr, len(scenes), C.byref(base), centre_x, centre_y, radius, hang0, frames,
                                       os.fsencode(directory), rec_id, encoder_threads, int(verbose), aa_flags(aa),
                                       TRACE_INTERIOR if interior else 0),
           allow=(HMRM_E_NOTERM,))


def render_multi(scenes, cam: Camera, allow_capped=False) -> np.ndarray:
    """One frame over several scenes (one per GPU): scene i renders the cyclic 16-row bands i, i+n, ..."""
    for s in scenes:
        s._sync_env()
    arr = (C.c_void_p * len(scenes))(*[s._h for s in scenes])
    fb = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
    _check(lib.hmrm_render_multi(arr, len(scenes), C.byref(cam), _ptr(fb), cam.width * 4),
           allow=(HMRM_E_NOTERM,) if allow_capped else ())
    return fb


def orbit_frame_owner(frame: int, n_devices: int) -> int:
    return int(lib.hmrm_orbit_frame_owner(frame, n_devices))


def band_local_rows(height, band_rows, band_index, band_count) -> int:
    return int(lib.hmrm_band_local_rows(height, band_rows, band_index, band_count))


class Config:
    """The reference's config grammar (ConsumeConfigStream, hmap.cpp:309-520)."""

    def __init__(self):
        self._h = C.c_void_p(lib.hmrm_config_create())

    def close(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.hmrm_config_destroy(self._h)
            self._h = None

    __del__ = close

    def consume_string(self, text: str):
        _check(lib.hmrm_config_consume_string(self._h, text.encode()))
        return self

    def consume_file(self, path: str):
        _check(lib.hmrm_config_consume_file(self._h, os.fsencode(path)))
        return self

    @property
    def log(self) -> str:
        return lib.hmrm_config_log(self._h).decode()

    @property
    def warnings(self) -> str:
        return lib.hmrm_config_warnings(self._h).decode()

    def camera(self) -> Camera:
        c = Camera()
        lib.hmrm_config_get_camera(self._h, C.byref(c))
        return c

    def scene_params(self) -> SceneParams:
        p = SceneParams()
        lib.hmrm_config_get_scene_params(self._h, C.byref(p))
        return p

    @property
    def cycle(self) -> int:
        return lib.hmrm_config_cycle(self._h)

    @property
    def recording_frame_count(self) -> int:
        return lib.hmrm_config_recording_frame_count(self._h)

    @property
    def heightmap_path(self) -> str:
        return lib.hmrm_config_heightmap_path(self._h).decode()

    @property
    def colormap_path(self) -> str:
        return lib.hmrm_config_colormap_path(self._h).decode()

    @property
    def record_mode(self) -> int:
        return lib.hmrm_config_record_mode(self._h)

    @property
    def devices(self) -> int:
        return lib.hmrm_config_devices(self._h)

    def antialias(self) -> int:
        """Additive `antialias n`: hmrm_render_aa's factor (1 = off)."""
        return int(lib.hmrm_config_antialias(self._h))

    def interior(self) -> bool:
        """Additive `interior on|off`: the CLI renders its single frame with hmrm_render_interior."""
        return bool(lib.hmrm_config_interior(self._h))

    def shadows(self) -> bool:
        """Additive `shadows on|off`: the CLI renders its single frame with hmrm_render_lit."""
        return bool(lib.hmrm_config_shadows(self._h))

    def shading(self) -> bool:
        """Additive `shading on|off`: the CLI renders its single frame with hmrm_render_shaded."""
        return bool(lib.hmrm_config_shading(self._h))

    def baked_light(self) -> int:
        """`baked_light off|sun|sky`: 0, 1 or 2."""
        return int(lib.hmrm_config_baked_light(self._h))

    def sky_light(self) -> bool:
        """Additive `sky_light on|off`: the CLI renders its single frame with hmrm_render_lit_sum over the sky directions of
        `sky_map_rings`."""
        return bool(lib.hmrm_config_sky_light(self._h))

    def sun_scope(self) -> int:
        """Additive `sun_scope single|all`: 0 | 1 -- whether shadows / shading also apply to antialiased and recorded frames."""
        return int(lib.hmrm_config_sun_scope(self._h))

    def sun_map_path(self) -> str:
        """Additive `sun_map <path.png>`: where the CLI writes the whole map's light map (Scene.cell_map with weight=True)."""
        return lib.hmrm_config_sun_map_path(self._h).decode()

    def sky_map_path(self) -> str:
        """Additive `sky_map <path.png>`: where the CLI writes the whole map's sky-view map (Scene.cell_map_sum over sky_directions)."""
        return lib.hmrm_config_sky_map_path(self._h).decode()

    def range_map_path(self) -> str:
        """Additive `range_map <path.pfm>`: where the CLI writes the camera's range plane (Scene.render_geometry); "" = none."""
        return lib.hmrm_config_range_map_path(self._h).decode()

    def sky_map_rings(self):
        """Additive `sky_map_rings r n`: (rings, per_ring) of that map's sky_directions."""
        r, n = C.c_int32(0), C.c_int32(0)
        lib.hmrm_config_sky_map_rings(self._h, C.byref(r), C.byref(n))
        return int(r.value), int(n.value)

    def sun_map_lift(self) -> float:
        """Additive `sun_map_lift v`: how far above the surface the rays of that map start."""
        return float(lib.hmrm_config_sun_map_lift(self._h))

    def sun(self) -> Sun:
        """The sun of the additive keys sun_dir, shadow_step_dist (absent: step_dist), shadow_max_steps, shadow_ambient, interior."""
        out = Sun()
        lib.hmrm_config_get_sun(self._h, C.byref(out))
        return out

    def water_scope(self) -> int:
        """Additive `water_scope frame|all`: 0 | 1 -- whether water also applies to antialiased, recorded and baked-light frames."""
        return int(lib.hmrm_config_water_scope(self._h))

    def water_light(self) -> int:
        """Additive `water_light off|sun`: 0 | 1 -- whether `water on` beside shadows / shading is the sun-lit water frame."""
        return int(lib.hmrm_config_water_light(self._h))

    def water_on(self) -> bool:
        """Additive `water on|off`: the CLI renders its single frame with hmrm_render_water."""
        return bool(lib.hmrm_config_water(self._h))

    def water(self) -> Water:
        """The water of the additive keys water_level, water_step_dist (absent: step_dist), water_max_steps, water_reflectivity,
        water_color (sets HMRM_WATER_OWN_COLOR), interior."""
        out = Water()
        lib.hmrm_config_get_water(self._h, C.byref(out))
        return out

    def haze_on(self) -> bool:
        """Additive `haze on|off`: the CLI renders its single frame with hmrm_render_haze."""
        return bool(lib.hmrm_config_haze(self._h))

    def haze(self):
        """The haze of the additive keys haze_start, haze_far, haze_entries, haze_color, haze_sky, interior, and its table
        (haze_law, haze_density) -> (Haze, uint8 array of haze.n entries)."""
        out = Haze()
        table = np.zeros(MAX_HAZE_ENTRIES, dtype=np.uint8)
        lib.hmrm_config_get_haze(self._h, C.byref(out), table.ctypes.data)
        return out, table[:int(out.n)].copy()

    def haze_law(self) -> int:
        """Additive `haze_law linear|exp|exp2`: HAZE_LINEAR | HAZE_EXP | HAZE_EXP2."""
        return int(lib.hmrm_config_haze_law(self._h))

    def haze_density(self) -> float:
        return float(lib.hmrm_config_haze_density(self._h))

    def haze_far(self) -> float:
        return float(lib.hmrm_config_haze_far(self._h))

    def views(self):
        """The cameras of the additive `view x y z hang vang` lines (at most 64): the main camera with each line's position and
        angles -> list of Camera."""
        n = int(lib.hmrm_config_view_count(self._h))
        arr = (Camera * max(n, 1))()
        lib.hmrm_config_get_views(self._h, arr)
        return [arr[k] for k in range(n)]

    @property
    def views_output(self) -> str:
        """Additive `views_output <prefix>`: "" = none."""
        return lib.hmrm_config_views_output(self._h).decode()

    @property
    def output_path(self) -> str:
        return lib.hmrm_config_output_path(self._h).decode()

    def take_heightmap_dirty(self) -> bool:
        return bool(lib.hmrm_config_take_heightmap_dirty(self._h))

    def _map(self, fn, comp):
        w, h = C.c_int32(), C.c_int32()
        p = fn(self._h, C.byref(w), C.byref(h))
        if not p:
            return None
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, comp)).copy()

    def height_rgb(self):
        return self._map(lib.hmrm_config_height_rgb, 3)

    def color_rgba(self):
        return self._map(lib.hmrm_config_color_rgba, 4)

    def create_scene(self) -> Scene:
        h = C.c_void_p()
        _check(lib.hmrm_config_create_scene(self._h, C.byref(h)))
        rgb = self.height_rgb()
        return Scene._adopt(h, rgb.shape[1], rgb.shape[0], self.scene_params())


def image_load(path: str, req_comp: int):
    """stbi_load(path,&w,&h,&n,req_comp) replacement -> (HxWxC uint8, channels_in_file)."""
    out = C.POINTER(C.c_uint8)()
    w, h, n = C.c_int32(), C.c_int32(), C.c_int32()
    _check(lib.hmrm_image_load(os.fsencode(path), req_comp, C.byref(out), C.byref(w), C.byref(h), C.byref(n)))
    comp = req_comp if req_comp else n.value
    arr = np.ctypeslib.as_array(out, shape=(h.value, w.value, comp)).copy()
    lib.hmrm_image_free(out)
    return arr, n.value


def image_load_memory(data: bytes, req_comp: int):
    out = C.POINTER(C.c_uint8)()
    w, h, n = C.c_int32(), C.c_int32(), C.c_int32()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    _check(lib.hmrm_image_load_memory(buf, len(data), req_comp, C.byref(out), C.byref(w), C.byref(h), C.byref(n)))
    comp = req_comp if req_comp else n.value
    arr = np.ctypeslib.as_array(out, shape=(h.value, w.value, comp)).copy()
    lib.hmrm_image_free(out)
    return arr, n.value


def png_encode(img: np.ndarray) -> bytes:
    """stbi_write_png_to_mem replacement (same bytes as stb_image_write v1.16)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim == 2:
        img = img[:, :, None]
    h, w, comp = img.shape
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t()
    _check(lib.hmrm_write_png_memory(w, h, comp, _ptr(img), w * comp, C.byref(out), C.byref(n)))
    data = bytes(np.ctypeslib.as_array(out, shape=(n.value,)))
    lib.hmrm_image_free(out)
    return data


def write_png(path: str, img: np.ndarray):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w, comp = img.shape
    _check(lib.hmrm_write_png(os.fsencode(path), w, h, comp, _ptr(img), w * comp))


def write_ppm(path: str, img: np.ndarray):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w, comp = img.shape
    _check(lib.hmrm_write_ppm(os.fsencode(path), w, h, comp, _ptr(img), w * comp))


def write_pfm(path: str, img: np.ndarray):
    """hmrm_write_pfm: an (h, w) or (h, w, 1) float32 array as "Pf", an (h, w, 3) one as "PF"; rows bottom to top, scale -1.0."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    h, w = img.shape[:2]
    comp = 1 if img.ndim == 2 else img.shape[2]
    _check(lib.hmrm_write_pfm(os.fsencode(path), w, h, comp, _ptr(img), w * comp * 4))
