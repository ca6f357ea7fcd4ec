"""Sun-lit water frames (hmrm_render_water_lit, hmrm_render_water_lit_device; include/hmrm.h) -- what needs no GPU: the replay of
tests/water_lit_replay.py pinned by the definition's four identities to the water, shaded and lit replays that exist (themselves
pinned to the C oracle) and to a scalar loop of one pixel at a time; the counts that keep tests/test_water_lit_gpu.py honest; the
constants and argument counts against the header; the refusals that need no scene, in the header's order; the config key
water_light."""
import ctypes as C
import math
import os
import re
from importlib import import_module

import numpy as np
import pytest

import lit_cases as lc
import segment_replay as sr
import shade_replay as sh
import water_lit_cases as wlc
import water_lit_replay as wl
from segment_cases import BG, GRID_WIDTHS, GW_IDS, MAP_H, MAP_W
from water_lit_cases import AMBIENT, FLOORS, REFLECTIVITY, sun_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def replays(hmrm, oracle):
    return wlc.Replays(hmrm, oracle)


@pytest.fixture(scope="module")
def lit_lake(hmrm, oracle, replays):
    """tests/lit_cases.py's replay over the lake map (its maps are set before any frame is replayed)."""
    b = lc.Replays(hmrm, oracle)
    b.rgb = replays.rgb
    b.heights = replays.heights
    return b


def shaded_of(replays, lit_lake, gw, proj, sampling, diffuse, shadows, ambient=AMBIENT):
    """hmrm_render_shaded's replay of the base camera over the lake map under the module's sun."""
    lit = lit_lake.lit(gw, proj, sampling, sun_of(proj), ambient=ambient) if shadows else None
    return sh.replay(replays.rays(gw, proj), replays.heights[gw], replays.cmap, replays.params[gw], 0.2 * gw, sun_of(proj), 0.3 * gw,
                     bg=BG, sampling=sampling, step_cap=wlc.BASE_CAP, ambient=ambient, diffuse=diffuse, shadows=shadows,
                     primary=replays.primary(gw, proj, sampling), lit=lit)


# ---- the four identities ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
def test_identities(replays, lit_lake, gw):
    """A level below every threshold or NaN, and r = 0 without own colour: the shaded replay (both flags off: the lit replay).
    HMRM_SHADE_NO_SHADOWS alone, and ambient = 255 under any flags: the water replay."""
    below = float(replays.params[gw].min_height) - 1.0
    for proj in (1, 2, 3):
        for sampling in (0, 1, 2):
            wet = replays.water(gw, proj, sampling)
            for diffuse, shadows in ((True, True), (False, True), (True, False)):
                shaded = shaded_of(replays, lit_lake, gw, proj, sampling, diffuse, shadows)
                for level in (below, float("nan")):
                    got = replays.frame(gw, proj, sampling, diffuse=diffuse, shadows=shadows, level=level)
                    assert got["water"].sum() == 0 and got["rgba"].tobytes() == shaded["rgba"].tobytes(), (proj, sampling, diffuse, shadows)
                    assert got["capped"] == shaded["capped"]
                got = replays.frame(gw, proj, sampling, diffuse=diffuse, shadows=shadows, reflectivity=0)
                assert got["water"].sum() >= 34 and got["rgba"].tobytes() == shaded["rgba"].tobytes(), (proj, sampling, diffuse, shadows)
                bright = replays.frame(gw, proj, sampling, diffuse=diffuse, shadows=shadows, ambient=255)
                assert bright["rgba"].tobytes() == wet["rgba"].tobytes(), (proj, sampling, diffuse, shadows)
                if shadows:  # (the shadow rays are marched all the same)
                    assert bright["shadowed"].sum() >= 2 and bright["mirror_shadowed"].sum() >= 2
            lit = lit_lake.lit(gw, proj, sampling, sun_of(proj), ambient=AMBIENT)
            assert replays.frame(gw, proj, sampling, diffuse=False, level=below)["rgba"].tobytes() == lit["rgba"].tobytes()
            assert replays.frame(gw, proj, sampling, diffuse=False, shadows=False)["rgba"].tobytes() == wet["rgba"].tobytes()
            # ... and the composition is neither of them: the sun reaches the water pixels, through both terms
            got = replays.frame(gw, proj, sampling)
            shaded = shaded_of(replays, lit_lake, gw, proj, sampling, True, True)
            w = wet["water"]
            assert (got["rgba"][w] != wet["rgba"][w]).any(axis=1).sum() >= 30
            assert (got["rgba"][w] != shaded["rgba"][w]).any(axis=1).sum() >= 20
            assert got["rgba"][~w].tobytes() == shaded["rgba"][~w].tobytes()
            # own colour with r = 0: the colour under the primary hit's weight, whatever the mirror ray found
            own = replays.frame(gw, proj, sampling, reflectivity=0, color=(40, 80, 160))
            want = (np.array([40, 80, 160], dtype=np.int64)[None, :] * own["w"][w, None] + 127) // 255
            assert np.array_equal(own["rgba"][w, 0:3], want) and (own["rgba"][:, 3] == 255).all()


# ---- one pixel at a time ----
def scalar_level(cell, heights, params, sun):
    """q of a hit cell, nearest sampling: the header's operations one by one in Python floats."""
    cx, cy = cell
    gw = float(params.grid_width)
    t = lambda x, y: float(heights[y, x]) + float(params.min_height)
    xm, xp, ym, yp = max(cx - 1, 0), min(cx + 1, MAP_W - 1), max(cy - 1, 0), min(cy + 1, MAP_H - 1)
    gx = (t(xp, cy) - t(xm, cy)) / (float(xp - xm) * gw) if xp > xm else 0.0
    gy = (t(cx, yp) - t(cx, ym)) / (float(yp - ym) * gw) if yp > ym else 0.0
    nx, ny = -gx, gy
    dot = (nx * sun[0] + ny * sun[1]) + sun[2]
    length = math.sqrt(((nx * nx + ny * ny) + 1.0) * ((sun[0] * sun[0] + sun[1] * sun[1]) + sun[2] * sun[2]))
    k = dot / length
    k = (k if k < 1.0 else 1.0) if k > 0.0 else 0.0
    return int(k * 255.0 + 0.5)


def test_scalar_cross_check(replays):
    """Plain Python: segment_replay.scalar_ray up to four times per pixel, the level of each hit cell, the weight and the blend in
    integers -- every fourth pixel of the three base frames, nearest sampling, with limits on the sun's and the water's rays,
    once with an own colour, once without shadow rays and once without diffuse levels."""
    gw = 0.5
    params, heights, cmap = replays.params[gw], replays.heights[gw], replays.cmap
    L_sun, L_water, cap, r, amb = 40, 25, 700, 100, 70
    level = replays.level(gw)
    n = wet_n = swapped = 0
    seen, seen_shadow = set(), set()

    def weight_of(point, cell, t, sun, diffuse, shadows):
        if shadows:
            status = sr.scalar_ray((point[0], point[1], t) + tuple(sun), heights, cmap, params, 0.3 * gw, BG, cap, True, L_sun)[0]
            seen_shadow.add(status)
            if status == sr.HIT:
                return amb
        return amb + ((255 - amb) * scalar_level(cell, heights, params, sun) + 127) // 255 if diffuse else 255

    weigh = lambda c, w: tuple((int(v) * w + 127) // 255 for v in c[:3])
    for proj, color, diffuse, shadows in zip((1, 2, 3), (None, (10, 20, 30), None), (True, True, False), (True, False, True)):
        sun = sun_of(proj)
        rays = replays.rays(gw, proj)
        want = replays.frame(gw, proj, 0, diffuse=diffuse, shadows=shadows, step_cap=cap, max_steps=L_water, reflectivity=r, color=color,
                             mirror_step=0.3 * gw, sun_max_steps=L_sun, ambient=amb)
        for i in range(0, rays.shape[0], 4):
            status, _s, point, cell, rgba, _d = sr.scalar_ray(rays[i], heights, cmap, params, 0.2 * gw, BG, cap, False, 0)
            rgba = tuple(int(v) for v in rgba)
            if status == sr.HIT:
                t = float(heights[cell[1], cell[0]]) + float(params.min_height)
                wp = weight_of(point, cell, t, sun, diffuse, shadows)
                if t <= level:
                    mray = (point[0], point[1], t, float(rays[i, 3]), float(rays[i, 4]), -float(rays[i, 5]))
                    m_status, _s2, mpoint, mcell, m, _d2 = sr.scalar_ray(mray, heights, cmap, params, 0.3 * gw, BG, cap, True, L_water)
                    seen.add(m_status)
                    m = tuple(int(v) for v in m)
                    if m_status == sr.HIT:
                        tm = float(heights[mcell[1], mcell[0]]) + float(params.min_height)
                        wm = weight_of(mpoint, mcell, tm, sun, diffuse, shadows)
                        swapped += wm != wp
                        m = weigh(m, wm)
                    b = weigh(rgba if color is None else color, wp)
                    rgba = tuple((b[k] * (255 - r) + m[k] * r + 127) // 255 for k in range(3)) + (255,)
                    wet_n += 1
                else:
                    rgba = weigh(rgba, wp) + (255,)
            assert tuple(int(v) for v in want["rgba"][i]) == rgba, (proj, i)
            n += 1
    assert n == 900 and wet_n >= 50 and swapped >= 5 and seen == {sr.MISS, sr.HIT, sr.END} and sr.HIT in seen_shadow and sr.MISS in seen_shadow


# ---- the counts that keep the GPU module honest ----
# Conditions on the replay alone, not measurements: every camera and sun of the GPU module's frames -- the base cameras at every grid
# width, the 101 x 67 cameras and the cameras inside the box, each under water_lit_cases.sun_of(projection) -- must show at least
# FLOORS = (34 water pixels, 5 mirror hits, 2 mirror hits shadowed, 2 mirror hits lit, 2 wet pixels whose primary hit is shadowed,
# 2 ... lit, 2 dry hits shadowed, 1 wave that holds a wet lane, a dry hit and a miss at once, 1 mirror hit whose weight differs from
# its primary hit's): a kernel that swaps the two weights, or skips one side's shadow rays, cannot pass.  (The GPU module's cases
# that change the water or the sun on purpose -- a level of -1 or +inf, a sun straight up, below the horizon, zero or NaN, sky only,
# straight down -- are what their names say and assert their own conditions.)  The counts found, per sampling mode 0, 1, 2:
BASE_COUNTS = {1: ((91, 21, 7, 14, 22, 69, 103, 7, 16), (79, 9, 5, 4, 10, 69, 138, 7, 7), (91, 21, 7, 14, 22, 69, 103, 7, 16)),
               2: ((38, 11, 2, 9, 10, 28, 27, 5, 8), (34, 5, 2, 3, 3, 31, 26, 5, 4), (38, 11, 2, 9, 10, 28, 27, 5, 8)),
               3: ((136, 59, 27, 32, 64, 72, 200, 6, 38), (131, 36, 20, 16, 55, 76, 234, 7, 24), (136, 59, 27, 32, 64, 72, 200, 6, 38))}
ODD_COUNTS = {1: ((613, 164, 72, 92, 157, 456, 692, 12, 109), (556, 89, 43, 46, 80, 476, 895, 12, 65), (613, 164, 72, 92, 157, 456, 692, 12, 109)),
              2: ((236, 51, 10, 41, 40, 196, 171, 6, 46), (213, 21, 10, 11, 24, 189, 205, 7, 16), (236, 51, 10, 41, 40, 196, 171, 6, 46)),
              3: ((190, 69, 34, 35, 83, 107, 244, 12, 39), (170, 37, 24, 13, 60, 110, 280, 12, 22), (190, 69, 34, 35, 83, 107, 244, 12, 39))}
INSIDE_COUNTS = {1: ((244, 42, 27, 15, 163, 81, 115, 1, 15), (214, 16, 13, 3, 125, 89, 137, 1, 5), (244, 42, 27, 15, 163, 81, 115, 1, 15)),
                 2: ((344, 48, 32, 16, 293, 51, 192, 3, 16), (275, 14, 5, 9, 222, 53, 246, 3, 12), (344, 48, 32, 16, 293, 51, 192, 3, 16)),
                 3: ((82, 43, 23, 20, 59, 23, 150, 9, 19), (66, 24, 14, 10, 43, 23, 160, 9, 10), (82, 43, 23, 20, 59, 23, 150, 9, 19))}


def meets(counts):
    return all(c >= f for c, f in zip(counts, FLOORS))


def test_floors_are_the_issues():
    assert FLOORS == (34, 5, 2, 2, 2, 2, 2, 1, 1)
    for proj, sun in wlc.SUNS.items():  # a low sun: 15 to 25 degrees above the horizon
        elevation = math.degrees(math.atan2(sun[2], math.hypot(sun[0], sun[1])))
        assert 14.9 <= elevation <= 25.0, (proj, elevation)


@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
def test_base_counts(replays, gw):
    for proj in (1, 2, 3):
        for sampling in (0, 1, 2):
            got = replays.frame(gw, proj, sampling)
            counts = wlc.counts(got)
            assert counts == BASE_COUNTS[proj][sampling] and meets(counts) and got["capped"] == 0, (proj, sampling, counts)
    # shadows only and shading only, once per projection: other frames on the same rays -- they differ from the frame with both at
    # least where a dry hit is shadowed or lit at another weight, and the floor for either kind of pixel is 2
    proj = GRID_WIDTHS.index(gw) + 1
    for sampling in (0, 1, 2):
        both = replays.frame(gw, proj, sampling)
        for diffuse, shadows in ((False, True), (True, False)):
            got = replays.frame(gw, proj, sampling, diffuse=diffuse, shadows=shadows)
            assert (got["rgba"] != both["rgba"]).any(axis=1).sum() >= 2 and got["water"].sum() >= 34, (proj, sampling, diffuse, shadows)
            assert meets(wlc.counts(got)) if shadows else got["shadowed"].sum() == 0


def test_odd_frame_counts(replays):
    gw = 0.5
    for proj in (1, 2, 3):
        for sampling in (0, 1, 2):
            counts = wlc.counts(replays.frame(gw, proj, sampling, width=101, height=67), 101)
            assert counts == ODD_COUNTS[proj][sampling] and meets(counts), (proj, sampling, counts)


def test_inside_counts(replays):
    for proj in (1, 2, 3):
        gw = GRID_WIDTHS[proj - 1]
        for sampling in (0, 1, 2):
            got = replays.inside_frame(gw, proj, sampling)
            counts = wlc.counts(got)
            assert counts == INSIDE_COUNTS[proj][sampling] and meets(counts) and got["capped"] == 0, (proj, sampling, counts)


def test_pass_structure_cases(replays):
    """What tests/test_water_lit_gpu.py's pass-structure cases rely on, in the replay alone."""
    gw = 0.5
    for proj in (1, 2, 3):
        every = replays.frame(gw, proj, 0, level=float("inf"), reflectivity=200)
        assert np.array_equal(every["water"], every["primary"]["status"] == wl.HIT) and every["mirror_shadowed"].sum() >= 2
        up = replays.frame(gw, proj, 0, sun=(0.0, 0.0, 1.0), sun_max_steps=40)
        assert up["shadowed"].sum() == 0 and up["mirror_shadowed"].sum() == 0 and up["capped"] == 0
        assert set(np.unique(up["shadow"]["status"])) <= {wl.END, wl.MISS}
        for direction in ((0.0, 0.0, 0.0), (float("nan"), 0.3, 0.5)):
            got = replays.frame(gw, proj, 0, sun=direction, sun_max_steps=60)
            hit = got["primary"]["status"] == wl.HIT
            assert (got["w"][hit & ~got["shadowed"]] == AMBIENT).all() and got["capped"] == 0  # (q = 0)
        low = replays.frame(gw, proj, 0, sun=(0.5, 0.5, -0.4))
        assert low["capped"] == 0 and low["shadowed"].sum() >= 2
        limits = replays.frame(gw, proj, 0, sun_max_steps=5, max_steps=11)
        ended = sum(int((limits[k]["status"] == wl.END).sum()) for k in ("shadow", "mirror", "mirror_shadow"))
        assert ended >= 5 and limits["capped"] == 0


# ---- the wrappers against the header ----
def test_constants_and_signatures_against_the_header(hmrm):
    header = open(os.path.join(ROOT, "include", "hmrm.h")).read()
    lib_py = import_module("heightmap-ray-marcher_amd.lib")
    lib = lib_py.lib
    for name, n_args in (("hmrm_render_water_lit", 7), ("hmrm_render_water_lit_device", 8), ("hmrm_config_water_light", 1)):
        assert name in hmrm.EXPORTED_SYMBOLS
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(getattr(lib, name).argtypes) == n_args, name
    for name in ("hmrm_render_water_lit", "hmrm_render_water_lit_device"):
        args = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert args.index("const hmrm_water *water") < args.index("const hmrm_sun *sun") < args.index("uint32_t shade_flags")
    assert int(re.search(r"#define\s+HMRM_SHADE_DIFFUSE\s+(\d+)u", header).group(1)) == lib_py.SHADE_DIFFUSE
    assert int(re.search(r"#define\s+HMRM_SHADE_NO_SHADOWS\s+(\d+)u", header).group(1)) == lib_py.SHADE_NO_SHADOWS
    assert int(re.search(r"#define\s+HMRM_WATER_OWN_COLOR\s+(\d+)u", header).group(1)) == hmrm.WATER_OWN_COLOR
    assert "THE SUN-LIT WATER FRAME composes hmrm_render_water and hmrm_render_shaded and adds nothing." in header
    assert callable(hmrm.Scene.render_water_lit) and callable(hmrm.Scene.render_water_lit_device) and callable(hmrm.Config.water_light)
    assert "render_water_lit.hip" in lib_py.KERNEL_SOURCES
    assert os.path.exists(os.path.join(ROOT, "heightmap-ray-marcher_amd", "csrc", "render_water_lit.hip"))
    # the family goes at the end of FrameFamily, and DevFrame keeps its size
    dispatch = open(os.path.join(ROOT, "heightmap-ray-marcher_amd", "csrc", "march_dispatch.hpp")).read()
    assert re.search(r"enum FrameFamily \{[^}]*kFrameWaterBakedAA, kFrameWaterLit \};", dispatch)
    assert "sizeof(DevFrame) == 352" in open(os.path.join(ROOT, "heightmap-ray-marcher_amd", "csrc", "frame.hpp")).read()


# ---- refusals that need no scene ----
def test_refusals_need_no_scene(hmrm):
    """For both entry points, with scene = NULL: hmrm_render_water's three of the water; then hmrm_render_shaded's four of the sun
    and shade_flags; then as hmrm_render_water / hmrm_render_water_device -- the camera, and only then the NULL scene."""
    lib = import_module("heightmap-ray-marcher_amd.lib").lib
    E = hmrm.HMRM_E_ARG
    fb = np.zeros((8, 8, 4), dtype=np.uint8)
    good_cam, bad_cam = hmrm.Camera.make(width=8, height=8), hmrm.Camera.make(width=0, height=8)
    good_w, good_s = hmrm.Water.make(1.0, 0.1), hmrm.Sun.make((0.3, 0.2, 0.5), 0.1)
    forms = {
        "host": lambda c, w, s, flags: lib.hmrm_render_water_lit(None, c, w, s, flags, fb.ctypes.data, 32),
        "device": lambda c, w, s, flags: lib.hmrm_render_water_lit_device(None, c, w, s, flags, fb.ctypes.data, 32, None),
    }
    for name, call in forms.items():
        def refused(word, *args):
            assert call(*args) == E and word in hmrm.last_error(), (name, word, hmrm.last_error())
        bad_s = hmrm.Sun.make((0.3, 0.2, 0.5), 0.1)
        bad_s.flags |= 2
        # the water first, whatever else is wrong
        refused("NULL water", C.byref(bad_cam), None, None, 8)
        bad = hmrm.Water.make(1.0, 0.1)
        bad.flags |= 4
        bad.reserved[1] = 1
        refused("hmrm_water.flags: undefined bit", C.byref(bad_cam), C.byref(bad), C.byref(bad_s), 8)
        bad = hmrm.Water.make(1.0, 0.1)
        bad.reserved[3] = 1
        refused("hmrm_water.reserved", C.byref(bad_cam), C.byref(bad), None, 8)
        # then the sun and the flags
        refused("NULL sun", C.byref(bad_cam), C.byref(good_w), None, 8)
        bad_s.reserved[0] = 1
        refused("hmrm_sun.flags: undefined bit", C.byref(bad_cam), C.byref(good_w), C.byref(bad_s), 8)
        bad_s = hmrm.Sun.make((0.3, 0.2, 0.5), 0.1)
        bad_s.reserved[6] = 1
        refused("hmrm_sun.reserved", C.byref(bad_cam), C.byref(good_w), C.byref(bad_s), 8)
        for flags in (4, 8, 0x80000000, 7):
            refused("shade_flags: undefined bit", C.byref(bad_cam), C.byref(good_w), C.byref(good_s), flags)
        # then hmrm_render_water's: the camera, then the scene
        for flags in (0, 1, 2, 3):
            refused("resolution", C.byref(bad_cam), C.byref(good_w), C.byref(good_s), flags)
            refused("camera is NULL", None, C.byref(good_w), C.byref(good_s), flags)
            refused("NULL argument", C.byref(good_cam), C.byref(good_w), C.byref(good_s), flags)
    # HMRM_TRACE_INTERIOR is a defined bit of either flags word
    inside_w, inside_s = hmrm.Water.make(1.0, 0.1, interior=True), hmrm.Sun.make((0.3, 0.2, 0.5), 0.1, interior=True)
    assert forms["host"](C.byref(good_cam), C.byref(inside_w), C.byref(inside_s), 1) == E and "NULL argument" in hmrm.last_error()


# ---- config ----
def test_config_water_light(hmrm):
    cfg = hmrm.Config()
    lib = import_module("heightmap-ray-marcher_amd.lib").lib

    def feed(text):  # (the end-of-stream validation wants maps: its failure does not undo the keys)
        lib.hmrm_config_consume_string(cfg._h, text.encode())
        return lib.hmrm_config_log(cfg._h).decode(), lib.hmrm_config_warnings(cfg._h).decode()

    assert cfg.water_light() == 0
    log, warn = feed("water_light sun\n")
    assert cfg.water_light() == 1 and log.endswith("water_light sun\n") and "water_light" not in warn
    log, warn = feed("water_light moon\n")
    assert cfg.water_light() == 1 and "WARNING: Unknown water_light: moon\n" in warn and log.endswith("water_light sun\n")
    log, warn = feed("water_light off\n")
    assert cfg.water_light() == 0 and log.endswith("water_light off\n") and warn.count("water_light") == 1
    assert cfg.water_on() is False and cfg.water_scope() == 0  # (the key alone turns nothing on)
    feed("water on\nshadows on\nwater_light sun\n")
    assert cfg.water_on() is True and cfg.water_light() == 1 and cfg.water_scope() == 0
    cfg.close()
