"""Antialiased, ticketed, recorded and baked-light water frames (hmrm_render_water_aa, hmrm_render_water_begin,
hmrm_render_water_device_begin, hmrm_record_orbit_water; include/hmrm.h) -- what needs no GPU: the replay of
tests/water_pipeline_cases.py pinned by its four identities to the water and the baked replays that exist and to a scalar loop of
one pixel at a time, the counts of every camera tests/test_water_pipeline_gpu.py uses, the constants and signatures against the
header, the refusals that need no scene, and the config key water_scope."""
import ctypes as C
import os
import re
from importlib import import_module

import numpy as np
import pytest

import baked_cases as bc
import segment_replay as sr
import water_cases as wc
import water_pipeline_cases as wp
import water_replay as wr
from baked_cases import FULL_SCALE
from segment_cases import BG, GRID_WIDTHS, GW_IDS, MAP_H, MAP_W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def replays(hmrm, oracle):
    return wp.Replays(hmrm, oracle)


@pytest.fixture(scope="module")
def baked_lake(hmrm, oracle, replays):
    """tests/baked_cases.py's replay over the lake map (its maps are set before any frame is replayed)."""
    b = bc.Replays(hmrm, oracle)
    b.rgb = replays.rgb
    b.heights = replays.heights
    return b


# ---- the replay's four identities ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
def test_identities(replays, baked_lake, gw):
    """L = D everywhere is the water replay; a level below every threshold and r = 0 without own colour are the baked replay;
    without BAKED at factor 1 the frame is the water replay's."""
    full = np.full((MAP_H, MAP_W), 777, dtype=np.uint16)
    below = float(replays.params[gw].min_height) - 1.0
    for proj in (1, 2, 3):
        for sampling in (0, 1, 2):
            plain = replays.water(gw, proj, sampling)
            baked = baked_lake.baked(gw, proj, sampling)
            assert plain["water"].sum() >= 34 and baked["hit"].sum() >= 100
            assert replays.frame(gw, proj, sampling, True, full, 777)["rgba"].tobytes() == plain["rgba"].tobytes()
            assert replays.frame(gw, proj, sampling, True, level=below)["rgba"].tobytes() == baked["rgba"].tobytes()
            assert replays.frame(gw, proj, sampling, True, reflectivity=0)["rgba"].tobytes() == baked["rgba"].tobytes()
            assert replays.frame(gw, proj, sampling, False)["rgba"].tobytes() == plain["rgba"].tobytes()
            # ... and the composition is none of them: the light reaches the water pixels, through both terms
            got = replays.frame(gw, proj, sampling, True)
            wet = plain["water"]
            assert (got["rgba"][wet] != plain["rgba"][wet]).any(axis=1).sum() >= 30
            assert (got["rgba"][wet] != baked["rgba"][wet]).any(axis=1).sum() >= 30
            # own colour with r = 0: the colour under the primary hit's light, whatever the mirror ray found
            own = replays.frame(gw, proj, sampling, True, reflectivity=0, color=(40, 80, 160))
            want = bc.pixel(np.array([40, 80, 160]), own["light"][wet, None], FULL_SCALE)
            assert np.array_equal(own["rgba"][wet, 0:3], want) and (own["rgba"][:, 3] == 255).all()
            assert own["rgba"][~wet].tobytes() == baked["rgba"][~wet].tobytes()


def test_of_camera_is_the_cache(hmrm, replays):
    """The replay of any camera (the recorder's and the capped rays' tests use it) gives the cached frames of the base cameras."""
    import segment_cases as sc
    gw = 0.5
    for proj, sampling, n in ((1, 0, 1), (2, 1, 2), (3, 2, 2)):
        cam = sc.camera(hmrm, gw, proj, False, sampling, width=20, height=15)
        for baked in (False, True):
            got, _ = replays.of_camera(cam, gw, replays.level(gw), n=n, baked=baked)
            assert got.tobytes() == replays.filtered(gw, proj, sampling, n, baked).tobytes(), (proj, sampling, n, baked)


# ---- one pixel at a time ----
def test_scalar_cross_check(replays):
    """Plain Python: segment_replay.scalar_ray twice, the plane's word of each hit cell, the pixel formula and the blend in
    integers -- every fourth pixel of the three base frames, nearest sampling, with a mirror limit and once with an own colour."""
    gw = 0.5
    params, heights, cmap, plane = replays.params[gw], replays.heights[gw], replays.cmap, replays.plane
    L, cap, r, D = 25, 700, 100, FULL_SCALE
    level = replays.level(gw)
    weight = lambda c, light: tuple(min(255, (int(v) * light + D // 2) // D) for v in c[:3])
    n = wet_n = swapped = 0
    seen = set()
    for proj, color in zip((1, 2, 3), (None, (10, 20, 30), None)):
        rays = replays.rays(gw, proj)
        want = replays.frame(gw, proj, 0, True, step_cap=cap, max_steps=L, reflectivity=r, color=color, mirror_step=0.3 * gw)
        for i in range(0, rays.shape[0], 4):
            status, _s, point, cell, rgba, _d = sr.scalar_ray(rays[i], heights, cmap, params, 0.2 * gw, BG, cap, False, 0)
            rgba = tuple(int(v) for v in rgba)
            if status == sr.HIT:
                t = float(heights[cell[1], cell[0]]) + float(params.min_height)
                lp = int(plane[cell[1], cell[0]])
                if t <= level:
                    mray = (point[0], point[1], t, float(rays[i, 3]), float(rays[i, 4]), -float(rays[i, 5]))
                    m_status, _s2, _p, mcell, m, _d2 = sr.scalar_ray(mray, heights, cmap, params, 0.3 * gw, BG, cap, True, L)
                    seen.add(m_status)
                    m = tuple(int(v) for v in m)
                    if m_status == sr.HIT:
                        lm = int(plane[mcell[1], mcell[0]])
                        swapped += lm != lp
                        m = weight(m, lm)
                    b = weight(rgba if color is None else color, lp)
                    rgba = tuple((b[k] * (255 - r) + m[k] * r + 127) // 255 for k in range(3)) + (255,)
                    wet_n += 1
                else:
                    rgba = weight(rgba, lp) + (255,)
            assert tuple(int(v) for v in want["rgba"][i]) == rgba, (proj, i)
            n += 1
    assert n == 900 and wet_n >= 50 and swapped >= 5 and seen == {sr.MISS, sr.HIT, sr.END}


# ---- the counts of every camera the GPU module uses ----
# (water samples, mirror hits, mirror misses, capped) per sampling mode 0, 1, 2 -- the same at every grid width
BASE_COUNTS = {1: ((91, 21, 70, 0), (79, 9, 70, 0), (91, 21, 70, 0)), 2: ((38, 11, 27, 0), (34, 5, 29, 0), (38, 11, 27, 0)),
               3: ((136, 59, 77, 0), (131, 36, 95, 0), (136, 59, 77, 0))}
INSIDE_SPHERICAL = ((344, 48, 296, 0), (275, 14, 261, 0), (344, 48, 296, 0))
FACTOR_4 = {1: ((382, 99, 283, 0), (352, 57, 295, 0), (382, 99, 283, 0)), 2: ((1362, 190, 1172, 0), (1073, 52, 1021, 0), (1362, 190, 1172, 0)),
            3: ((191, 79, 112, 0), (180, 40, 140, 0), (191, 79, 112, 0))}
# (output pixels whose block mixes wet and dry samples, ... hit and miss samples)
BASE_MIXES_2 = {1: ((21, 36), (23, 34), (21, 36)), 2: ((16, 22), (16, 21), (16, 22)), 3: ((53, 23), (56, 22), (53, 23))}
MIXES_2 = {**BASE_MIXES_2, 2: ((23, 13), (31, 11), (23, 13))}  # (the antialiased cases' spherical camera is the inside one)
MIXES_4 = {1: ((47, 45), (42, 45), (47, 45)), 2: ((35, 20), (40, 21), (35, 20)), 3: ((49, 34), (50, 34), (49, 34))}
FACTOR_8 = (((641, 162, 479, 0), (34, 31)), ((591, 96, 495, 0), (33, 31)))
ODD = {1: ((613, 164, 449, 0), (556, 89, 467, 0), (613, 164, 449, 0)), 2: ((236, 51, 185, 0), (213, 21, 192, 0), (236, 51, 185, 0)),
       3: ((190, 69, 121, 0), (170, 37, 133, 0), (190, 69, 121, 0))}
AA_CASES = tuple(zip(GRID_WIDTHS, (1, 2, 3), (False, True, False)))  # (as tests/test_baked_gpu.py zips them)


def floors(counts, differs):
    water, hit, miss, capped = counts
    return water >= 34 and hit >= 5 and miss >= 27 and capped == 0 and differs >= 5


@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
def test_base_counts(replays, gw):
    """Every base case at 40 x 30 -- which is also the factor-2 super frame of the 20 x 15 cameras: the water module's minima,
    at least 5 mirror hits under another light word than their primary hit's (here: every one of them), and blocks of 2 x 2
    samples that mix wet and dry, hit and miss."""
    for proj in (1, 2, 3):
        for sampling in (0, 1, 2):
            got = replays.frame(gw, proj, sampling, True)
            counts, differs = wc.counts(got["water"]), wp.light_differs(got)
            assert counts == BASE_COUNTS[proj][sampling] and differs == counts[1] and floors(counts, differs), (proj, sampling, counts, differs)
            mixes = wp.block_mixes(got["water"], 20, 15, 2)
            assert mixes == BASE_MIXES_2[proj][sampling] and mixes[0] >= 3 and mixes[1] >= 1, (proj, sampling, mixes)


def test_antialiased_counts(replays):
    for gw, proj, inside in AA_CASES:
        for sampling in (0, 1, 2):
            for n, table, mix_table in ((2, INSIDE_SPHERICAL if inside else BASE_COUNTS[proj], MIXES_2[proj]), (4, FACTOR_4[proj], MIXES_4[proj])):
                got = replays.frame(gw, proj, sampling, True, inside=inside, width=20 * n, height=15 * n)
                counts, differs, mixes = wc.counts(got["water"]), wp.light_differs(got), wp.block_mixes(got["water"], 20, 15, n)
                assert counts == table[sampling] and floors(counts, differs), (n, proj, sampling, counts, differs)
                assert mixes == mix_table[sampling] and mixes[0] >= 3 and mixes[1] >= 1, (n, proj, sampling, mixes)
    for sampling in (0, 1):  # factor 8 at 13 x 9: the super frame is 104 x 72
        got = replays.frame(0.5, 1, sampling, True, width=104, height=72)
        counts, differs, mixes = wc.counts(got["water"]), wp.light_differs(got), wp.block_mixes(got["water"], 13, 9, 8)
        assert (counts, mixes) == FACTOR_8[sampling] and floors(counts, differs) and mixes[0] >= 3 and mixes[1] >= 1


def test_odd_frame_counts(replays):
    """101 x 67: at least one 8 x 8 wave tile holds wet, dry and miss lanes."""
    gw = 0.5
    for proj in (1, 2, 3):
        for sampling in (0, 1, 2):
            got = replays.frame(gw, proj, sampling, True, width=101, height=67)
            counts, differs = wc.counts(got["water"]), wp.light_differs(got)
            assert counts == ODD[proj][sampling] and floors(counts, differs), (proj, sampling, counts)
            want = got["water"]
            kind = np.where(want["water"], 2, np.where(want["primary"]["status"] == wr.HIT, 1, 0)).reshape(67, 101)
            mixed = sum(1 for y in range(0, 67, 8) for x in range(0, 101, 8) if np.unique(kind[y:y + 8, x:x + 8]).size == 3)
            assert mixed >= 1, (proj, sampling)


# ---- the wrappers against the header ----
def test_constants_and_signatures_against_the_header(hmrm):
    header = open(os.path.join(ROOT, "include", "hmrm.h")).read()
    m = re.search(r"#define\s+HMRM_WATER_BAKED\s+(\d+)u", header)
    assert m and int(m.group(1)) == hmrm.WATER_BAKED == 1
    assert int(re.search(r"#define\s+HMRM_WATER_OWN_COLOR\s+(\d+)u", header).group(1)) == hmrm.WATER_OWN_COLOR
    lib = import_module("heightmap-ray-marcher_amd.lib").lib
    for name in ("hmrm_render_water_aa", "hmrm_render_water_begin", "hmrm_render_water_device_begin", "hmrm_record_orbit_water",
                 "hmrm_config_water_scope"):
        assert name in hmrm.EXPORTED_SYMBOLS
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(getattr(lib, name).argtypes), name
    assert "uint32_t water_mode" in re.search(r"hmrm_render_water_aa\s*\(([^;]*)\)", header).group(1)
    for method in ("render_water_aa", "render_water_begin", "render_water_device_begin"):
        assert callable(getattr(hmrm.Scene, method))
    assert callable(hmrm.record_orbit_water) and callable(hmrm.Config.water_scope)
    lib_py = import_module("heightmap-ray-marcher_amd.lib")
    for unit in ("render_water_aa.hip", "render_water_baked.hip", "render_water_baked_aa.hip"):
        assert unit in lib_py.KERNEL_SOURCES and os.path.exists(os.path.join(ROOT, "heightmap-ray-marcher_amd", "csrc", unit))


# ---- refusals that need no scene ----
def test_refusals_need_no_scene(hmrm, tmp_path):
    """For all four entry points, with scene = NULL: NULL water, an undefined flag bit and reserved bytes; then an undefined bit
    of water_mode; then hmrm_render_aa's (tickets: hmrm_render_begin_flags') in their order -- the camera before the factor --
    and only then the NULL scene.  The recorder refuses water and mode before its own arguments and writes nothing."""
    lib_py = import_module("heightmap-ray-marcher_amd.lib")
    lib = lib_py.lib
    E = hmrm.HMRM_E_ARG
    fb = np.zeros((8, 8, 4), dtype=np.uint8)
    good_cam, bad_cam = hmrm.Camera.make(width=8, height=8), hmrm.Camera.make(width=0, height=8)
    good = hmrm.Water.make(1.0, 0.1)
    ticket = C.c_int32(7)
    # (cam, water, mode, factor) -> rc, for the three frame entry points; the ticketed ones take the factor in their flags
    forms = {
        "aa": lambda c, w, mode, n: lib.hmrm_render_water_aa(None, c, w, mode, n, fb.ctypes.data, 32),
        "begin": lambda c, w, mode, n: lib.hmrm_render_water_begin(None, c, w, mode, lib_py.aa_flags(n), C.byref(ticket)),
        "device_begin": lambda c, w, mode, n: lib.hmrm_render_water_device_begin(None, c, w, mode, fb.ctypes.data, 32, lib_py.aa_flags(n),
                                                                                 C.byref(ticket)),
    }
    for name, call in forms.items():
        def refused(word, *args):
            assert call(*args) == E and word in hmrm.last_error(), (name, word, hmrm.last_error())
        refused("NULL water", C.byref(bad_cam), None, 2, 3)
        bad = hmrm.Water.make(1.0, 0.1)
        bad.flags |= 4
        bad.reserved[1] = 1
        refused("flags: undefined bit", C.byref(bad_cam), C.byref(bad), 2, 3)
        bad = hmrm.Water.make(1.0, 0.1)
        bad.reserved[3] = 1
        refused("reserved", C.byref(bad_cam), C.byref(bad), 2, 3)
        for mode in (2, 4, 0x80000000, 3):
            refused("water_mode: undefined bit", C.byref(bad_cam), C.byref(good), mode, 3)
        for mode in (0, hmrm.WATER_BAKED):
            refused("resolution", C.byref(bad_cam), C.byref(good), mode, 3)
            refused("camera is NULL", None, C.byref(good), mode, 3)
            refused("antialias factor", C.byref(good_cam), C.byref(good), mode, 3)
            for n in (1, 2, 4, 8):
                refused("NULL argument", C.byref(good_cam), C.byref(good), mode, n)
    # the tickets' flags: an unknown bit comes behind the camera and ahead of the scene
    assert lib.hmrm_render_water_begin(None, C.byref(good_cam), C.byref(good), 0, 0x10000, C.byref(ticket)) == E and "flags" in hmrm.last_error()
    assert lib.hmrm_render_water_begin(None, C.byref(bad_cam), C.byref(good), 0, 0x10000, C.byref(ticket)) == E and "resolution" in hmrm.last_error()
    assert lib.hmrm_render_water_begin(None, C.byref(good_cam), C.byref(good), 0, lib_py.NO_PROBE, C.byref(ticket)) == E \
        and "NULL argument" in hmrm.last_error()
    # the recorder
    rec = lambda w, mode, cam=bad_cam: lib.hmrm_record_orbit_water(None, 0, C.byref(cam), 0.0, 0.0, 1.0, 0.0, 2, os.fsencode(str(tmp_path)), 5, 1, 0,
                                                                   0, w, mode)
    assert rec(None, 2) == E and "NULL water" in hmrm.last_error()
    bad = hmrm.Water.make(1.0, 0.1)
    bad.flags |= 8
    assert rec(C.byref(bad), 2) == E and "flags: undefined bit" in hmrm.last_error()
    assert rec(C.byref(good), 2) == E and "water_mode: undefined bit" in hmrm.last_error()
    assert rec(C.byref(good), hmrm.WATER_BAKED) == E and "bad argument" in hmrm.last_error()
    assert not list(tmp_path.iterdir())


# ---- config ----
def test_config_water_scope(hmrm):
    cfg = hmrm.Config()
    lib = import_module("heightmap-ray-marcher_amd.lib").lib

    def feed(text):  # (the end-of-stream validation wants maps: its failure does not undo the keys)
        lib.hmrm_config_consume_string(cfg._h, text.encode())
        return lib.hmrm_config_log(cfg._h).decode(), lib.hmrm_config_warnings(cfg._h).decode()

    assert cfg.water_scope() == 0
    log, warn = feed("water_scope all\n")
    assert cfg.water_scope() == 1 and log.endswith("water_scope all\n") and "water_scope" not in warn
    log, warn = feed("water_scope everything\n")
    assert cfg.water_scope() == 1 and "WARNING: Unknown water_scope: everything\n" in warn and log.endswith("water_scope all\n")
    log, warn = feed("water_scope frame\n")
    assert cfg.water_scope() == 0 and log.endswith("water_scope frame\n") and warn.count("water_scope") == 1
    assert cfg.water_on() is False  # (the scope alone turns nothing on)
    feed("water on\nwater_scope all\n")
    assert cfg.water_on() is True and cfg.water_scope() == 1
    cfg.close()
