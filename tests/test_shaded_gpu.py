"""Diffuse sun shading on the GPU (hmrm_render_shaded; include/hmrm.h).  Every frame is compared BYTEWISE with
tests/shade_replay.py, the definition in numpy, which tests/test_shaded_cpu.py pins to the lit replay, to the C oracle, to a
scalar loop and to a ramp's analytic normal; one test pins the kernels to hmrm_trace_rays records and the device's own
threshold table without the replay's march.  Map, grid widths and cameras are those of tests/segment_cases.py at 40 x 30
unless said otherwise, shadow step_dist 0.3 * grid width, ambient 96."""
import numpy as np
import pytest

import gpu_support as gs
import lit_replay as lr
import ray_replay
import segment_cases as sc
import segment_replay as sr
import shade_cases as shc
import shade_replay as shr
from gpu_support import KERNEL_VARIANTS, PROJ_IDS, SAMPLINGS, env, gpu, kernel_variant, same_frame, samplings_of
from segment_cases import BG, GRID_WIDTHS, GW_IDS, MAP_H, MAP_W
from shade_cases import AMBIENT, SUNS

pytestmark = pytest.mark.gpu

MODES = ((True, True), (True, False))  # (diffuse, shadows): HMRM_SHADE_DIFFUSE, HMRM_SHADE_DIFFUSE | HMRM_SHADE_NO_SHADOWS


class World(gs.Scenes, shc.Replays):
    pass


world = gs.world_fixture(World)


def sun_of(gpu, gw, direction, **kw):
    kw.setdefault("ambient", AMBIENT)
    return gpu.Sun.make(direction, kw.pop("step_dist", 0.3 * gw), **kw)


def lit_hits(want):
    return int(((want["primary"]["status"] == lr.HIT) & ~want["shadowed"]).sum())


# ---- 1. the base cases: 3 projections x 3 grid widths x 4 variants x 3 samplings x 3 suns, with and without shadows ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_shaded_frame_is_the_replay(world, proj, variant, gw):
    gpu, scene = world.gpu, world.scenes[gw]
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            cam = sc.camera(gpu, gw, proj, False, sampling)
            for sun in SUNS:
                for diffuse, shadows in MODES:
                    want = world.shaded(gw, proj, sampling, sun, diffuse, shadows)
                    assert lit_hits(want) >= 100 and want["capped"] == 0 and (not shadows or want["shadowed"].sum() >= 20)
                    fb = scene.render_shaded(cam, sun_of(gpu, gw, sun), diffuse=diffuse, shadows=shadows)
                    same_frame(fb, want["rgba"], f"shaded proj {proj} {variant} gw {gw} sampling {sampling} sun {sun} shadows {shadows}")


# ---- 2. ragged tiles ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_shaded_odd_frame(world, proj, variant):
    """101 x 67: no multiple of the 8 x 16 tile, more than one workgroup each way."""
    gw = 0.5
    sun = SUNS[proj - 1]
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            cam = sc.camera(world.gpu, gw, proj, False, sampling, width=101, height=67)
            for diffuse, shadows in MODES:
                want = world.shaded(gw, proj, sampling, sun, diffuse, shadows, width=101, height=67)
                assert lit_hits(want) >= 500 and want["capped"] == 0
                fb = world.scenes[gw].render_shaded(cam, sun_of(world.gpu, gw, sun), diffuse=diffuse, shadows=shadows)
                same_frame(fb, want["rgba"], f"101 x 67 proj {proj} {variant} sampling {sampling} shadows {shadows}")


# ---- 3. the three identities ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_identities(world, variant):
    """shade_flags 0 == render_lit; HMRM_SHADE_NO_SHADOWS alone == render (== render_interior with the flag and the inside
    camera); ambient = 255 == render under any flags."""
    gpu = world.gpu
    with kernel_variant(variant):
        for gw in GRID_WIDTHS:
            scene = world.scenes[gw]
            for proj in (1, 2, 3):
                for sampling in samplings_of(variant):
                    cam = sc.camera(gpu, gw, proj, False, sampling)
                    sun = sun_of(gpu, gw, SUNS[0])
                    plain = scene.render(cam).tobytes()
                    lit = scene.render_lit(cam, sun).tobytes()
                    assert lit != plain
                    assert scene.render_shaded(cam, sun, diffuse=False, shadows=True).tobytes() == lit, (gw, proj, sampling)
                    assert scene.render_shaded(cam, sun, diffuse=False, shadows=False).tobytes() == plain, (gw, proj, sampling)
                    full = sun_of(gpu, gw, SUNS[0], ambient=255)
                    for diffuse in (False, True):
                        for shadows in (False, True):
                            assert scene.render_shaded(cam, full, diffuse=diffuse, shadows=shadows).tobytes() == plain, (gw, proj, sampling, diffuse, shadows)
                    inside = sc.camera(gpu, gw, proj, True, sampling)
                    isun = sun_of(gpu, gw, SUNS[2], interior=True)
                    assert scene.render_shaded(inside, isun, diffuse=False, shadows=False).tobytes() == scene.render_interior(inside).tobytes()
                    assert scene.render_shaded(inside, isun, diffuse=False, shadows=True).tobytes() == scene.render_lit(inside, isun).tobytes()


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_ambient_0(world, variant):
    """ambient = 0: w = q, a level-0 pixel is black."""
    gpu, gw = world.gpu, 0.5
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            for sampling in samplings_of(variant):
                cam = sc.camera(gpu, gw, proj, False, sampling)
                for diffuse, shadows in MODES:
                    want = world.shaded(gw, proj, sampling, SUNS[1], diffuse, shadows, ambient=0)
                    hit = want["primary"]["status"] == lr.HIT
                    assert np.array_equal(want["w"][hit & ~want["shadowed"]], want["q"][hit & ~want["shadowed"]].astype(np.int64))
                    assert (want["rgba"][hit & (want["w"] == 0), 0:3] == 0).all() and (want["rgba"][:, 3] == 255).all()
                    fb = world.scenes[gw].render_shaded(cam, sun_of(gpu, gw, SUNS[1], ambient=0), diffuse=diffuse, shadows=shadows)
                    same_frame(fb, want["rgba"], f"ambient 0 proj {proj} sampling {sampling} {variant} shadows {shadows}")


# ---- 4. straight down over the whole map: every border cell, the one-sided differences ----
_down = {}


def down_replay(world, oracle, sampling, sun, shadows):
    gw = 0.5
    key = (sampling, sun, shadows)
    if key not in _down:
        cam = shc.down_camera(world.gpu, gw, sampling)
        rays = ray_replay.camera_rays(oracle, oracle.make_cfg(cam, world.params[gw], MAP_W, MAP_H))
        _down[key] = shr.replay(rays, world.heights[gw], world.cmap, world.params[gw], 0.2 * gw, sun, 0.3 * gw, bg=BG, sampling=sampling,
                                step_cap=shc.BASE_CAP, ambient=AMBIENT, shadows=shadows)
    return _down[key]


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_straight_down_over_the_whole_map(world, oracle, variant):
    gpu, gw = world.gpu, 0.5
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            cam = shc.down_camera(gpu, gw, sampling)
            for diffuse, shadows in MODES:
                want = down_replay(world, oracle, sampling, SUNS[0], shadows)
                hit = want["primary"]["status"] == lr.HIT
                assert hit.sum() == MAP_W * MAP_H and len(set(zip(want["primary"]["cell_x"][hit].tolist(), want["primary"]["cell_y"][hit].tolist()))) == MAP_W * MAP_H
                fb = world.scenes[gw].render_shaded(cam, sun_of(gpu, gw, SUNS[0]), diffuse=diffuse, shadows=shadows)
                same_frame(fb, want["rgba"], f"straight down sampling {sampling} {variant} shadows {shadows}")


# ---- 5. small maps: a component of the gradient is the constant 0 ----
SMALL = {"1x48": (slice(0, MAP_H), slice(7, 8)), "64x1": (slice(9, 10), slice(0, MAP_W)), "1x1": (slice(20, 21), slice(30, 31)),
         "2x2": (slice(20, 22), slice(30, 32))}


@pytest.mark.parametrize("shape", list(SMALL))
def test_small_maps(world, oracle, shape):
    gpu, gw = world.gpu, 0.5
    ys, xs = SMALL[shape]
    rgb, cmap = np.ascontiguousarray(world.rgb[ys, xs]), np.ascontiguousarray(world.cmap[ys, xs])
    mh, mw = rgb.shape[0:2]
    params = world.params[gw]
    heights = oracle.update_heightmap(rgb, params)
    scene = gpu.Scene(rgb, cmap, params)
    try:
        for sampling in SAMPLINGS:
            # (two pixels per cell, at least 8 each way; hang = 0: the frame's columns run along world y)
            down = shc.down_camera(gpu, gw, sampling, width=max(8, 2 * mh), height=max(8, 2 * mw), map_w=mw, map_h=mh)
            side = gpu.Camera.make(width=24, height=24, projection=1, hfov=gpu.degrees_to_rads(80), hang=gpu.degrees_to_rads(-50),
                                   vang=gpu.degrees_to_rads(112), pos=(-3.0 * gw, 4.0 * gw, 7.0 * gw), step_dist=0.2 * gw, bg=BG,
                                   sampling=sampling)
            for cam, least in ((down, 30), (side, 0)):
                rays = ray_replay.camera_rays(oracle, oracle.make_cfg(cam, params, mw, mh))
                for diffuse, shadows in MODES:
                    want = shr.replay(rays, heights, cmap, params, 0.2 * gw, SUNS[0], 0.3 * gw, bg=BG, sampling=sampling,
                                      step_cap=shc.BASE_CAP, ambient=AMBIENT, shadows=shadows)
                    hit = want["primary"]["status"] == lr.HIT
                    assert hit.sum() >= least and want["capped"] == 0
                    if least:  # (every cell of the map is some pixel's hit)
                        assert len(set(zip(want["primary"]["cell_x"][hit].tolist(), want["primary"]["cell_y"][hit].tolist()))) == mw * mh
                    for variant in KERNEL_VARIANTS:
                        if sampling in samplings_of(variant):
                            with kernel_variant(variant):
                                fb = scene.render_shaded(cam, sun_of(gpu, gw, SUNS[0]), diffuse=diffuse, shadows=shadows)
                            same_frame(fb, want["rgba"], f"{shape} sampling {sampling} {variant} shadows {shadows}")
    finally:
        scene.close()


# ---- 6. the plateau at luminance 255 under a vertical sun ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_plateau_under_a_vertical_sun(world, oracle, variant):
    """Flat ground under dir = (0, 0, 1): q = 255, and the shadow rays END after max_steps = 50 and leave the pixels lit -- the
    plateau's pixels are render's, the call returns HMRM_OK."""
    gpu, gw = world.gpu, 0.5
    rgb = world.rgb.copy()
    rgb[6:40, 2:40] = 255
    params = world.params[gw]
    heights = oracle.update_heightmap(rgb, params)
    scene = gpu.Scene(rgb, world.cmap, params)
    up = (0.0, 0.0, 1.0)
    try:
        with kernel_variant(variant):
            for proj in (1, 2, 3):
                for sampling in samplings_of(variant):
                    cam = sc.camera(gpu, gw, proj, False, sampling)
                    want = shr.replay(world.rays(gw, proj), heights, world.cmap, params, 0.2 * gw, up, 0.3 * gw, bg=BG, sampling=sampling,
                                      step_cap=shc.BASE_CAP, max_steps=50, ambient=AMBIENT)
                    hit = want["primary"]["status"] == lr.HIT
                    flat = hit & (want["q"] == 255)
                    assert flat.sum() >= 20 and (hit & (want["q"] < 255)).sum() >= 20 and want["capped"] == 0 and not want["shadowed"].any()
                    fb = scene.render_shaded(cam, sun_of(gpu, gw, up, max_steps=50))  # (raises unless HMRM_OK)
                    same_frame(fb, want["rgba"], f"plateau proj {proj} sampling {sampling} {variant}")
                    plain = scene.render(cam).reshape(-1, 4)
                    assert fb.reshape(-1, 4)[flat].tobytes() == plain[flat].tobytes()
    finally:
        scene.close()


# ---- 7. suns nothing special-cases ----
ODD_SUNS = [(0.5, 0.4, -0.3), (0.0, 0.0, 0.0), (np.nan, 0.5, 0.3), (0.5, np.nan, 0.3), (0.5, 0.4, np.nan), (np.inf, 0.5, 0.3),
            (0.5, -np.inf, 0.3), (0.5, 0.4, np.inf), (0.5, 0.4, -np.inf), (0.0, 0.7, 0.2), (-0.6, 0.0, 0.0)]
ODD_CAP = 300


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_odd_suns(world, variant):
    """A sun below the horizon, a zero direction, NaN and inf components, axis-parallel suns, at HMRM_STEP_CAP = 300: with
    shadows HMRM_E_NOTERM where render_lit gives it, and the replay's bytes; without shadows HMRM_OK."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    some_capped = some_level = False
    with kernel_variant(variant), env(HMRM_STEP_CAP=ODD_CAP):
        for k, sun in enumerate(ODD_SUNS):
            proj = 1 + k % 3
            sampling = samplings_of(variant)[k % len(samplings_of(variant))]
            cam = sc.camera(gpu, gw, proj, False, sampling)
            s = sun_of(gpu, gw, sun)
            want = world.shaded(gw, proj, sampling, sun, True, True, step_cap=ODD_CAP)
            if want["capped"]:
                some_capped = True
                with pytest.raises(gpu.HmrmError) as e:
                    scene.render_shaded(cam, s)
                assert e.value.code == gpu.HMRM_E_NOTERM and f"{want['capped']} ray(s)" in str(e.value), (sun, want["capped"], str(e.value))
                with pytest.raises(gpu.HmrmError) as e:
                    scene.render_lit(cam, s)
                assert e.value.code == gpu.HMRM_E_NOTERM and f"{want['capped']} ray(s)" in str(e.value)
            else:
                scene.render_lit(cam, s)
            same_frame(scene.render_shaded(cam, s, allow_capped=True), want["rgba"], f"sun {sun} proj {proj} sampling {sampling} {variant}")
            bare = world.shaded(gw, proj, sampling, sun, True, False, step_cap=ODD_CAP)
            assert bare["capped"] == 0
            same_frame(scene.render_shaded(cam, s, shadows=False), bare["rgba"], f"sun {sun}, no shadows, proj {proj} sampling {sampling} {variant}")
            hit = bare["primary"]["status"] == lr.HIT
            if not np.isfinite(sun).all() or not any(sun):
                assert (bare["q"][hit] == 0).all()
            else:
                some_level = some_level or bool((bare["q"][hit] > 0).any())
    assert some_capped and some_level


# ---- 8. HMRM_TRACE_INTERIOR: the primary rays under the interior rule ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_interior_flag(world, proj, variant):
    gpu = world.gpu
    with kernel_variant(variant):
        for gw in GRID_WIDTHS:
            for sampling in samplings_of(variant):
                cam = sc.camera(gpu, gw, proj, True, sampling)
                for diffuse, shadows in MODES:
                    want = world.shaded(gw, proj, sampling, SUNS[2], diffuse, shadows, inside=True)
                    assert lit_hits(want) >= 60 and want["capped"] == 0
                    fb = world.scenes[gw].render_shaded(cam, sun_of(gpu, gw, SUNS[2], interior=True), diffuse=diffuse, shadows=shadows)
                    same_frame(fb, want["rgba"], f"interior flag proj {proj} gw {gw} sampling {sampling} {variant} shadows {shadows}")


# ---- 9. a height update between two shaded frames: the neighbours come from the live table ----
def test_update_between_shaded_frames(world, oracle):
    gpu, gw = world.gpu, 0.5
    scene = gpu.Scene(world.rgb, world.cmap, world.params[gw])
    try:
        params2 = gpu.SceneParams.make(0.0, 11.0 * gw, grid_width=gw)
        heights2 = oracle.update_heightmap(world.rgb, params2)
        for sampling in SAMPLINGS:  # (first frames of every sampling mode before the update: the float table exists by then)
            cam = sc.camera(gpu, gw, 1, False, sampling)
            for diffuse, shadows in MODES:
                same_frame(scene.render_shaded(cam, sun_of(gpu, gw, SUNS[0]), diffuse=diffuse, shadows=shadows),
                           world.shaded(gw, 1, sampling, SUNS[0], diffuse, shadows)["rgba"], f"before the update, sampling {sampling}")
        scene.update(params2)
        for sampling in SAMPLINGS:
            cam = sc.camera(gpu, gw, 1, False, sampling)
            for diffuse, shadows in MODES:
                want2 = shr.replay(world.rays(gw, 1), heights2, world.cmap, params2, 0.2 * gw, SUNS[0], 0.3 * gw, bg=BG, sampling=sampling,
                                   step_cap=shc.BASE_CAP, ambient=AMBIENT, shadows=shadows)
                assert want2["rgba"].tobytes() != world.shaded(gw, 1, sampling, SUNS[0], diffuse, shadows)["rgba"].tobytes()
                for variant in KERNEL_VARIANTS:
                    if sampling in samplings_of(variant):
                        with kernel_variant(variant):
                            same_frame(scene.render_shaded(cam, sun_of(gpu, gw, SUNS[0]), diffuse=diffuse, shadows=shadows), want2["rgba"],
                                       f"after the update, sampling {sampling} {variant} shadows {shadows}")
    finally:
        scene.close()


# ---- 10. against the device's own records and table, without the replay's march ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_shaded_frame_is_trace_rays_plus_numpy_weights(world, proj, variant):
    """hmrm_trace_rays of the camera's rays (cell and point of every hit, from the GPU), the threshold table read back from the
    device, the weights in numpy: the HMRM_SHADE_NO_SHADOWS frame."""
    gpu = world.gpu
    gw = GRID_WIDTHS[proj - 1]
    scene, sun, params = world.scenes[gw], SUNS[proj - 1], world.params[gw]
    _recs, thr = scene.read_records()
    assert params.min_height == 0.0 and thr.shape == (MAP_H, MAP_W)  # (thr + 0.0 is thr: it stands in for heightmap_buf below)
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            cam = sc.camera(gpu, gw, proj, False, sampling)
            primary = scene.trace_rays(world.rays(gw, proj), 0.2 * gw, bg=BG, sampling=sampling)
            hit = primary["status"] == sr.HIT
            w = shr.weights(primary, thr, params, sampling, sun, AMBIENT, True, np.zeros(primary.shape[0], dtype=bool))
            assert hit.sum() >= 124 and len(np.unique(w[hit])) >= 30
            want = shr.apply(primary["rgba"], w)
            fb = scene.render_shaded(cam, sun_of(gpu, gw, sun), shadows=False)
            same_frame(fb, want, f"records + table proj {proj} {variant} sampling {sampling}")


# ---- 11. CLI ----
def test_cli_shading_key(world, tmp_path):
    gpu, gw = world.gpu, 0.5
    keys = f"sun_dir 0.6 0.5 0.35\nshadow_ambient {AMBIENT}\nshadow_step_dist {0.3 * gw:.17g}\nshading on\n"
    cfgp, text, outp = gs.cli_config(gpu, world, tmp_path, gw, extra=keys)
    cfg = gpu.Config().consume_file(str(cfgp))
    assert cfg.shading() is True and cfg.shadows() is False
    cfg.close()
    bare = world.shaded(gw, 1, 0, SUNS[0], True, False)["rgba"].reshape(30, 40, 4)
    full = world.shaded(gw, 1, 0, SUNS[0], True, True)["rgba"].reshape(30, 40, 4)
    r = gs.run_hmap(gpu, cfgp)
    assert "shading on\n" in r.stdout and "with sun shading in" in r.stdout
    assert open(outp, "rb").read() == gpu.png_encode(np.ascontiguousarray(bare))
    cfgp.write_text(text + keys + "shadows on\n")
    r = gs.run_hmap(gpu, cfgp)
    assert "with sun shading and sun shadows" in r.stdout
    assert open(outp, "rb").read() == gpu.png_encode(np.ascontiguousarray(full)) != gpu.png_encode(np.ascontiguousarray(bare))
    # ... ignored, with a warning, together with antialias > 1
    cfgp.write_text(text + keys + "antialias 2\n")
    r = gs.run_hmap(gpu, cfgp)
    assert "WARNING: shading is ignored with antialias > 1" in r.stderr and "shadows is ignored" not in r.stderr
