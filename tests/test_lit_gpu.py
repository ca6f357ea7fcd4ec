"""Sun shadows on the GPU (hmrm_render_lit; include/hmrm.h).  Every frame is compared BYTEWISE with tests/lit_replay.py, the
definition in numpy, which tests/test_lit_cpu.py pins to the C oracle and to a scalar loop; one test pins the lit kernels to
hmrm_trace_rays + hmrm_trace_segments without the replay.  Map, grid widths and cameras are those of tests/segment_cases.py
at 40 x 30 (the smallest at which every instantiation family runs), shadow step_dist 0.3 * grid width."""
import numpy as np
import pytest

import gpu_support as gs
import lit_cases as lc
import lit_replay as lr
import ray_replay
import segment_cases as sc
import segment_replay as sr
from gpu_support import KERNEL_VARIANTS, PROJ_IDS, env, gpu, kernel_variant, same_frame, samplings_of
from lit_cases import AMBIENT, SUNS
from segment_cases import BG, GRID_WIDTHS, GW_IDS, MAP_H, MAP_W

pytestmark = pytest.mark.gpu


class World(gs.Scenes, lc.Replays):
    pass


world = gs.world_fixture(World)


def sun_of(gpu, gw, direction, **kw):
    return gpu.Sun.make(direction, kw.pop("step_dist", 0.3 * gw), **kw)


# ---- 1. the base cases: 3 projections x 3 samplings x 3 grid widths x 4 variants x 3 suns ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_lit_frame_is_the_replay(world, proj, variant, gw):
    gpu, scene = world.gpu, world.scenes[gw]
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            cam = sc.camera(gpu, gw, proj, False, sampling)
            for sun in SUNS:
                want = world.lit(gw, proj, sampling, sun)
                shadowed, lit, capped = lc.counts(want)
                assert shadowed >= 20 and lit >= 100 and capped == 0, (shadowed, lit, capped)
                fb = scene.render_lit(cam, sun_of(gpu, gw, sun, ambient=AMBIENT))
                same_frame(fb, want["rgba"], f"lit proj {proj} {variant} gw {gw} sampling {sampling} sun {sun}")


# ---- 2. ragged tiles ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_lit_odd_frame(world, proj, variant):
    """101 x 67: no multiple of the 8 x 16 tile, more than one workgroup each way."""
    gw = 0.5
    cam = sc.camera(world.gpu, gw, proj, False, width=101, height=67)
    want = world.lit(gw, proj, 0, SUNS[proj - 1], width=101, height=67)
    shadowed, lit, capped = lc.counts(want)
    assert shadowed >= 100 and lit >= 500 and capped == 0
    with kernel_variant(variant):
        same_frame(world.scenes[gw].render_lit(cam, sun_of(world.gpu, gw, SUNS[proj - 1])), want["rgba"], f"101 x 67 proj {proj} {variant}")


# ---- 3. the lit kernels against the existing ones, without the replay ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_lit_frame_is_trace_rays_plus_trace_segments(world, proj, variant):
    """hmrm_trace_rays of the camera's rays, numpy glue for the origins and t, hmrm_trace_segments of the shadow rays: the same
    shadowed set and the same pixels as the one launch."""
    gpu = world.gpu
    gw = GRID_WIDTHS[proj - 1]
    scene, sun = world.scenes[gw], SUNS[proj - 1]
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            cam = sc.camera(gpu, gw, proj, False, sampling)
            primary = scene.trace_rays(world.rays(gw, proj), 0.2 * gw, bg=BG, sampling=sampling)
            t = lr.hit_thresholds(primary, world.heights[gw], world.params[gw], sampling)
            idx, srays = lr.shadow_rays(primary, t, sun)
            shadow = scene.trace_segments(srays, 0.3 * gw, bg=BG, sampling=sampling, interior=True)
            shadowed = np.zeros(primary.shape[0], dtype=bool)
            shadowed[idx] = shadow["status"] == sr.HIT
            assert shadowed.sum() >= 20 and (shadow["status"] != sr.HIT).sum() >= 100
            full = scene.render_lit(cam, sun_of(gpu, gw, sun, ambient=255))
            dark = scene.render_lit(cam, sun_of(gpu, gw, sun, ambient=0))
            assert full.tobytes() == primary["rgba"].tobytes()
            want = primary["rgba"].copy()
            want[shadowed, 0:3] = 0
            same_frame(dark, want, f"two passes proj {proj} {variant} sampling {sampling}")


# ---- 4. ambient ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_ambient_255_is_render(world, variant):
    gpu = world.gpu
    with kernel_variant(variant):
        for gw in GRID_WIDTHS:
            for proj in (1, 2, 3):
                for sampling in samplings_of(variant):
                    cam = sc.camera(gpu, gw, proj, False, sampling)
                    fb = world.scenes[gw].render_lit(cam, sun_of(gpu, gw, SUNS[0], ambient=255))
                    assert fb.tobytes() == world.scenes[gw].render(cam).tobytes(), (gw, proj, sampling)


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("ambient", [0, 1])
def test_ambient_0_and_1(world, ambient, variant):
    gpu, gw = world.gpu, 0.5
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            want = world.lit(gw, proj, 0, SUNS[1], ambient=ambient)
            sh = want["shadowed"]
            assert sh.sum() >= 20 and (want["rgba"][sh, 0:3] <= ambient).all() and (want["rgba"][:, 3] == 255).all()
            if ambient == 1:  # (c + 127) // 255: 1 from 128 on
                assert (want["rgba"][sh, 0:3] == 1).any() and (want["rgba"][sh, 0:3] == 0).any()
            fb = world.scenes[gw].render_lit(sc.camera(gpu, gw, proj, False), sun_of(gpu, gw, SUNS[1], ambient=ambient))
            same_frame(fb, want["rgba"], f"ambient {ambient} proj {proj} {variant}")


# ---- 5. the sun straight up: shadow rays that never leave the grid ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_vertical_sun(world, variant):
    """dir = (0, 0, 1): no shadow ray hits (the ray rises from the surface of its own cell -- z = t is not below t) and none
    leaves the grid.  With max_steps = 50 they END: render's frame whatever the ambient, HMRM_OK.  Without a limit they run
    to HMRM_STEP_CAP = 300: the same bytes and HMRM_E_NOTERM, one capped ray per hit pixel."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            for sampling in samplings_of(variant):
                cam = sc.camera(gpu, gw, proj, False, sampling)
                plain = scene.render(cam)
                want = world.lit(gw, proj, sampling, (0.0, 0.0, 1.0), max_steps=50, ambient=3)
                hits = int((want["primary"]["status"] == lr.HIT).sum())
                assert (want["shadow"]["status"] == sr.END).all() and hits >= 124 and want["capped"] == 0
                same_frame(plain, want["rgba"], "the replay's vertical sun is render")
                assert scene.render_lit(cam, sun_of(gpu, gw, (0.0, 0.0, 1.0), max_steps=50, ambient=3)).tobytes() == plain.tobytes()
                with env(HMRM_STEP_CAP=300):
                    capd = world.lit(gw, proj, sampling, (0.0, 0.0, 1.0), step_cap=300, ambient=3)
                    assert (capd["shadow"]["status"] == sr.CAPPED).all() and capd["capped"] == hits
                    with pytest.raises(gpu.HmrmError) as e:
                        scene.render_lit(cam, sun_of(gpu, gw, (0.0, 0.0, 1.0), ambient=3))
                    assert e.value.code == gpu.HMRM_E_NOTERM and f"{hits} ray(s)" in str(e.value)
                    assert scene.render_lit(cam, sun_of(gpu, gw, (0.0, 0.0, 1.0), ambient=3), allow_capped=True).tobytes() == plain.tobytes()
                    # a limit at the cap or above it is the cap's: CAPPED, counted; one below: END, not counted
                    with pytest.raises(gpu.HmrmError):
                        scene.render_lit(cam, sun_of(gpu, gw, (0.0, 0.0, 1.0), max_steps=300))
                    assert scene.render_lit(cam, sun_of(gpu, gw, (0.0, 0.0, 1.0), max_steps=299)).tobytes() == plain.tobytes()


# ---- 6. suns nothing special-cases ----
ODD_SUNS = [(0.5, 0.4, -0.3), (0.0, 0.0, 0.0), (np.nan, 0.5, 0.3), (0.5, np.nan, 0.3), (0.5, 0.4, np.nan), (np.inf, 0.5, 0.3),
            (0.5, -np.inf, 0.3), (0.5, 0.4, np.inf), (0.5, 0.4, -np.inf), (0.0, 0.7, 0.2), (-0.6, 0.0, 0.0)]
ODD_CAP = 300


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_odd_suns(world, variant):
    """A sun below the horizon, a zero direction (every shadow ray runs to the cap), NaN and inf components, axis-parallel
    suns, and step_dist = 0: the same arithmetic, at HMRM_STEP_CAP = 300."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    statuses = set()
    with kernel_variant(variant), env(HMRM_STEP_CAP=ODD_CAP):
        for k, sun in enumerate(ODD_SUNS + [SUNS[0]]):
            proj = 1 + k % 3
            sampling = samplings_of(variant)[k % len(samplings_of(variant))]
            step = 0.0 if k == len(ODD_SUNS) else None  # (the last one: an ordinary sun with a zero step)
            want = world.lit(gw, proj, sampling, sun, step_cap=ODD_CAP, sun_step=step)
            statuses |= set(want["shadow"]["status"].tolist())
            cam = sc.camera(gpu, gw, proj, False, sampling)
            s = sun_of(gpu, gw, sun) if step is None else sun_of(gpu, gw, sun, step_dist=0.0)
            if want["capped"]:
                with pytest.raises(gpu.HmrmError) as e:
                    scene.render_lit(cam, s)
                assert e.value.code == gpu.HMRM_E_NOTERM and f"{want['capped']} ray(s)" in str(e.value), (sun, want["capped"], str(e.value))
            same_frame(scene.render_lit(cam, s, allow_capped=True), want["rgba"], f"sun {sun} proj {proj} sampling {sampling} {variant}")
    assert statuses == {sr.MISS, sr.HIT, sr.CAPPED}


# ---- 7. origins that are not strictly inside: t == max_height; a box that does not start at 0 ----
def plateau_maps():
    rgb, cmap = sc.maps()
    rgb = rgb.copy()
    rgb[6:40, 2:40] = 255  # luminance 255: heightmap_buf == max_height there (at least 34 such hit pixels in every case below)
    return rgb, cmap


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_plateau_at_max_height(world, oracle, variant):
    gpu, gw = world.gpu, 0.5
    rgb, cmap = plateau_maps()
    params = world.params[gw]
    heights = oracle.update_heightmap(rgb, params)
    scene = gpu.Scene(rgb, cmap, params)
    try:
        with kernel_variant(variant):
            for proj in (1, 2, 3):
                for sampling in samplings_of(variant):
                    for sun in (SUNS[0], (0.3, -0.8, -0.05)):
                        want = lr.replay(world.rays(gw, proj), heights, cmap, params, 0.2 * gw, sun, 0.3 * gw, bg=BG, sampling=sampling,
                                         step_cap=lc.BASE_CAP, ambient=AMBIENT)
                        hit = want["primary"]["status"] == lr.HIT
                        on_top = hit & (want["t"] == params.max_height)
                        assert on_top.sum() >= 30 and want["capped"] == 0, (proj, sampling, int(on_top.sum()))
                        cam = sc.camera(gpu, gw, proj, False, sampling)
                        same_frame(scene.render_lit(cam, sun_of(gpu, gw, sun)), want["rgba"], f"plateau proj {proj} sampling {sampling} sun {sun} {variant}")
    finally:
        scene.close()


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_min_height_not_zero(world, oracle, variant):
    """min_height = 1.5 gw: t = heightmap_buf + min_height lies above max_height for the tall cells (distance() as written)."""
    gpu, gw = world.gpu, 0.5
    params = gpu.SceneParams.make(1.5 * gw, 8.0 * gw, grid_width=gw)
    heights = oracle.update_heightmap(world.rgb, params)
    scene = gpu.Scene(world.rgb, world.cmap, params)
    try:
        with kernel_variant(variant):
            for proj in (1, 2, 3):
                sampling = samplings_of(variant)[proj % len(samplings_of(variant))]
                cam = sc.camera(gpu, gw, proj, False, sampling)
                rays = ray_replay.camera_rays(oracle, oracle.make_cfg(cam, params, MAP_W, MAP_H))
                want = lr.replay(rays, heights, world.cmap, params, 0.2 * gw, SUNS[0], 0.3 * gw, bg=BG, sampling=sampling,
                                 step_cap=lc.BASE_CAP, ambient=AMBIENT)
                shadowed, lit, capped = lc.counts(want)
                hit = want["primary"]["status"] == lr.HIT
                assert shadowed >= 20 and lit >= 100 and capped == 0 and (hit & (want["t"] >= params.max_height)).sum() >= 10
                same_frame(scene.render_lit(cam, sun_of(gpu, gw, SUNS[0])), want["rgba"], f"min_height proj {proj} sampling {sampling} {variant}")
    finally:
        scene.close()


# ---- 8. HMRM_TRACE_INTERIOR: the primary rays under the interior rule too ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_interior_flag(world, proj, variant):
    gpu = world.gpu
    with kernel_variant(variant):
        for gw in GRID_WIDTHS:
            for sampling in samplings_of(variant):
                cam = sc.camera(gpu, gw, proj, True, sampling)
                want = world.lit(gw, proj, sampling, SUNS[2], inside=True)
                shadowed, lit, capped = lc.counts(want)
                assert shadowed >= 20 and lit >= 60 and capped == 0, (shadowed, lit)
                fb = world.scenes[gw].render_lit(cam, sun_of(gpu, gw, SUNS[2], interior=True))
                same_frame(fb, want["rgba"], f"interior flag proj {proj} gw {gw} sampling {sampling} {variant}")
        # without the flag the inside camera's frame is render's: all sky and background for perspective and spherical
        gw = 0.5
        cam = sc.camera(gpu, gw, proj, True)
        off = world.scenes[gw].render_lit(cam, sun_of(gpu, gw, SUNS[2], ambient=0))
        if proj != 3:
            assert off.tobytes() == world.scenes[gw].render(cam).tobytes()
        want_off = lr.replay(world.rays(gw, proj, True), world.heights[gw], world.cmap, world.params[gw], 0.2 * gw, SUNS[2], 0.3 * gw,
                             bg=BG, step_cap=lc.BASE_CAP, ambient=0)
        same_frame(off, want_off["rgba"], f"inside camera, flag off, proj {proj}")


# ---- 9. a height update between two lit frames ----
def test_update_between_lit_frames(world, oracle):
    gpu, gw = world.gpu, 0.5
    scene = gpu.Scene(world.rgb, world.cmap, world.params[gw])
    try:
        cam = sc.camera(gpu, gw, 1, False)
        same_frame(scene.render_lit(cam, sun_of(gpu, gw, SUNS[0])), world.lit(gw, 1, 0, SUNS[0])["rgba"], "before the update")
        params2 = gpu.SceneParams.make(0.0, 11.0 * gw, grid_width=gw)
        scene.update(params2)
        heights2 = oracle.update_heightmap(world.rgb, params2)
        want2 = lr.replay(world.rays(gw, 1), heights2, world.cmap, params2, 0.2 * gw, SUNS[0], 0.3 * gw, bg=BG, step_cap=lc.BASE_CAP,
                          ambient=AMBIENT)
        assert want2["rgba"].tobytes() != world.lit(gw, 1, 0, SUNS[0])["rgba"].tobytes() and lc.counts(want2)[0] >= 20
        for variant in KERNEL_VARIANTS:
            with kernel_variant(variant):
                same_frame(scene.render_lit(cam, sun_of(gpu, gw, SUNS[0])), want2["rgba"], f"after the update, {variant}")
    finally:
        scene.close()


# ---- 10. CLI ----
def test_cli_shadow_keys(world, tmp_path):
    gpu, gw = world.gpu, 0.5
    keys = f"shadows on\nsun_dir 0.6 0.5 0.35\nshadow_ambient {AMBIENT}\nshadow_step_dist {0.3 * gw:.17g}\n"
    cfgp, text, outp = gs.cli_config(gpu, world, tmp_path, gw, extra=keys)
    cfg = gpu.Config().consume_file(str(cfgp))
    assert cfg.shadows() is True and cfg.sun().step_dist == 0.3 * gw
    scene = cfg.create_scene()
    want = scene.render_lit(cfg.camera(), cfg.sun())
    plain = scene.render(cfg.camera())
    scene.close()
    cfg.close()
    same_frame(want, world.lit(gw, 1, 0, SUNS[0])["rgba"], "the config's camera and sun are the tests'")
    r = gs.run_hmap(gpu, cfgp)
    assert "shadows on\n" in r.stdout and "sun_dir 0.6 0.5 0.35\n" in r.stdout and "with sun shadows" in r.stdout
    assert open(outp, "rb").read() == gpu.png_encode(want) != gpu.png_encode(plain)
    # shadow_step_dist absent: the camera's step_dist
    cfgp.write_text(text + "shadows on\nsun_dir 0.6 0.5 0.35\n")
    r = gs.run_hmap(gpu, cfgp)
    want02 = world.lit(gw, 1, 0, SUNS[0], sun_step=0.2 * gw)
    assert open(outp, "rb").read() == gpu.png_encode(np.ascontiguousarray(want02["rgba"].reshape(30, 40, 4)))
    # ... ignored, with a warning, together with antialias > 1
    cfgp.write_text(text + keys + "antialias 2\n")
    r = gs.run_hmap(gpu, cfgp)
    assert "WARNING: shadows is ignored with antialias > 1" in r.stderr
