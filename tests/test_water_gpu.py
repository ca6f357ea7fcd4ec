"""Water frames on the GPU (hmrm_render_water, hmrm_render_water_device; include/hmrm.h).  Every frame is compared BYTEWISE with
tests/water_replay.py, the definition in numpy, which tests/test_water_cpu.py pins to the C oracle and to a scalar loop; one test
pins the water kernels to hmrm_trace_rays + hmrm_trace_segments without the replay.  The lake map, the level, grid widths and
cameras are those of tests/water_cases.py at 40 x 30 (the smallest at which every instantiation family runs), mirror step_dist
0.2 * grid width."""
import numpy as np
import pytest

import gpu_support as gs
import lit_replay as lr
import ray_replay
import segment_cases as sc
import segment_replay as sr
import water_cases as wc
import water_replay as wr
from gpu_support import KERNEL_VARIANTS, PROJ_IDS, env, gpu, kernel_variant, same_frame, samplings_of  # noqa: F401
from segment_cases import BG, GRID_WIDTHS, GW_IDS, MAP_H, MAP_W
from water_cases import REFLECTIVITY

pytestmark = pytest.mark.gpu


class World(gs.Scenes, wc.Replays):
    pass


world = gs.world_fixture(World)


def water_of(gpu, world, gw, **kw):
    return gpu.Water.make(kw.pop("level", world.level(gw)), kw.pop("step_dist", 0.2 * gw), **kw)


def replay_of(world, rays, heights, cmap, params, gw, sampling, level, **kw):
    """A replay outside the world's cache: maps, parameters or rays of a test's own."""
    return wr.replay(rays, heights, cmap, params, 0.2 * gw, level, kw.pop("mirror_step", 0.2 * gw), bg=BG, sampling=sampling,
                     step_cap=kw.pop("step_cap", wc.BASE_CAP), reflectivity=kw.pop("reflectivity", REFLECTIVITY), **kw)


# ---- 1. the base cases: 3 projections x 3 samplings x 3 grid widths x 4 variants ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_water_frame_is_the_replay(world, proj, variant, gw):
    gpu, scene = world.gpu, world.scenes[gw]
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            cam = sc.camera(gpu, gw, proj, False, sampling)
            want = world.water(gw, proj, sampling)
            water, hit, miss, capped = wc.counts(want)
            assert water >= 30 and hit >= 5 and miss >= 25 and capped == 0, (water, hit, miss, capped)
            fb = scene.render_water(cam, water_of(gpu, world, gw, reflectivity=REFLECTIVITY))
            same_frame(fb, want["rgba"], f"water proj {proj} {variant} gw {gw} sampling {sampling}")


# ---- 2. ragged tiles, waves that mix water lanes, dry hits and misses ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [2, 3], ids=["sph", "ortho"])
def test_water_odd_frame(world, proj, variant):
    """101 x 67: no multiple of the 8 x 16 tile, more than one workgroup each way; at least one 8 x 8 wave tile holds all three
    kinds of lane."""
    gw = 0.5
    sampling = samplings_of(variant)[(proj - 2) % len(samplings_of(variant))]
    cam = sc.camera(world.gpu, gw, proj, False, sampling, width=101, height=67)
    want = world.water(gw, proj, sampling, width=101, height=67)
    water, hit, miss, capped = wc.counts(want)
    assert water >= 100 and hit >= 25 and miss >= 50 and capped == 0, (water, hit, miss, capped)
    kind = np.where(want["water"], 2, np.where(want["primary"]["status"] == wr.HIT, 1, 0)).reshape(67, 101)
    mixed = sum(1 for y in range(0, 67, 8) for x in range(0, 101, 8) if np.unique(kind[y:y + 8, x:x + 8]).size == 3)
    assert mixed >= 1, mixed
    with kernel_variant(variant):
        fb = world.scenes[gw].render_water(cam, water_of(world.gpu, world, gw, reflectivity=REFLECTIVITY))
        same_frame(fb, want["rgba"], f"101 x 67 proj {proj} sampling {sampling} {variant}")


# ---- 3. the water kernels against the existing ones, without the replay ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_water_frame_is_trace_rays_plus_trace_segments(world, proj, variant):
    """hmrm_trace_rays of the camera's rays, numpy glue for the origins, t and the mirrored directions, hmrm_trace_segments of
    the mirror rays: the same water set and the same pixels as the one launch."""
    gpu = world.gpu
    gw = GRID_WIDTHS[proj - 1]
    scene, level = world.scenes[gw], world.level(gw)
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            cam = sc.camera(gpu, gw, proj, False, sampling)
            rays = world.rays(gw, proj)
            primary = scene.trace_rays(rays, 0.2 * gw, bg=BG, sampling=sampling)
            t = lr.hit_thresholds(primary, world.heights[gw], world.params[gw], sampling)
            idx, mrays = wr.mirror_rays(rays, primary, t, level)
            mirror = scene.trace_segments(mrays, 0.2 * gw, bg=BG, sampling=sampling, interior=True)
            assert idx.size >= 30 and (mirror["status"] == sr.HIT).sum() >= 5 and (mirror["status"] == sr.MISS).sum() >= 25
            assert np.array_equal(idx, world.water(gw, proj, sampling)["mirror_index"])
            for r, color in ((255, None), (REFLECTIVITY, None), (77, (200, 10, 90))):
                want = primary["rgba"].copy()
                base = want[idx] if color is None else np.tile(np.array(color + (255,), dtype=np.uint8), (idx.size, 1))
                want[idx] = wr.blend(base, mirror["rgba"], r)
                fb = scene.render_water(cam, water_of(gpu, world, gw, reflectivity=r, color=color))
                same_frame(fb, want, f"two passes proj {proj} {variant} sampling {sampling} r {r} colour {color}")


# ---- 4. the device form ----
def test_device_form_on_a_stream(world):
    """The frame in a torch tensor with padded rows, on a non-default torch stream: the host form's bytes, the padding untouched,
    take_capped for that stream; hmrm_debug_kernel_choice and a following plain frame are as they would have been."""
    import torch
    gpu, gw = world.gpu, 0.05
    scene = world.scenes[gw]
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    for proj, sampling, color in ((1, 0, None), (2, 1, (9, 99, 199)), (3, 2, None)):
        cam = sc.camera(gpu, gw, proj, False, sampling)
        w = water_of(gpu, world, gw, reflectivity=REFLECTIVITY, color=color)
        before, choice = scene.render(cam).tobytes(), scene.kernel_choice()
        host = scene.render_water(cam, w)
        same_frame(host, world.water(gw, proj, sampling, color=color)["rgba"], f"host form proj {proj}")
        t = torch.full((30, 48), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        scene.render_water_device(cam, w, t.data_ptr(), 48 * 4, stream=stream.cuda_stream)
        assert scene.take_capped(stream.cuda_stream) == 0  # (waits for the stream)
        got = t.cpu().numpy()
        assert (got[:, 40:] == 0x5A5A5A5A).all()
        assert np.ascontiguousarray(got[:, :40]).view(np.uint8).reshape(30, 40, 4).tobytes() == host.tobytes(), proj
        assert scene.kernel_choice() == choice and scene.render(cam).tobytes() == before
    # the device form's own refusals: the stride
    cam = sc.camera(gpu, gw, 1, False)
    t = torch.zeros((30, 48), dtype=torch.int32, device="cuda")
    for stride in (40 * 4 - 4, 40 * 4 + 2):
        with pytest.raises(gpu.HmrmError) as e:
            scene.render_water_device(cam, water_of(gpu, world, gw), t.data_ptr(), stride)
        assert e.value.code == gpu.HMRM_E_ARG and "stride" in str(e.value)


# ---- 5. reflectivity and the water's own colour ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_reflectivity_0_is_render(world, variant):
    gpu = world.gpu
    with kernel_variant(variant):
        for gw in GRID_WIDTHS:
            for proj in (1, 2, 3):
                for sampling in samplings_of(variant):
                    cam = sc.camera(gpu, gw, proj, False, sampling)
                    fb = world.scenes[gw].render_water(cam, water_of(gpu, world, gw, reflectivity=0))
                    assert fb.tobytes() == world.scenes[gw].render(cam).tobytes(), (gw, proj, sampling)


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("r,color", [(255, None), (1, None), (254, (3, 250, 128)), (0, (40, 80, 160))])
def test_reflectivity_and_own_colour(world, r, color, variant):
    gpu, gw = world.gpu, 0.5
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            sampling = samplings_of(variant)[proj % len(samplings_of(variant))]
            want = world.water(gw, proj, sampling, reflectivity=r, color=color)
            wet = want["water"]
            assert wet.sum() >= 30 and (want["rgba"][:, 3] == 255).all()
            if r == 255:
                assert want["rgba"][wet].tobytes() == want["mirror"]["rgba"].tobytes()
            if r == 0:
                assert (want["rgba"][wet, 0:3] == np.array(color, dtype=np.uint8)).all()
            fb = world.scenes[gw].render_water(sc.camera(gpu, gw, proj, False, sampling), water_of(gpu, world, gw, reflectivity=r, color=color))
            same_frame(fb, want["rgba"], f"r {r} colour {color} proj {proj} sampling {sampling} {variant}")


# ---- 6. levels ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_levels(world, variant):
    """A level below every threshold and a NaN level are render's frame; +inf makes every hit pixel mirror."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            for sampling in samplings_of(variant):
                cam = sc.camera(gpu, gw, proj, False, sampling)
                plain = scene.render(cam).tobytes()
                for level in (-1.0, float("nan"), -float("inf")):
                    assert scene.render_water(cam, water_of(gpu, world, gw, level=level, reflectivity=255)).tobytes() == plain, (proj, sampling, level)
                want = world.water(gw, proj, sampling, level=float("inf"), reflectivity=200)
                assert np.array_equal(want["water"], want["primary"]["status"] == wr.HIT) and want["water"].sum() >= 124 and want["capped"] == 0
                same_frame(scene.render_water(cam, water_of(gpu, world, gw, level=float("inf"), reflectivity=200)), want["rgba"],
                           f"level +inf proj {proj} sampling {sampling} {variant}")


# ---- 7. looking straight down: mirror rays that never leave the grid ----
def lake_spot(world, gw, half=3):
    """The centre (world x, y) of a flooded cell whose (2 half + 1)^2 neighbourhood is flooded too."""
    fl = world.flooded
    for y in range(half, MAP_H - half):
        for x in range(half, MAP_W - half):
            if fl[y - half:y + half + 1, x - half:x + half + 1].all():
                return (x + 0.5) * gw, -(y + 0.5) * gw
    raise AssertionError("the lake has no such spot")


def down_camera(gpu, world, gw, sampling):
    deg = gpu.degrees_to_rads
    x, y = lake_spot(world, gw)
    # (ortho_width is per pixel column: the plane is 2.4 x 1.8 cells, inside the 7 x 7 flooded cells whatever its rotation, with
    # more than the bilinear mode's half cell to spare)
    return gpu.Camera.make(width=12, height=9, projection=3, hfov=deg(80), hang=deg(sc.HANG_DEG), vang=deg(180), pos=(x, y, 14.0 * gw),
                           ortho_width=0.2 * gw, step_dist=0.2 * gw, bg=BG, sampling=sampling)


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_straight_down(world, oracle, variant):
    """An orthographic camera looking straight down on the lake: every pixel is water, the mirror rays go straight up, none hits
    and none leaves the grid.  With max_steps = 50 they END: HMRM_OK, every pixel the miss shade of dz = +1 blended in.
    Without a limit they run to HMRM_STEP_CAP = 300: the same bytes and HMRM_E_NOTERM, one capped ray per water pixel.
    A limit at the cap is the cap's, one below it an END; a mirror step of 0 stays on the spot and runs to the cap too."""
    gpu, gw = world.gpu, 0.5
    scene, params, heights, level = world.scenes[gw], world.params[gw], world.heights[gw], world.level(gw)
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            cam = down_camera(gpu, world, gw, sampling)
            rays = ray_replay.camera_rays(oracle, oracle.make_cfg(cam, params, MAP_W, MAP_H))
            assert (rays[:, 5] == -1.0).all()
            want = replay_of(world, rays, heights, world.cmap, params, gw, sampling, level, max_steps=50)
            n = int(want["water"].sum())
            assert n == 12 * 9 and (want["mirror"]["status"] == sr.END).all() and want["capped"] == 0
            sky = ray_replay.miss_shade(np.array([1.0]), BG)
            assert (want["mirror"]["rgba"] == sky[0]).all()
            assert want["rgba"].tobytes() == wr.blend(want["primary"]["rgba"], np.tile(sky, (n, 1)), REFLECTIVITY).tobytes()
            same_frame(scene.render_water(cam, water_of(gpu, world, gw, max_steps=50)), want["rgba"], f"straight down, limit 50, sampling {sampling} {variant}")
            with env(HMRM_STEP_CAP=300):
                capd = replay_of(world, rays, heights, world.cmap, params, gw, sampling, level, step_cap=300)
                assert (capd["mirror"]["status"] == sr.CAPPED).all() and capd["capped"] == n
                assert capd["rgba"].tobytes() == want["rgba"].tobytes()
                with pytest.raises(gpu.HmrmError) as e:
                    scene.render_water(cam, water_of(gpu, world, gw))
                assert e.value.code == gpu.HMRM_E_NOTERM and f"{n} ray(s)" in str(e.value)
                same_frame(scene.render_water(cam, water_of(gpu, world, gw), allow_capped=True), want["rgba"], f"straight down, capped, {variant}")
                # a limit at the cap or above it is the cap's: CAPPED, counted; one below: END, not counted
                with pytest.raises(gpu.HmrmError):
                    scene.render_water(cam, water_of(gpu, world, gw, max_steps=300))
                same_frame(scene.render_water(cam, water_of(gpu, world, gw, max_steps=299)), want["rgba"], f"straight down, limit 299, {variant}")
                still = replay_of(world, rays, heights, world.cmap, params, gw, sampling, level, step_cap=300, mirror_step=0.0)
                assert still["capped"] == n and still["rgba"].tobytes() == want["rgba"].tobytes()
                with pytest.raises(gpu.HmrmError) as e:
                    scene.render_water(cam, water_of(gpu, world, gw, step_dist=0.0))
                assert e.value.code == gpu.HMRM_E_NOTERM and f"{n} ray(s)" in str(e.value)
                same_frame(scene.render_water(cam, water_of(gpu, world, gw, step_dist=0.0), allow_capped=True), want["rgba"], f"step 0, {variant}")


# ---- 8. maps of a test's own: a lake at max_height, a lake under the alpha-0 block, an alpha-0 cell on the far shore ----
def own_scene_frames(world, oracle, variant, rgb, cmap, params, gw, level, what, check, cams=((1, False), (2, False), (3, False))):
    """The replayed and the rendered frames of a scene of the test's own under every camera and sampling mode of the variant;
    check(want) asserts that the case is there."""
    gpu = world.gpu
    heights = oracle.update_heightmap(rgb, params)
    scene = gpu.Scene(rgb, cmap, params)
    try:
        with kernel_variant(variant):
            for proj, inside in cams:
                for sampling in samplings_of(variant):
                    cam = sc.camera(gpu, gw, proj, inside, sampling)
                    rays = ray_replay.camera_rays(oracle, oracle.make_cfg(cam, params, MAP_W, MAP_H))
                    want = replay_of(world, rays, heights, cmap, params, gw, sampling, level)
                    check(want, proj, sampling)
                    fb = scene.render_water(cam, water_of(gpu, world, gw, level=level, reflectivity=REFLECTIVITY))
                    same_frame(fb, want["rgba"], f"{what} proj {proj} sampling {sampling} {variant}")
    finally:
        scene.close()


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_lake_at_max_height(world, oracle, variant):
    """Luminance 255: t == max_height, the mirror ray's origin is not strictly inside and goes through distance() as written."""
    gw = 0.5
    rgb, cmap = sc.maps()
    rgb = rgb.copy()
    rgb[6:40, 2:40] = 255
    params = world.params[gw]

    def check(want, proj, sampling):
        on_top = want["water"] & (want["t"] == params.max_height)
        assert on_top.sum() >= 30 and want["capped"] == 0, (proj, sampling, int(on_top.sum()))

    own_scene_frames(world, oracle, variant, rgb, cmap, params, gw, float(params.max_height), "plateau lake", check)


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_lake_under_alpha_0_and_alpha_0_shore(world, oracle, variant):
    """The lake extended under the colour map's alpha-0 texels: water cells whose primary pixel is the background.  And the
    cells the base cases' mirror rays hit made alpha-0: mirror pixels that are the background."""
    gw = 0.5
    params, level = world.params[gw], world.level(gw)
    clear = world.cmap[:, :, 3] == 0
    assert clear.sum() >= 8
    rgb = world.rgb.copy()
    rgb[clear] = wc.LAKE_LUM
    bg = np.array(BG + (255,), dtype=np.uint8)

    def check_under(want, proj, sampling):
        p = want["primary"]
        on_clear = want["water"] & clear[np.maximum(p["cell_y"], 0), np.maximum(p["cell_x"], 0)]
        assert want["capped"] == 0 and (on_clear.sum() >= 1 if proj == 3 else True), (proj, sampling)
        if sampling != 1:
            assert (p["rgba"][on_clear] == bg).all()

    own_scene_frames(world, oracle, variant, rgb, world.cmap, params, gw, level, "lake under alpha 0", check_under)

    cmap = world.cmap.copy()
    for proj in (1, 2, 3):
        m = world.water(gw, proj, 0)["mirror"]
        hit = m["status"] == sr.HIT
        cmap[m["cell_y"][hit], m["cell_x"][hit], 3] = 0

    def check_shore(want, proj, sampling):
        m = want["mirror"]
        hit = m["status"] == sr.HIT
        cleared = hit & (cmap[np.maximum(m["cell_y"], 0), np.maximum(m["cell_x"], 0), 3] == 0)
        # (the cells were picked from the nearest mode's hits: the bilinear mode's mirror rays find fewer of them)
        assert cleared.sum() >= (1 if sampling == 1 else 5) and (m["rgba"][cleared] == bg).all() and want["capped"] == 0, (proj, sampling, int(cleared.sum()))

    own_scene_frames(world, oracle, variant, world.rgb, cmap, params, gw, level, "alpha-0 shore", check_shore)


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_min_height_not_zero(world, oracle, variant):
    """min_height = 1.5 gw: a box that does not start at 0; the level is the lake's threshold there plus the margin."""
    gpu, gw = world.gpu, 0.5
    params = gpu.SceneParams.make(1.5 * gw, 8.0 * gw, grid_width=gw)
    heights = oracle.update_heightmap(world.rgb, params)
    y, x = np.argwhere(world.flooded)[0]
    level = float(heights[y, x]) + 1.5 * gw + 6.5 * gw / 255.0 / 4.0

    def check(want, proj, sampling):
        water, hit, miss, capped = wc.counts(want)
        assert water >= 30 and hit >= 1 and miss >= 20 and capped == 0, (proj, sampling, water, hit, miss)

    own_scene_frames(world, oracle, variant, world.rgb, world.cmap, params, gw, level, "min_height", check)


# ---- 9. HMRM_TRACE_INTERIOR: the primary rays under the interior rule ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_interior_flag(world, proj, variant):
    gpu = world.gpu
    with kernel_variant(variant):
        for gw in GRID_WIDTHS:
            for sampling in samplings_of(variant):
                cam = sc.camera(gpu, gw, proj, True, sampling)
                want = world.water(gw, proj, sampling, inside=True)
                water, hit, miss, capped = wc.counts(want)
                assert water >= 20 and hit >= 5 and miss >= 5 and capped == 0, (water, hit, miss)
                fb = world.scenes[gw].render_water(cam, water_of(gpu, world, gw, interior=True))
                same_frame(fb, want["rgba"], f"interior flag proj {proj} gw {gw} sampling {sampling} {variant}")
        # without the flag the inside camera's frame is render's with its own water: none for perspective and spherical
        gw = 0.5
        cam = sc.camera(gpu, gw, proj, True)
        off = world.scenes[gw].render_water(cam, water_of(gpu, world, gw, reflectivity=255))
        if proj != 3:
            assert off.tobytes() == world.scenes[gw].render(cam).tobytes()
        want_off = replay_of(world, world.rays(gw, proj, True), world.heights[gw], world.cmap, world.params[gw], gw, 0, world.level(gw),
                             reflectivity=255)
        same_frame(off, want_off["rgba"], f"inside camera, flag off, proj {proj}")


# ---- 10. a height update that drains the lake between two water frames ----
def test_update_drains_the_lake(world, oracle):
    gpu, gw = world.gpu, 0.5
    scene = gpu.Scene(world.rgb, world.cmap, world.params[gw])
    try:
        cam = sc.camera(gpu, gw, 1, False)
        w = water_of(gpu, world, gw, reflectivity=REFLECTIVITY)
        same_frame(scene.render_water(cam, w), world.water(gw, 1, 0)["rgba"], "before the update")
        params2 = gpu.SceneParams.make(1.5 * gw, 8.0 * gw, grid_width=gw)  # (every threshold rises above the level)
        scene.update(params2)
        heights2 = oracle.update_heightmap(world.rgb, params2)
        rays2 = ray_replay.camera_rays(oracle, oracle.make_cfg(cam, params2, MAP_W, MAP_H))
        want2 = replay_of(world, rays2, heights2, world.cmap, params2, gw, 0, world.level(gw))
        assert want2["water"].sum() == 0 and (want2["primary"]["status"] == wr.HIT).sum() >= 100
        for variant in KERNEL_VARIANTS:
            with kernel_variant(variant):
                fb = scene.render_water(cam, w)
                same_frame(fb, want2["rgba"], f"after the update, {variant}")
                assert fb.tobytes() == scene.render(cam).tobytes()
    finally:
        scene.close()


# ---- 11. CLI ----
def test_cli_water_keys(world, tmp_path):
    gpu, gw = world.gpu, 0.5
    keys = f"water on\nwater_level {world.level(gw):.17g}\nwater_reflectivity {REFLECTIVITY}\n"
    cfgp, text, outp = gs.cli_config(gpu, world, tmp_path, gw, extra=keys)
    cfg = gpu.Config().consume_file(str(cfgp))
    assert cfg.water_on() is True and cfg.water().step_dist == 0.2 * gw and cfg.water().level == world.level(gw)
    scene = cfg.create_scene()
    want = scene.render_water(cfg.camera(), cfg.water())
    plain = scene.render(cfg.camera())
    scene.close()
    cfg.close()
    same_frame(want, world.water(gw, 1, 0)["rgba"], "the config's camera and water are the tests'")
    r = gs.run_hmap(gpu, cfgp)
    assert "water on\n" in r.stdout and f"water_reflectivity {REFLECTIVITY}\n" in r.stdout and "with water at level" in r.stdout
    assert open(outp, "rb").read() == gpu.png_encode(want) != gpu.png_encode(plain)
    # the water's own colour, its own step and a limit
    cfgp.write_text(text + keys + f"water_color 20 60 120\nwater_step_dist {0.3 * gw:.17g}\nwater_max_steps 25\n")
    r = gs.run_hmap(gpu, cfgp)
    own = world.water(gw, 1, 0, color=(20, 60, 120), mirror_step=0.3 * gw, max_steps=25)
    assert "water_color 20 60 120\n" in r.stdout
    assert open(outp, "rb").read() == gpu.png_encode(np.ascontiguousarray(own["rgba"].reshape(30, 40, 4)))
    # ... ignored, with a warning, beside antialias > 1 and beside shadows
    cfgp.write_text(text + keys + "antialias 2\n")
    assert "WARNING: water is ignored with antialias > 1" in gs.run_hmap(gpu, cfgp).stderr
    cfgp.write_text(text + keys + "shadows on\n")
    r = gs.run_hmap(gpu, cfgp)
    assert "WARNING: water is ignored with shadows" in r.stderr and "with sun shadows" in r.stdout
