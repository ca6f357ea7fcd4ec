"""Sun-lit water frames on the GPU (hmrm_render_water_lit, hmrm_render_water_lit_device; include/hmrm.h).  Every frame is compared
BYTEWISE with tests/water_lit_replay.py, the definition in numpy composed of the replays that exist, which
tests/test_water_lit_cpu.py pins to those replays and to a scalar loop; one test pins the kernels to hmrm_trace_rays plus three
hmrm_trace_segments batches without the replay.  The lake map, level, grid widths and cameras are tests/water_cases.py's at
40 x 30, the suns tests/water_lit_cases.py's (a low sun per projection whose counts test_water_lit_cpu.py holds to its floors),
shadow step_dist 0.3 * grid width, mirror step_dist 0.2 * grid width."""
import numpy as np
import pytest

import gpu_support as gs
import lit_replay as lr
import ray_replay
import segment_cases as sc
import segment_replay as sr
import shade_replay as sh
import water_cases as wc
import water_lit_cases as wlc
import water_lit_replay as wl
import water_replay as wr
from gpu_support import KERNEL_VARIANTS, PROJ_IDS, env, gpu, kernel_variant, same_frame, samplings_of  # noqa: F401
from segment_cases import BG, GRID_WIDTHS, GW_IDS, MAP_H, MAP_W
from water_lit_cases import AMBIENT, REFLECTIVITY, sun_of

pytestmark = pytest.mark.gpu

NEAREST_ONLY = ("rec", "simple")  # (the literal loop of this family serves nearest sampling only)


class World(gs.Scenes, wlc.Replays):
    pass


world = gs.world_fixture(World)


def water_of(gpu, world, gw, **kw):
    return gpu.Water.make(kw.pop("level", world.level(gw)), kw.pop("step_dist", 0.2 * gw), **kw)


def sun_for(gpu, gw, proj=1, **kw):
    return gpu.Sun.make(kw.pop("dir", sun_of(proj)), kw.pop("step_dist", 0.3 * gw), ambient=kw.pop("ambient", AMBIENT), **kw)


def replay_of(rays, heights, cmap, params, gw, sampling, level, sun, **kw):
    """A replay outside the world's cache: maps, parameters or rays of a test's own."""
    return wl.replay(rays, heights, cmap, params, 0.2 * gw, level, kw.pop("mirror_step", 0.2 * gw), sun, kw.pop("sun_step", 0.3 * gw),
                     bg=BG, sampling=sampling, step_cap=kw.pop("step_cap", wc.BASE_CAP), reflectivity=kw.pop("reflectivity", REFLECTIVITY),
                     ambient=kw.pop("ambient", AMBIENT), **kw)


# ---- 1. the base cases: 3 projections x 3 samplings x 3 grid widths x 4 variants; shadows only and shading only once per projection ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_frame_is_the_replay(world, proj, variant, gw):
    gpu, scene = world.gpu, world.scenes[gw]
    with kernel_variant(variant):
        for sampling in samplings_of(variant, NEAREST_ONLY):
            cam = sc.camera(gpu, gw, proj, False, sampling)
            want = world.frame(gw, proj, sampling)
            assert all(c >= f for c, f in zip(wlc.counts(want), wlc.FLOORS)) and want["capped"] == 0, wlc.counts(want)
            fb = scene.render_water_lit(cam, water_of(gpu, world, gw), sun_for(gpu, gw, proj))
            same_frame(fb, want["rgba"], f"lit water proj {proj} {variant} gw {gw} sampling {sampling}")


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("diffuse,shadows", [(False, True), (True, False)], ids=["shadows_only", "shading_only"])
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_shadows_only_and_shading_only(world, proj, diffuse, shadows, variant):
    gpu = world.gpu
    gw = GRID_WIDTHS[proj - 1]
    with kernel_variant(variant):
        for sampling in samplings_of(variant, NEAREST_ONLY):
            cam = sc.camera(gpu, gw, proj, False, sampling)
            want = world.frame(gw, proj, sampling, diffuse=diffuse, shadows=shadows)
            fb = world.scenes[gw].render_water_lit(cam, water_of(gpu, world, gw), sun_for(gpu, gw, proj), diffuse=diffuse, shadows=shadows)
            same_frame(fb, want["rgba"], f"diffuse {diffuse} shadows {shadows} proj {proj} {variant} sampling {sampling}")


# ---- 2. ragged tiles, waves that mix wet lanes, dry hits and misses ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_odd_frame(world, proj, variant):
    """101 x 67: no multiple of the 8 x 16 tile, more than one workgroup each way."""
    gw = 0.5
    modes = samplings_of(variant, NEAREST_ONLY)
    sampling = modes[proj % len(modes)]
    cam = sc.camera(world.gpu, gw, proj, False, sampling, width=101, height=67)
    want = world.frame(gw, proj, sampling, width=101, height=67)
    assert all(c >= f for c, f in zip(wlc.counts(want, 101), wlc.FLOORS)) and want["capped"] == 0, wlc.counts(want, 101)
    with kernel_variant(variant):
        fb = world.scenes[gw].render_water_lit(cam, water_of(world.gpu, world, gw), sun_for(world.gpu, gw, proj))
        same_frame(fb, want["rgba"], f"101 x 67 proj {proj} sampling {sampling} {variant}")


# ---- 3. the kernels against the existing ones, without the replay ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_frame_is_trace_rays_plus_three_segment_batches(world, proj, variant):
    """hmrm_trace_rays of the camera's rays, then hmrm_trace_segments three times -- the primary hits' shadow rays, the mirror rays,
    the mirror hits' shadow rays -- with numpy glue for origins, thresholds, weights and the blend: the one launch's pixels."""
    gpu = world.gpu
    gw = GRID_WIDTHS[proj - 1]
    scene, level, sun = world.scenes[gw], world.level(gw), sun_of(proj)
    heights, params = world.heights[gw], world.params[gw]
    with kernel_variant(variant):
        for sampling in samplings_of(variant, NEAREST_ONLY):
            cam = sc.camera(gpu, gw, proj, False, sampling)
            rays = world.rays(gw, proj)
            primary = scene.trace_rays(rays, 0.2 * gw, bg=BG, sampling=sampling)
            t = lr.hit_thresholds(primary, heights, params, sampling)
            sidx, srays = lr.shadow_rays(primary, t, sun)
            shadow = scene.trace_segments(srays, 0.3 * gw, bg=BG, sampling=sampling, interior=True)
            idx, mrays = wr.mirror_rays(rays, primary, t, level)
            mirror = scene.trace_segments(mrays, 0.2 * gw, bg=BG, sampling=sampling, interior=True)
            midx, msrays = lr.shadow_rays(mirror, lr.hit_thresholds(mirror, heights, params, sampling), sun)
            mshadow = scene.trace_segments(msrays, 0.3 * gw, bg=BG, sampling=sampling, interior=True)
            shadowed = np.zeros(primary.shape[0], dtype=bool)
            shadowed[sidx] = shadow["status"] == sr.HIT
            mshadowed = np.zeros(mirror.shape[0], dtype=bool)
            mshadowed[midx] = mshadow["status"] == sr.HIT
            assert idx.size >= 34 and midx.size >= 5 and mshadowed.sum() >= 2 and shadowed.sum() >= 4
            for r, color in ((REFLECTIVITY, None), (77, (200, 10, 90))):
                base = primary["rgba"].copy()
                if color is not None:
                    base[idx] = np.array(color + (255,), dtype=np.uint8)
                want = sh.apply(base, sh.weights(primary, heights, params, sampling, sun, AMBIENT, True, shadowed))
                m = sh.apply(mirror["rgba"], sh.weights(mirror, heights, params, sampling, sun, AMBIENT, True, mshadowed))
                want[idx] = wr.blend(want[idx], m, r)
                fb = scene.render_water_lit(cam, water_of(gpu, world, gw, reflectivity=r, color=color), sun_for(gpu, gw, proj))
                same_frame(fb, want, f"four batches proj {proj} {variant} sampling {sampling} r {r} colour {color}")


# ---- 4. the device form ----
def test_device_form_on_a_stream(world):
    """The frame in a torch tensor with padded rows of an odd pixel stride, on a non-default torch stream: the host form's bytes, the
    padding untouched, take_capped for that stream."""
    import torch
    gpu, gw = world.gpu, 0.05
    scene = world.scenes[gw]
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    for proj, sampling, color in ((1, 0, None), (2, 1, (9, 99, 199)), (3, 2, None)):
        cam = sc.camera(gpu, gw, proj, False, sampling)
        w, s = water_of(gpu, world, gw, color=color), sun_for(gpu, gw, proj)
        host = scene.render_water_lit(cam, w, s)
        same_frame(host, world.frame(gw, proj, sampling, color=color)["rgba"], f"host form proj {proj}")
        t = torch.full((30, 47), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        scene.render_water_lit_device(cam, w, s, t.data_ptr(), 47 * 4, stream=stream.cuda_stream)
        assert scene.take_capped(stream.cuda_stream) == 0  # (waits for the stream)
        got = t.cpu().numpy()
        assert (got[:, 40:] == 0x5A5A5A5A).all()
        assert np.ascontiguousarray(got[:, :40]).view(np.uint8).reshape(30, 40, 4).tobytes() == host.tobytes(), proj
    cam = sc.camera(gpu, gw, 1, False)
    t = torch.zeros((30, 48), dtype=torch.int32, device="cuda")
    for stride in (40 * 4 - 4, 40 * 4 + 2):
        with pytest.raises(gpu.HmrmError) as e:
            scene.render_water_lit_device(cam, water_of(gpu, world, gw), sun_for(gpu, gw), t.data_ptr(), stride)
        assert e.value.code == gpu.HMRM_E_ARG and "stride" in str(e.value)


# ---- 5. the four identities against the existing entry points, and the edge values ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_identities(world, variant):
    """A level below every threshold or NaN, and r = 0 without own colour: hmrm_render_shaded (with both flags off:
    hmrm_render_lit).  HMRM_SHADE_NO_SHADOWS alone, and ambient = 255 under any flags: hmrm_render_water."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            sun = sun_for(gpu, gw, proj)
            for sampling in samplings_of(variant, NEAREST_ONLY):
                cam = sc.camera(gpu, gw, proj, False, sampling)
                for diffuse, shadows in ((True, True), (False, True), (True, False)):
                    shaded = scene.render_shaded(cam, sun, diffuse=diffuse, shadows=shadows).tobytes()
                    for level in (-1.0, float("nan")):
                        got = scene.render_water_lit(cam, water_of(gpu, world, gw, level=level, reflectivity=255), sun, diffuse=diffuse, shadows=shadows)
                        assert got.tobytes() == shaded, (proj, sampling, diffuse, shadows, level)
                    got = scene.render_water_lit(cam, water_of(gpu, world, gw, reflectivity=0), sun, diffuse=diffuse, shadows=shadows)
                    assert got.tobytes() == shaded, (proj, sampling, diffuse, shadows, "r = 0")
                assert scene.render_water_lit(cam, water_of(gpu, world, gw, level=-1.0), sun, diffuse=False).tobytes() == scene.render_lit(cam, sun).tobytes()
                wet = scene.render_water(cam, water_of(gpu, world, gw)).tobytes()
                assert scene.render_water_lit(cam, water_of(gpu, world, gw), sun, diffuse=False, shadows=False).tobytes() == wet, (proj, sampling)
                bright = sun_for(gpu, gw, proj, ambient=255)
                for diffuse, shadows in ((True, True), (False, True), (True, False)):
                    got = scene.render_water_lit(cam, water_of(gpu, world, gw), bright, diffuse=diffuse, shadows=shadows)
                    assert got.tobytes() == wet, (proj, sampling, diffuse, shadows, "ambient 255")


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("r,color,ambient", [(0, (40, 80, 160), AMBIENT), (1, None, 0), (254, (3, 250, 128), AMBIENT), (255, None, AMBIENT)])
def test_reflectivity_own_colour_and_ambient_0(world, r, color, ambient, variant):
    gpu, gw = world.gpu, 0.5
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            modes = samplings_of(variant, NEAREST_ONLY)
            sampling = modes[proj % len(modes)]
            want = world.frame(gw, proj, sampling, reflectivity=r, color=color, ambient=ambient)
            assert want["water"].sum() >= 34 and (want["rgba"][:, 3] == 255).all()
            fb = world.scenes[gw].render_water_lit(sc.camera(gpu, gw, proj, False, sampling), water_of(gpu, world, gw, reflectivity=r, color=color),
                                                   sun_for(gpu, gw, proj, ambient=ambient))
            same_frame(fb, want["rgba"], f"r {r} colour {color} ambient {ambient} proj {proj} sampling {sampling} {variant}")


# ---- 6. the pass structure ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_passes(world, variant):
    """+inf: every hit is wet, every pass runs.  -1: no pass 2 or 3 (the identities above compare it with hmrm_render_shaded; here
    with the replay).  A sun straight up shadows nothing and needs max_steps to end; a sun below the horizon, a zero and a NaN
    direction go through the same arithmetic."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            for sampling in samplings_of(variant, NEAREST_ONLY):
                cam = sc.camera(gpu, gw, proj, False, sampling)
                want = world.frame(gw, proj, sampling, level=float("inf"), reflectivity=200)
                assert np.array_equal(want["water"], want["primary"]["status"] == wl.HIT) and want["water"].sum() >= 124 and want["capped"] == 0
                same_frame(scene.render_water_lit(cam, water_of(gpu, world, gw, level=float("inf"), reflectivity=200), sun_for(gpu, gw, proj)),
                           want["rgba"], f"level +inf proj {proj} sampling {sampling} {variant}")
                dry = world.frame(gw, proj, sampling, level=-1.0)
                assert dry["water"].sum() == 0 and dry["shadowed"].sum() >= 2
                same_frame(scene.render_water_lit(cam, water_of(gpu, world, gw, level=-1.0), sun_for(gpu, gw, proj)), dry["rgba"],
                           f"level -1 proj {proj} sampling {sampling} {variant}")
            sampling = samplings_of(variant, NEAREST_ONLY)[-1]
            cam = sc.camera(gpu, gw, proj, False, sampling)
            for what, direction, limit in (("up", (0.0, 0.0, 1.0), 40), ("below the horizon", (0.5, 0.5, -0.4), 0), ("zero", (0.0, 0.0, 0.0), 60),
                                           ("nan", (float("nan"), 0.3, 0.5), 0)):
                want = world.frame(gw, proj, sampling, sun=direction, sun_max_steps=limit)
                assert want["capped"] == 0
                if what == "up":
                    assert want["shadowed"].sum() == 0 and want["mirror_shadowed"].sum() == 0 and (want["shadow"]["status"] == wl.END).sum() >= 1
                if what in ("zero", "nan"):
                    hit = want["primary"]["status"] == wl.HIT
                    assert (want["w"][hit & ~want["shadowed"]] == AMBIENT).all()  # (q = 0)
                fb = scene.render_water_lit(cam, water_of(gpu, world, gw), sun_for(gpu, gw, proj, dir=direction, max_steps=limit))
                same_frame(fb, want["rgba"], f"sun {what} proj {proj} sampling {sampling} {variant}")


def test_sky_only(world):
    """A camera that sees no terrain: one pass, the plain frame."""
    gpu, gw = world.gpu, 0.5
    deg = gpu.degrees_to_rads
    for proj in (1, 2, 3):
        pos = sc.camera_pos(gw, False)
        cam = gpu.Camera.make(width=40, height=30, projection=proj, hfov=deg(sc.hfov_deg(proj)), hang=deg(sc.HANG_DEG), vang=deg(10.0),
                              pos=(pos[0], pos[1], 40.0 * gw), ortho_width=0.2 * gw, step_dist=0.2 * gw, bg=BG, sampling=0)
        plain = world.scenes[gw].render(cam)
        fb = world.scenes[gw].render_water_lit(cam, water_of(gpu, world, gw), sun_for(gpu, gw, proj))
        assert fb.tobytes() == plain.tobytes(), proj


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_step_limits(world, variant):
    """sun.max_steps and water.max_steps at and below the cap: END rays are never counted, a limit at the cap is the cap's."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    with kernel_variant(variant), env(HMRM_STEP_CAP=wc.BASE_CAP):
        for proj, sun_limit, water_limit in ((1, 7, 0), (2, 0, 9), (3, 5, 11)):
            sampling = samplings_of(variant, NEAREST_ONLY)[-1]
            cam = sc.camera(gpu, gw, proj, False, sampling)
            want = world.frame(gw, proj, sampling, sun_max_steps=sun_limit, max_steps=water_limit)
            ended = (want["shadow"]["status"] == wl.END).sum() + (want["mirror"]["status"] == wl.END).sum() + (want["mirror_shadow"]["status"] == wl.END).sum()
            assert ended >= 5 and want["capped"] == 0
            fb = scene.render_water_lit(cam, water_of(gpu, world, gw, max_steps=water_limit), sun_for(gpu, gw, proj, max_steps=sun_limit))
            same_frame(fb, want["rgba"], f"limits {sun_limit} {water_limit} proj {proj} {variant}")


# ---- 7. capped rays: a camera straight down on the lake ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_straight_down(world, oracle, variant):
    """An orthographic camera looking straight down on the lake without water.max_steps: every pixel is water, the mirror rays go
    straight up and run to HMRM_STEP_CAP = 300; the frame is valid, the call returns HMRM_E_NOTERM and the count is the replay's sum
    over all four kinds of ray.  A sun straight up without a limit caps the primary hits' shadow rays too; sun.max_steps and
    water.max_steps at the cap are the cap's, one below it they make END rays, which are never counted."""
    from test_water_gpu import down_camera
    gpu, gw = world.gpu, 0.5
    scene, params, heights, level = world.scenes[gw], world.params[gw], world.heights[gw], world.level(gw)
    n = 12 * 9
    with kernel_variant(variant), env(HMRM_STEP_CAP=300):
        for sampling in samplings_of(variant, NEAREST_ONLY):
            cam = down_camera(gpu, world, gw, sampling)
            rays = ray_replay.camera_rays(oracle, oracle.make_cfg(cam, params, MAP_W, MAP_H))
            for direction, sun_limit, water_limit, capped in ((sun_of(3), 0, 0, None), ((0.0, 0.0, 1.0), 0, 0, 2 * n), ((0.0, 0.0, 1.0), 300, 300, 2 * n),
                                                              ((0.0, 0.0, 1.0), 299, 0, n), ((0.0, 0.0, 1.0), 0, 299, n), ((0.0, 0.0, 1.0), 299, 299, 0)):
                want = replay_of(rays, heights, world.cmap, params, gw, sampling, level, direction, step_cap=300, sun_max_steps=sun_limit,
                                 max_steps=water_limit)
                ends = sr.END if water_limit == 299 else sr.CAPPED
                assert want["water"].sum() == n and (want["mirror"]["status"] == ends).all()
                if capped is not None:
                    assert want["capped"] == capped
                w, s = water_of(gpu, world, gw, max_steps=water_limit), sun_for(gpu, gw, 3, dir=direction, max_steps=sun_limit)
                if want["capped"]:
                    with pytest.raises(gpu.HmrmError) as e:
                        scene.render_water_lit(cam, w, s)
                    assert e.value.code == gpu.HMRM_E_NOTERM and f"{want['capped']} ray(s)" in str(e.value), (str(e.value), want["capped"])
                same_frame(scene.render_water_lit(cam, w, s, allow_capped=True), want["rgba"],
                           f"straight down sampling {sampling} limits {sun_limit} {water_limit} {variant}")


# ---- 8. HMRM_TRACE_INTERIOR through the water, through the sun, through both ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_interior_flag(world, proj, variant):
    gpu = world.gpu
    gw = GRID_WIDTHS[proj - 1]
    with kernel_variant(variant):
        for sampling in samplings_of(variant, NEAREST_ONLY):
            cam = wlc.inside_camera(gpu, gw, proj, sampling)
            want = world.inside_frame(gw, proj, sampling)
            assert all(c >= f for c, f in zip(wlc.counts(want), wlc.FLOORS)) and want["capped"] == 0, wlc.counts(want)
            for by_water, by_sun in ((True, False), (False, True), (True, True)):
                fb = world.scenes[gw].render_water_lit(cam, water_of(gpu, world, gw, interior=by_water), sun_for(gpu, gw, proj, interior=by_sun))
                same_frame(fb, want["rgba"], f"interior flag water {by_water} sun {by_sun} proj {proj} sampling {sampling} {variant}")


# ---- 9. a height update that drains the lake; the scene's kernel choice ----
def test_update_drains_the_lake(world, oracle):
    gpu, gw = world.gpu, 0.5
    scene = gpu.Scene(world.rgb, world.cmap, world.params[gw])
    try:
        cam = sc.camera(gpu, gw, 1, False)
        w, s = water_of(gpu, world, gw), sun_for(gpu, gw, 1)
        same_frame(scene.render_water_lit(cam, w, s), world.frame(gw, 1, 0)["rgba"], "before the update")
        params2 = gpu.SceneParams.make(1.5 * gw, 8.0 * gw, grid_width=gw)  # (every threshold rises above the level)
        scene.update(params2)
        heights2 = oracle.update_heightmap(world.rgb, params2)
        rays2 = ray_replay.camera_rays(oracle, oracle.make_cfg(cam, params2, MAP_W, MAP_H))
        want2 = replay_of(rays2, heights2, world.cmap, params2, gw, 0, world.level(gw), sun_of(1))
        assert want2["water"].sum() == 0 and (want2["primary"]["status"] == wl.HIT).sum() >= 100
        for variant in KERNEL_VARIANTS:
            with kernel_variant(variant):
                fb = scene.render_water_lit(cam, w, s)
                same_frame(fb, want2["rgba"], f"after the update, {variant}")
                assert fb.tobytes() == scene.render_shaded(cam, s).tobytes()
    finally:
        scene.close()


def test_kernel_choice_is_left_alone(world):
    """Eight sun-lit water frames are never the probe and not counted towards it; a plain frame afterwards is the replay's."""
    gpu, gw = world.gpu, 0.5
    scene = gpu.Scene(world.rgb, world.cmap, world.params[gw])
    try:
        cam = sc.camera(gpu, gw, 1, False)
        choice = scene.kernel_choice()
        for _ in range(8):
            scene.render_water_lit(cam, water_of(gpu, world, gw), sun_for(gpu, gw, 1))
        assert scene.kernel_choice() == choice
        same_frame(scene.render(cam), world.primary(gw, 1, 0)["rgba"], "a plain frame afterwards")
    finally:
        scene.close()


# ---- 10. CLI ----
def test_cli_water_light(world, tmp_path):
    gpu, gw = world.gpu, 0.5
    sun = sun_of(1)
    keys = (f"water on\nwater_level {world.level(gw):.17g}\nwater_reflectivity {REFLECTIVITY}\n"
            f"sun_dir {sun[0]:.17g} {sun[1]:.17g} {sun[2]:.17g}\nshadow_ambient {AMBIENT}\nshadow_step_dist {0.3 * gw:.17g}\n")
    cfgp, text, outp = gs.cli_config(gpu, world, tmp_path, gw, extra=keys)
    png = lambda want: gpu.png_encode(np.ascontiguousarray(want["rgba"].reshape(30, 40, 4)))
    for extra, diffuse, shadows, said in (("shadows on\n", False, True, "with sun shadows"), ("shading on\n", True, False, "with sun shading"),
                                          ("shadows on\nshading on\n", True, True, "with sun shading and sun shadows")):
        cfgp.write_text(text + keys + "water_light sun\n" + extra)
        cfg = gpu.Config().consume_file(str(cfgp))
        assert cfg.water_light() == 1
        cfg.close()
        r = gs.run_hmap(gpu, cfgp)
        assert "ignored" not in r.stderr and "water_light sun\n" in r.stdout and f"with water at level" in r.stdout and said in r.stdout
        assert open(outp, "rb").read() == png(world.frame(gw, 1, 0, diffuse=diffuse, shadows=shadows)), extra
        # under `water_scope all` too
        cfgp.write_text(text + keys + "water_light sun\nwater_scope all\n" + extra)
        r = gs.run_hmap(gpu, cfgp)
        assert "ignored" not in r.stderr
        assert open(outp, "rb").read() == png(world.frame(gw, 1, 0, diffuse=diffuse, shadows=shadows)), extra
    # beside antialias 2 the existing warning stands; without the key the old warning text is unchanged
    cfgp.write_text(text + keys + "water_light sun\nshadows on\nantialias 2\n")
    assert "WARNING: water is ignored with antialias > 1" in gs.run_hmap(gpu, cfgp).stderr
    cfgp.write_text(text + keys + "shadows on\n")
    r = gs.run_hmap(gpu, cfgp)
    assert "WARNING: water is ignored with shadows" in r.stderr and "with sun shadows" in r.stdout
    cfgp.write_text(text + keys + "water_light off\nshading on\n")
    assert "WARNING: water is ignored with shading" in gs.run_hmap(gpu, cfgp).stderr
