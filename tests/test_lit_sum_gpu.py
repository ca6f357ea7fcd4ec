"""Accumulated lit frames on the GPU (hmrm_render_lit_sum; include/hmrm.h).  Every plane is compared BYTEWISE with
tests/lit_sum_cases.py's replay -- a composition of tests/shade_replay.py's weights, which tests/test_lit_sum_cpu.py pins -- or,
without the replay, with frames of hmrm_render_shaded and hmrm_render_geometry from the same GPU.  Map, grid widths and cameras
are those of tests/segment_cases.py at 40 x 30 unless said otherwise (a partial tile row and sky-only waves in every frame),
shadow step_dist 0.3 * grid width, ambient 96."""
import functools

import numpy as np
import pytest

import gpu_support as gs
import lit_sum_cases as lsc
import segment_cases as sc
from gpu_support import KERNEL_VARIANTS, PROJ_IDS, env, gpu, kernel_variant, same_frame
from lit_sum_cases import AMBIENT, NO_HIT, SUNS
from segment_cases import GRID_WIDTHS, GW_IDS

pytestmark = pytest.mark.gpu

MODES = ((False, True), (True, True), (True, False))  # (diffuse, shadows): shade_flags 0, DIFFUSE, DIFFUSE | NO_SHADOWS
ALL_MODES = MODES + ((False, False),)
UP = (0.0, 0.0, 1.0)
samplings_of = functools.partial(gs.samplings_of, nearest_only=("rec", "simple"))  # (the literal loop too: nearest sampling only)


class World(gs.Scenes, lsc.Replays):
    pass


world = gs.world_fixture(World)


def same_light(got, want_light, what):
    want = want_light.reshape(got.shape)
    assert got.dtype == np.uint16
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        y, x = bad[0]
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.size} sums differ; first ({x}, {y}): got {got[y, x]}, want {want[y, x]}")


def same_planes(got, want, what):
    fb, light = got
    same_frame(fb, want["rgba"], what + ", rgba")
    same_light(light, want["light"], what + ", light")


def sun_of(gpu, gw, direction=(9.0, 9.0, -9.0), **kw):
    """(the direction is not looked at: a sun below the horizon would darken every frame that did look)"""
    kw.setdefault("ambient", AMBIENT)
    return gpu.Sun.make(direction, kw.pop("step_dist", 0.3 * gw), **kw)


# ---- 1. the replay sweep, K = 3 ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_lit_sum_is_the_replay(world, proj, variant, gw):
    gpu, scene = world.gpu, world.scenes[gw]
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            cam = sc.camera(gpu, gw, proj, False, sampling)
            for diffuse, shadows in MODES:
                want = world.lit_sum(gw, proj, sampling, SUNS, diffuse, shadows)
                assert want["hit"].sum() >= 100 and want["capped"] == 0
                what = f"proj {proj} {variant} gw {gw} sampling {sampling} diffuse {diffuse} shadows {shadows}"
                same_planes(scene.render_lit_sum(cam, sun_of(gpu, gw), SUNS, diffuse=diffuse, shadows=shadows, light=True), want, what)
                same_frame(scene.render_lit_sum(cam, sun_of(gpu, gw), SUNS, diffuse=diffuse, shadows=shadows), want["rgba"], what + ", rgba alone")
                same_light(scene.render_lit_sum(cam, sun_of(gpu, gw), SUNS, diffuse=diffuse, shadows=shadows, light=True, rgba=False),
                           want["light"], what + ", light alone")


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_lit_sum_odd_frame(world, variant):
    """101 x 67: no multiple of the 8 x 16 tile, more than one workgroup each way."""
    gpu, gw, proj = world.gpu, 0.5, 1
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            cam = sc.camera(gpu, gw, proj, False, sampling, width=101, height=67)
            want = world.lit_sum(gw, proj, sampling, SUNS, True, True, width=101, height=67)
            assert want["hit"].sum() >= 500 and want["capped"] == 0
            same_planes(world.scenes[gw].render_lit_sum(cam, sun_of(gpu, gw), SUNS, diffuse=True, light=True), want,
                        f"101 x 67 {variant} sampling {sampling}")


# ---- 2. K = 1 is hmrm_render_shaded; copies of one direction ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_one_direction_is_render_shaded(world, variant):
    """K = 1 against Scene.render_shaded on the same GPU with sun.dir = dirs[0], under all four shade_flags; K = 2 and K = 7
    copies of that direction give the same frame, with light = K * w."""
    gpu = world.gpu
    with kernel_variant(variant):
        for gw in GRID_WIDTHS:
            scene = world.scenes[gw]
            for proj in (1, 2, 3):
                for sampling in samplings_of(variant):
                    cam = sc.camera(gpu, gw, proj, False, sampling)
                    d = SUNS[(proj + sampling) % 3]
                    for diffuse, shadows in ALL_MODES:
                        what = (variant, gw, proj, sampling, diffuse, shadows)
                        one = scene.render_shaded(cam, sun_of(gpu, gw, d), diffuse=diffuse, shadows=shadows)
                        fb, light = scene.render_lit_sum(cam, sun_of(gpu, gw), [d], diffuse=diffuse, shadows=shadows, light=True)
                        assert fb.tobytes() == one.tobytes(), what
                        hit = light != NO_HIT
                        assert hit.sum() >= 100 and light[hit].max() <= 255
                        if not diffuse and not shadows:
                            assert fb.tobytes() == scene.render(cam).tobytes() and (light[hit] == 255).all(), what
                        for k in (2, 7):
                            fbk, lightk = scene.render_lit_sum(cam, sun_of(gpu, gw), [d] * k, diffuse=diffuse, shadows=shadows, light=True)
                            assert fbk.tobytes() == one.tobytes(), (what, k)
                            assert np.array_equal(lightk[hit], k * light[hit]) and (lightk[~hit] == NO_HIT).all(), (what, k)


# ---- 3. K = 256 ----
SKY_CASES = ((1, 0), (2, 1), (3, 2))


@pytest.mark.parametrize("variant", ("leap", "group"))
def test_sky_of_256_directions_is_the_replay(world, variant):
    gpu, gw = world.gpu, 0.5
    dirs = gpu.sky_directions(16, 16)
    with kernel_variant(variant):
        for proj, sampling in SKY_CASES:
            cam = sc.camera(gpu, gw, proj, False, sampling)
            for diffuse in (False, True):
                want = world.lit_sum(gw, proj, sampling, dirs, diffuse, True, max_steps=40)
                assert want["capped"] == 0 and np.unique(want["S"][want["hit"]]).size >= 59
                got = world.scenes[gw].render_lit_sum(cam, sun_of(gpu, gw, max_steps=40), dirs, diffuse=diffuse, light=True)
                same_planes(got, want, f"sky 256 {variant} proj {proj} sampling {sampling} diffuse {diffuse}")
                back = world.scenes[gw].render_lit_sum(cam, sun_of(gpu, gw, max_steps=40), dirs[::-1], diffuse=diffuse, light=True)
                assert back[0].tobytes() == got[0].tobytes() and back[1].tobytes() == got[1].tobytes()


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_sky_of_256_directions_is_the_sum_of_256_shaded_frames(world, variant):
    """Without the replay: over an all-white opaque colour map the R channel of render_shaded is the weight w, so the light
    plane must be the numpy sum of 256 such frames on hit pixels -- taken from a render_geometry cell plane -- and 0xFFFF
    elsewhere; the directions reversed give the same planes."""
    gpu, gw = world.gpu, 0.5
    dirs = gpu.sky_directions(16, 16)
    white = np.full_like(world.cmap, 255)
    scene = gpu.Scene(world.rgb, white, world.params[gw])
    try:
        with kernel_variant(variant):
            proj, sampling = SKY_CASES[KERNEL_VARIANTS.index(variant) % 3]
            sampling = sampling if sampling in samplings_of(variant) else 0
            cam = sc.camera(gpu, gw, proj, False, sampling)
            hit = scene.render_geometry(cam, rgba=False, range=False, slope=False)["cell"] >= 0
            assert hit.sum() >= 100
            total = np.zeros(hit.shape, dtype=np.int64)
            for d in dirs:
                total += scene.render_shaded(cam, sun_of(gpu, gw, tuple(d), max_steps=40), diffuse=True, shadows=True)[:, :, 0]
            fb, light = scene.render_lit_sum(cam, sun_of(gpu, gw, max_steps=40), dirs, diffuse=True, light=True)
            assert np.array_equal(light[hit].astype(np.int64), total[hit]) and (light[~hit] == NO_HIT).all()
            assert np.unique(light[hit]).size >= 59
            # (white under the sum: the pixel formula on c = 255)
            assert np.array_equal(fb[hit][:, 0].astype(np.int64), lsc.pixel(255, total[hit], 256))
            back = scene.render_lit_sum(cam, sun_of(gpu, gw, max_steps=40), dirs[::-1], diffuse=True, light=True)
            assert back[0].tobytes() == fb.tobytes() and back[1].tobytes() == light.tobytes()
    finally:
        scene.close()


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_top_of_the_range(world, variant):
    """K = 256, HMRM_SHADE_NO_SHADOWS, ambient 255: light is 65280 on every hit and rgba is render's frame."""
    gpu, gw = world.gpu, 0.05
    dirs = gpu.sky_directions(16, 16)
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            sampling = samplings_of(variant)[proj % len(samplings_of(variant))]
            cam = sc.camera(gpu, gw, proj, False, sampling)
            for diffuse in (False, True):
                fb, light = world.scenes[gw].render_lit_sum(cam, sun_of(gpu, gw, ambient=255), dirs, diffuse=diffuse, shadows=False, light=True)
                hit = world.primary(gw, proj, sampling)["status"].reshape(30, 40) == 1
                assert hit.sum() >= 100 and (light[hit] == 65280).all() and (light[~hit] == NO_HIT).all()
                assert fb.tobytes() == world.scenes[gw].render(cam).tobytes()


# ---- 4. HMRM_TRACE_INTERIOR, strides ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_interior_flag(world, proj, variant):
    gpu = world.gpu
    with kernel_variant(variant):
        for gw in GRID_WIDTHS:
            for sampling in samplings_of(variant):
                cam = sc.camera(gpu, gw, proj, True, sampling)
                for diffuse, shadows in MODES[:2]:
                    want = world.lit_sum(gw, proj, sampling, SUNS, diffuse, shadows, inside=True)
                    assert want["hit"].sum() >= 60 and want["capped"] == 0
                    got = world.scenes[gw].render_lit_sum(cam, sun_of(gpu, gw, interior=True), SUNS, diffuse=diffuse, shadows=shadows, light=True)
                    same_planes(got, want, f"interior flag proj {proj} gw {gw} sampling {sampling} {variant} diffuse {diffuse}")


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_rows_wider_than_the_frame_keep_their_padding(world, variant):
    gpu, gw = world.gpu, 1.0
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            sampling = samplings_of(variant)[proj % len(samplings_of(variant))]
            cam = sc.camera(gpu, gw, proj, False, sampling)
            want = world.lit_sum(gw, proj, sampling, SUNS, True, True)
            fb, light = world.scenes[gw].render_lit_sum(cam, sun_of(gpu, gw), SUNS, diffuse=True, light=True, pad_px=5)
            assert fb.shape == (30, 45, 4) and light.shape == (30, 45)
            assert (fb[:, 40:] == 0xA5).all() and (light[:, 40:] == 0xA5A5).all()
            same_planes((np.ascontiguousarray(fb[:, :40]), np.ascontiguousarray(light[:, :40])), want, f"padded rows proj {proj} {variant}")


# ---- 5. the device entry ----
def test_device_entry_on_a_stream(world):
    """Planes and directions in torch tensors, a non-default torch stream, a light pointer that is 2-byte and not 4-byte aligned,
    take_capped for that stream; a misaligned pointer is refused and nothing is written."""
    import torch
    gpu, gw = world.gpu, 0.05
    scene = world.scenes[gw]
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    d_dirs = torch.tensor(np.asarray(SUNS, dtype=np.float64), device="cuda")
    for proj, inside, sampling, (diffuse, shadows) in ((1, False, 0, MODES[0]), (2, True, 1, MODES[1]), (3, False, 2, MODES[2])):
        cam = sc.camera(gpu, gw, proj, inside, sampling)
        want = world.lit_sum(gw, proj, sampling, SUNS, diffuse, shadows, inside=inside)
        rgba = torch.zeros((30, 48), dtype=torch.int32, device="cuda")
        light = torch.full((30 * 44 + 8,), 0x5A5A, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        lptr = light.data_ptr() + 2
        assert lptr % 4 == 2
        scene.render_lit_sum_device(cam, sun_of(gpu, gw, interior=inside), d_dirs.data_ptr(), 3, rgba=(rgba.data_ptr(), 48 * 4), light=(lptr, 88),
                                    diffuse=diffuse, shadows=shadows, stream=stream.cuda_stream)
        assert scene.take_capped(stream.cuda_stream) == 0  # (waits for the stream)
        host = rgba.cpu().numpy()
        same_frame(host[:, :40].copy().view(np.uint8).reshape(30, 40, 4), want["rgba"], f"device entry proj {proj}, rgba")
        assert (host[:, 40:] == 0).all()
        lh = light.cpu().numpy().view(np.uint16)
        assert lh[0] == 0x5A5A and (lh[1 + 30 * 44:] == 0x5A5A).all()
        rows = lh[1:1 + 30 * 44].reshape(30, 44)
        same_light(np.ascontiguousarray(rows[:, :40]), want["light"], f"device entry proj {proj}, light")
        assert (rows[:, 40:] == 0x5A5A).all()
    # refused before anything is launched: an odd light pointer, an rgba pointer off its element, directions off 8 bytes
    cam = sc.camera(gpu, gw, 1, False, 0)
    rgba = torch.full((30 * 40 + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    light = torch.full((30 * 40 + 4,), 0x5A5A, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    for kw, word in ((dict(rgba=(rgba.data_ptr(), 160), light=(light.data_ptr() + 1, 80)), "light must be 2-byte aligned"),
                     (dict(rgba=(rgba.data_ptr() + 2, 160), light=(light.data_ptr(), 80)), "rgba must be 4-byte aligned")):
        with pytest.raises(gpu.HmrmError) as e:
            scene.render_lit_sum_device(cam, sun_of(gpu, gw), d_dirs.data_ptr(), 3, stream=stream.cuda_stream, **kw)
        assert e.value.code == gpu.HMRM_E_ARG and word in str(e.value)
    with pytest.raises(gpu.HmrmError) as e:
        scene.render_lit_sum_device(cam, sun_of(gpu, gw), d_dirs.data_ptr() + 4, 2, rgba=(rgba.data_ptr(), 160), stream=stream.cuda_stream)
    assert e.value.code == gpu.HMRM_E_ARG and "d_dirs must be 8-byte aligned" in str(e.value)
    torch.cuda.synchronize()
    assert (rgba.cpu().numpy() == 0x5A5A5A5A).all() and (light.cpu().numpy() == 0x5A5A).all()


# ---- 6. the step cap ----
CAP = 300


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_capped_shadow_rays_count_per_ray(world, variant):
    """(one sun, straight up, straight up) at HMRM_STEP_CAP = 300: a ray straight up never leaves the grid, so two rays of every
    hit pixel reach the cap -- HMRM_E_NOTERM names 2 x the hit pixels, the planes are the replay's (a capped ray leaves its
    direction lit), the device entry's take_capped gives the same count; with max_steps = 50 they END: HMRM_OK and 0."""
    import torch
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    dirs = (SUNS[2], UP, UP)  # (no shadow ray towards this sun comes near 300 steps: it leaves over the map's near side)
    d_dirs = torch.tensor(np.asarray(dirs, dtype=np.float64), device="cuda")
    with kernel_variant(variant), env(HMRM_STEP_CAP=CAP):
        for proj in (1, 2, 3):
            sampling = samplings_of(variant)[proj % len(samplings_of(variant))]
            cam = sc.camera(gpu, gw, proj, False, sampling)
            want = world.lit_sum(gw, proj, sampling, dirs, True, True, step_cap=CAP)
            hits = int(want["hit"].sum())
            assert hits >= 100 and want["capped"] == 2 * hits
            with pytest.raises(gpu.HmrmError) as e:
                scene.render_lit_sum(cam, sun_of(gpu, gw), dirs, diffuse=True, light=True)
            assert e.value.code == gpu.HMRM_E_NOTERM and f"{2 * hits} ray(s)" in str(e.value), (hits, str(e.value))
            same_planes(scene.render_lit_sum(cam, sun_of(gpu, gw), dirs, diffuse=True, light=True, allow_capped=True), want,
                        f"capped proj {proj} {variant}")
            light = torch.zeros((30, 40), dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            scene.render_lit_sum_device(cam, sun_of(gpu, gw), d_dirs.data_ptr(), 3, light=(light.data_ptr(), 80), diffuse=True)
            assert scene.take_capped(0, allow_capped=True) == 2 * hits
            same_light(light.cpu().numpy().view(np.uint16), want["light"], f"capped, device entry, proj {proj} {variant}")
            ended = world.lit_sum(gw, proj, sampling, dirs, True, True, step_cap=CAP, max_steps=50)
            assert ended["capped"] == 0
            same_planes(scene.render_lit_sum(cam, sun_of(gpu, gw, max_steps=50), dirs, diffuse=True, light=True), ended,  # (raises unless HMRM_OK)
                        f"ended proj {proj} {variant}")
            scene.render_lit_sum_device(cam, sun_of(gpu, gw, max_steps=50), d_dirs.data_ptr(), 3, light=(light.data_ptr(), 80), diffuse=True)
            assert scene.take_capped(0) == 0


ODD_DIRS = (SUNS[0], (np.nan, 0.5, 0.3), (0.5, 0.4, np.inf), SUNS[1], (0.0, 0.0, 0.0), (0.5, -np.inf, 0.3), (0.5, 0.4, -0.3), SUNS[2],
            (0.5, 0.4, np.nan))


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_odd_directions_between_the_suns(world, variant):
    """NaN, infinite, zero and below-horizon directions between the suns, at HMRM_STEP_CAP = 300: the same arithmetic."""
    gpu, gw = world.gpu, 0.5
    with kernel_variant(variant), env(HMRM_STEP_CAP=CAP):
        for proj in (1, 2, 3):
            sampling = samplings_of(variant)[(proj + 1) % len(samplings_of(variant))]
            cam = sc.camera(gpu, gw, proj, False, sampling)
            for diffuse, shadows in MODES:
                want = world.lit_sum(gw, proj, sampling, ODD_DIRS, diffuse, shadows, step_cap=CAP)
                got = world.scenes[gw].render_lit_sum(cam, sun_of(gpu, gw), ODD_DIRS, diffuse=diffuse, shadows=shadows, light=True,
                                                      allow_capped=True)
                same_planes(got, want, f"odd directions proj {proj} {variant} diffuse {diffuse} shadows {shadows}")
                if want["capped"]:
                    with pytest.raises(gpu.HmrmError) as e:
                        world.scenes[gw].render_lit_sum(cam, sun_of(gpu, gw), ODD_DIRS, diffuse=diffuse, shadows=shadows)
                    assert e.value.code == gpu.HMRM_E_NOTERM and f"{want['capped']} ray(s)" in str(e.value)
                assert shadows or want["capped"] == 0  # (without shadow rays nothing is capped here)


# ---- 7. not a frame for the probe; the live table ----
def test_not_a_frame_for_the_probe(world, oracle):
    """hmrm_debug_kernel_choice is unchanged after 8 calls and a plain render afterwards is the replayed frame; a call after
    hmrm_scene_update uses the new heights."""
    gpu, gw = world.gpu, 0.5
    scene = gpu.Scene(world.rgb, world.cmap, world.params[gw])
    try:
        cam = sc.camera(gpu, gw, 1, False, 0, width=101, height=67)
        choice = scene.kernel_choice()
        want = world.lit_sum(gw, 1, 0, SUNS, True, True, width=101, height=67)
        for _ in range(8):
            same_planes(scene.render_lit_sum(cam, sun_of(gpu, gw), SUNS, diffuse=True, light=True), want, "8 calls")
        assert scene.kernel_choice() == choice
        same_frame(scene.render(cam), world.primary(gw, 1, 0, False, 101, 67)["rgba"], "a plain frame afterwards")
        before = scene.render_lit_sum(sc.camera(gpu, gw, 1, False, 0), sun_of(gpu, gw), SUNS, diffuse=True, light=True)
        same_planes(before, world.lit_sum(gw, 1, 0, SUNS, True, True), "before the update")
        params2 = gpu.SceneParams.make(0.0, 11.0 * gw, grid_width=gw)
        scene.update(params2)
        other = lsc.Replays(gpu, oracle)
        other.params[gw] = params2
        other.heights[gw] = oracle.update_heightmap(world.rgb, params2)
        want2 = other.lit_sum(gw, 1, 0, SUNS, True, True)
        assert want2["light"].tobytes() != before[1].tobytes()
        for variant in KERNEL_VARIANTS:
            with kernel_variant(variant):
                same_planes(scene.render_lit_sum(sc.camera(gpu, gw, 1, False, 0), sun_of(gpu, gw), SUNS, diffuse=True, light=True), want2,
                            f"after the update, {variant}")
    finally:
        scene.close()


# ---- 8. CLI ----
def test_cli_sky_light_key(world, tmp_path):
    gpu, gw = world.gpu, 0.5
    cfgp, text, outp = gs.cli_config(gpu, world, tmp_path, gw, output=False)
    keys = f"sun_dir 0 0 -1\nshadow_ambient {AMBIENT}\nshadow_step_dist {0.3 * gw:.17g}\nsky_light on\n"
    # the default rings: 4 x 16 directions, no diffuse levels
    cfgp.write_text(text + f"output {outp}\n" + keys)
    r = gs.run_hmap(gpu, cfgp)
    assert "sky_light on\n" in r.stdout and "rendered 1200 rays with sky light from 64 directions" in r.stdout and "ignored" not in r.stderr
    want = world.lit_sum(gw, 1, 0, gpu.sky_directions(4, 16), False, True)
    assert open(outp, "rb").read() == gpu.png_encode(np.ascontiguousarray(want["rgba"].reshape(30, 40, 4)))
    # sky_map_rings 3 7 with shading on, bilinear sampling and a limit
    cfgp.write_text(text + f"output {outp}\n" + keys + "sky_map_rings 3 7\nshading on\nsampling bilinear\nshadow_max_steps 40\n")
    r = gs.run_hmap(gpu, cfgp)
    assert "rendered 1200 rays with sky light from 21 directions" in r.stdout and "ignored" not in r.stderr
    want = world.lit_sum(gw, 1, 1, gpu.sky_directions(3, 7), True, True, max_steps=40)
    assert open(outp, "rb").read() == gpu.png_encode(np.ascontiguousarray(want["rgba"].reshape(30, 40, 4)))
    # the three cases in which the key is ignored, whatever sun_scope says
    plain = gpu.png_encode(np.ascontiguousarray(world.primary(gw, 1, 0)["rgba"].reshape(30, 40, 4)))
    cfgp.write_text(text + f"output {outp}\n" + keys + "sun_scope all\ndevices 2\n")
    with env(HMRM_OVERSUBSCRIBE_DEVICES=1):  # (a one-GPU box keeps `devices 2`: two scenes on the one device)
        r = gs.run_hmap(gpu, cfgp)
    assert "WARNING: sky_light is ignored with devices > 1" in r.stderr and "sky light from" not in r.stdout
    assert open(outp, "rb").read() == plain
    cfgp.write_text(text + f"output {outp}\n" + keys + "sun_scope all\nantialias 2\n")
    r = gs.run_hmap(gpu, cfgp)
    assert "WARNING: sky_light is ignored with antialias > 1" in r.stderr and "sky light from" not in r.stdout
    rec = tmp_path / "rec"
    cfgp.write_text(text + f"output {rec}\n" + keys + "sun_scope all\nrecord orbit\nrecording_frame_count 1\n")
    r = gs.run_hmap(gpu, cfgp)
    assert "WARNING: sky_light is ignored with record orbit" in r.stderr and "sky light from" not in r.stdout
