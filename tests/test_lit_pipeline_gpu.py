"""Antialiased, ticketed and recorded sun-lit frames on the GPU (hmrm_render_shaded_aa, hmrm_render_shaded_begin,
hmrm_render_shaded_device_begin, hmrm_record_orbit_shaded; include/hmrm.h).  Every frame is compared BYTEWISE with the
definition: aa_box.box_filter of tests/shade_replay.py's frame of the super camera (tests/lit_pipeline_cases.py), which
tests/test_lit_pipeline_cpu.py pins to the C oracle; one test compares the GPU with itself instead (the antialiased frame
against the filtered hmrm_render_shaded frame of the super camera).  Map, grid widths, cameras and suns are those of
tests/segment_cases.py / tests/shade_cases.py, shadow step_dist 0.3 * grid width, ambient 96."""
import ctypes as C
import math

import numpy as np
import pytest

import gpu_support as gs
import lit_pipeline_cases as lp
import lit_replay as lr
import segment_cases as sc
import shade_cases as shc
import shade_replay as shr
from aa_box import box_filter, super_camera
from gpu_support import KERNEL_VARIANTS, PROJ_IDS, SAMPLINGS, env, gpu, kernel_variant, same_frame, samplings_of
from segment_cases import BG, GRID_WIDTHS, GW_IDS, MAP_H, MAP_W
from shade_cases import AMBIENT, SUNS

pytestmark = pytest.mark.gpu

UP = (0.0, 0.0, 1.0)


class World(gs.Scenes, shc.Replays):
    pass


world = gs.world_fixture(World)


def sun_of(gpu, gw, direction, **kw):
    kw.setdefault("ambient", AMBIENT)
    return gpu.Sun.make(direction, kw.pop("step_dist", 0.3 * gw), **kw)


def camera_of(gpu, gw, proj, sampling, shape, inside=False):
    return sc.camera(gpu, gw, proj, inside, sampling, width=shape[0], height=shape[1])


# ---- 1. the base sweep at n = 2: 3 projections x 3 grid widths x 4 variants x 3 samplings x 3 suns x 3 modes ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_antialiased_lit_frame_is_the_filtered_replay(world, proj, variant, gw):
    gpu, scene = world.gpu, world.scenes[gw]
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            cam = camera_of(gpu, gw, proj, sampling, lp.BASE)
            for sun in SUNS:
                for diffuse, shadows in lp.MODES:
                    want, replay = lp.expected(world, gw, proj, sampling, sun, diffuse, shadows, lp.BASE)
                    lp.check_content(replay, lp.BASE, sampling, shadows, (gw, proj, sampling, sun))
                    fb = scene.render_shaded(cam, sun_of(gpu, gw, sun), diffuse=diffuse, shadows=shadows, aa=2)
                    same_frame(fb, want, f"n 2 proj {proj} {variant} gw {gw} sampling {sampling} sun {sun} diffuse {diffuse} shadows {shadows}")


# ---- 2. the other shapes: ragged tiles, one block per wave, more than one workgroup each way ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("shape", lp.OTHER_SHAPES, ids=[f"{w}x{h}_n{n}" for w, h, n in lp.OTHER_SHAPES])
def test_other_shapes(world, shape, variant):
    gpu = world.gpu
    with kernel_variant(variant):
        for case_shape, gw, proj, sun in lp.other_cases():
            if case_shape != shape:
                continue
            for sampling in samplings_of(variant):
                cam = camera_of(gpu, gw, proj, sampling, shape)
                for diffuse, shadows in lp.MODES:
                    want, replay = lp.expected(world, gw, proj, sampling, sun, diffuse, shadows, shape)
                    lp.check_content(replay, shape, sampling, shadows, (gw, proj, sampling, sun))
                    fb = world.scenes[gw].render_shaded(cam, sun_of(gpu, gw, sun), diffuse=diffuse, shadows=shadows, aa=shape[2])
                    same_frame(fb, want, f"{shape} proj {proj} {variant} gw {gw} sampling {sampling} diffuse {diffuse} shadows {shadows}")


# ---- 3. without the replay: the GPU's own frame of the super camera, filtered ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_antialiased_frame_is_the_filtered_super_frame_of_the_gpu(world, variant):
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            for sampling in samplings_of(variant):
                cam = sc.camera(gpu, gw, proj, False, sampling, width=13, height=9)
                sun = sun_of(gpu, gw, SUNS[proj - 1])
                for n in (2, 4, 8):
                    for shadows in (True, False):
                        big = scene.render_shaded(super_camera(gpu, cam, n), sun, shadows=shadows)
                        fb = scene.render_shaded(cam, sun, shadows=shadows, aa=n)
                        same_frame(fb, box_filter(big, n), f"13 x 9 n {n} proj {proj} {variant} sampling {sampling} shadows {shadows}")


# ---- 4. the four identities of the definition ----
def shaded_aa(gpu, scene, cam, sun, diffuse, shadows, factor):
    """hmrm_render_shaded_aa itself, whatever the factor (Scene.render_shaded calls hmrm_render_shaded for aa = 1)."""
    fb = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
    rc = gpu.lib.lib.hmrm_render_shaded_aa(scene._h, C.byref(cam), C.byref(sun), gpu.shade_flags(diffuse, shadows), factor,
                                           fb.ctypes.data_as(C.c_void_p), cam.width * 4)
    assert rc == gpu.HMRM_OK, gpu.last_error()
    return fb


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_identities(world, variant):
    """Factor 1 is render_shaded; HMRM_SHADE_NO_SHADOWS alone is render_aa (with HMRM_TRACE_INTERIOR and the inside camera the
    filtered render_interior frame); ambient = 255 is render_aa under any flags; shade_flags = 0 is the antialiased render_lit
    frame."""
    gpu = world.gpu
    with kernel_variant(variant):
        for gw in GRID_WIDTHS:
            scene = world.scenes[gw]
            for proj in (1, 2, 3):
                for sampling in samplings_of(variant):
                    n = (2, 4, 8)[(proj + sampling) % 3]
                    cam = camera_of(gpu, gw, proj, sampling, (10, 8, n))
                    big = super_camera(gpu, cam, n)
                    sun = sun_of(gpu, gw, SUNS[0])
                    what = (gw, proj, sampling, n)
                    for diffuse, shadows in lp.MODES:
                        assert shaded_aa(gpu, scene, cam, sun, diffuse, shadows, 1).tobytes() == \
                            scene.render_shaded(cam, sun, diffuse=diffuse, shadows=shadows).tobytes(), what
                    plain = scene.render_aa(cam, n).tobytes()
                    assert scene.render_shaded(cam, sun, diffuse=False, shadows=False, aa=n).tobytes() == plain, what
                    full = sun_of(gpu, gw, SUNS[0], ambient=255)
                    for diffuse in (False, True):
                        for shadows in (False, True):
                            assert scene.render_shaded(cam, full, diffuse=diffuse, shadows=shadows, aa=n).tobytes() == plain, (what, diffuse, shadows)
                    lit = box_filter(scene.render_lit(big, sun), n).tobytes()
                    assert lit != plain
                    assert scene.render_shaded(cam, sun, diffuse=False, shadows=True, aa=n).tobytes() == lit, what
                    assert scene.render_lit(cam, sun, aa=n).tobytes() == lit, what
                    inside = camera_of(gpu, gw, proj, sampling, (10, 8, n), inside=True)
                    isun = sun_of(gpu, gw, SUNS[2], interior=True)
                    assert scene.render_shaded(inside, isun, diffuse=False, shadows=False, aa=n).tobytes() == \
                        box_filter(scene.render_interior(super_camera(gpu, inside, n)), n).tobytes(), what


# ---- 5. tickets ----
def test_host_and_device_lit_tickets_are_the_synchronous_frame(world):
    torch = pytest.importorskip("torch")
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    for proj in (1, 2, 3):
        for n in (1, 2, 4):
            cam = camera_of(gpu, gw, proj, proj - 1, (20, 15, n))
            sun = sun_of(gpu, gw, SUNS[proj - 1])
            for diffuse, shadows in lp.MODES:
                sync = scene.render_shaded(cam, sun, diffuse=diffuse, shadows=shadows, aa=n)
                t = scene.render_shaded_begin(cam, sun, diffuse=diffuse, shadows=shadows, aa=n, no_probe=bool(n & 2))  # (HMRM_NO_PROBE is accepted)
                got = scene.render_wait(t, (cam.height, cam.width))
                scene.render_release(t)
                same_frame(got, sync, f"host ticket proj {proj} n {n} diffuse {diffuse} shadows {shadows}")
                dev = torch.zeros((cam.height, cam.width, 4), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                t = scene.render_shaded_device_begin(cam, sun, dev.data_ptr(), cam.width * 4, diffuse=diffuse, shadows=shadows, aa=n,
                                                     no_probe=bool(n & 4))
                scene.render_device_wait(t)
                same_frame(dev.cpu().numpy(), sync, f"device ticket proj {proj} n {n} diffuse {diffuse} shadows {shadows}")


def test_burst_of_mixed_tickets_and_the_scene_after_it(world, oracle):
    """Nine tickets in flight on one scene -- plain, lit and shaded frames at factors 1, 2 and 4 -- waited for out of order, each
    against its own expectation; the sun is gone by the time the frames are waited for.  Lit frames leave the scene's kernel
    choice alone, and a plain render afterwards is the oracle's."""
    gpu, gw, proj, sampling = world.gpu, 0.5, 1, 0
    scene = gpu.Scene(world.rgb, world.cmap, world.params[gw])
    try:
        before = scene.kernel_choice()
        kinds = {"plain": (False, False), "lit": (False, True), "shaded": (True, True)}
        burst = []
        for kind, n in (("shaded", 2), ("plain", 1), ("lit", 4), ("plain", 4), ("shaded", 1), ("lit", 2), ("shaded", 4), ("plain", 2), ("lit", 1)):
            shape = (40 // n, 32 // n, n)  # (the same 40 x 32 super frame)
            cam = camera_of(gpu, gw, proj, sampling, shape)
            diffuse, shadows = kinds[kind]
            want, _ = lp.expected(world, gw, proj, sampling, SUNS[0], diffuse, shadows, shape)
            if kind == "plain":
                t = scene.render_begin(cam, aa=n)
            else:
                sun = sun_of(gpu, gw, SUNS[0])
                t = scene.render_shaded_begin(cam, sun, diffuse=diffuse, shadows=shadows, aa=n)
                C.memset(C.addressof(sun), 0xFF, C.sizeof(sun))  # (the call has copied it)
                del sun
            burst.append((kind, n, cam, t, want))
        assert len({t for _k, _n, _c, t, _w in burst}) == 9
        assert len({w.tobytes() for _k, _n, _c, _t, w in burst}) == 9
        for k in (4, 8, 0, 6, 2, 7, 1, 5, 3):
            kind, n, cam, t, want = burst[k]
            got = scene.render_wait(t, (cam.height, cam.width))
            scene.render_release(t)
            same_frame(got, want, f"burst ticket {k}: {kind} n {n}")
        assert scene.kernel_choice() == before
        cam = camera_of(gpu, gw, proj, sampling, (40, 30, 1))
        ofb = oracle.render(oracle.make_cfg(cam, world.params[gw], MAP_W, MAP_H), world.heights[gw], world.cmap)[0]
        same_frame(scene.render(cam), np.asarray(ofb), "plain render after the burst")
        assert scene.kernel_choice() == before
    finally:
        scene.close()


def test_device_ticket_into_a_wider_stride(world):
    torch = pytest.importorskip("torch")
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    for shape, pad in (((20, 15, 2), 4), ((10, 8, 4), 52), ((5, 4, 8), 1024)):
        w, h, n = shape
        cam = camera_of(gpu, gw, 3, 0, shape)
        want, _ = lp.expected(world, gw, 3, 0, SUNS[1], True, True, shape)
        stride = w * 4 + pad
        dev = torch.full((h, stride), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t = scene.render_shaded_device_begin(cam, sun_of(gpu, gw, SUNS[1]), dev.data_ptr(), stride, aa=n)
        scene.render_device_wait(t)
        got = dev.cpu().numpy()
        same_frame(np.ascontiguousarray(got[:, :w * 4]).reshape(h, w, 4), want, f"stride {stride} {shape}")
        assert (got[:, w * 4:] == 0x5A).all(), shape
    with pytest.raises(gpu.HmrmError):  # (a device stride must be a multiple of 4)
        scene.render_shaded_device_begin(cam, sun_of(gpu, gw, SUNS[1]), dev.data_ptr(), w * 4 + 2, aa=n)


# ---- 6. capped samples through a host ticket ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_capped_samples_are_counted_per_sample(world, variant):
    """The sun straight up at HMRM_STEP_CAP = 300, n = 2: every hit sample's shadow ray runs to the cap -- the wait returns
    HMRM_E_NOTERM with the number of hit samples of the 40 x 30 super frame and the filtered frame; with max_steps = 50 the
    shadow rays END and the wait returns HMRM_OK.  No primary ray of these frames is capped at 300."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    with kernel_variant(variant), env(HMRM_STEP_CAP=300):
        for proj in (1, 2, 3):
            for sampling in samplings_of(variant):
                cam = camera_of(gpu, gw, proj, sampling, lp.BASE)
                want, replay = lp.expected(world, gw, proj, sampling, UP, True, True, lp.BASE, step_cap=300)
                hits = int((replay["primary"]["status"] == lr.HIT).sum())
                assert replay["capped"] == hits >= 124
                t = scene.render_shaded_begin(cam, sun_of(gpu, gw, UP), aa=2)
                with pytest.raises(gpu.HmrmError) as e:
                    scene.render_wait(t, (cam.height, cam.width))
                assert e.value.code == gpu.HMRM_E_NOTERM and f"{hits} ray(s)" in str(e.value), (proj, sampling, hits, str(e.value))
                got = scene.render_wait(t, (cam.height, cam.width))  # (reported once; the frame is valid)
                scene.render_release(t)
                same_frame(got, want, f"capped proj {proj} sampling {sampling} {variant}")
                t = scene.render_shaded_begin(cam, sun_of(gpu, gw, UP, max_steps=50), aa=2)
                got = scene.render_wait(t, (cam.height, cam.width))  # (raises unless HMRM_OK)
                scene.render_release(t)
                same_frame(got, want, f"END proj {proj} sampling {sampling} {variant}")


# ---- 7. hmrm_scene_update between begin and wait ----
def test_update_between_begin_and_wait(world, oracle):
    gpu, gw = world.gpu, 0.5
    scene = gpu.Scene(world.rgb, world.cmap, world.params[gw])
    try:
        params2 = gpu.SceneParams.make(0.0, 11.0 * gw, grid_width=gw)
        heights2 = oracle.update_heightmap(world.rgb, params2)
        for sampling in SAMPLINGS:
            cam = camera_of(gpu, gw, 1, sampling, lp.BASE)
            old, _ = lp.expected(world, gw, 1, sampling, SUNS[0], True, True, lp.BASE)
            new = shr.replay(world.rays(gw, 1), heights2, world.cmap, params2, 0.2 * gw, SUNS[0], 0.3 * gw, bg=BG, sampling=sampling,
                             step_cap=shc.BASE_CAP, ambient=AMBIENT)
            new = box_filter(new["rgba"].reshape(30, 40, 4), 2)
            assert new.tobytes() != old.tobytes()
            t = scene.render_shaded_begin(cam, sun_of(gpu, gw, SUNS[0]), aa=2)
            scene.update(params2)
            t2 = scene.render_shaded_begin(cam, sun_of(gpu, gw, SUNS[0]), aa=2)
            same_frame(scene.render_wait(t, (15, 20)), old, f"begun before the update, sampling {sampling}")
            same_frame(scene.render_wait(t2, (15, 20)), new, f"begun after the update, sampling {sampling}")
            scene.render_release(t)
            scene.render_release(t2)
            scene.update(world.params[gw])
    finally:
        scene.close()


# ---- 8. HMRM_TRACE_INTERIOR under n = 2 ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_interior_flag(world, proj, variant):
    """The inside camera (orthographic: a frame that mixes interior origins with exterior rays that enter)."""
    gpu = world.gpu
    with kernel_variant(variant):
        for gw in GRID_WIDTHS:
            for sampling in samplings_of(variant):
                cam = camera_of(gpu, gw, proj, sampling, lp.BASE, inside=True)
                for diffuse, shadows in lp.MODES:
                    want, replay = lp.expected(world, gw, proj, sampling, SUNS[2], diffuse, shadows, lp.BASE, inside=True)
                    assert replay["capped"] == 0 and int(((replay["primary"]["status"] == lr.HIT) & ~replay["shadowed"]).sum()) >= 60
                    fb = world.scenes[gw].render_shaded(cam, sun_of(gpu, gw, SUNS[2], interior=True), diffuse=diffuse, shadows=shadows, aa=2)
                    same_frame(fb, want, f"interior proj {proj} gw {gw} sampling {sampling} {variant} diffuse {diffuse} shadows {shadows}")


# ---- 9. recording ----
def orbit_of(gw):
    """The CLI's orbit (hmap_main.cpp): around the map's centre through the camera's position."""
    cx, cy = MAP_W * gw / 2.0, -(MAP_H * gw) / 2.0
    dx, dy = cx - (-6.0 * gw), cy - 8.0 * gw
    return cx, cy, math.sqrt(dx * dx + dy * dy), math.atan2(dy, dx)


def test_record_orbit_shaded(world, tmp_path):
    gpu, gw, frames = world.gpu, 0.5, 3
    scene = world.scenes[gw]
    base = camera_of(gpu, gw, 1, 0, lp.BASE)
    cx, cy, radius, hang0 = orbit_of(gw)
    sun = sun_of(gpu, gw, SUNS[0])
    out = tmp_path / "lit"
    out.mkdir()
    gpu.record_orbit_shaded([scene], base, cx, cy, radius, hang0, frames, str(out), 55, sun, aa=2, encoder_threads=2)
    assert sorted(p.name for p in out.iterdir()) == [f"hmap_55_{k}.png" for k in range(frames)]
    pngs = set()
    for k in range(frames):
        cam = gpu.orbit_camera(base, cx, cy, radius, hang0, k, frames)
        sync = scene.render_shaded(cam, sun, aa=2)
        assert (out / f"hmap_55_{k}.png").read_bytes() == gpu.png_encode(sync), k
        pngs.add(gpu.png_encode(sync))
    assert len(pngs) == frames
    want0, _ = lp.expected(world, gw, 1, 0, SUNS[0], True, True, lp.BASE)  # (frame 0 of the orbit is the base pose up to rounding)
    assert scene.render_shaded(base, sun, aa=2).tobytes() == want0.tobytes()
    # sun = NULL: the files of hmrm_record_orbit_flags
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    gpu.record_orbit_shaded([scene], base, cx, cy, radius, hang0, frames, str(a), 56, None, aa=2, encoder_threads=2)
    gpu.record_orbit_multi([scene], base, cx, cy, radius, hang0, frames, str(b), 56, encoder_threads=2, aa=2)
    assert sorted(p.name for p in a.iterdir()) == sorted(p.name for p in b.iterdir()) == [f"hmap_56_{k}.png" for k in range(frames)]
    for k in range(frames):
        assert (a / f"hmap_56_{k}.png").read_bytes() == (b / f"hmap_56_{k}.png").read_bytes(), k
        assert (a / f"hmap_56_{k}.png").read_bytes() != (out / f"hmap_55_{k}.png").read_bytes()


# ---- 10. CLI ----
def test_cli_sun_scope_all(world, tmp_path):
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    cfgp, text, outp = gs.cli_config(gpu, world, tmp_path, gw, output=False, width=20, height=15)
    keys = f"sun_dir 0.6 0.5 0.35\nshadow_ambient {AMBIENT}\nshadow_step_dist {0.3 * gw:.17g}\nsun_scope all\nantialias 2\nshading on\n"
    bare, _ = lp.expected(world, gw, 1, 0, SUNS[0], True, False, lp.BASE)
    full, _ = lp.expected(world, gw, 1, 0, SUNS[0], True, True, lp.BASE)
    cfgp.write_text(text + f"output {outp}\n" + keys)
    r = gs.run_hmap(gpu, cfgp)
    assert "sun_scope all\n" in r.stdout and "rendered 1200 rays at antialias 2 with sun shading in" in r.stdout and "ignored" not in r.stderr
    assert open(outp, "rb").read() == gpu.png_encode(bare)
    cfgp.write_text(text + f"output {outp}\n" + keys + "shadows on\n")
    r = gs.run_hmap(gpu, cfgp)
    assert "at antialias 2 with sun shading and sun shadows in" in r.stdout and "ignored" not in r.stderr
    assert open(outp, "rb").read() == gpu.png_encode(full) != gpu.png_encode(bare)
    # record orbit: the reference's lines, the synchronous frames of the same orbit
    rec = tmp_path / "rec"
    cfgp.write_text(text + f"output {rec}\n" + keys + "shadows on\nrecord orbit\nrecording_frame_count 3\n")
    cfg = gpu.Config().consume_file(str(cfgp))
    base, sun = cfg.camera(), cfg.sun()
    assert cfg.sun_scope() == 1 and (base.width, base.height) == (20, 15)
    cfg.close()
    r = gs.run_hmap(gpu, cfgp)
    assert r.stdout.rstrip().endswith("Done recording.") and r.stdout.count("Saved screenshot at ") == 3 and "ignored" not in r.stderr
    files = sorted(rec.iterdir(), key=lambda p: int(p.stem.rsplit("_", 1)[1]))
    assert len(files) == 3
    cx, cy, radius, hang0 = orbit_of(gw)
    for k, f in enumerate(files):
        assert f.name.endswith(f"_{k}.png")
        cam = gpu.orbit_camera(base, cx, cy, radius, hang0, k, 3)
        assert f.read_bytes() == gpu.png_encode(scene.render_shaded(cam, sun, aa=2)), k
