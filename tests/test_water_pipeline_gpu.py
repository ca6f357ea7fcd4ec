"""Antialiased, ticketed, recorded and baked-light water frames on the GPU (hmrm_render_water_aa, hmrm_render_water_begin,
hmrm_render_water_device_begin, hmrm_record_orbit_water; include/hmrm.h).  Every frame is compared BYTEWISE with
tests/water_pipeline_cases.py's replay -- a composition of the water and the baked replays and the box filter, which
tests/test_water_pipeline_cpu.py pins -- or, without the replay, with frames of hmrm_render_water and hmrm_render_baked from the
same GPU.  The lake map, the level, grid widths and cameras are those of tests/water_cases.py at 40 x 30 unless said otherwise;
the plane is the formula plane of tests/baked_cases.py (full scale 1000); mirror step_dist 0.2 * grid width."""
import math

import numpy as np
import pytest

import aa_box
import cell_map_replay as cmr
import gpu_support as gs
import segment_cases as sc
import water_pipeline_cases as wp
import water_replay as wr
from baked_cases import FULL_SCALE
from gpu_support import KERNEL_VARIANTS, PROJ_IDS, env, gpu, kernel_variant, same_frame, samplings_of  # noqa: F401
from segment_cases import GRID_WIDTHS, GW_IDS, MAP_H, MAP_W
from test_water_gpu import down_camera
from water_cases import REFLECTIVITY

pytestmark = pytest.mark.gpu

AA_CASES = tuple(zip(GRID_WIDTHS, (1, 2, 3), (False, True, False)))  # (as tests/test_baked_gpu.py zips them)


class World(gs.Scenes, wp.Replays):
    def __init__(self, gpu, oracle):
        super().__init__(gpu, oracle)
        for s in self.scenes.values():
            s.set_light(self.plane, FULL_SCALE)

    def relight(self, gw):
        """The formula plane back into the scene of a test that set another one."""
        self.scenes[gw].set_light(self.plane, FULL_SCALE)
        return self.scenes[gw]


world = gs.world_fixture(World)


def water_of(gpu, world, gw, **kw):
    return gpu.Water.make(kw.pop("level", world.level(gw)), kw.pop("step_dist", 0.2 * gw), **kw)


def orbit_of(gw):
    """The CLI's orbit (hmap_main.cpp): around the map's centre through the camera's position."""
    cx, cy = MAP_W * gw / 2.0, -(MAP_H * gw) / 2.0
    dx, dy = cx - (-6.0 * gw), cy - 8.0 * gw
    return cx, cy, math.sqrt(dx * dx + dy * dy), math.atan2(dy, dx)


# ---- 1. baked water against the replay ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_baked_water_frame_is_the_replay(world, proj, variant, gw):
    gpu, scene = world.gpu, world.scenes[gw]
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            cam = sc.camera(gpu, gw, proj, False, sampling)
            want = world.frame(gw, proj, sampling, True)
            assert wp.light_differs(want) >= 5
            fb = scene.render_water_aa(cam, water_of(gpu, world, gw, reflectivity=REFLECTIVITY), baked=True)
            same_frame(fb, want["rgba"], f"baked water proj {proj} {variant} gw {gw} sampling {sampling}")


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_baked_water_odd_frame(world, variant):
    """101 x 67: partial tiles, more than one workgroup each way, waves that mix wet, dry and miss lanes
    (tests/test_water_pipeline_cpu.py counts them)."""
    gpu, gw = world.gpu, 0.5
    proj = 1 + KERNEL_VARIANTS.index(variant) % 3
    sampling = samplings_of(variant)[KERNEL_VARIANTS.index(variant) % len(samplings_of(variant))]
    cam = sc.camera(gpu, gw, proj, False, sampling, width=101, height=67)
    want = world.frame(gw, proj, sampling, True, width=101, height=67)
    with kernel_variant(variant):
        same_frame(world.scenes[gw].render_water_aa(cam, water_of(gpu, world, gw), baked=True), want["rgba"],
                   f"101 x 67 proj {proj} sampling {sampling} {variant}")


# ---- 2. antialiased against the filtered replay ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("factor", [2, 4])
def test_antialiased_frame_is_the_filtered_replay(world, factor, variant):
    gpu = world.gpu
    with kernel_variant(variant):
        for gw, proj, inside in AA_CASES:
            scene = world.scenes[gw]
            for sampling in samplings_of(variant):
                cam = sc.camera(gpu, gw, proj, inside, sampling, width=20, height=15)
                for baked in (False, True):
                    fb = scene.render_water_aa(cam, water_of(gpu, world, gw, interior=inside), factor=factor, baked=baked)
                    same_frame(fb, world.filtered(gw, proj, sampling, factor, baked, inside=inside),
                               f"aa {factor} {variant} gw {gw} proj {proj} sampling {sampling} baked {baked}")


def test_factor_eight_one_and_three(world):
    """Factor 8 at 13 x 9: the super frame is 104 x 72 with a partial tile row, and every wave is one output pixel whose 64
    samples may be wet, dry and miss at once.  Factor 1 is render_water; factor 3 is refused."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    w = water_of(gpu, world, gw)
    with kernel_variant("leap"):
        cam = sc.camera(gpu, gw, 1, False, 1, width=13, height=9)
        for baked in (False, True):
            same_frame(scene.render_water_aa(cam, w, factor=8, baked=baked), world.filtered(gw, 1, 1, 8, baked, width=13, height=9),
                       f"aa 8, leaps, baked {baked}")
    with kernel_variant("simple"):
        cam0 = sc.camera(gpu, gw, 1, False, 0, width=13, height=9)
        for baked in (False, True):
            same_frame(scene.render_water_aa(cam0, w, factor=8, baked=baked), world.filtered(gw, 1, 0, 8, baked, width=13, height=9),
                       f"aa 8, the literal loop, baked {baked}")
    for proj in (1, 2, 3):
        for sampling in (0, 1, 2):
            cam = sc.camera(gpu, gw, proj, False, sampling)
            assert scene.render_water_aa(cam, w, factor=1).tobytes() == scene.render_water(cam, w).tobytes(), (proj, sampling)
    for baked in (False, True):
        with pytest.raises(gpu.HmrmError) as e:
            scene.render_water_aa(cam, w, factor=3, baked=baked)
        assert e.value.code == gpu.HMRM_E_ARG and "antialias factor" in str(e.value)


# ---- 3. GPU against GPU, without the replay ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_identities_on_the_gpu(world, variant):
    """render_water_aa(cam, n) is the box filter of render_water(super camera); L = D everywhere is render_water; a level below
    every threshold and r = 0 are render_baked."""
    gpu = world.gpu
    with kernel_variant(variant):
        for gw, proj, inside in AA_CASES:
            scene = world.scenes[gw]
            for sampling in samplings_of(variant):
                small = sc.camera(gpu, gw, proj, inside, sampling, width=20, height=15)
                w = water_of(gpu, world, gw, interior=inside)
                for n in (2, 4):
                    sup = scene.render_water(aa_box.super_camera(gpu, small, n), w)
                    assert scene.render_water_aa(small, w, factor=n).tobytes() == aa_box.box_filter(sup, n).tobytes(), (gw, proj, sampling, n)
                cam = sc.camera(gpu, gw, proj, inside, sampling)
                baked = scene.render_baked(cam, interior=inside).tobytes()
                assert scene.render_water_aa(cam, water_of(gpu, world, gw, interior=inside, level=-1.0), baked=True).tobytes() == baked
                assert scene.render_water_aa(cam, water_of(gpu, world, gw, interior=inside, reflectivity=0), baked=True).tobytes() == baked
                assert scene.render_water_aa(small, water_of(gpu, world, gw, interior=inside, reflectivity=0), factor=2, baked=True).tobytes() == \
                    scene.render_baked(small, interior=inside, factor=2).tobytes()
                scene.set_light(np.full((MAP_H, MAP_W), 65535, dtype=np.uint16), 65535)
                try:
                    assert scene.render_water_aa(cam, w, baked=True).tobytes() == scene.render_water(cam, w).tobytes(), (gw, proj, sampling)
                finally:
                    world.relight(gw)


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("r,color", [(0, (40, 80, 160)), (254, (3, 250, 128))])
def test_own_colour_under_light(world, r, color, variant):
    gpu, gw = world.gpu, 0.5
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            sampling = samplings_of(variant)[proj % len(samplings_of(variant))]
            want = world.frame(gw, proj, sampling, True, reflectivity=r, color=color)
            cam = sc.camera(gpu, gw, proj, False, sampling)
            fb = world.scenes[gw].render_water_aa(cam, water_of(gpu, world, gw, reflectivity=r, color=color), baked=True)
            same_frame(fb, want["rgba"], f"own colour r {r} proj {proj} sampling {sampling} {variant}")
            small = sc.camera(gpu, gw, proj, False, sampling, width=20, height=15)
            fb = world.scenes[gw].render_water_aa(small, water_of(gpu, world, gw, reflectivity=r, color=color), factor=2, baked=True)
            same_frame(fb, world.filtered(gw, proj, sampling, 2, True, reflectivity=r, color=color), f"own colour r {r} aa 2 proj {proj} {variant}")


# ---- 4. tickets ----
def test_tickets_in_flight_on_one_scene(world):
    """Water tickets at factors 1, 2, 4 and 8 with and without BAKED, a plain and a baked ticket, all in flight on one scene: each
    gives its replay.  A new plane set while four baked water tickets are in flight: those finish with the old plane, the next
    begin sees the new one."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    cam = sc.camera(gpu, gw, 1, False, 1, width=20, height=15)
    plain_cam = sc.camera(gpu, gw, 1, False, 0)
    w = water_of(gpu, world, gw)
    tickets = [(scene.render_water_begin(cam, w, baked=baked, aa=n, no_probe=(n == 4)), n, baked) for n in (1, 2, 4, 8) for baked in (False, True)]
    w.level = -1.0  # (the water was copied at begin)
    plain = scene.render_begin(plain_cam)
    baked_t = scene.render_baked_begin(plain_cam)
    assert len({t for t, _n, _b in tickets} | {plain, baked_t}) == 10
    same_frame(scene.render_wait(plain, (30, 40)), world.primary(gw, 1, 0)["rgba"], "the plain ticket")
    scene.render_release(plain)
    same_frame(scene.render_wait(baked_t, (30, 40)), world.frame(gw, 1, 0, True, level=-1.0)["rgba"], "the baked ticket")
    scene.render_release(baked_t)
    for t, n, baked in reversed(tickets):
        same_frame(scene.render_wait(t, (15, 20)), world.filtered(gw, 1, 1, n, baked), f"water ticket, factor {n}, baked {baked}")
        scene.render_release(t)
    other = np.ascontiguousarray(world.plane[::-1, ::-1])
    assert other.tobytes() != world.plane.tobytes()
    big = sc.camera(gpu, gw, 1, False, 0, width=101, height=67)
    w = water_of(gpu, world, gw)
    try:
        tickets = [scene.render_water_begin(big, w, baked=True) for _ in range(4)]
        scene.set_light(other, FULL_SCALE)
        late = scene.render_water_begin(big, w, baked=True)
        for t in tickets:
            same_frame(scene.render_wait(t, (67, 101)), world.frame(gw, 1, 0, True, width=101, height=67)["rgba"], "begun before the new plane")
            scene.render_release(t)
        same_frame(scene.render_wait(late, (67, 101)), world.frame(gw, 1, 0, True, other, width=101, height=67)["rgba"], "begun after the new plane")
        scene.render_release(late)
    finally:
        world.relight(gw)


def test_device_ticket_keeps_the_padding(world):
    import torch
    gpu, gw = world.gpu, 0.05
    scene = world.scenes[gw]
    for proj, inside, sampling, n, baked in ((1, False, 0, 1, True), (2, True, 1, 2, False), (3, False, 2, 4, True)):
        cam = sc.camera(gpu, gw, proj, inside, sampling, width=20, height=15)
        buf = torch.full((15, 27), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t = scene.render_water_device_begin(cam, water_of(gpu, world, gw, interior=inside), buf.data_ptr(), 27 * 4, baked=baked, aa=n)
        scene.render_device_wait(t)
        host = buf.cpu().numpy()
        assert (host[:, 20:] == 0x5A5A5A5A).all()
        same_frame(host[:, :20].copy().view(np.uint8).reshape(15, 20, 4), world.filtered(gw, proj, sampling, n, baked, inside=inside),
                   f"device ticket proj {proj} factor {n} baked {baked}")
    with pytest.raises(gpu.HmrmError) as e:
        scene.render_water_device_begin(cam, water_of(gpu, world, gw), buf.data_ptr(), 27 * 4 + 2)
    assert e.value.code == gpu.HMRM_E_ARG and "stride_bytes" in str(e.value)


def test_no_light_plane_is_refused_by_all_four(world, tmp_path):
    gpu, gw = world.gpu, 0.5
    scene = gpu.Scene(world.rgb, world.cmap, world.params[gw])
    try:
        import torch
        cam = sc.camera(gpu, gw, 1, False, 0)
        w = water_of(gpu, world, gw)
        scene.set_light(world.plane, FULL_SCALE)
        same_frame(scene.render_water_aa(cam, w, baked=True), world.frame(gw, 1, 0, True)["rgba"], "with the plane")
        scene.clear_light()
        buf = torch.zeros((30, 40), dtype=torch.int32, device="cuda")
        for call in (lambda: scene.render_water_aa(cam, w, baked=True), lambda: scene.render_water_aa(cam, w, factor=2, baked=True),
                     lambda: scene.render_water_begin(cam, w, baked=True),
                     lambda: scene.render_water_device_begin(cam, w, buf.data_ptr(), 40 * 4, baked=True),
                     lambda: gpu.record_orbit_water([scene], cam, 16.0, -12.0, 20.0, 0.0, 2, str(tmp_path), 7, w, baked=True)):
            with pytest.raises(gpu.HmrmError) as e:
                call()
            assert e.value.code == gpu.HMRM_E_ARG and "the scene has no light plane" in str(e.value)
        assert not list(tmp_path.iterdir())
        # without BAKED nothing asks for the plane
        same_frame(scene.render_water_aa(cam, w), world.frame(gw, 1, 0, False)["rgba"], "without the plane")
    finally:
        scene.close()


# ---- 5. capped rays ----
def test_capped_rays_at_factor_two(world):
    """tests/test_water_gpu.py's camera looking straight down on the lake, at factor 2 under HMRM_STEP_CAP = 300: the mirror rays
    go straight up and run to the cap -- HMRM_E_NOTERM with the replay's count, one per capped sample, and a valid frame."""
    gpu, gw = world.gpu, 0.5
    scene, level = world.scenes[gw], world.level(gw)
    for sampling, baked in ((0, True), (2, False)):
        cam = down_camera(gpu, world, gw, sampling)
        with env(HMRM_STEP_CAP=300):
            want_fb, want = world.of_camera(cam, gw, level, n=2, baked=baked, step_cap=300)
            assert want["capped"] >= 300 and (want["mirror"]["status"] == wr.CAPPED).sum() == want["capped"]
            with pytest.raises(gpu.HmrmError) as e:
                scene.render_water_aa(cam, water_of(gpu, world, gw), factor=2, baked=baked)
            assert e.value.code == gpu.HMRM_E_NOTERM and f"{want['capped']} ray(s)" in str(e.value), (want["capped"], str(e.value))
            same_frame(scene.render_water_aa(cam, water_of(gpu, world, gw), factor=2, baked=baked, allow_capped=True), want_fb,
                       f"straight down, capped, factor 2, sampling {sampling}")


# ---- 6. the recorder ----
def test_record_orbit_water(world, tmp_path):
    gpu, gw, frames = world.gpu, 0.5, 3
    scene = world.scenes[gw]
    base = sc.camera(gpu, gw, 1, False, 1)
    cx, cy, radius, hang0 = orbit_of(gw)
    gpu.record_orbit_water([scene], base, cx, cy, radius, hang0, frames, str(tmp_path), 55, water_of(gpu, world, gw), baked=True, aa=2,
                           encoder_threads=2)
    assert sorted(p.name for p in tmp_path.iterdir()) == [f"hmap_55_{k}.png" for k in range(frames)]
    pngs = set()
    for k in range(frames):
        cam = gpu.orbit_camera(base, cx, cy, radius, hang0, k, frames)
        frame, replayed = world.of_camera(cam, gw, world.level(gw), n=2, baked=True)
        if k == 0:
            assert replayed["water"].sum() >= 34
        want = gpu.png_encode(frame)
        assert (tmp_path / f"hmap_55_{k}.png").read_bytes() == want, k
        pngs.add(want)
    assert len(pngs) == frames


# ---- 7. CLI ----
def test_cli_water_scope(world, tmp_path):
    gpu, gw = world.gpu, 0.5
    cfgp, _, outp = gs.cli_config(gpu, world, tmp_path, gw, output=False)
    keys = f"water on\nwater_level {world.level(gw):.17g}\nwater_reflectivity {REFLECTIVITY}\n"

    def text(width, height):
        return gs.cli_preamble(gw, tmp_path / "h.ppm", tmp_path / "c.png", width=width, height=height)

    def run(body, **kw):
        cfgp.write_text(body)
        with env(**kw):
            return gs.run_hmap(gpu, cfgp)

    # water_scope all with antialias 2
    r = run(text(20, 15) + f"output {outp}\n" + keys + "water_scope all\nantialias 2\n")
    assert "water_scope all\n" in r.stdout and "with water at level" in r.stdout and "at antialias 2" in r.stdout and "ignored" not in r.stderr
    assert open(outp, "rb").read() == gpu.png_encode(world.filtered(gw, 1, 0, 2, False))
    # ... with baked_light sky (sky_map_rings 3 7): the count of open directions per cell over the lake map, full scale 21
    shadow = f"shadow_step_dist {0.3 * gw:.17g}\nshadow_max_steps 40\n"
    dirs = gpu.sky_directions(3, 7)
    count = sum((cmr.statuses(world.heights[gw], world.cmap, world.params[gw], 0, tuple(d), 0.3 * gw, max_steps=40) != cmr.HIT).astype(np.uint16)
                for d in dirs)
    r = run(text(20, 15) + f"output {outp}\n" + keys + shadow + "water_scope all\nbaked_light sky\nsky_map_rings 3 7\nantialias 2\n")
    assert "baked light: 21 direction(s), full scale 21\n" in r.stdout and "under baked light" in r.stdout and "ignored" not in r.stderr
    assert open(outp, "rb").read() == gpu.png_encode(world.filtered(gw, 1, 0, 2, True, plane=count, full_scale=21))
    # ... with record orbit, 1 frame
    rec = tmp_path / "rec"
    r = run(text(40, 30) + f"output {rec}\n" + keys + "water_scope all\nrecord orbit\nrecording_frame_count 1\n")
    assert r.stdout.rstrip().endswith("Done recording.") and "ignored" not in r.stderr
    files = list(rec.iterdir())
    assert len(files) == 1 and files[0].name.endswith("_0.png")
    cx, cy, radius, hang0 = orbit_of(gw)
    cam0 = gpu.orbit_camera(sc.camera(gpu, gw, 1, False, 0), cx, cy, radius, hang0, 0, 1)
    assert files[0].read_bytes() == gpu.png_encode(world.of_camera(cam0, gw, world.level(gw))[0])
    # water_scope frame still warns as before
    r = run(text(20, 15) + f"output {outp}\n" + keys + "water_scope frame\nantialias 2\n")
    assert "WARNING: water is ignored with antialias > 1" in r.stderr and "with water" not in r.stdout
    r = run(text(40, 30) + f"output {outp}\n" + keys + shadow + "baked_light sky\nsky_map_rings 3 7\n")
    assert "WARNING: water is ignored with baked_light" in r.stderr and "under baked light" in r.stdout and "with water" not in r.stdout
    # devices 2 warns, whatever the scope
    r = run(text(40, 30) + f"output {outp}\n" + keys + "water_scope all\ndevices 2\n", HMRM_OVERSUBSCRIBE_DEVICES=1)
    assert "WARNING: water is ignored with devices > 1" in r.stderr and "with water" not in r.stdout
    # shadows without baked_light: ignored as before
    r = run(text(40, 30) + f"output {outp}\n" + keys + "water_scope all\nshadows on\n")
    assert "WARNING: water is ignored with shadows" in r.stderr and "with sun shadows" in r.stdout


# ---- 8. not a frame for the probe ----
def test_not_a_frame_for_the_probe(world):
    """kernel_choice() is unchanged after 8 water frames, antialiased and baked ones among them, and a plain frame afterwards is
    the replay."""
    gpu, gw = world.gpu, 0.5
    scene = gpu.Scene(world.rgb, world.cmap, world.params[gw])
    try:
        scene.set_light(world.plane, FULL_SCALE)
        cam = sc.camera(gpu, gw, 1, False, 0, width=101, height=67)
        small = sc.camera(gpu, gw, 1, False, 0, width=20, height=15)
        w = water_of(gpu, world, gw)
        choice = scene.kernel_choice()
        want = world.frame(gw, 1, 0, True, width=101, height=67)
        for k in range(8):
            same_frame(scene.render_water_aa(cam, w, baked=True), want["rgba"], "8 frames")
            same_frame(scene.render_water_aa(small, w, factor=2, baked=bool(k & 1)), world.filtered(gw, 1, 0, 2, bool(k & 1)), "8 antialiased frames")
        assert scene.kernel_choice() == choice
        same_frame(scene.render(cam), want["water"]["primary"]["rgba"], "a plain frame afterwards")
    finally:
        scene.close()
