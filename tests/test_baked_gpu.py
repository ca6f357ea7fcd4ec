"""Baked-light frames on the GPU (hmrm_render_baked, the scene's light plane and their ticketed and recorded forms;
include/hmrm.h).  Every frame is compared BYTEWISE with tests/baked_cases.py's replay -- a composition of the primary replays
and the plane, which tests/test_baked_cpu.py pins -- or, without the replay, with frames of hmrm_render, hmrm_render_geometry,
hmrm_render_shaded and hmrm_render_lit_sum from the same GPU.  Map, grid widths and cameras are those of tests/segment_cases.py
at 40 x 30 unless said otherwise (a partial tile row and sky-only waves in every frame); the plane is the formula plane of
tests/baked_cases.py (full scale 1000) or its byte twin (full scale 255)."""
import functools
import math

import numpy as np
import pytest

import aa_box
import baked_cases as bc
import cell_map_replay as cmr
import gpu_support as gs
import lit_replay as lr
import ray_replay
import segment_cases as sc
import segment_replay as sr
from baked_cases import BASE_CAP, FULL_SCALE
from gpu_support import KERNEL_VARIANTS, PROJ_IDS, SAMPLINGS, env, gpu, kernel_variant, same_frame
from lit_cases import SUNS
from segment_cases import BG, GRID_WIDTHS, GW_IDS, MAP_H, MAP_W
from shade_cases import AMBIENT

pytestmark = pytest.mark.gpu

samplings_of = functools.partial(gs.samplings_of, nearest_only=("rec", "simple"))  # (the literal loop too: nearest sampling only)


class World(gs.Scenes, bc.Replays):
    def filtered(self, gw, proj, sampling, n, plane=None, full_scale=FULL_SCALE, inside=False, width=20, height=15):
        """The replayed antialiased frame: the baked frame of the n x n larger camera, box-filtered."""
        want = self.baked(gw, proj, sampling, plane, full_scale, inside, width * n, height * n)
        return aa_box.box_filter(want["rgba"].reshape(height * n, width * n, 4), n)

    def of_camera(self, cam, gw, plane, full_scale, n=1, interior=False):
        """The replayed (antialiased) baked frame of any camera, from the oracle's rays of its super camera."""
        sup = aa_box.super_camera(self.gpu, cam, n)
        rays = ray_replay.camera_rays(self.oracle, self.oracle.make_cfg(sup, self.params[gw], MAP_W, MAP_H))
        kw = dict(bg=BG, sampling=cam.sampling, step_cap=BASE_CAP)
        if interior:
            primary = sr.replay(rays, self.heights[gw], self.cmap, self.params[gw], cam.step_dist, interior=True, **kw)
        else:
            primary = ray_replay.replay(rays, self.heights[gw], self.cmap, self.params[gw], cam.step_dist, **kw)
        hit = primary["status"] == lr.HIT
        light = bc.light_of(primary, plane, self.params[gw], cam.sampling)
        frame = bc.apply(primary["rgba"], hit, light, full_scale).reshape(sup.height, sup.width, 4)
        return aa_box.box_filter(frame, n)


world = gs.world_fixture(World)


def planes_of(world):
    return ((world.plane, FULL_SCALE, "u16"), (world.plane8, 255, "u8"))


def one_sun_plane(world, gw, sampling, sun):
    q = cmr.levels(world.heights[gw], world.params[gw], sampling, sun)
    return cmr.weights(world.heights[gw].shape, None, q, cmr.WEIGHT | cmr.DIFFUSE | cmr.NO_SHADOWS, AMBIENT)


# ---- 1. the replay sweep ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_baked_frame_is_the_replay(world, proj, variant, gw):
    gpu, scene = world.gpu, world.scenes[gw]
    with kernel_variant(variant):
        for plane, full_scale, name in planes_of(world):
            scene.set_light(plane, full_scale)
            for sampling in samplings_of(variant):
                for inside in (False, True):
                    cam = sc.camera(gpu, gw, proj, inside, sampling)
                    want = world.baked(gw, proj, sampling, plane, full_scale, inside=inside)
                    assert want["hit"].sum() >= 100 and want["capped"] == 0
                    assert (want["rgba"] != want["primary"]["rgba"]).any(axis=1).sum() >= 0.9 * want["hit"].sum()
                    same_frame(scene.render_baked(cam, interior=inside), want["rgba"],
                               f"proj {proj} {variant} gw {gw} sampling {sampling} inside {inside} plane {name}")


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_baked_odd_frame(world, variant):
    """101 x 67: no multiple of the 8 x 16 tile, more than one workgroup each way."""
    gpu, gw, proj = world.gpu, 0.5, 1
    world.scenes[gw].set_light(world.plane, FULL_SCALE)
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            cam = sc.camera(gpu, gw, proj, False, sampling, width=101, height=67)
            want = world.baked(gw, proj, sampling, width=101, height=67)
            assert want["hit"].sum() >= 500 and want["capped"] == 0
            same_frame(world.scenes[gw].render_baked(cam), want["rgba"], f"101 x 67 {variant} sampling {sampling}")


# ---- 2. identities, without the replay ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_full_light_everywhere_is_render(world, variant):
    """L = D everywhere: Scene.render, and with interior=True Scene.render_interior, byte for byte."""
    gpu = world.gpu
    with kernel_variant(variant):
        for gw, full_scale in zip(GRID_WIDTHS, (1, 255, 65535)):
            scene = world.scenes[gw]
            scene.set_light(np.full((MAP_H, MAP_W), full_scale, dtype=np.uint16), full_scale)
            for proj in (1, 2, 3):
                for sampling in samplings_of(variant):
                    assert scene.render_baked(sc.camera(gpu, gw, proj, False, sampling)).tobytes() == \
                        scene.render(sc.camera(gpu, gw, proj, False, sampling)).tobytes(), (variant, gw, proj, sampling)
                    inside = sc.camera(gpu, gw, proj, True, sampling)
                    assert scene.render_baked(inside, interior=True).tobytes() == scene.render_interior(inside).tobytes(), \
                        (variant, gw, proj, sampling, "inside")


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_nearest_modes_are_a_composition_of_three_calls(world, variant):
    """Scene.render's pixels, render_geometry's cell plane and the plane Scene.light() returns, composed in numpy."""
    gpu = world.gpu
    with kernel_variant(variant):
        for gw in GRID_WIDTHS:
            scene = world.scenes[gw]
            scene.set_light(world.plane, FULL_SCALE)
            plane, full_scale = scene.light()
            assert full_scale == FULL_SCALE and plane.tobytes() == world.plane.tobytes()
            for proj in (1, 2, 3):
                for sampling in (s for s in samplings_of(variant) if s != 1):
                    cam = sc.camera(gpu, gw, proj, False, sampling)
                    rgba = scene.render(cam).reshape(-1, 4)
                    cell = scene.render_geometry(cam, rgba=False, range=False, slope=False)["cell"].reshape(-1)
                    hit = cell >= 0
                    assert hit.sum() >= 100
                    light = np.where(hit, plane.reshape(-1).astype(np.int64)[np.where(hit, cell, 0)], 0)
                    same_frame(scene.render_baked(cam), bc.apply(rgba, hit, light, full_scale), f"composition {variant} gw {gw} proj {proj} sampling {sampling}")


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_baked_suns_give_the_hillshade(world, variant):
    """bake_light with WEIGHT | DIFFUSE | NO_SHADOWS: one sun gives render_shaded(diffuse=True, shadows=False)'s frame, the three
    suns render_lit_sum(..., diffuse=True, shadows=False)'s, in the nearest-cell modes."""
    gpu = world.gpu
    with kernel_variant(variant):
        for gw in GRID_WIDTHS:
            scene = world.scenes[gw]
            for sampling in (s for s in samplings_of(variant) if s != 1):
                for proj in (1, 2, 3):
                    cam = sc.camera(gpu, gw, proj, False, sampling)
                    sun = gpu.Sun.make(SUNS[proj % 3], 0.3 * gw, ambient=AMBIENT)
                    scene.bake_light([SUNS[proj % 3]], 0.3 * gw, weight=True, diffuse=True, shadows=False, sampling=sampling, ambient=AMBIENT)
                    assert scene.light()[1] == 255
                    assert scene.render_baked(cam).tobytes() == scene.render_shaded(cam, sun, diffuse=True, shadows=False).tobytes(), \
                        (variant, gw, sampling, proj)
                scene.bake_light(SUNS, 0.3 * gw, weight=True, diffuse=True, shadows=False, sampling=sampling, ambient=AMBIENT)
                assert scene.light()[1] == 765
                for proj in (1, 2, 3):
                    cam = sc.camera(gpu, gw, proj, False, sampling)
                    sun = gpu.Sun.make((9.0, 9.0, -9.0), 0.3 * gw, ambient=AMBIENT)
                    assert scene.render_baked(cam).tobytes() == scene.render_lit_sum(cam, sun, SUNS, diffuse=True, shadows=False).tobytes(), \
                        (variant, gw, sampling, proj, "three suns")


def test_bake_light_writes_the_words_of_cell_map_sum(world):
    """Status mode and WEIGHT mode, and K = 256 once with max_steps = 40: Scene.light() is cell_map_sum's map byte for byte, the
    full scale K or 255 K."""
    gpu = world.gpu
    for gw, sampling in zip(GRID_WIDTHS, SAMPLINGS):
        scene = world.scenes[gw]
        for kw, scale in ((dict(), 3), (dict(weight=True), 765), (dict(weight=True, diffuse=True), 765)):
            scene.bake_light(SUNS, 0.3 * gw, lift=0.01 * gw, sampling=sampling, ambient=AMBIENT, **kw)
            plane, full_scale = scene.light()
            want = scene.cell_map_sum(SUNS, 0.3 * gw, lift=0.01 * gw, sampling=sampling, ambient=AMBIENT, **kw)
            assert full_scale == scale and plane.tobytes() == want.tobytes(), (gw, kw)
            assert np.unique(plane).size >= 3
    sky = gpu.sky_directions(16, 16)
    scene = world.scenes[0.5]
    scene.bake_light(sky, 0.15, max_steps=40)
    plane, full_scale = scene.light()
    assert full_scale == 256 and plane.tobytes() == scene.cell_map_sum(sky, 0.15, max_steps=40).tobytes() and plane.max() <= 256
    point = (16.0, -12.0, 9.0)
    scene.bake_light([point], 0.15, point=True)
    plane, full_scale = scene.light()
    assert full_scale == 1 and plane.tobytes() == scene.cell_map_sum([point], 0.15, point=True).tobytes() and set(np.unique(plane)) <= {0, 1}


def test_device_entry_takes_cell_map_sum_device_output(world):
    """A torch tensor that cell_map_sum_device filled on a non-default stream goes in through set_light_device on that stream
    -- no host sync in between -- and gives the frame of the host path; a byte plane with padded rows is widened on the device."""
    import torch
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    cam = sc.camera(gpu, gw, 1, False, 1)
    scene.bake_light(SUNS, 0.15, weight=True, diffuse=True, ambient=AMBIENT)
    want_plane, _ = scene.light()
    want = scene.render_baked(cam)
    scene.clear_light()
    d_targets = torch.tensor(np.asarray(SUNS, dtype=np.float64), device="cuda")
    d_map = torch.zeros((MAP_H, MAP_W + 6), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    scene.cell_map_sum_device(d_map.data_ptr(), 2 * (MAP_W + 6), d_targets.data_ptr(), 3, 0.15, weight=True, diffuse=True, ambient=AMBIENT,
                              stream=stream.cuda_stream)
    scene.set_light_device(d_map.data_ptr(), 2 * (MAP_W + 6), 765, stream=stream.cuda_stream)
    plane, full_scale = scene.light()
    assert full_scale == 765 and plane.tobytes() == want_plane.tobytes()
    assert scene.render_baked(cam).tobytes() == want.tobytes()
    d_bytes = torch.tensor(np.pad(world.plane8, ((0, 0), (0, 3)), constant_values=7), device="cuda")
    torch.cuda.synchronize()
    scene.set_light_device(d_bytes.data_ptr(), MAP_W + 3, 255, u16=False, stream=stream.cuda_stream)
    plane, full_scale = scene.light()
    assert full_scale == 255 and np.array_equal(plane, world.plane8.astype(np.uint16))
    same_frame(scene.render_baked(cam), world.baked(gw, 1, 1, world.plane8, 255)["rgba"], "byte plane from the device")
    # refusals, in the header's order, with a scene: the old plane stays
    for args, word in (((None, 128, 1000), "NULL plane"), ((d_map.data_ptr(), 128, 0), "full_scale"), ((d_map.data_ptr(), 128, 65536), "full_scale"),
                       ((d_map.data_ptr(), 126, 1000), "below a row"), ((d_map.data_ptr(), 129, 1000), "even"),
                       ((d_map.data_ptr() + 1, 128, 1000), "2-byte aligned")):
        with pytest.raises(gpu.HmrmError) as e:
            scene.set_light_device(args[0], args[1], args[2], stream=stream.cuda_stream)
        assert e.value.code == gpu.HMRM_E_ARG and word in str(e.value), (word, str(e.value))
    assert scene.light()[1] == 255 and np.array_equal(scene.light()[0], world.plane8.astype(np.uint16))


# ---- 3. antialiasing ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("factor", [2, 4])
def test_antialiased_frame_is_the_filtered_replay(world, factor, variant):
    gpu = world.gpu
    with kernel_variant(variant):
        for gw, proj, inside in zip(GRID_WIDTHS, (1, 2, 3), (False, True, False)):
            scene = world.scenes[gw]
            scene.set_light(world.plane, FULL_SCALE)
            for sampling in samplings_of(variant):
                cam = sc.camera(gpu, gw, proj, inside, sampling, width=20, height=15)
                same_frame(scene.render_baked(cam, interior=inside, factor=factor), world.filtered(gw, proj, sampling, factor, inside=inside),
                           f"aa {factor} {variant} gw {gw} proj {proj} sampling {sampling}")


def test_factor_eight_and_factor_one(world):
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    scene.set_light(world.plane, FULL_SCALE)
    cam = sc.camera(gpu, gw, 1, False, 1, width=20, height=15)
    same_frame(scene.render_baked(cam, factor=8), world.filtered(gw, 1, 1, 8), "aa 8")
    with kernel_variant("simple"):
        cam0 = sc.camera(gpu, gw, 1, False, 0, width=20, height=15)
        same_frame(scene.render_baked(cam0, factor=8), world.filtered(gw, 1, 0, 8), "aa 8, the literal loop")
    for proj in (1, 2, 3):
        cam = sc.camera(gpu, gw, proj, False, 0)
        assert scene.render_baked(cam, factor=1).tobytes() == scene.render_baked(cam).tobytes()
        same_frame(scene.render_baked(cam, factor=1), world.baked(gw, proj, 0)["rgba"], f"factor 1 proj {proj}")
    with pytest.raises(gpu.HmrmError) as e:
        scene.render_baked(cam, factor=3)
    assert e.value.code == gpu.HMRM_E_ARG and "antialias factor" in str(e.value)


# ---- 4. tickets ----
def test_tickets_in_flight_on_one_scene(world):
    """Four baked tickets with different factors and a plain one in flight: each gives its replay.  A new plane set while four
    are in flight: those finish with the old plane, the next begin sees the new one."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    scene.set_light(world.plane, FULL_SCALE)
    cam = sc.camera(gpu, gw, 1, False, 1, width=20, height=15)
    plain_cam = sc.camera(gpu, gw, 1, False, 0)
    tickets = [(scene.render_baked_begin(cam, aa=n, no_probe=(n == 4)), n) for n in (1, 2, 4, 8)]
    plain = scene.render_begin(plain_cam)
    assert len({t for t, _n in tickets} | {plain}) == 5
    same_frame(scene.render_wait(plain, (30, 40)), world.primary(gw, 1, 0)["rgba"], "the plain ticket")
    scene.render_release(plain)
    for t, n in reversed(tickets):
        same_frame(scene.render_wait(t, (15, 20)), world.filtered(gw, 1, 1, n), f"baked ticket, factor {n}")
        scene.render_release(t)
    other = np.ascontiguousarray(world.plane[::-1, ::-1])
    assert other.tobytes() != world.plane.tobytes()
    big = sc.camera(gpu, gw, 1, False, 0, width=101, height=67)
    tickets = [scene.render_baked_begin(big) for _ in range(4)]
    scene.set_light(other, FULL_SCALE)
    late = scene.render_baked_begin(big)
    for t in tickets:
        same_frame(scene.render_wait(t, (67, 101)), world.baked(gw, 1, 0, width=101, height=67)["rgba"], "begun before the new plane")
        scene.render_release(t)
    same_frame(scene.render_wait(late, (67, 101)), world.baked(gw, 1, 0, other, width=101, height=67)["rgba"], "begun after the new plane")
    scene.render_release(late)


def test_device_ticket_keeps_the_padding(world):
    import torch
    gpu, gw = world.gpu, 0.05
    scene = world.scenes[gw]
    scene.set_light(world.plane8, 255)
    for proj, inside, sampling, n in ((1, False, 0, 1), (2, True, 1, 2), (3, False, 2, 4)):
        cam = sc.camera(gpu, gw, proj, inside, sampling, width=20, height=15)
        buf = torch.full((15, 27), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t = scene.render_baked_device_begin(cam, buf.data_ptr(), 27 * 4, interior=inside, aa=n)
        scene.render_device_wait(t)
        host = buf.cpu().numpy()
        assert (host[:, 20:] == 0x5A5A5A5A).all()
        same_frame(host[:, :20].copy().view(np.uint8).reshape(15, 20, 4), world.filtered(gw, proj, sampling, n, world.plane8, 255, inside),
                   f"device ticket proj {proj} factor {n}")
    with pytest.raises(gpu.HmrmError) as e:
        scene.render_baked_device_begin(cam, buf.data_ptr(), 27 * 4 + 2)
    assert e.value.code == gpu.HMRM_E_ARG and "stride_bytes" in str(e.value)


def test_update_leaves_the_plane_and_clear_light_refuses(world, tmp_path):
    gpu, gw = world.gpu, 0.5
    scene = gpu.Scene(world.rgb, world.cmap, world.params[gw])
    try:
        cam = sc.camera(gpu, gw, 1, False, 0)
        assert scene.light() == (None, 0)
        with pytest.raises(gpu.HmrmError) as e:
            scene.render_baked(cam)
        assert e.value.code == gpu.HMRM_E_ARG and "the scene has no light plane" in str(e.value)
        scene.set_light(world.plane, FULL_SCALE)
        same_frame(scene.render_baked(cam), world.baked(gw, 1, 0)["rgba"], "before the update")
        scene.update(gpu.SceneParams.make(0.0, 11.0 * gw, grid_width=gw))
        plane, full_scale = scene.light()
        assert full_scale == FULL_SCALE and plane.tobytes() == world.plane.tobytes()
        rgba = scene.render(cam).reshape(-1, 4)
        cell = scene.render_geometry(cam, rgba=False, range=False, slope=False)["cell"].reshape(-1)
        hit = cell >= 0
        light = np.where(hit, plane.reshape(-1).astype(np.int64)[np.where(hit, cell, 0)], 0)
        after = scene.render_baked(cam)
        same_frame(after, bc.apply(rgba, hit, light, full_scale), "after the update: the new heights under the old plane")
        assert after.tobytes() != world.baked(gw, 1, 0)["rgba"].tobytes()
        scene.clear_light()
        assert scene.light() == (None, 0)
        for call in (lambda: scene.render_baked(cam), lambda: scene.render_baked(cam, factor=2), lambda: scene.render_baked_begin(cam),
                     lambda: gpu.record_orbit_baked([scene], cam, 16.0, -12.0, 20.0, 0.0, 2, str(tmp_path), 7)):
            with pytest.raises(gpu.HmrmError) as e:
                call()
            assert e.value.code == gpu.HMRM_E_ARG and "the scene has no light plane" in str(e.value)
        assert not list(tmp_path.iterdir())
        assert scene.render(cam).tobytes() == rgba.tobytes()
    finally:
        scene.close()


# ---- 5. recording ----
def orbit_of(gw):
    """The CLI's orbit (hmap_main.cpp): around the map's centre through the camera's position."""
    cx, cy = MAP_W * gw / 2.0, -(MAP_H * gw) / 2.0
    dx, dy = cx - (-6.0 * gw), cy - 8.0 * gw
    return cx, cy, math.sqrt(dx * dx + dy * dy), math.atan2(dy, dx)


def test_record_orbit_baked(world, tmp_path):
    gpu, gw, frames = world.gpu, 0.5, 3
    scene = world.scenes[gw]
    scene.set_light(world.plane, FULL_SCALE)
    base = sc.camera(gpu, gw, 1, False, 1)
    cx, cy, radius, hang0 = orbit_of(gw)
    gpu.record_orbit_baked([scene], base, cx, cy, radius, hang0, frames, str(tmp_path), 55, aa=2, encoder_threads=2)
    assert sorted(p.name for p in tmp_path.iterdir()) == [f"hmap_55_{k}.png" for k in range(frames)]
    pngs = set()
    for k in range(frames):
        cam = gpu.orbit_camera(base, cx, cy, radius, hang0, k, frames)
        want = gpu.png_encode(world.of_camera(cam, gw, world.plane, FULL_SCALE, n=2))
        assert (tmp_path / f"hmap_55_{k}.png").read_bytes() == want, k
        pngs.add(want)
    assert len(pngs) == frames


# ---- 6. saturation, padded rows, the step cap, the probe ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_saturation_and_padded_rows(world, variant):
    """D = 100 under the formula plane: most hit pixels over-brighten and saturate at 255; rows 5 pixels wider keep their padding."""
    gpu, gw = world.gpu, 1.0
    scene = world.scenes[gw]
    scene.set_light(world.plane, 100)
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            sampling = samplings_of(variant)[proj % len(samplings_of(variant))]
            cam = sc.camera(gpu, gw, proj, False, sampling)
            want = world.baked(gw, proj, sampling, world.plane, 100)
            assert (want["rgba"][want["hit"], 0:3] == 255).any(axis=1).sum() >= 50
            fb = scene.render_baked(cam, pad_px=5)
            assert fb.shape == (30, 45, 4) and (fb[:, 40:] == 0xA5).all()
            same_frame(np.ascontiguousarray(fb[:, :40]), want["rgba"], f"saturation, padded rows, proj {proj} {variant}")


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_capped_primary_rays(world, variant):
    """HMRM_STEP_CAP = 300.  The inside spherical camera: a few rays near the zenith never leave the grid -- HMRM_E_NOTERM with
    the replayed count and the replayed frame.  Straight up from inside, orthographic (tests/test_segments_gpu.py's camera): every
    ray is capped, none is reweighted."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    scene.set_light(world.plane, FULL_SCALE)
    with kernel_variant(variant), env(HMRM_STEP_CAP=300):
        for sampling in samplings_of(variant):
            cam = sc.camera(gpu, gw, 2, True, sampling)
            want = world.baked(gw, 2, sampling, inside=True, step_cap=300)
            assert want["capped"] >= 1 and want["hit"].sum() >= 100
            with pytest.raises(gpu.HmrmError) as e:
                scene.render_baked(cam, interior=True)
            assert e.value.code == gpu.HMRM_E_NOTERM and f"{want['capped']} ray(s)" in str(e.value), (want["capped"], str(e.value))
            same_frame(scene.render_baked(cam, interior=True, allow_capped=True), want["rgba"], f"capped, {variant} sampling {sampling}")
        up = gpu.Camera.make(width=16, height=8, projection=3, hfov=gpu.degrees_to_rads(80), hang=0.0, vang=0.0, pos=(10.25, -10.25, 3.9),
                             ortho_width=0.25, step_dist=0.1, bg=BG)
        with pytest.raises(gpu.HmrmError) as e:
            scene.render_baked(up, interior=True)
        assert e.value.code == gpu.HMRM_E_NOTERM and "128 ray(s)" in str(e.value)
        assert scene.render_baked(up, interior=True, allow_capped=True).tobytes() == scene.render_interior(up, allow_capped=True).tobytes()


def test_not_a_frame_for_the_probe(world):
    """kernel_choice() is unchanged after 8 baked frames and a plain frame afterwards is the replay."""
    gpu, gw = world.gpu, 0.5
    scene = gpu.Scene(world.rgb, world.cmap, world.params[gw])
    try:
        scene.set_light(world.plane, FULL_SCALE)
        cam = sc.camera(gpu, gw, 1, False, 0, width=101, height=67)
        choice = scene.kernel_choice()
        want = world.baked(gw, 1, 0, width=101, height=67)
        for _ in range(8):
            same_frame(scene.render_baked(cam), want["rgba"], "8 frames")
        assert scene.kernel_choice() == choice
        same_frame(scene.render(cam), want["primary"]["rgba"], "a plain frame afterwards")
    finally:
        scene.close()


# ---- 7. CLI ----
def test_cli_baked_light_key(world, tmp_path):
    gpu, gw = world.gpu, 0.5
    cfgp, _, outp = gs.cli_config(gpu, world, tmp_path, gw, output=False)

    def text(width, height):
        return gs.cli_preamble(gw, tmp_path / "h.ppm", tmp_path / "c.png", width=width, height=height)

    sun = SUNS[0]
    keys = (f"sun_dir {sun[0]:.17g} {sun[1]:.17g} {sun[2]:.17g}\nshadow_ambient {AMBIENT}\nshadow_step_dist {0.3 * gw:.17g}\n"
            f"shadow_max_steps 40\n")

    def run(body, **kw):
        cfgp.write_text(body)
        with env(**kw):
            return gs.run_hmap(gpu, cfgp)

    hillshade = one_sun_plane(world, gw, 0, sun)
    # baked_light sun with shading on: the hillshade of sun_dir, baked once, under the plain frame
    r = run(text(40, 30) + f"output {outp}\n" + keys + "baked_light sun\nshading on\n")
    assert "baked_light sun\n" in r.stdout and "baked light: 1 direction(s), full scale 255\n" in r.stdout and "ignored" not in r.stderr
    assert open(outp, "rb").read() == gpu.png_encode(np.ascontiguousarray(world.baked(gw, 1, 0, hillshade, 255)["rgba"].reshape(30, 40, 4)))
    # baked_light sky with sky_map_rings 3 7 and antialias 2: the count of open directions per cell, full scale 21
    dirs = gpu.sky_directions(3, 7)
    count = sum((cmr.statuses(world.heights[gw], world.cmap, world.params[gw], 0, tuple(d), 0.3 * gw, max_steps=40) != cmr.HIT).astype(np.uint16)
                for d in dirs)
    r = run(text(20, 15) + f"output {outp}\n" + keys + "baked_light sky\nsky_map_rings 3 7\nantialias 2\n")
    assert "baked light: 21 direction(s), full scale 21\n" in r.stdout and "ignored" not in r.stderr
    assert open(outp, "rb").read() == gpu.png_encode(world.filtered(gw, 1, 0, 2, count, 21))
    # record orbit, 1 frame
    rec = tmp_path / "rec"
    r = run(text(40, 30) + f"output {rec}\n" + keys + "baked_light sun\nshading on\nrecord orbit\nrecording_frame_count 1\n")
    assert "baked light: 1 direction(s), full scale 255\n" in r.stdout and r.stdout.rstrip().endswith("Done recording.") and "ignored" not in r.stderr
    files = list(rec.iterdir())
    assert len(files) == 1 and files[0].name.endswith("_0.png")
    cx, cy, radius, hang0 = orbit_of(gw)
    cam0 = gpu.orbit_camera(sc.camera(gpu, gw, 1, False, 0), cx, cy, radius, hang0, 0, 1)
    assert files[0].read_bytes() == gpu.png_encode(world.of_camera(cam0, gw, hillshade, 255))
    # the two warnings
    plain = gpu.png_encode(np.ascontiguousarray(world.primary(gw, 1, 0)["rgba"].reshape(30, 40, 4)))
    r = run(text(40, 30) + f"output {outp}\n" + keys + "baked_light sun\nshading on\ndevices 2\n", HMRM_OVERSUBSCRIBE_DEVICES=1)
    assert "WARNING: baked_light is ignored with devices > 1" in r.stderr and "baked light:" not in r.stdout
    r = run(text(40, 30) + f"output {outp}\n" + keys + "baked_light sun\nshading on\nsky_light on\n")
    assert "WARNING: sky_light is ignored with baked_light" in r.stderr and "baked light: 1 direction(s)" in r.stdout and "sky light from" not in r.stdout
    assert open(outp, "rb").read() != plain
    assert open(outp, "rb").read() == gpu.png_encode(np.ascontiguousarray(world.baked(gw, 1, 0, hillshade, 255)["rgba"].reshape(30, 40, 4)))
