"""Accumulated cell maps on the GPU (hmrm_cell_map_sum; include/hmrm.h).  Every map is compared BYTEWISE with the sum of
tests/cell_map_replay.py's maps over the targets (tests/cell_sum_cases.py), whose content tests/test_cell_map_sum_cpu.py pins;
two tests pin the kernels to Scene.cell_map on the same GPU without the replay.  Maps, grid widths, suns and observer points are
those of tests/cell_map_cases.py: step_dist 0.3 grid widths in direction mode, 1/64 with max_steps 64 in point mode, ambient 128."""
import functools
import os

import numpy as np
import pytest

import cell_map_cases as cc
import cell_map_replay as cmr
import cell_sum_cases as cs
import gpu_support as gs
import segment_cases as sc
from cell_map_cases import AMBIENT, GRID_WIDTHS, GW_IDS, MAP_H, MAP_W, MODES, SETTINGS, SUNS
from gpu_support import KERNEL_VARIANTS, SAMPLINGS, env, gpu, kernel_variant

pytestmark = pytest.mark.gpu

RECTS = ((3, 5, 29, 13), (63, 47, 1, 1), (0, 0, 64, 1), (56, 40, 8, 8))
SMALL_CAP = cs.SMALL_CAP
samplings_of = functools.partial(gs.samplings_of, nearest_only=("rec", "simple"))  # (the literal loop too: nearest sampling only)
same_map = functools.partial(gs.same_cells, dtype=np.uint16)


class World(gs.Scenes, cc.Replays):
    def __init__(self, gpu, oracle):
        super().__init__(gpu, oracle)
        self.scenes_b = {gw: gpu.Scene(self.rgb_b, self.cmap_b, self.params[gw]) for gw in (0.5, 0.05)}

    def close(self):
        super().close()
        for s in self.scenes_b.values():
            s.close()


world = gs.world_fixture(World)


# ---- 1. the replay sweep on map A: the three suns in one launch ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_sum_is_the_summed_replay(world, variant, gw):
    """K = 3 x {status, WEIGHT, WEIGHT + DIFFUSE, WEIGHT + DIFFUSE + NO_SHADOWS} x {lift 0 without a limit, lift 0.25 gw with
    max_steps 40} per sampling mode."""
    scene = world.scenes[gw]
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            for lift_gw, limit in SETTINGS:
                for flags in MODES:
                    want = cs.summed(world, gw, sampling, SUNS, 0.3 * gw, flags, lift_gw * gw, limit)
                    got = scene.cell_map_sum(SUNS, 0.3 * gw, lift=lift_gw * gw, max_steps=limit, sampling=sampling, ambient=AMBIENT,
                                             **cc.flags_kw(flags))
                    same_map(got, want, f"{variant} gw {gw} sampling {sampling} lift {lift_gw} limit {limit} flags {flags}")


# ---- 2. K = 1 with WEIGHT is hmrm_cell_map's map, widened ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_one_target_is_cell_map_widened(world, variant):
    gw = 0.5
    scene = world.scenes[gw]
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            for flags in MODES[1:]:
                for point, target, step, lift, limit in ((False, SUNS[1], 0.3 * gw, 0.25 * gw, 40),
                                                         (True, cc.point_inside(gw), cc.POINT_STEP, 0.25 * gw, cc.POINT_STEPS)):
                    kw = dict(cc.flags_kw(flags), point=point)
                    one = scene.cell_map(target, step, lift=lift, max_steps=limit, sampling=sampling, ambient=AMBIENT, **kw)
                    got = scene.cell_map_sum([target], step, lift=lift, max_steps=limit, sampling=sampling, ambient=AMBIENT, **kw)
                    assert len(np.unique(one)) >= 2
                    same_map(got, one.astype(np.uint16), f"K = 1 {variant} sampling {sampling} flags {flags} point {point}")


# ---- 3. without the replay: 256 sky directions against 256 launches of hmrm_cell_map on the same GPU ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_sky_sum_is_256_cell_maps(world, variant):
    """Map B whole (37 x 21: partial tiles on both sides), K = 256 from sky_directions(16, 16): status mode and WEIGHT | DIFFUSE;
    the same targets reversed give the same map."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes_b[gw]
    sky = gpu.sky_directions(16, 16)
    assert sky.shape == (256, 3)
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            for flags in (0, cmr.WEIGHT | cmr.DIFFUSE):
                kw = dict(lift=0.25 * gw, max_steps=40, sampling=sampling, ambient=AMBIENT, **cc.flags_kw(flags))
                want = np.zeros((cc.B_H, cc.B_W), dtype=np.int64)
                for t in sky:
                    one = scene.cell_map(t, 0.3 * gw, **kw)
                    want += one.astype(np.int64) if flags & cmr.WEIGHT else (one != cmr.HIT)
                assert len(np.unique(want)) >= 30, "a flat sum would show nothing"
                got = scene.cell_map_sum(sky, 0.3 * gw, **kw)
                same_map(got, want, f"sky {variant} sampling {sampling} flags {flags}")
                same_map(scene.cell_map_sum(sky[::-1], 0.3 * gw, **kw), want, f"sky reversed {variant} sampling {sampling} flags {flags}")


# ---- 4. the top of the range ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_top_of_the_range(world, variant):
    """K = 256, WEIGHT | NO_SHADOWS, ambient 255: every word is 256 * 255 = 65280."""
    gw = 0.5
    sky = world.gpu.sky_directions(16, 16)
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            got = world.scenes_b[gw].cell_map_sum(sky, 0.3 * gw, sampling=sampling, ambient=255, weight=True, shadows=False)
            assert got.shape == (cc.B_H, cc.B_W) and got.dtype == np.uint16 and (got == 65280).all(), np.unique(got)


# ---- 5. point mode: a cumulative viewshed of two observers ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_point_mode(world, variant):
    with kernel_variant(variant):
        for gw in GRID_WIDTHS:
            for sampling in samplings_of(variant):
                for lift in (0.0, 0.25 * gw):
                    for flags in (cmr.TOWARDS_POINT, cmr.TOWARDS_POINT | cmr.WEIGHT | cmr.DIFFUSE):
                        want = cs.summed(world, gw, sampling, cs.points(gw), cc.POINT_STEP, flags, lift, cc.POINT_STEPS)
                        got = world.scenes[gw].cell_map_sum(cs.points(gw), cc.POINT_STEP, lift=lift, max_steps=cc.POINT_STEPS,
                                                            sampling=sampling, ambient=AMBIENT, **cc.flags_kw(flags))
                        same_map(got, want, f"points lift {lift} {variant} gw {gw} sampling {sampling} flags {flags}")


# ---- 6. rects and strides ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_rects_and_strides(world, variant):
    """Each rect is the same slice of the whole map's summed replay, written into rows 6 bytes wider than the rect's words; the
    words between the rows stay as they were."""
    gw = 0.5
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            for flags in (0, cmr.WEIGHT | cmr.DIFFUSE):
                whole = cs.summed(world, gw, sampling, SUNS, 0.3 * gw, flags)
                for x0, y0, w, h in RECTS:
                    out = world.scenes[gw].cell_map_sum(SUNS, 0.3 * gw, sampling=sampling, ambient=AMBIENT, rect=(x0, y0, w, h),
                                                        stride_bytes=2 * w + 6, **cc.flags_kw(flags))
                    assert out.shape == (h, w + 3)
                    same_map(np.ascontiguousarray(out[:, :w]), whole[y0:y0 + h, x0:x0 + w],
                             f"rect {(x0, y0, w, h)} {variant} sampling {sampling} flags {flags}")
                    assert (out[:, w:] == 0xA5A5).all(), f"canaries of rect {(x0, y0, w, h)}"


def test_rect_and_stride_refusals(world):
    gpu, scene = world.gpu, world.scenes[0.5]
    for rect in ((0, 0, 0, 4), (0, 0, 4, 0), (-1, 0, 4, 4), (0, -1, 4, 4), (61, 0, 4, 4), (0, 45, 4, 4), (0, 0, -3, 4), (0, 0, 65, 1),
                 (2147483647, 0, 2, 1)):
        with pytest.raises(gpu.HmrmError) as e:
            scene.cell_map_sum(SUNS, 0.15, rect=rect, stride_bytes=160)
        assert e.value.code == gpu.HMRM_E_ARG and "rect" in str(e.value), rect
    for stride in (15, 14, 8, 0):  # (below 2 * w)
        with pytest.raises(gpu.HmrmError) as e:
            scene.cell_map_sum(SUNS, 0.15, rect=(0, 0, 8, 2), stride_bytes=stride)
        assert e.value.code == gpu.HMRM_E_ARG and "stride_bytes is below" in str(e.value), stride
    for stride in (17, 19, 2 * MAP_W + 1):  # (odd)
        with pytest.raises(gpu.HmrmError) as e:
            scene.cell_map_sum(SUNS, 0.15, rect=(0, 0, 8, 2), stride_bytes=stride)
        assert e.value.code == gpu.HMRM_E_ARG and "must be even" in str(e.value), stride


# ---- 7. the device entry ----
def test_device_entry(world):
    import torch
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    flags = cmr.WEIGHT | cmr.DIFFUSE
    stride = 2 * MAP_W + 22
    kw = dict(lift=0.25 * gw, max_steps=40, sampling=1, ambient=AMBIENT, **cc.flags_kw(flags))
    host = scene.cell_map_sum(SUNS, 0.3 * gw, **kw)
    same_map(host, cs.summed(world, gw, 1, SUNS, 0.3 * gw, flags, 0.25 * gw, 40), "host entry")
    first = 256 + 2  # (an even address that is not a multiple of 4: only 2-byte alignment is asked)
    d_buf = torch.full((first + MAP_H * stride + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    d_targets = torch.tensor(SUNS, dtype=torch.float64, device="cuda")
    assert d_buf.data_ptr() % 4 == 0 and d_targets.data_ptr() % 8 == 0
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    scene.cell_map_sum_device(d_buf.data_ptr() + first, stride, d_targets.data_ptr(), len(SUNS), 0.3 * gw, stream=stream.cuda_stream, **kw)
    assert scene.take_capped(stream.cuda_stream) == 0  # (waits for the stream; END rays are not counted)
    out = d_buf.cpu().numpy()
    rows = out[first:first + MAP_H * stride].reshape(MAP_H, stride)
    words = np.ascontiguousarray(rows[:, :2 * MAP_W]).view(np.uint16)
    same_map(words, host, "device entry")
    assert (rows[:, 2 * MAP_W:] == 0xA5).all() and (out[:first] == 0xA5).all() and (out[first + MAP_H * stride:] == 0xA5).all(), "the canaries"
    with pytest.raises(gpu.HmrmError) as e:
        scene.cell_map_sum_device(d_buf.data_ptr() + first + 1, stride, d_targets.data_ptr(), len(SUNS), 0.3 * gw,
                                  stream=stream.cuda_stream, **kw)
    assert e.value.code == gpu.HMRM_E_ARG and "2-byte aligned" in str(e.value)
    torch.cuda.synchronize()
    assert (d_buf.cpu().numpy() == out).all()


# ---- 8. capped rays are counted per ray ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_caps_are_counted_per_ray(world, variant):
    """(one sun, straight up, straight up) at HMRM_STEP_CAP = 300: the interior rays straight up never leave the grid, twice per
    cell -- HMRM_E_NOTERM with the replay's sums from the host entry, twice the replay's CAPPED cells from the device entry's
    take_capped; with max_steps = 50 the same rays END: HMRM_OK and nothing counted."""
    import torch
    gpu, gw = world.gpu, 0.5
    scene = world.scenes_b[gw]
    d_targets = torch.tensor(cs.CAP_TARGETS, dtype=torch.float64, device="cuda")
    d_out = torch.zeros((cc.B_H, cc.B_W), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with kernel_variant(variant), env(HMRM_STEP_CAP=SMALL_CAP):
        for sampling in samplings_of(variant):
            up_capped = int((world.status(gw, sampling, cs.UP, 0.3 * gw, 0.25 * gw, 0, False, SMALL_CAP, "B") == cmr.CAPPED).sum())
            assert up_capped >= 500
            assert cs.capped_rays(world, gw, sampling, cs.CAP_TARGETS, 0.3 * gw, 0.25 * gw, 0, SMALL_CAP, "B") == 2 * up_capped
            kw = dict(lift=0.25 * gw, sampling=sampling)
            want = cs.summed(world, gw, sampling, cs.CAP_TARGETS, 0.3 * gw, 0, 0.25 * gw, 0, step_cap=SMALL_CAP, which="B")
            with pytest.raises(gpu.HmrmError) as e:
                scene.cell_map_sum(cs.CAP_TARGETS, 0.3 * gw, **kw)
            assert e.value.code == gpu.HMRM_E_NOTERM and f"{2 * up_capped} ray(s)" in str(e.value), (up_capped, str(e.value))
            same_map(scene.cell_map_sum(cs.CAP_TARGETS, 0.3 * gw, allow_capped=True, **kw), want, f"capped {variant} sampling {sampling}")
            scene.cell_map_sum_device(d_out.data_ptr(), 2 * cc.B_W, d_targets.data_ptr(), 3, 0.3 * gw, stream=stream.cuda_stream, **kw)
            assert scene.take_capped(stream.cuda_stream, allow_capped=True) == 2 * up_capped
            same_map(d_out.cpu().numpy().view(np.uint16), want, f"capped, device entry {variant} sampling {sampling}")
            ended = cs.summed(world, gw, sampling, cs.CAP_TARGETS, 0.3 * gw, 0, 0.25 * gw, 50, step_cap=SMALL_CAP, which="B")
            assert cs.capped_rays(world, gw, sampling, cs.CAP_TARGETS, 0.3 * gw, 0.25 * gw, 50, SMALL_CAP, "B") == 0
            same_map(scene.cell_map_sum(cs.CAP_TARGETS, 0.3 * gw, max_steps=50, **kw), ended, f"END {variant} sampling {sampling}")
            scene.cell_map_sum_device(d_out.data_ptr(), 2 * cc.B_W, d_targets.data_ptr(), 3, 0.3 * gw, max_steps=50,
                                      stream=stream.cuda_stream, **kw)
            assert scene.take_capped(stream.cuda_stream) == 0


# ---- 9. targets nothing special-cases ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_odd_targets(world, variant):
    """A NaN component, an infinite component and the zero direction (which never moves: under the small cap) between the three
    suns, status and WEIGHT + DIFFUSE: the same arithmetic, the summed replay."""
    gw = 0.5
    scene = world.scenes_b[gw]
    with kernel_variant(variant), env(HMRM_STEP_CAP=SMALL_CAP):
        for sampling in samplings_of(variant):
            for flags in (0, cmr.WEIGHT | cmr.DIFFUSE):
                want = cs.summed(world, gw, sampling, cs.ODD_TARGETS, 0.3 * gw, flags, 0.25 * gw, 0, step_cap=SMALL_CAP, which="B")
                got = scene.cell_map_sum(cs.ODD_TARGETS, 0.3 * gw, lift=0.25 * gw, sampling=sampling, ambient=AMBIENT, allow_capped=True,
                                         **cc.flags_kw(flags))
                same_map(got, want, f"odd targets {variant} sampling {sampling} flags {flags}")


# ---- 10. an accumulated cell map is not a frame ----
def test_not_a_frame(world, oracle):
    gpu, gw = world.gpu, 0.5
    params = world.params[gw]
    scene = gpu.Scene(world.rgb, world.cmap, params)
    try:
        choice = scene.kernel_choice()
        for _ in range(8):
            for flags in MODES:
                scene.cell_map_sum(SUNS, 0.3 * gw, ambient=AMBIENT, **cc.flags_kw(flags))
        assert scene.kernel_choice() == choice
        cam = sc.camera(gpu, gw, 1, False, 0)
        want = oracle.render(oracle.make_cfg(cam, params, MAP_W, MAP_H), world.heights[gw], world.cmap)[0]
        assert scene.render(cam).tobytes() == want.tobytes() and scene.kernel_choice() == choice
        params2 = gpu.SceneParams.make(0.0, 11.0 * gw, grid_width=gw)
        heights2 = oracle.update_heightmap(world.rgb, params2)
        scene.update(params2)
        for sampling in SAMPLINGS:
            for flags in (0, cmr.WEIGHT | cmr.DIFFUSE):
                want2 = np.zeros((MAP_H, MAP_W), dtype=np.int64)
                for sun in SUNS:
                    b = cmr.replay(heights2, world.cmap, params2, sun, 0.3 * gw, flags=flags, sampling=sampling, ambient=AMBIENT,
                                   step_cap=cc.BASE_CAP)
                    want2 += b.astype(np.int64) if flags & cmr.WEIGHT else (b != cmr.HIT)
                assert not np.array_equal(want2, cs.summed(world, gw, sampling, SUNS, 0.3 * gw, flags))
                same_map(scene.cell_map_sum(SUNS, 0.3 * gw, sampling=sampling, ambient=AMBIENT, **cc.flags_kw(flags)), want2,
                         f"after the update, sampling {sampling} flags {flags}")
    finally:
        scene.close()


# ---- 11. CLI ----
def test_cli_sky_map_key(world, tmp_path):
    gpu, gw = world.gpu, 0.5
    sunp, skyp = str(tmp_path / "light.png"), str(tmp_path / "sky.png")
    cfgp, text, _ = gs.cli_config(gpu, world, tmp_path, gw)
    text += f"sun_dir 0.6 0.5 0.35\nshadow_ambient {AMBIENT}\nshadow_step_dist {0.3 * gw:.17g}\nsky_map {skyp}\n"
    runs = (("", (4, 16), 0, 0.0, 0, False),
            (f"sampling bilinear\nsky_map_rings 3 7\nshadow_max_steps 40\nsun_map_lift {0.25 * gw:.17g}\nsun_map {sunp}\n", (3, 7), 1, 0.25 * gw, 40, True),
            ("sky_map_rings 16 17\n", (4, 16), 0, 0.0, 0, False))
    for keys, (r, n), sampling, lift, limit, sun_too in runs:
        cfgp.write_text(text + keys)
        K = r * n
        counts = world.scenes[gw].cell_map_sum(gpu.sky_directions(r, n), 0.3 * gw, lift=lift, max_steps=limit, sampling=sampling)
        assert counts.max() <= K and len(np.unique(counts)) >= 8
        want = ((counts.astype(np.int64) * 255 + K // 2) // K).astype(np.uint8)
        res = gs.run_hmap(gpu, cfgp)
        assert f"sky_map {skyp}\n" in res.stdout and f"Saved sky map at {skyp}" in res.stdout and "Saved screenshot at" in res.stdout
        assert ("Saved sun map at" in res.stdout) == sun_too and os.path.exists(sunp) == sun_too
        assert ("sky_map_rings must give" in res.stderr) == (keys == "sky_map_rings 16 17\n")
        assert open(skyp, "rb").read() == gpu.png_encode(want), keys
        os.remove(skyp)
        if sun_too:
            assert res.stdout.index("Saved sun map at") < res.stdout.index("Saved sky map at")
            os.remove(sunp)
