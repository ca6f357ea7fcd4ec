"""Cell maps on the GPU (hmrm_cell_map; include/hmrm.h).  Every map is compared BYTEWISE with tests/cell_map_replay.py, the
definition in numpy, whose content tests/test_cell_map_cpu.py pins; one test pins the kernels to hmrm_trace_segments on the same
GPU without the replay's march.  Maps, grid widths, suns and observer points are those of tests/cell_map_cases.py: step_dist
0.3 grid widths in direction mode, 1/64 with max_steps 64 in point mode, ambient 128."""
import functools
import os

import numpy as np
import pytest

import cell_map_cases as cc
import cell_map_replay as cmr
import gpu_support as gs
import segment_cases as sc
from cell_map_cases import AMBIENT, GRID_WIDTHS, GW_IDS, MAP_H, MAP_W, MODES, SETTINGS, SUNS
from gpu_support import KERNEL_VARIANTS, SAMPLINGS, env, gpu, kernel_variant

pytestmark = pytest.mark.gpu

RECTS = ((3, 5, 29, 13), (63, 47, 1, 1), (0, 0, 64, 1), (56, 40, 8, 8))
SMALL_CAP = 300
samplings_of = functools.partial(gs.samplings_of, nearest_only=("rec", "simple"))  # (the literal loop too: nearest sampling only)
same_map = functools.partial(gs.same_cells, dtype=np.uint8)


class World(gs.Scenes, cc.Replays):
    def __init__(self, gpu, oracle):
        super().__init__(gpu, oracle)
        self.scenes_b = {gw: gpu.Scene(self.rgb_b, self.cmap_b, self.params[gw]) for gw in (0.5, 0.05)}

    def close(self):
        super().close()
        for s in self.scenes_b.values():
            s.close()


world = gs.world_fixture(World)


# ---- 1. the base sweep on map A ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_cell_map_is_the_replay(world, variant, gw):
    """3 suns x {status, WEIGHT, WEIGHT + DIFFUSE, WEIGHT + DIFFUSE + NO_SHADOWS} x {lift 0 without a limit, lift 0.25 gw with
    max_steps 40} per sampling mode."""
    scene = world.scenes[gw]
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            for sun in SUNS:
                for lift_gw, limit in SETTINGS:
                    for flags in MODES:
                        want = world.bytes(gw, sampling, sun, 0.3 * gw, flags, lift_gw * gw, limit)
                        got = scene.cell_map(sun, 0.3 * gw, lift=lift_gw * gw, max_steps=limit, sampling=sampling, ambient=AMBIENT,
                                             **cc.flags_kw(flags))
                        same_map(got, want, f"{variant} gw {gw} sampling {sampling} sun {sun} lift {lift_gw} limit {limit} flags {flags}")


# ---- 2. point mode: a viewshed from above the box and from inside it ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_point_mode(world, variant):
    with kernel_variant(variant):
        for gw in GRID_WIDTHS:
            cases = [(cc.point_above(gw), 0.0), (cc.point_above(gw), 0.25 * gw), (cc.point_inside(gw), 0.25 * gw)]
            for sampling in samplings_of(variant):
                for target, lift in cases:
                    for flags in (cmr.TOWARDS_POINT, cmr.TOWARDS_POINT | cmr.WEIGHT | cmr.DIFFUSE):
                        want = world.bytes(gw, sampling, target, cc.POINT_STEP, flags, lift, cc.POINT_STEPS)
                        got = world.scenes[gw].cell_map(target, cc.POINT_STEP, lift=lift, max_steps=cc.POINT_STEPS, sampling=sampling,
                                                        ambient=AMBIENT, **cc.flags_kw(flags))
                        same_map(got, want, f"point {target} lift {lift} {variant} gw {gw} sampling {sampling} flags {flags}")


# ---- 3. geometry: partial tiles, rects, strides ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_map_b_whole(world, variant):
    """37 x 21: partial tiles on both sides."""
    with kernel_variant(variant):
        for gw in (0.5, 0.05):
            for sampling in samplings_of(variant):
                for flags in MODES:
                    want = world.bytes(gw, sampling, SUNS[1], 0.3 * gw, flags, 0.25 * gw, 40, which="B")
                    got = world.scenes_b[gw].cell_map(SUNS[1], 0.3 * gw, lift=0.25 * gw, max_steps=40, sampling=sampling, ambient=AMBIENT,
                                                      **cc.flags_kw(flags))
                    same_map(got, want, f"map B {variant} gw {gw} sampling {sampling} flags {flags}")


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_rects_and_strides(world, variant):
    """Each rect is the same slice of the whole map's replay, written into rows 5 bytes wider than the rect; the bytes between
    the rows stay as they were."""
    gw = 0.5
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            for flags in (0, cmr.WEIGHT | cmr.DIFFUSE):
                whole = world.bytes(gw, sampling, SUNS[0], 0.3 * gw, flags)
                for x0, y0, w, h in RECTS:
                    out = world.scenes[gw].cell_map(SUNS[0], 0.3 * gw, sampling=sampling, ambient=AMBIENT, rect=(x0, y0, w, h),
                                                    stride_bytes=w + 5, **cc.flags_kw(flags))
                    assert out.shape == (h, w + 5)
                    same_map(np.ascontiguousarray(out[:, :w]), whole[y0:y0 + h, x0:x0 + w], f"rect {(x0, y0, w, h)} {variant} sampling {sampling} flags {flags}")
                    assert (out[:, w:] == 0xA5).all(), f"canaries of rect {(x0, y0, w, h)}"


def test_rect_and_stride_refusals(world):
    gpu, scene = world.gpu, world.scenes[0.5]
    for rect in ((0, 0, 0, 4), (0, 0, 4, 0), (-1, 0, 4, 4), (0, -1, 4, 4), (61, 0, 4, 4), (0, 45, 4, 4), (0, 0, -3, 4), (0, 0, 65, 1),
                 (2147483647, 0, 2, 1)):
        with pytest.raises(gpu.HmrmError) as e:
            scene.cell_map(SUNS[0], 0.15, rect=rect, stride_bytes=80)
        assert e.value.code == gpu.HMRM_E_ARG and "rect" in str(e.value), rect
    with pytest.raises(gpu.HmrmError) as e:
        scene.cell_map(SUNS[0], 0.15, rect=(0, 0, 8, 2), stride_bytes=7)
    assert e.value.code == gpu.HMRM_E_ARG and "stride_bytes" in str(e.value)


# ---- 4. without the replay: the status bytes are hmrm_trace_segments' on the same GPU ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_status_is_trace_segments_of_numpy_rays(world, variant):
    gw = 0.5
    scene, params, heights = world.scenes_b[gw], world.params[gw], world.heights_b[gw]
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            for point, target, step, lift, limit in ((False, SUNS[2], 0.3 * gw, 0.0, 0), (False, SUNS[0], 0.3 * gw, 0.25 * gw, 40),
                                                     (True, cc.point_above(gw), cc.POINT_STEP, 0.25 * gw, cc.POINT_STEPS)):
                rays, _cx, _cy = cmr.cell_rays(heights, params, sampling, target, lift, point)
                rec = scene.trace_segments(rays, step, sampling=sampling, interior=True, max_steps=limit)
                want = rec["status"].astype(np.uint8).reshape(cc.B_H, cc.B_W)
                assert (want == cmr.HIT).sum() >= 50 and (want != cmr.HIT).sum() >= 50
                got = scene.cell_map(target, step, lift=lift, max_steps=limit, point=point, sampling=sampling)
                same_map(got, want, f"trace_segments {variant} sampling {sampling} point {point}")


# ---- 5. the device entry ----
def test_device_entry(world):
    import torch
    gw = 0.5
    scene = world.scenes[gw]
    flags = cmr.WEIGHT | cmr.DIFFUSE
    stride = MAP_W + 11
    host = scene.cell_map(SUNS[0], 0.3 * gw, lift=0.25 * gw, max_steps=40, sampling=1, ambient=AMBIENT, **cc.flags_kw(flags))
    same_map(host, world.bytes(gw, 1, SUNS[0], 0.3 * gw, flags, 0.25 * gw, 40), "host entry")
    d_buf = torch.full((256 + 1 + MAP_H * stride + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    scene.cell_map_device(d_buf.data_ptr() + 257, stride, SUNS[0], 0.3 * gw, lift=0.25 * gw, max_steps=40, sampling=1, ambient=AMBIENT,
                          stream=stream.cuda_stream, **cc.flags_kw(flags))  # (an odd address: only byte alignment is asked)
    assert scene.take_capped(stream.cuda_stream) == 0  # (waits for the stream; END rays are not counted)
    out = d_buf.cpu().numpy()
    rows = out[257:257 + MAP_H * stride].reshape(MAP_H, stride)
    same_map(np.ascontiguousarray(rows[:, :MAP_W]), host, "device entry")
    assert (rows[:, MAP_W:] == 0xA5).all() and (out[:257] == 0xA5).all() and (out[257 + MAP_H * stride:] == 0xA5).all(), "the canaries"


# ---- 6. caps, ends, and targets nothing special-cases ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_caps_and_ends(world, variant):
    """Straight up at HMRM_STEP_CAP = 300: the interior rays never leave the grid -- HMRM_E_NOTERM, the replay's count, the replay's
    bytes; with max_steps = 50 the same rays END and the call returns HMRM_OK."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes_b[gw]
    up = (0.0, 0.0, 1.0)
    with kernel_variant(variant), env(HMRM_STEP_CAP=SMALL_CAP):
        for sampling in samplings_of(variant):
            want = world.status(gw, sampling, up, 0.3 * gw, 0.25 * gw, 0, False, SMALL_CAP, "B")
            capped = int((want == cmr.CAPPED).sum())
            assert capped >= 500
            with pytest.raises(gpu.HmrmError) as e:
                scene.cell_map(up, 0.3 * gw, lift=0.25 * gw, sampling=sampling)
            assert e.value.code == gpu.HMRM_E_NOTERM and f"{capped} ray(s)" in str(e.value), (capped, str(e.value))
            same_map(scene.cell_map(up, 0.3 * gw, lift=0.25 * gw, sampling=sampling, allow_capped=True), want, f"capped {variant} sampling {sampling}")
            ended = world.status(gw, sampling, up, 0.3 * gw, 0.25 * gw, 50, False, SMALL_CAP, "B")
            assert int((ended == cmr.END).sum()) == capped and not (ended == cmr.CAPPED).any()
            same_map(scene.cell_map(up, 0.3 * gw, lift=0.25 * gw, max_steps=50, sampling=sampling), ended, f"END {variant} sampling {sampling}")


ODD_TARGETS = [(np.nan, 0.5, 0.35), (0.6, np.inf, 0.35), (0.0, 0.0, 0.0)]


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_odd_targets(world, variant):
    """A NaN component, an infinite component and the zero direction (which never moves: under the small cap), status and
    WEIGHT + DIFFUSE: the same arithmetic, the replay's bytes."""
    gw = 0.5
    scene = world.scenes_b[gw]
    with kernel_variant(variant), env(HMRM_STEP_CAP=SMALL_CAP):
        for k, target in enumerate(ODD_TARGETS):
            sampling = samplings_of(variant)[k % len(samplings_of(variant))]
            for flags in (0, cmr.WEIGHT | cmr.DIFFUSE):
                want = world.bytes(gw, sampling, target, 0.3 * gw, flags, 0.25 * gw, 0, step_cap=SMALL_CAP, which="B")
                got = scene.cell_map(target, 0.3 * gw, lift=0.25 * gw, sampling=sampling, ambient=AMBIENT, allow_capped=True, **cc.flags_kw(flags))
                same_map(got, want, f"target {target} {variant} sampling {sampling} flags {flags}")
            if not any(target):
                assert (world.status(gw, sampling, target, 0.3 * gw, 0.25 * gw, 0, False, SMALL_CAP, "B") == cmr.CAPPED).sum() >= 500


# ---- 7. a cell map is not a frame ----
def test_not_a_frame(world, oracle):
    gpu, gw = world.gpu, 0.5
    params = world.params[gw]
    scene = gpu.Scene(world.rgb, world.cmap, params)
    try:
        choice = scene.kernel_choice()
        for _ in range(8):
            for flags in MODES:
                scene.cell_map(SUNS[0], 0.3 * gw, ambient=AMBIENT, **cc.flags_kw(flags))
        assert scene.kernel_choice() == choice
        cam = sc.camera(gpu, gw, 1, False, 0)
        want = oracle.render(oracle.make_cfg(cam, params, MAP_W, MAP_H), world.heights[gw], world.cmap)[0]
        assert scene.render(cam).tobytes() == want.tobytes() and scene.kernel_choice() == choice
        params2 = gpu.SceneParams.make(0.0, 11.0 * gw, grid_width=gw)
        heights2 = oracle.update_heightmap(world.rgb, params2)
        scene.update(params2)
        for sampling in SAMPLINGS:
            for flags in (0, cmr.WEIGHT | cmr.DIFFUSE):
                want2 = cmr.replay(heights2, world.cmap, params2, SUNS[0], 0.3 * gw, flags=flags, sampling=sampling, ambient=AMBIENT,
                                   step_cap=cc.BASE_CAP)
                assert want2.tobytes() != world.bytes(gw, sampling, SUNS[0], 0.3 * gw, flags).tobytes()
                same_map(scene.cell_map(SUNS[0], 0.3 * gw, sampling=sampling, ambient=AMBIENT, **cc.flags_kw(flags)), want2,
                         f"after the update, sampling {sampling} flags {flags}")
    finally:
        scene.close()


# ---- 8. CLI ----
def test_cli_sun_map_key(world, tmp_path):
    gpu, gw = world.gpu, 0.5
    mapp = str(tmp_path / "light.png")
    cfgp, text, _ = gs.cli_config(gpu, world, tmp_path, gw)
    text += f"sun_dir 0.6 0.5 0.35\nshadow_ambient {AMBIENT}\nshadow_step_dist {0.3 * gw:.17g}\nsun_map {mapp}\n"
    runs = (("", cmr.WEIGHT, 0.0), ("shading on\n", cmr.WEIGHT | cmr.DIFFUSE | cmr.NO_SHADOWS, 0.0),
            (f"shading on\nshadows on\nsampling bilinear\nsun_map_lift {0.25 * gw:.17g}\n", cmr.WEIGHT | cmr.DIFFUSE, 0.25 * gw))
    for keys, flags, lift in runs:
        cfgp.write_text(text + keys)
        sampling = 1 if "bilinear" in keys else 0
        want = world.bytes(gw, sampling, SUNS[0], 0.3 * gw, flags, lift)
        r = gs.run_hmap(gpu, cfgp)
        assert f"sun_map {mapp}\n" in r.stdout and f"Saved sun map at {mapp}" in r.stdout and "Saved screenshot at" in r.stdout
        assert open(mapp, "rb").read() == gpu.png_encode(want), keys
        os.remove(mapp)
