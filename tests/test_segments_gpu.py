"""Segments and interior origins on the GPU (hmrm_trace_segments, hmrm_trace_segments_device, hmrm_render_interior;
include/hmrm.h).  Every record array and every frame is compared BYTEWISE with tests/segment_replay.py, which
tests/test_segments_cpu.py pins to ray_replay.replay (rules off), to the C oracle (interior rule) and to a scalar loop.
The map, grid widths and cameras are those of tests/test_trace_rays_gpu.py (tests/segment_cases.py): the smallest at
which every instantiation family runs."""
import numpy as np
import pytest

import gpu_support as gs
import ray_replay
import segment_cases as sc
import segment_replay as sr
from gpu_support import KERNEL_VARIANTS, SAMPLINGS, env, gpu, kernel_variant, same_frame, same_records
from segment_cases import BG, GRID_WIDTHS, GW_IDS, MAP_H, MAP_W

pytestmark = pytest.mark.gpu

MIXED_N = 3637  # not a multiple of 64
ODD_CAP = 4096


class World(gs.Scenes, gs.Maps):
    """Scenes per grid width; rays and replayed records per case, computed once and never modified."""

    def __init__(self, gpu, oracle):
        super().__init__(gpu, oracle)
        self._cache = {}

    def rays(self, gw, proj, inside, width=40, height=30):
        return sc.camera_rays(self.gpu, self.oracle, gw, proj, inside, width, height)

    def replay(self, key, rays, gw, sampling=0, **kw):
        """sr.replay(...) cached under `key` (read-only)."""
        if key not in self._cache:
            r = sr.replay(rays, self.heights[gw], self.cmap, self.params[gw], 0.2 * gw, bg=BG, sampling=sampling, **kw)
            r.setflags(write=False)
            self._cache[key] = r
        return self._cache[key]

    def interior_case(self, gw, proj, sampling, width=40, height=30):
        rays = self.rays(gw, proj, True, width, height)
        return rays, self.replay(("in", gw, proj, sampling, width, height), rays, gw, sampling, interior=True)

    def mixed(self, gw):
        """The rays of the three projections, outside and inside cameras, permuted with a fixed seed, truncated to MIXED_N."""
        key = ("mixed", gw)
        if key not in self._cache:
            rays = np.concatenate([self.rays(gw, proj, inside) for proj in (1, 2, 3) for inside in (False, True)])
            rays = np.ascontiguousarray(rays[np.random.RandomState(7).permutation(rays.shape[0])[:MIXED_N]])
            rays.setflags(write=False)
            self._cache[key] = rays
        return self._cache[key]

    def odd(self, gw):
        key = ("odd", gw)
        if key not in self._cache:
            rays = sc.odd_rays(gw, self.rays(gw, 1, False)[::8])
            rays.setflags(write=False)
            self._cache[key] = rays
        return self._cache[key]


world = gs.world_fixture(World)


# ---- 1. rules off ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_rules_off_equals_trace_rays(world, variant):
    with kernel_variant(variant):
        for gw in GRID_WIDTHS:
            rays = world.mixed(gw)
            assert rays.shape[0] == MIXED_N and MIXED_N % 64 != 0
            for sampling in SAMPLINGS:
                plain = world.scenes[gw].trace_rays(rays, 0.2 * gw, bg=BG, sampling=sampling)
                got, st = world.scenes[gw].trace_segments(rays, 0.2 * gw, bg=BG, sampling=sampling, stats=True)
                same_records(got, plain, f"rules off {variant} gw {gw} sampling {sampling}")
                assert (plain["status"] == ray_replay.HIT).sum() > 500 and st.capped == 0 and st.rays == MIXED_N
                zeros = np.zeros(MIXED_N, dtype=np.uint32)
                got0 = world.scenes[gw].trace_segments(rays, 0.2 * gw, bg=BG, sampling=sampling, per_ray_max_steps=zeros)
                assert got0.tobytes() == plain.tobytes(), "per-ray limits of 0 are no limits"


# ---- 2. interior camera rays ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=["persp", "sph", "ortho"])
def test_interior_camera_rays(world, proj, variant, gw):
    scene = world.scenes[gw]
    with kernel_variant(variant):
        for sampling in (SAMPLINGS if variant != "rec" else (0,)):
            rays, want = world.interior_case(gw, proj, sampling)
            hit = want["status"] == sr.HIT
            assert hit.sum() > (100 if proj == 3 else 750)
            got, st = scene.trace_segments(rays, 0.2 * gw, bg=BG, sampling=sampling, interior=True, stats=True)
            same_records(got, want, f"interior proj {proj} {variant} gw {gw} sampling {sampling}")
            assert (st.rays, st.steps, st.hits, st.capped) == (rays.shape[0], int(want["steps"].sum()), int(hit.sum()), 0)
            if proj != 3:  # the same rays without the rule: every one a miss, as in the reference
                off = scene.trace_segments(rays, 0.2 * gw, bg=BG, sampling=sampling)
                assert (off["status"] == sr.MISS).all() and (off["steps"] == 0).all()
                assert off["entry_d"].tobytes() == got["entry_d"].tobytes() and (got["entry_d"] < 0.0).all()


def test_orthographic_frame_mixes_both_origins(world):
    """The inside orthographic camera at grid width 0.5: 52 interior origins and 111 exterior rays that enter."""
    gw = 0.5
    rays, want = world.interior_case(gw, 3, 0)
    c0, c1 = ray_replay.box(world.params[gw], MAP_W, MAP_H)
    inside = sr.strictly_inside(rays[:, 0:3], c0, c1)
    enters_from_outside = ~inside & ~((want["entry_d"] == np.inf) | (want["entry_d"] < 0.0))
    assert (int(inside.sum()), int(enters_from_outside.sum())) == (52, 111)


# ---- 3. rays no camera makes ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_rays_no_camera_makes(world, variant, gw):
    rays = world.odd(gw)
    assert 550 <= rays.shape[0] <= 900
    c0, c1 = ray_replay.box(world.params[gw], MAP_W, MAP_H)
    assert sr.strictly_inside(rays[:, 0:3], c0, c1).sum() > 350
    samplings = SAMPLINGS if (gw == 0.5 and variant != "rec") else (0,)
    with kernel_variant(variant), env(HMRM_STEP_CAP=ODD_CAP):
        for sampling in samplings:
            want = world.replay(("odd", gw, sampling), rays, gw, sampling, interior=True, step_cap=ODD_CAP)
            capped = int((want["status"] == sr.CAPPED).sum())
            assert capped >= 12 and (want["status"] == sr.HIT).sum() > 150 and (want["status"] == sr.MISS).sum() > 100
            got, st = world.scenes[gw].trace_segments(rays, 0.2 * gw, bg=BG, sampling=sampling, interior=True, stats=True,
                                                      allow_capped=True)
            same_records(got, want, f"odd rays {variant} gw {gw} sampling {sampling}")
            assert st.capped == capped
            if sampling == 0:  # ... and the rule off: rays_no_camera's interior origins all miss, bytewise the plain entry
                off = world.replay(("odd off", gw), rays, gw, 0, step_cap=ODD_CAP)
                got_off = world.scenes[gw].trace_segments(rays, 0.2 * gw, bg=BG, allow_capped=True)
                same_records(got_off, off, f"odd rays, rule off {variant} gw {gw}")
                assert got_off.tobytes() == world.scenes[gw].trace_rays(rays, 0.2 * gw, bg=BG, allow_capped=True).tobytes()


# ---- 4. limits ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_limits(world, variant):
    gpu = world.gpu
    for gw in GRID_WIDTHS:
        scene = world.scenes[gw]
        rays = np.concatenate([world.rays(gw, 2, True), world.rays(gw, 1, False)[:37]])
        n = rays.shape[0]
        assert n % 64 != 0
        per = np.random.RandomState(3).choice([0, 0, 1, 2, 5, 17, 40, 300], size=n).astype(np.uint32)
        with kernel_variant(variant):
            for L in (1, 7, 40):
                want = world.replay(("lim", gw, L), rays, gw, interior=True, max_steps=L)
                got, st = scene.trace_segments(rays, 0.2 * gw, bg=BG, interior=True, max_steps=L, stats=True)  # (OK: no capped ray)
                same_records(got, want, f"uniform limit {L} {variant} gw {gw}")
                assert (want["status"] == sr.END).sum() > 300 and st.capped == 0
            want = world.replay(("lim per", gw), rays, gw, interior=True, per_ray=per)
            same_records(scene.trace_segments(rays, 0.2 * gw, bg=BG, interior=True, per_ray_max_steps=per), want,
                         f"per-ray limits {variant} gw {gw}")
            want = world.replay(("lim both", gw), rays, gw, interior=True, per_ray=per, max_steps=7)
            same_records(scene.trace_segments(rays, 0.2 * gw, bg=BG, interior=True, per_ray_max_steps=per, max_steps=7), want,
                         f"both limits {variant} gw {gw}")
            if gw == 0.5:
                # L >= the step cap: CAPPED as before, counted, HMRM_E_NOTERM; L = cap - 1: END, not counted
                with env(HMRM_STEP_CAP=50):
                    want = world.replay(("lim cap", gw), rays, gw, interior=True, max_steps=50, step_cap=50)
                    with pytest.raises(gpu.HmrmError) as e:
                        scene.trace_segments(rays, 0.2 * gw, bg=BG, interior=True, max_steps=50)
                    assert e.value.code == gpu.HMRM_E_NOTERM
                    got, st = scene.trace_segments(rays, 0.2 * gw, bg=BG, interior=True, max_steps=50, stats=True, allow_capped=True)
                    same_records(got, want, f"limit == cap {variant}")
                    assert st.capped == (want["status"] == sr.CAPPED).sum() > 100 and (want["status"] != sr.END).all()
                    want = world.replay(("lim cap-1", gw), rays, gw, interior=True, max_steps=49, step_cap=50)
                    got, st = scene.trace_segments(rays, 0.2 * gw, bg=BG, interior=True, max_steps=49, stats=True)
                    same_records(got, want, f"limit == cap - 1 {variant}")
                    assert st.capped == 0 and (want["status"] == sr.END).sum() > 100


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_vertical_rays_reach_the_cap(world, variant):
    gw = 0.5
    o = [10.25, -10.25, 3.9]
    rays = np.array([o + [0.0, 0.0, 1.0], o + [0.0, 0.0, 0.0], o + [0.0, 0.0, -1.0]])
    want = sr.replay(rays, world.heights[gw], world.cmap, world.params[gw], 0.1, bg=BG, interior=True, step_cap=500)
    assert want["status"].tolist() == [sr.CAPPED, sr.CAPPED, sr.HIT] and want["steps"].tolist() == [500, 500, 32]
    with kernel_variant(variant), env(HMRM_STEP_CAP=500):
        got, st = world.scenes[gw].trace_segments(rays, 0.1, bg=BG, interior=True, stats=True, allow_capped=True)
    same_records(got, want, f"vertical rays {variant}")
    assert st.capped == 2
    assert got["entry_d"].tobytes() == np.array([-3.9, -np.inf, -0.10000000000000009]).tobytes()


# ---- 5. device entry ----
@pytest.mark.parametrize("with_limits", [False, True])
def test_device_entry(world, with_limits):
    import torch
    gw = 0.5
    scene = world.scenes[gw]
    rays = np.concatenate([world.rays(gw, 2, True), world.rays(gw, 3, True)[:37]])
    n = rays.shape[0]
    per = np.random.RandomState(4).choice([0, 3, 9, 40], size=n).astype(np.uint32)
    want = world.replay(("dev", with_limits), rays, gw, interior=True, max_steps=25, per_ray=per if with_limits else None)
    assert (want["status"] == sr.END).sum() > 100 and (want["status"] == sr.HIT).sum() > 100
    d_rays = torch.from_numpy(rays.copy()).cuda()
    d_lim = torch.from_numpy(per.view(np.int32).copy()).cuda()
    d_buf = torch.full((256 + n * 56 + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    scene.trace_segments_device(d_rays.data_ptr(), n, d_buf.data_ptr() + 256, 0.2 * gw, bg=BG, interior=True, max_steps=25,
                                d_max_steps_ptr=d_lim.data_ptr() if with_limits else 0, stream=stream.cuda_stream)
    assert scene.take_capped(stream.cuda_stream) == 0  # (waits for the stream; END rays are not counted)
    out = d_buf.cpu().numpy()
    assert out[256:256 + n * 56].tobytes() == want.tobytes()
    assert (out[:256] == 0xA5).all() and (out[256 + n * 56:] == 0xA5).all(), "the canaries around the records"
    scene.trace_segments_device(0, 0, 0, 0.2 * gw, stream=stream.cuda_stream)  # n == 0 launches nothing
    assert scene.trace_segments(np.zeros((0, 6)), 0.2 * gw, interior=True).shape == (0,)


# ---- 6. a big batch: tile rows beyond 32768 go to blockIdx.z ----
def test_big_batch(world):
    gw = 0.5
    n = 32768 * 128 + 200
    assert n > 4194304
    base = np.concatenate([world.rays(gw, 2, True), world.rays(gw, 1, False)[:37]])
    m = base.shape[0]
    per = (np.arange(m) % 9 + 1).astype(np.uint32)  # short per-ray limits
    want = world.replay(("big", gw), base, gw, interior=True, per_ray=per)
    assert (want["status"] == sr.END).sum() > 300
    idx = np.arange(n) % m
    got = world.scenes[gw].trace_segments(base[idx], 0.2 * gw, bg=BG, interior=True, per_ray_max_steps=per[idx])
    assert got.shape == (n,) and np.array_equal(got.view(np.uint8), want[idx].view(np.uint8))


# ---- 7. render_interior ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_render_interior_is_the_replay(world, variant, gw):
    gpu = world.gpu
    scene = world.scenes[gw]
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            for sampling in SAMPLINGS:
                cam = sc.camera(gpu, gw, proj, True, sampling)
                _rays, want = world.interior_case(gw, proj, sampling)
                fb = scene.render_interior(cam)
                same_frame(fb, want["rgba"], f"render_interior proj {proj} {variant} gw {gw} sampling {sampling}")
                if sampling == 0 and proj != 3:
                    # hmrm_render of the same camera is still all sky and background: no ray enters (fails without the feature:
                    # the interior frame has hits where render has none)
                    plain = scene.render(cam)
                    off = world.replay(("in off", gw, proj), _rays, gw, 0)
                    same_frame(plain, off["rgba"], f"render, inside camera, proj {proj}")
                    hit = want["status"] == sr.HIT
                    assert (off["status"] == sr.HIT).sum() == 0 and hit.sum() > 750
                    # a hit on a texel with alpha 0 is painted with the background (hmap.cpp:1020), which is also the miss
                    # shade of a falling ray, so only part of the hits show: 439 (perspective) and 236 (spherical) in the replay
                    shows = (want["rgba"] != off["rgba"]).any(axis=1)
                    assert (shows <= hit).all() and shows.sum() == {1: 439, 2: 236}[proj]
                    assert (fb != plain).any(axis=2).sum() == shows.sum()
        # a camera outside the box: hmrm_render's frame, byte for byte
        for proj in (1, 2, 3):
            cam = sc.camera(gpu, gw, proj, False)
            assert scene.render_interior(cam).tobytes() == scene.render(cam).tobytes(), proj


@pytest.mark.parametrize("proj", [1, 2, 3], ids=["persp", "sph", "ortho"])
def test_render_interior_odd_frame(world, proj):
    """101 x 67: no multiple of the 16 x 8 tile, more than one workgroup each way."""
    gw = 0.5
    cam = sc.camera(world.gpu, gw, proj, True, width=101, height=67)
    _rays, want = world.interior_case(gw, proj, 0, 101, 67)
    assert (want["status"] == sr.HIT).sum() > (100 if proj == 3 else 4000)
    same_frame(world.scenes[gw].render_interior(cam), want["rgba"], f"101 x 67 proj {proj}")


def test_render_interior_reports_capped_rays(world):
    """Straight up from inside, orthographic: every origin is interior, no ray leaves the grid or hits."""
    gpu = world.gpu
    gw = 0.5
    cam = gpu.Camera.make(width=16, height=8, projection=3, hfov=gpu.degrees_to_rads(80), hang=0.0, vang=0.0,
                          pos=(10.25, -10.25, 3.9), ortho_width=0.25, step_dist=0.1, bg=BG)
    cfg = world.oracle.make_cfg(cam, world.params[gw], MAP_W, MAP_H)
    rays = ray_replay.camera_rays(world.oracle, cfg)
    want = sr.replay(rays, world.heights[gw], world.cmap, world.params[gw], 0.1, bg=BG, interior=True, step_cap=300)
    assert (want["status"] == sr.CAPPED).all() and (rays[:, 5] > 0.99).all()
    with env(HMRM_STEP_CAP=300):
        with pytest.raises(gpu.HmrmError) as e:
            world.scenes[gw].render_interior(cam)
        assert e.value.code == gpu.HMRM_E_NOTERM and "128 ray(s)" in str(e.value)
        same_frame(world.scenes[gw].render_interior(cam, allow_capped=True), want["rgba"], "capped interior frame")


# ---- 8. twin scenes: interior frames and segment batches are not frames of the probe ----
def test_interior_frames_and_segments_leave_the_probe_alone(world, oracle, capfd):
    """As tests/test_trace_rays_gpu.py::test_a_batch_is_not_a_frame: between ordinary frames of cameras that never repeat,
    interior frames and segment batches leave kernel_choice()'s sequence and the probe's frame (the sixth full frame) as on
    a twin scene that ran neither."""
    gpu = world.gpu
    gw = 0.5
    params, heights = world.params[gw], world.heights[gw]
    rays, want = world.interior_case(gw, 2, 0)
    icam = sc.camera(gpu, gw, 1, True, width=64, height=208)
    irays = world.rays(gw, 1, True, 64, 208)
    iwant = world.replay(("twin", gw), irays, gw, 0, interior=True)

    def cam_of(k):
        c = sc.camera(gpu, gw, 1, False, sampling=1, width=64, height=208)
        c.step_dist = 0.02 * gw
        c.pos[0] += 0.01 * k  # never repeats
        return c

    frames = []
    for k in range(8):
        c = cam_of(k)
        frames.append((c, oracle.render(oracle.make_cfg(c, params, MAP_W, MAP_H), heights, world.cmap)[0]))
    logs = {}
    with env(HMRM_ORDER_VERBOSE=1):
        for extra in (True, False):
            scene = gpu.Scene(world.rgb, world.cmap, params)
            capfd.readouterr()
            seq, probe_at = [], []

            def note(op):
                seq.append(scene.kernel_choice())
                if "hmrm probe:" in capfd.readouterr().err:
                    probe_at.append(op)

            def extras():
                if extra:
                    same_records(scene.trace_segments(rays, 0.2 * gw, bg=BG, interior=True, max_steps=40),
                                 world.replay(("twin seg", gw), rays, gw, 0, interior=True, max_steps=40), "segments between frames")
                    same_frame(scene.render_interior(icam), iwant["rgba"], "interior frame between frames")

            for k in range(8):
                cam, ofb = frames[k]
                assert np.array_equal(scene.render(cam), ofb), k
                note(k)
                if k in (0, 3, 5, 6):
                    extras()
            logs[extra] = (seq, probe_at)
            scene.close()
    assert logs[True] == logs[False], logs
    assert logs[False][1] == [6], "the sixth full frame is probed, the next launch reads the verdict"


# ---- 9. scene.update ----
def test_update_changes_the_thresholds(world, oracle):
    gpu = world.gpu
    gw = 0.5
    scene = gpu.Scene(world.rgb, world.cmap, world.params[gw])
    rays, want = world.interior_case(gw, 1, 0)
    cam = sc.camera(gpu, gw, 1, True)
    same_records(scene.trace_segments(rays, 0.2 * gw, bg=BG, interior=True), want, "before the update")
    same_frame(scene.render_interior(cam), want["rgba"], "before the update")
    params2 = gpu.SceneParams.make(0.0, 11.0 * gw, grid_width=gw)
    scene.update(params2)
    heights2 = oracle.update_heightmap(world.rgb, params2)
    want2 = sr.replay(rays, heights2, world.cmap, params2, 0.2 * gw, bg=BG, interior=True)
    assert want2.tobytes() != want.tobytes()
    for variant in KERNEL_VARIANTS:
        with kernel_variant(variant):
            same_records(scene.trace_segments(rays, 0.2 * gw, bg=BG, interior=True), want2, f"after the update, {variant}")
            same_frame(scene.render_interior(cam), want2["rgba"], f"after the update, {variant}")
    scene.close()


# ---- 10. CLI ----
def test_cli_interior_key(world, tmp_path):
    gpu = world.gpu
    gw = 0.5
    cfgp, text, outp = gs.cli_config(gpu, world, tmp_path, gw, True, "interior on\n", proj=2)
    cfg = gpu.Config().consume_file(str(cfgp))
    assert cfg.interior() is True
    scene = cfg.create_scene()
    want = scene.render_interior(cfg.camera())
    plain = scene.render(cfg.camera())
    scene.close()
    cfg.close()
    _rays, replayed = world.interior_case(gw, 2, 0)
    same_frame(want, replayed["rgba"], "the config's camera is the tests' spherical inside camera")
    r = gs.run_hmap(gpu, cfgp)
    assert "interior on\n" in r.stdout and "under the interior rule" in r.stdout
    assert open(outp, "rb").read() == gpu.png_encode(want) != gpu.png_encode(plain)
    # ... ignored, with a warning, together with antialias > 1
    cfgp.write_text(text + "interior on\nantialias 2\n")
    r = gs.run_hmap(gpu, cfgp)
    assert "WARNING: interior is ignored with antialias > 1" in r.stderr
