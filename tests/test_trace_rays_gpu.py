"""Ray queries on the GPU (hmrm_trace_rays, hmrm_trace_rays_device, hmrm_pick; include/hmrm.h): caller-supplied rays
through the march kernels, every record compared BYTEWISE -- against the C oracle for camera rays (rgba, steps, entry_d
from oracle.render(per_pixel=True), point and cell from steps - 1 sequential adds), against tests/ray_replay.py (pinned
to the oracle by tests/test_trace_rays_cpu.py) for rays no camera makes.  One 64 x 48 map (not square, not a multiple of
16, alpha-0 texels, zero-height cells) at grid widths 1.0, 0.5 and 0.05: one kernel instantiation family each."""
import numpy as np
import pytest

import gpu_support as gs
import ray_replay
import segment_cases as sc
from gpu_support import KERNEL_VARIANTS, PROJ_IDS, SAMPLINGS, env, gpu, kernel_variant, same_records
from segment_cases import BG, GRID_WIDTHS, GW_IDS, MAP_H, MAP_W

pytestmark = pytest.mark.gpu

MIXED_N = 3637  # not a multiple of 64


class World(gs.Scenes, gs.Maps):
    """The scenes (one per grid width), and the oracle's rays and expected records per (grid width, projection, camera,
    sampling), computed once and never modified."""

    def __init__(self, gpu, oracle):
        super().__init__(gpu, oracle)
        self._cache = {}

    def camera(self, gw, proj, inside, sampling=0, width=40, height=30):
        """segment_cases' camera, but the inside orthographic plane is 0.02 cells wide, not 3."""
        cam = sc.camera(self.gpu, gw, proj, inside, sampling, width, height)
        if inside:
            cam.ortho_width = 0.02 * gw
        return cam

    def camera_case(self, gw, proj, inside, sampling):
        """-> (rays n x 6, expected records, camera)"""
        key = (gw, proj, inside, sampling)
        if key not in self._cache:
            cam = self.camera(gw, proj, inside, sampling)
            cfg = self.oracle.make_cfg(cam, self.params[gw], MAP_W, MAP_H)
            rays = ray_replay.camera_rays(self.oracle, cfg)
            want = ray_replay.expected_from_oracle(self.oracle, cfg, self.heights[gw], self.cmap, rays, self.params[gw])
            rays.setflags(write=False)
            want.setflags(write=False)
            self._cache[key] = (rays, want, cam)
        return self._cache[key]

    def mixed(self, gw, sampling):
        """The rays of the three projections, outside and inside cameras, in one batch: permuted with a fixed seed (different
        origins and directions inside one wave) and truncated to MIXED_N."""
        key = ("mixed", gw, sampling)
        if key not in self._cache:
            parts = [self.camera_case(gw, proj, inside, sampling) for proj in (1, 2, 3) for inside in (False, True)]
            rays = np.concatenate([p[0] for p in parts])
            want = np.concatenate([p[1] for p in parts])
            perm = np.random.RandomState(7).permutation(rays.shape[0])[:MIXED_N]
            rays, want = np.ascontiguousarray(rays[perm]), np.ascontiguousarray(want[perm])
            rays.setflags(write=False)
            want.setflags(write=False)
            self._cache[key] = (rays, want)
        return self._cache[key]


world = gs.world_fixture(World)


# ---- 1. camera-ray parity with the oracle ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_camera_rays_equal_the_oracle(world, proj, variant, gw):
    scene = world.scenes[gw]
    with kernel_variant(variant):
        for sampling in SAMPLINGS:
            for inside in (False, True):
                rays, want, cam = world.camera_case(gw, proj, inside, sampling)
                hit = want["status"] == ray_replay.HIT
                if inside:  # d < 0: intersection() reports a miss for every ray (AABB.cpp:38-40)
                    assert not hit.any() and (want["entry_d"] < 0.0).all() and (want["steps"] == 0).all()
                else:  # terrain, sky and below-horizon background (an orthographic camera's rays all look down: no sky)
                    assert hit.sum() > 100 and (~hit & (rays[:, 5] <= 0.0)).sum() > 50
                    assert proj == 3 or (~hit & (rays[:, 5] > 0.0)).sum() > 50
                got, st = scene.trace_rays(rays, cam.step_dist, bg=BG, sampling=sampling, stats=True)
                same_records(got, want, f"proj {proj} {variant} gw {gw} sampling {sampling} inside {inside}")
                assert (st.rays, st.steps, st.hits, st.capped) == (rays.shape[0], int(want["steps"].sum()), int(hit.sum()), 0)


# ---- 2. mixed batch ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_mixed_batch(world, variant):
    with kernel_variant(variant):
        for gw in GRID_WIDTHS:
            for sampling in SAMPLINGS:
                rays, want = world.mixed(gw, sampling)
                assert rays.shape[0] == MIXED_N and MIXED_N % 64 != 0
                got = world.scenes[gw].trace_rays(rays, 0.2 * gw, bg=BG, sampling=sampling)
                same_records(got, want, f"mixed {variant} gw {gw} sampling {sampling}")
                # the structured-array form of the same batch
                if sampling == 0:
                    got2 = world.scenes[gw].trace_rays(world.gpu.as_rays(rays), 0.2 * gw, bg=BG)
                    assert got2.tobytes() == got.tobytes()


# ---- 3. rays no camera makes ----
def odd_rays(world, gw):
    """About 500 rays: scaled directions, exact axis-parallel rays, starts on a box face, NaN / inf components, rays along box
    edges, zero directions, random unnormalised rays.  None runs forever: every ray whose x, y never move points down."""
    base = world.mixed(gw, 0)[0]
    W, H, top = MAP_W * gw, MAP_H * gw, 8.0 * gw
    out = []
    a = base[:150].copy()
    a[:, 3:6] *= 3.7
    out.append(a)
    b = base[150:270].copy()
    b[:, 3:6] *= 2.0 ** -3
    out.append(b)
    # straight down from above: cell centres, exact cell boundaries, the map's edges
    for k in range(40):
        x = (k * 1.5 + (0.5 if k % 2 else 0.0)) * gw
        y = -((k * 1.1) % MAP_H + (0.5 if k % 3 else 0.0)) * gw
        out.append([[x, y, top + 3.0 * gw, 0.0, 0.0, -1.0]])
    out.append([[0.0, 0.0, top + gw, 0.0, 0.0, -1.0], [W, -H, top + gw, 0.0, 0.0, -1.0], [W, 0.0, top + gw, 0.0, 0.0, -1.0]])
    # along +x / -x / -y / +y through the box at mid height (dz == 0 exactly; x / 0 in AABB.cpp:62-63)
    for k in range(20):
        y = -(k * 2.3 + 0.25) * gw
        out.append([[-2.0 * gw, y, 4.0 * gw, 1.0, 0.0, 0.0], [W + 2.0 * gw, y, 3.0 * gw, -1.0, 0.0, 0.0]])
        x = (k * 3.1 + 0.75) * gw
        out.append([[x, 2.0 * gw, 2.5 * gw, 0.0, -1.0, 0.0], [x, -H - 2.0 * gw, 5.0 * gw, 0.0, 1.0, 0.0]])
    # starting exactly on a box face
    for k in range(10):
        out.append([[(5.0 + 4 * k) * gw, -(3.0 + 3 * k) * gw, top, 0.3, -0.2, -1.0],
                    [0.0, -(2.5 + 4 * k) * gw, 6.0 * gw, 1.0, -0.1, -0.2],
                    [(7.0 + 5 * k) * gw, 0.0, 7.0 * gw, 0.1, -1.0, -0.3],
                    [(7.0 + 5 * k) * gw, -(3.0 + k) * gw, 0.0, 0.1, -0.2, 1.0]])
    # along box edges (two coordinates exactly on faces) and through corners
    out.append([[-gw, 0.0, top, 1.0, 0.0, 0.0], [-gw, -H, top, 1.0, 0.0, 0.0], [-gw, 0.0, 0.0, 1.0, 0.0, 0.0],
                [0.0, gw, top, 0.0, -1.0, 0.0], [W, gw, top, 0.0, -1.0, 0.0], [0.0, 0.0, top + gw, 0.0, 0.0, -1.0],
                [-gw, gw, top + gw, 1.0, -1.0, -1.0], [W + gw, -H - gw, top + gw, -1.0, 1.0, -1.0]])
    # a NaN or an infinity in every component of pos and dir, on rays that otherwise hit
    seed_rays = base[np.nonzero(world.mixed(gw, 0)[1]["status"] == ray_replay.HIT)[0][:3]]
    for r in seed_rays:
        for comp in range(6):
            for v in (np.nan, np.inf, -np.inf):
                q = r.copy()
                q[comp] = v
                out.append([q])
    # zero directions, outside and inside the box
    out.append([[-gw, gw, 3.0 * gw, 0.0, 0.0, 0.0], [10.0 * gw, -10.0 * gw, 3.0 * gw, 0.0, 0.0, 0.0], [10.0 * gw, -10.0 * gw, top + gw, 0.0, 0.0, 0.0]])
    # random origins around the box, random unnormalised directions that move sideways
    rng = np.random.RandomState(11)
    for _ in range(130):
        o = np.array([rng.uniform(-0.5, 1.5) * W, -rng.uniform(-0.5, 1.5) * H, rng.uniform(-0.5, 2.5) * top])
        d = rng.uniform(-1.0, 1.0, 3) * rng.choice([0.01, 1.0, 40.0])
        d[rng.randint(2)] += np.copysign(0.3, d[0]) * max(1.0, np.abs(d).max())
        out.append([np.concatenate([o, d])])
    rays = np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, 6) for x in out])
    sideways = (rays[:, 3] != 0.0) | (rays[:, 4] != 0.0)
    assert (sideways | (rays[:, 5] <= 0.0) | ~np.isfinite(rays).all(axis=1)).all()
    return rays


@pytest.fixture(scope="module")
def odd(world, oracle):
    out = {}
    for gw in GRID_WIDTHS:
        rays = odd_rays(world, gw)
        out[gw] = (rays, {s: ray_replay.replay(rays, world.heights[gw], world.cmap, world.params[gw], 0.2 * gw, bg=BG, sampling=s)
                          for s in SAMPLINGS})
    return out


@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_rays_no_camera_makes(world, odd, variant, gw):
    rays, want = odd[gw]
    assert 450 <= rays.shape[0] <= 700
    hit = want[0]["status"] == ray_replay.HIT
    assert 100 < hit.sum() < rays.shape[0] - 100 and want[0]["steps"].max() < 1 << 20
    with kernel_variant(variant):
        for sampling in SAMPLINGS:
            got = world.scenes[gw].trace_rays(rays, 0.2 * gw, bg=BG, sampling=sampling)
            same_records(got, want[sampling], f"odd rays {variant} gw {gw} sampling {sampling}")


# ---- 4. step cap ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_step_cap(world, variant):
    gw = 1.0
    scene = world.scenes[gw]
    rays, want = world.mixed(gw, 0)
    rays, want = rays[:200].copy(), want[:200].copy()
    assert want["steps"].max() < 1000 and world.heights[gw][6, 42] == 0.0
    # from below the box, straight up, under a zero-height cell: it never leaves its cell and never hits
    rays[100] = [42.5, -6.5, -3.0, 0.0, 0.0, 1.0]
    with kernel_variant(variant):
        free = scene.trace_rays(np.delete(rays, 100, axis=0), 0.2, bg=BG)
        same_records(free, np.delete(want, 100), f"{variant}: the ordinary rays")
        with env(HMRM_STEP_CAP=1000):
            with pytest.raises(world.gpu.HmrmError) as e:
                scene.trace_rays(rays, 0.2, bg=BG)
            assert e.value.code == world.gpu.HMRM_E_NOTERM
            got, st = scene.trace_rays(rays, 0.2, bg=BG, stats=True, allow_capped=True)
    assert st.capped == 1 and st.rays == 200
    r = got[100]
    assert r["status"] == ray_replay.CAPPED and r["steps"] == 1000 and (r["cell_x"], r["cell_y"]) == (-1, -1)
    assert (r["point"] == 0.0).all() and r["entry_d"] == 3.0
    assert r["rgba"].tolist() == [232, 255, 255, 255]  # the sky for dir.z = 1 over this background (hmap.cpp:1044-1051)
    assert np.delete(got, 100).tobytes() == free.tobytes()
    # ... and the same record from the replay under the same cap
    cap = ray_replay.replay(rays[100:101], world.heights[gw], world.cmap, world.params[gw], 0.2, bg=BG, step_cap=1000)
    assert got[100:101].tobytes() == cap.tobytes()


# ---- 5. device entry ----
@pytest.mark.parametrize("n", [MIXED_N, 1])
def test_device_entry(world, n):
    import torch
    gw = 0.5
    scene = world.scenes[gw]
    rays, want = world.mixed(gw, 0)
    rays, want = rays[:n], want[:n]
    host = scene.trace_rays(rays, 0.2 * gw, bg=BG)
    same_records(host, want, "host entry")
    d_rays = torch.from_numpy(rays.copy()).cuda()
    d_hits = torch.full((n * 56 + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    scene.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), 0.2 * gw, bg=BG, stream=stream.cuda_stream)
    assert scene.take_capped(stream.cuda_stream) == 0  # (waits for the stream)
    out = d_hits.cpu().numpy()
    assert out[:n * 56].tobytes() == host.tobytes()
    assert (out[n * 56:] == 0xA5).all(), "the canary behind the records"
    # n == 0 launches nothing and touches nothing
    scene.trace_rays_device(0, 0, 0, 0.2 * gw, stream=stream.cuda_stream)
    assert scene.trace_rays(np.zeros((0, 6)), 0.2 * gw).shape == (0,)


# ---- 6. a big batch: tile rows beyond 32768 go to blockIdx.z ----
def test_big_batch(world):
    # (0.3 s on an MI355X box: no budget guard needed)
    gw = 0.5
    n = 32768 * 128 + 200
    rays, want = world.mixed(gw, 0)
    idx = np.arange(n) % MIXED_N
    got = world.scenes[gw].trace_rays(rays[idx], 0.2 * gw, bg=BG)
    exp = want[idx]
    assert got.shape == (n,) and np.array_equal(got.view(np.uint8), exp.view(np.uint8))


# ---- 7. a batch is not a frame ----
def test_a_batch_is_not_a_frame(world, oracle, capfd):
    """Traces between frames leave the scene's probe ("sixth full frame"), its verdict and every frame as on a twin scene
    that traced nothing.  The frames are bilinear, tiny-step and skim the terrain: the probe's other kernel then is the plain
    groups without any leap, tens of times slower here, so the verdict does not hang on timing noise; WHEN the probe ran
    shows in the library's own report (HMRM_ORDER_VERBOSE) at the launch that reads the verdict."""
    gpu = world.gpu
    gw = 0.5
    params = world.params[gw]
    heights = world.heights[gw]
    rays, want = world.mixed(gw, 0)

    def cam_of(k):
        c = world.camera(gw, 1, False, sampling=1, width=64, height=208)
        c.step_dist = 0.02 * gw
        c.pos[0] += 0.01 * k  # never repeats
        return c

    def frame_of(k):
        c = cam_of(k)
        return c, oracle.render(oracle.make_cfg(c, params, MAP_W, MAP_H), heights, world.cmap)[0]

    frames = [frame_of(k) for k in range(8)]
    logs = {}
    with env(HMRM_ORDER_VERBOSE=1):
        for traced in (True, False):
            scene = gpu.Scene(world.rgb, world.cmap, params)
            capfd.readouterr()
            seq, probe_at = [], []

            def note(op):
                seq.append(scene.kernel_choice())
                if "hmrm probe:" in capfd.readouterr().err:
                    probe_at.append(op)

            def trace():
                if traced:
                    same_records(scene.trace_rays(rays, 0.2 * gw, bg=BG), want, "trace between frames")

            cam, ofb = frames[0]
            assert np.array_equal(scene.render(cam), ofb)
            note(0)
            trace()
            for k in range(1, 6):
                cam, ofb = frames[k]
                assert np.array_equal(scene.render(cam), ofb), k
                note(k)
            cam, ofb = frames[6]
            t = scene.render_begin(cam)
            trace()
            assert np.array_equal(scene.render_wait(t, (cam.height, cam.width)), ofb)
            scene.render_release(t)
            note(6)
            trace()
            cam, ofb = frames[7]
            assert np.array_equal(scene.render(cam), ofb)
            note(7)
            logs[traced] = (seq, probe_at)
            scene.close()
    assert logs[True] == logs[False], logs
    assert logs[False][1] == [6], "the sixth full frame is probed, the next launch reads the verdict"
    assert all(c in (0, 1, 3) for c in logs[False][0])


# ---- 8. scene.update ----
def test_update_changes_the_thresholds(world, oracle):
    gpu = world.gpu
    gw = 0.5
    scene = gpu.Scene(world.rgb, world.cmap, world.params[gw])
    rays, want, cam = world.camera_case(gw, 1, False, 0)
    same_records(scene.trace_rays(rays, cam.step_dist, bg=BG), want, "before the update")
    params2 = gpu.SceneParams.make(0.0, 11.0 * gw, grid_width=gw)
    scene.update(params2)
    heights2 = oracle.update_heightmap(world.rgb, params2)
    cfg2 = oracle.make_cfg(cam, params2, MAP_W, MAP_H)
    rays2 = ray_replay.camera_rays(oracle, cfg2)
    assert rays2.tobytes() == rays.tobytes()  # (the camera did not move)
    want2 = ray_replay.expected_from_oracle(oracle, cfg2, heights2, world.cmap, rays2, params2)
    assert want2.tobytes() != want.tobytes()
    for variant in KERNEL_VARIANTS:
        with kernel_variant(variant):
            same_records(scene.trace_rays(rays, cam.step_dist, bg=BG), want2, f"after the update, {variant}")
    scene.close()


# ---- 9. pick ----
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_pick(world, oracle, proj):
    gw = 0.5
    scene = world.scenes[gw]
    for sampling in SAMPLINGS:
        rays, want, cam = world.camera_case(gw, proj, False, sampling)
        W, H = cam.width, cam.height
        cfg = oracle.make_cfg(cam, world.params[gw], MAP_W, MAP_H)
        fb, _t, _c, steps, entry = oracle.render(cfg, world.heights[gw], world.cmap, per_pixel=True)
        if sampling == 0:
            assert np.array_equal(scene.render(cam), fb)
        pixels = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2), (W // 2, H - 1), (7, 22), (13, 17), (31, 9),
                  (20, 25), (3, 28), (38, 14)]
        assert len(set(pixels)) == 12
        kinds = set()
        for px, py in pixels:
            rec = scene.pick(cam, px, py)
            assert rec["rgba"].tolist() == fb[py, px].tolist(), (px, py)
            assert int(rec["steps"]) == int(steps[py, px]) and rec["entry_d"].tobytes() == entry[py, px].tobytes(), (px, py)
            pos, dirv, _ = oracle.probe_ray(cfg, px, py)
            one = scene.trace_rays(np.concatenate([pos, dirv])[None, :], cam.step_dist, bg=BG, sampling=sampling)
            assert rec.tobytes() == one[0].tobytes() == want[py * W + px].tobytes(), (px, py)
            kinds.add(int(rec["status"]))
        assert kinds == {ray_replay.MISS, ray_replay.HIT}
    with pytest.raises(world.gpu.HmrmError) as e:
        scene.pick(cam, W, 0)
    assert e.value.code == world.gpu.HMRM_E_ARG
