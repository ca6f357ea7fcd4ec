"""The staging buffers and ticket pools behind the host-memory entry points (DeviceScratch, acquire_ticket).
One scene over a 64 x 64 map takes every host-memory entry point three times in a row -- a small size, a strictly larger one that
forces its scratch to be re-allocated, the small one again -- with the families interleaved, so that the buffers two of them
share (targets / directions, entry distances / the probe of hmrm_pick) change hands in between.  Every result is compared BYTEWISE
with the device-memory twin of the same call written into a torch tensor, which uses no scene scratch (hmrm_render_stats: with a
fresh scene's; hmrm_pick: with the oracle's ray traced by hmrm_trace_rays_device).  Then both ticket pools are filled to their 64
slots, refused at the 65th begin, and every frame is compared with hmrm_render's."""
import numpy as np
import pytest

import scenes
import segment_cases as sc
from gpu_support import gpu

pytestmark = pytest.mark.gpu

MAP = 64
GW = 0.5
FRAMES = ((8, 8), (24, 16), (8, 8))
BATCHES = (5, 300, 5)
RECTS = ((3, 5, 4, 4), (10, 7, 20, 12), (3, 5, 4, 4))  # x0, y0, w, h
N_DIRS = (3, 40, 3)
MAX_TICKETS = 64  # kMaxRing
AMBIENT = 96
NO_HIT = 0xFFFF  # a light sum where the primary ray hit nothing


@pytest.fixture(scope="module")
def world(gpu):
    rgb, cmap = scenes.small_maps(MAP, MAP, 47)
    params = sc.scene_params(gpu, GW)
    scene = gpu.Scene(rgb, cmap, params)
    yield gpu, scene, rgb, cmap, params
    scene.close()


def directions(k):
    """k directions above the horizon, none alike."""
    a = np.arange(k, dtype=np.float64)
    return np.ascontiguousarray(np.stack([np.cos(0.7 * a + 0.3), np.sin(0.7 * a + 0.3), 0.25 + 0.02 * a], axis=1))


def rays(n, seed):
    """n rays from above the map down into it, every seventh one upwards (a miss)."""
    rng = np.random.RandomState(seed)
    r = np.empty((n, 6), dtype=np.float64)
    r[:, 0] = rng.uniform(0.1, 0.9, n) * MAP * GW
    r[:, 1] = -rng.uniform(0.1, 0.9, n) * MAP * GW
    r[:, 2] = 12.0 * GW
    r[:, 3:5] = rng.uniform(-1.0, 1.0, (n, 2))
    r[:, 5] = -1.0
    r[3::7, 5] = 1.0
    return r


def device_bytes(t):
    return t.cpu().numpy().tobytes()


def test_small_large_small(world, oracle):
    import torch
    gpu, scene, rgb, cmap, params = world
    fresh = gpu.Scene(rgb, cmap, params)  # (hmrm_render_stats has no device twin: a scene whose scratch every call finds empty or equal)
    sun = gpu.Sun.make((9.0, 9.0, -9.0), 0.3 * GW, ambient=AMBIENT)
    step = 0.3 * GW
    seen = set()
    try:
        for rnd, ((W, H), n, rect, k) in enumerate(zip(FRAMES, BATCHES, RECTS, N_DIRS)):
            what = f"round {rnd}"
            cam = sc.camera(gpu, GW, 1, False, 0, width=W, height=H)
            sph = sc.camera(gpu, GW, 2, False, 0, width=W, height=H)

            # hmrm_render
            d = torch.zeros((H, W), dtype=torch.int32, device="cuda")
            scene.render_rows_device(cam, d.data_ptr(), W * 4, 0, H)
            assert scene.take_capped(0) == 0
            frame = scene.render(cam)
            assert frame.tobytes() == device_bytes(d), what + ", render"

            # hmrm_pick: a perspective camera, then a spherical one (its tables go behind the probe's doubles)
            for c in (cam, sph):
                cfg = oracle.make_cfg(c, params, MAP, MAP)
                for px, py in ((0, 0), (W - 1, H - 1), (W // 2, H // 2)):
                    pos, dirv, _ = oracle.probe_ray(cfg, px, py)
                    d_ray = torch.tensor(np.concatenate([pos, dirv]), dtype=torch.float64, device="cuda")
                    d_hit = torch.zeros(7, dtype=torch.int64, device="cuda")
                    scene.trace_rays_device(d_ray.data_ptr(), 1, d_hit.data_ptr(), c.step_dist, bg=sc.BG)
                    assert scene.take_capped(0) == 0
                    assert scene.pick(c, px, py).tobytes() == device_bytes(d_hit), (what, "pick", c.projection, px, py)

            # hmrm_render_stats: the per-pixel arrays
            fb, st, steps, entry = scene.render_stats(cam, per_pixel=True)
            fb2, st2, steps2, entry2 = fresh.render_stats(cam, per_pixel=True)
            assert fb.tobytes() == fb2.tobytes() == frame.tobytes(), what + ", stats frame"
            assert steps.tobytes() == steps2.tobytes() and entry.tobytes() == entry2.tobytes(), what + ", per-pixel arrays"
            assert (st.rays, st.steps, st.hits, st.capped) == (st2.rays, st2.steps, st2.hits, st2.capped) and st.steps == int(steps.sum())

            # hmrm_render_geometry: all four planes
            planes = scene.render_geometry(cam)
            d_rgba = torch.zeros((H, W), dtype=torch.int32, device="cuda")
            d_cell = torch.zeros((H, W), dtype=torch.int32, device="cuda")
            d_range = torch.zeros((H, W), dtype=torch.float32, device="cuda")
            d_slope = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda")
            scene.render_geometry_device(cam, rgba=(d_rgba.data_ptr(), W * 4), cell=(d_cell.data_ptr(), W * 4),
                                         range=(d_range.data_ptr(), W * 4), slope=(d_slope.data_ptr(), W * 8))
            assert scene.take_capped(0) == 0
            for name, t in (("rgba", d_rgba), ("cell", d_cell), ("range", d_range), ("slope", d_slope)):
                assert planes[name].tobytes() == device_bytes(t), f"{what}, geometry {name}"
            hit = planes["cell"] >= 0
            assert planes["rgba"].tobytes() == frame.tobytes()
            assert hit.any() and not hit.all(), what + ": the frame must mix terrain and sky (the CPU oracle counts 14 / 50 and 155 / 229)"

            # hmrm_render_lit_sum: both planes, k directions (staged where hmrm_cell_map_sum stages its targets)
            dirs = directions(k)
            lit, light = scene.render_lit_sum(cam, sun, dirs, diffuse=True, light=True)
            d_dirs = torch.tensor(dirs, device="cuda")
            d_lit = torch.zeros((H, W), dtype=torch.int32, device="cuda")
            d_light = torch.zeros((H, W), dtype=torch.int16, device="cuda")
            scene.render_lit_sum_device(cam, sun, d_dirs.data_ptr(), k, rgba=(d_lit.data_ptr(), W * 4), light=(d_light.data_ptr(), W * 2),
                                        diffuse=True)
            assert scene.take_capped(0) == 0
            assert lit.tobytes() == device_bytes(d_lit) and light.tobytes() == device_bytes(d_light), what + ", lit sum"
            assert ((light == NO_HIT) == ~hit).all()

            # hmrm_trace_rays
            r = rays(n, 100 + rnd)
            d_rays = torch.tensor(r, device="cuda")
            d_hits = torch.zeros(7 * n, dtype=torch.int64, device="cuda")
            scene.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), 0.2 * GW, bg=sc.BG)
            assert scene.take_capped(0) == 0
            hits, tst = scene.trace_rays(r, 0.2 * GW, bg=sc.BG, stats=True)
            assert hits.tobytes() == device_bytes(d_hits), what + ", trace_rays"
            assert tst.rays == n and tst.steps == int(hits["steps"].sum()) and tst.hits == int((hits["status"] == gpu.RAY_HIT).sum())
            seen |= set(hits["status"].tolist())

            # hmrm_trace_segments with per-ray limits
            limits = np.random.RandomState(200 + rnd).randint(0, 40, n).astype(np.uint32)
            d_limits = torch.tensor(limits.view(np.int32), device="cuda")
            d_hits = torch.zeros(7 * n, dtype=torch.int64, device="cuda")
            scene.trace_segments_device(d_rays.data_ptr(), n, d_hits.data_ptr(), 0.2 * GW, bg=sc.BG, max_steps=30,
                                        d_max_steps_ptr=d_limits.data_ptr())
            assert scene.take_capped(0) == 0
            segs = scene.trace_segments(r, 0.2 * GW, bg=sc.BG, max_steps=30, per_ray_max_steps=limits)
            assert segs.tobytes() == device_bytes(d_hits), what + ", trace_segments"
            seen |= set(segs["status"].tolist())

            # hmrm_cell_map
            x0, y0, w, h = rect
            cells = scene.cell_map(dirs[0], step, lift=0.1 * GW, weight=True, diffuse=True, ambient=AMBIENT, rect=rect)
            d_cells = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
            scene.cell_map_device(d_cells.data_ptr(), w, dirs[0], step, lift=0.1 * GW, weight=True, diffuse=True, ambient=AMBIENT, rect=rect)
            assert scene.take_capped(0) == 0
            assert cells.shape == (h, w) and cells.tobytes() == device_bytes(d_cells), what + ", cell_map"

            # hmrm_cell_map_sum: its targets go where the lit sum's directions went
            sums = scene.cell_map_sum(dirs, step, lift=0.1 * GW, weight=True, diffuse=True, ambient=AMBIENT, rect=rect)
            d_sums = torch.zeros((h, w), dtype=torch.int16, device="cuda")
            scene.cell_map_sum_device(d_sums.data_ptr(), 2 * w, d_dirs.data_ptr(), k, step, lift=0.1 * GW, weight=True, diffuse=True,
                                      ambient=AMBIENT, rect=rect)
            assert scene.take_capped(0) == 0
            assert sums.shape == (h, w) and sums.tobytes() == device_bytes(d_sums), what + ", cell_map_sum"
        assert {gpu.RAY_MISS, gpu.RAY_HIT, gpu.RAY_END} <= seen
    finally:
        fresh.close()


def ticket_camera(gpu, i):
    """A camera per ticket: frames that differ tell a slot handed out twice from one handed out once."""
    cam = sc.camera(gpu, GW, 1, False, 0, width=8, height=8)
    cam.hang = gpu.degrees_to_rads(-50.0 + 0.5 * i)
    return cam


def test_ticket_pools_fill_refuse_and_refill(world):
    import torch
    gpu, scene, *_ = world
    cams = [ticket_camera(gpu, i) for i in range(MAX_TICKETS + 1)]
    want = [scene.render(c).tobytes() for c in cams]
    assert len(set(want)) == len(want)  # (the CPU oracle renders 65 different frames for these cameras)

    # the read-back ring
    tickets = {scene.render_begin(cams[i]): i for i in range(MAX_TICKETS)}
    assert sorted(tickets) == list(range(MAX_TICKETS))
    with pytest.raises(gpu.HmrmError) as e:
        scene.render_begin(cams[MAX_TICKETS])
    assert e.value.code == gpu.HMRM_E_ARG and "hmrm_render_begin: every frame of the ring is in use (release one)" in str(e.value)
    assert scene.render_wait(17, (8, 8)).tobytes() == want[tickets[17]]
    scene.render_release(17)
    assert scene.render_begin(cams[MAX_TICKETS]) == 17
    tickets[17] = MAX_TICKETS
    for t, i in tickets.items():
        assert scene.render_wait(t, (8, 8)).tobytes() == want[i], (t, i)
        scene.render_release(t)

    # the device tickets
    frames = torch.zeros((MAX_TICKETS + 1, 8, 8), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    tickets = {scene.render_device_begin(cams[i], frames[i].data_ptr(), 32): i for i in range(MAX_TICKETS)}
    assert sorted(tickets) == list(range(MAX_TICKETS))
    with pytest.raises(gpu.HmrmError) as e:
        scene.render_device_begin(cams[MAX_TICKETS], frames[MAX_TICKETS].data_ptr(), 32)
    assert e.value.code == gpu.HMRM_E_ARG and "hmrm_render_device_begin: 64 frames in flight (wait for one)" in str(e.value)
    scene.render_device_wait(40)
    assert scene.render_device_begin(cams[MAX_TICKETS], frames[MAX_TICKETS].data_ptr(), 32) == 40
    for t in tickets:
        scene.render_device_wait(t)
    host = frames.cpu().numpy()
    for i in range(MAX_TICKETS + 1):
        assert host[i].tobytes() == want[i], i
