"""Ray queries (hmrm_trace_rays, hmrm_trace_rays_device, hmrm_pick; include/hmrm.h) -- what needs no GPU: the record
layouts, the argument refusals (made before the scene pointer or any HIP call is touched), and the numpy replay of the
reference's per-ray body (tests/ray_replay.py) pinned bytewise to the C oracle on camera rays of every projection and
sampling mode -- which is what lets tests/test_trace_rays_gpu.py use the replay for rays no camera can express."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import ray_replay
import scenes

MAP_W, MAP_H = 64, 48


def test_record_layouts(hmrm):
    """(a) ctypes structures, numpy dtypes and the header's sizes agree: 48 / 56 / 16 bytes, same field offsets."""
    assert C.sizeof(hmrm.Ray) == 48 and C.sizeof(hmrm.RayHit) == 56 and C.sizeof(hmrm.TraceParams) == 16
    assert hmrm.RAY_DTYPE.itemsize == 48 and hmrm.RAY_HIT_DTYPE.itemsize == 56
    for struct, dt in ((hmrm.Ray, hmrm.RAY_DTYPE), (hmrm.RayHit, hmrm.RAY_HIT_DTYPE)):
        assert [name for name, _ in struct._fields_] == list(dt.names)
        for name, _ in struct._fields_:
            assert getattr(struct, name).offset == dt.fields[name][1], name
            assert getattr(struct, name).size == dt.fields[name][0].itemsize, name
    assert hmrm.RAY_HIT_DTYPE == ray_replay.RAY_HIT_DTYPE
    assert [hmrm.RayHit.entry_d.offset, hmrm.RayHit.steps.offset, hmrm.RayHit.cell_x.offset, hmrm.RayHit.rgba.offset,
            hmrm.RayHit.status.offset, hmrm.RayHit.reserved.offset] == [24, 32, 36, 44, 48, 52]
    assert (hmrm.RAY_MISS, hmrm.RAY_HIT, hmrm.RAY_CAPPED) == (ray_replay.MISS, ray_replay.HIT, ray_replay.CAPPED) == (0, 1, 2)
    rays = hmrm.as_rays(np.arange(12, dtype=np.float64).reshape(2, 6))
    assert rays.dtype == hmrm.RAY_DTYPE and rays.shape == (2,) and rays["dir"][1].tolist() == [9.0, 10.0, 11.0]
    with pytest.raises(ValueError):
        hmrm.as_rays(np.zeros((3, 5)))


def test_argument_refusals_need_no_scene(hmrm):
    """(b) every refusal of hmrm.h, with scene = NULL: HMRM_E_ARG and a message, before the scene is looked at."""
    lib = import_module("heightmap-ray-marcher_amd.lib").lib
    p = hmrm.TraceParams.make(0.25)
    rays = np.zeros(4, dtype=hmrm.RAY_DTYPE)
    hits = np.zeros(4, dtype=hmrm.RAY_HIT_DTYPE)
    r, h = rays.ctypes.data, hits.ctypes.data
    bad = hmrm.TraceParams.make(0.25, sampling=3)
    cases = [
        ("NULL params", (None, r, 4, h), "NULL"),
        ("NULL rays", (C.byref(p), None, 4, h), "NULL"),
        ("NULL hits", (C.byref(p), r, 4, None), "NULL"),
        ("n < 0", (C.byref(p), r, -1, h), "negative"),
        ("n > 2^29", (C.byref(p), r, (1 << 29) + 1, h), "2^29"),
        ("sampling", (C.byref(bad), r, 4, h), "sampling"),
        ("sampling, n = 0", (C.byref(bad), r, 0, h), "sampling"),
    ]
    for what, (pp, rr, n, hh), word in cases:
        rc = lib.hmrm_trace_rays(None, pp, rr, n, hh, None)
        assert rc == hmrm.HMRM_E_ARG and word in hmrm.last_error(), (what, rc, hmrm.last_error())
        rc = lib.hmrm_trace_rays_device(None, pp, rr, n, hh, None)
        assert rc == hmrm.HMRM_E_ARG and word in hmrm.last_error(), (what, rc, hmrm.last_error())
    # well-formed arguments and no scene: still an argument error, never a crash
    assert lib.hmrm_trace_rays(None, C.byref(p), r, 4, h, None) == hmrm.HMRM_E_ARG
    assert lib.hmrm_trace_rays_device(None, C.byref(p), r, 4, h, None) == hmrm.HMRM_E_ARG
    # hmrm_pick: the camera is checked first, then the pointers
    hit = hmrm.RayHit()
    cam = hmrm.Camera.make(width=8, height=8)
    zero = hmrm.Camera.make(width=0, height=8)
    assert lib.hmrm_pick(None, C.byref(zero), 0, 0, C.byref(hit)) == hmrm.HMRM_E_ARG and "resolution" in hmrm.last_error()
    assert lib.hmrm_pick(None, None, 0, 0, C.byref(hit)) == hmrm.HMRM_E_ARG
    assert lib.hmrm_pick(None, C.byref(cam), 0, 0, C.byref(hit)) == hmrm.HMRM_E_ARG
    assert lib.hmrm_pick(None, C.byref(cam), 0, 0, None) == hmrm.HMRM_E_ARG


def _maps():
    rgb, cmap = scenes.small_maps(MAP_W, MAP_H, 31)
    rgb[5:9, 40:47] = 0  # some zero-height cells
    return rgb, cmap


@pytest.mark.parametrize("sampling", [0, 1, 2], ids=["nearest", "bilinear", "f32"])
@pytest.mark.parametrize("proj", [1, 2, 3], ids=["persp", "sph", "ortho"])
def test_replay_is_the_oracle_on_camera_rays(hmrm, oracle, proj, sampling):
    """(c) ray_replay.replay == oracle.render(per_pixel=True) on the oracle's own camera rays: rgba, steps, entry_d
    bytewise, and the status against the frame (a hit ray's pixel is its texel or the alpha-0 background)."""
    rgb, cmap = _maps()
    params = hmrm.SceneParams.make(0.0, 6.0, grid_width=0.5)
    cam = hmrm.Camera.make(width=40, height=30, projection=proj, hfov=hmrm.degrees_to_rads(150 if proj == 2 else 80),
                           hang=hmrm.degrees_to_rads(-50), vang=hmrm.degrees_to_rads(112), pos=(-4.0, 5.0, 12.0),
                           ortho_width=0.9, step_dist=0.2, bg=(12, 34, 56), sampling=sampling)
    heights = oracle.update_heightmap(rgb, params)
    cfg = oracle.make_cfg(cam, params, MAP_W, MAP_H)
    rays = ray_replay.camera_rays(oracle, cfg)
    fb, total, capped, steps, entry = oracle.render(cfg, heights, cmap, per_pixel=True)
    assert capped == 0
    got = ray_replay.replay(rays, heights, cmap, params, cam.step_dist, bg=(12, 34, 56), sampling=sampling)
    assert got["entry_d"].tobytes() == entry.reshape(-1).tobytes(), "distance() (AABB.cpp:49-77)"
    assert np.array_equal(got["steps"].astype(np.int64), steps.reshape(-1)), "height loads per ray (hmap.cpp:1013)"
    assert got["rgba"].tobytes() == fb.tobytes(), "pixels (hmap.cpp:1018-1057)"
    assert int(got["steps"].sum()) == total
    # ... and the whole record array against the one derived from the oracle's outputs (point and cell: steps - 1 adds)
    want = ray_replay.expected_from_oracle(oracle, cfg, heights, cmap, rays, params)
    assert got.tobytes() == want.tobytes()
    hit = got["status"] == ray_replay.HIT
    assert 0 < hit.sum() < hit.size and (got["reserved"] == 0).all()
    assert ((got["cell_x"] >= 0) == hit).all() and (got["point"][~hit] == 0.0).all()


def test_replay_honours_the_step_cap(hmrm, oracle):
    """A ray that never leaves its cell and never hits is CAPPED with steps == cap and the miss shade, as the oracle's."""
    rgb, cmap = _maps()
    params = hmrm.SceneParams.make(0.0, 6.0, grid_width=1.0)
    heights = oracle.update_heightmap(rgb, params)
    assert heights[6, 42] == 0.0
    rays = np.array([[42.5, -6.5, -3.0, 0.0, 0.0, 1.0], [42.5, -6.5, 9.0, 0.0, 0.0, -1.0]])
    got = ray_replay.replay(rays, heights, cmap, params, 0.25, bg=(1, 2, 3), step_cap=1000)
    assert got["status"].tolist() == [ray_replay.CAPPED, ray_replay.HIT] and got["steps"][0] == 1000
    assert got["rgba"][0].tolist() == [221, 242, 255, 255] and (got["cell_x"][0], got["cell_y"][0]) == (-1, -1)
    assert (got["cell_x"][1], got["cell_y"][1]) == (42, 6)
