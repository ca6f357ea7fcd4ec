"""The march kernels' per-ray level state (csrc/frame.hpp level_state_table, march.hpp `ls`) on the GPU: small frames over small
maps chosen so that every pyramid level, the whole-map level and every clamp of the window geometry and of the level policy
is reached -- oblong maps that are no multiple of any window size (windows overhang both edges), a 1024 x 1024 map (the
256-cell level and the whole map), a flat map (seen from low outside it rays stay at the top level; seen from above they
start at the level their descent leaves room for), needles and a canyon (height-limited descents
down to min_level and finest_pause) -- under all three projections, rays whose cell index falls along x and along y, a camera
in the binade-dense corner at the origin, step_dist 0.25 and 2.0 (min_level 0 and above), three grid widths, the three
kernels, the three sampling modes, an antialiased frame, a lit and shaded frame and a ray batch.

Pixels and per-pixel step counts are compared with the CPU oracle.  The traversal counters (steps, rays, hits, groups,
attempts, leaps, leaped steps, and the attempts per level of the instrumented kernel's modes 5 and 23) are compared with
tests/golden/level_state_counts.json, recorded with the build of commit e2d4f14, the last one whose attempts derived the
window geometry from the level number on every attempt: the state is a restatement, no counter may move.

Re-record (only for a change that is meant to change the traversal): python tests/test_level_state_gpu.py --record"""
import json
import os
import sys

import numpy as np
import pytest

from gpu_support import env, gpu

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "level_state_counts.json")
FIELDS = ("steps", "rays", "hits", "groups", "leap_attempts", "leaps", "leaped_steps")
SMALL, RAGGED = (24, 16), (40, 33)  # (a frame inside one row of 8 x 8-pixel wave tiles; partial tiles on both axes)


def _flat(w, h, v=90):
    rgb = np.full((h, w, 3), v, dtype=np.uint8)
    cmap = np.zeros((h, w, 4), dtype=np.uint8)
    cmap[:, :, 0] = (np.arange(w, dtype=np.int64)[None, :] * 7 % 256).astype(np.uint8)
    cmap[:, :, 1] = (np.arange(h, dtype=np.int64)[:, None] * 5 % 256).astype(np.uint8)
    cmap[:, :, 2], cmap[:, :, 3] = 99, 255
    return rgb, cmap


def make_maps(hmrm, key):
    import scenes
    if key == "oblong":
        return scenes.small_maps(300, 260, 11)
    if key == "tall":
        return scenes.small_maps(20, 700, 12)
    if key == "sq1024":
        return hmrm.synth.synth_maps(1024)
    if key == "flat":
        return _flat(256, 192)
    if key in ("needles", "canyon"):
        return hmrm.synth.content_maps(512, key)
    raise KeyError(key)


MAP_KEYS = ("oblong", "tall", "sq1024", "flat", "needles", "canyon")

# name -> (map, grid width, pose, projection, frame, step_dist in cells, sampling, HMRM_KERNEL)
# poses (in cells, scaled by the grid width): "front" looks across the map from off the corner at the origin (cell indices
# rise along x and y), "back" from off the opposite corner (both fall: the windows' `back` strides), "over" is a spherical
# all-round view from above the map's middle (all four sign combinations), "corner" sits just above the origin corner, where
# x and y cross a binade every few steps, "low" looks down the canyon's corridor from below the raised terrain.
CASES = {
    "oblong/persp/front": ("oblong", 1.0, "front", 1, RAGGED, 0.25, 0, None),
    "oblong/persp/back": ("oblong", 1.0, "back", 1, SMALL, 0.25, 0, None),
    "oblong/sph/over": ("oblong", 1.0, "over", 2, RAGGED, 0.25, 0, None),
    "oblong/ortho/back": ("oblong", 1.0, "back", 3, SMALL, 2.0, 0, None),
    "oblong/sph/over/gw0.5": ("oblong", 0.5, "over", 2, SMALL, 0.25, 0, None),
    "oblong/persp/back/gw0.05": ("oblong", 0.05, "back", 1, RAGGED, 0.25, 0, None),
    "oblong/sph/corner": ("oblong", 1.0, "corner", 2, SMALL, 0.25, 0, None),
    "oblong/sph/corner/gw0.05": ("oblong", 0.05, "corner", 2, SMALL, 2.0, 0, None),
    "tall/sph/over": ("tall", 1.0, "over", 2, RAGGED, 0.25, 0, None),
    "tall/persp/back/step2": ("tall", 1.0, "back", 1, SMALL, 2.0, 0, None),
    "tall/ortho/front/gw0.5": ("tall", 0.5, "front", 3, SMALL, 0.25, 0, None),
    "sq1024/persp/front": ("sq1024", 1.0, "front", 1, RAGGED, 0.25, 0, None),
    "sq1024/sph/over": ("sq1024", 1.0, "over", 2, SMALL, 0.25, 0, None),
    "sq1024/ortho/back/step2": ("sq1024", 1.0, "back", 3, SMALL, 2.0, 0, None),
    "sq1024/persp/back/rec": ("sq1024", 1.0, "back", 1, SMALL, 0.25, 0, "rec"),
    "sq1024/sph/over/group": ("sq1024", 1.0, "over", 2, SMALL, 0.25, 0, "group"),
    "sq1024/persp/front/bilinear": ("sq1024", 1.0, "front", 1, SMALL, 0.25, 1, None),
    "sq1024/persp/back/f32/gw0.05": ("sq1024", 0.05, "back", 1, SMALL, 0.25, 2, None),
    "flat/sph/over": ("flat", 1.0, "over", 2, RAGGED, 0.25, 0, None),
    "flat/persp/back/step2": ("flat", 1.0, "back", 1, SMALL, 2.0, 0, None),
    "flat/persp/front": ("flat", 1.0, "front", 1, RAGGED, 0.25, 0, None),
    "flat/persp/low": ("flat", 1.0, "low", 1, RAGGED, 0.25, 0, None),
    "needles/persp/front": ("needles", 1.0, "front", 1, RAGGED, 0.25, 0, None),
    "needles/sph/over/step2": ("needles", 1.0, "over", 2, SMALL, 2.0, 0, None),
    "needles/persp/back/rec": ("needles", 1.0, "back", 1, SMALL, 0.25, 0, "rec"),
    "needles/ortho/front/bilinear/gw0.5": ("needles", 0.5, "front", 3, SMALL, 0.25, 1, None),
    "canyon/persp/low": ("canyon", 1.0, "low", 1, RAGGED, 0.25, 0, None),
    "canyon/sph/low/step2": ("canyon", 1.0, "low", 2, SMALL, 2.0, 0, None),
    "canyon/persp/low/gw0.05": ("canyon", 0.05, "low", 1, SMALL, 0.25, 0, None),
}
# the frames rendered through the other entry points (each from one of the cases above)
AA_CASE, SHADED_CASE, RAYS_CASE = "oblong/persp/back", "needles/persp/front", "oblong/sph/over"
# per-level attempt counts (the instrumented kernel's modes 5 and 23) are recorded for these
LEVEL_CASES = ("sq1024/persp/front", "sq1024/sph/over", "sq1024/ortho/back/step2", "oblong/sph/over", "flat/sph/over",
               "flat/persp/front", "flat/persp/low", "needles/persp/front", "canyon/persp/low", "canyon/sph/low/step2")


def scene_params(hmrm, map_shape, gw):
    size = float(max(map_shape[0], map_shape[1])) * gw
    return hmrm.SceneParams.make(min_height=0.0, max_height=size / 16.0, grid_width=gw)


def camera(hmrm, map_shape, gw, pose, proj, frame, step_cells, sampling):
    mh, mw = map_shape[0], map_shape[1]
    s = float(max(mw, mh))
    deg = hmrm.degrees_to_rads
    kw = dict(width=frame[0], height=frame[1], projection=proj, step_dist=step_cells * gw, sampling=sampling, bg=(3, 5, 7),
              hfov=deg(90.0), ortho_width=1.3 * s / frame[0] * gw)
    if pose == "front":
        pos, hang, vang = (-s / 8.0, s / 8.0, s / 4.0), -45.0, 115.0
    elif pose == "back":
        pos, hang, vang = (mw + s / 8.0, -mh - s / 8.0, s / 4.0), 135.0, 115.0
    elif pose == "over":
        pos, hang, vang = (mw * 0.5 + 0.3, -mh * 0.5 - 0.4, s / 8.0), 20.0, 120.0
        kw["hfov"] = deg(360.0)
    elif pose == "corner":
        pos, hang, vang = (0.3, -0.2, s / 16.0 + 0.5), -45.0, 100.0
        kw["hfov"] = deg(200.0)
    elif pose == "low":
        pos, hang, vang = (-s / 8.0, s / 8.0, s / 32.0), -45.0, 93.0
    else:
        raise KeyError(pose)
    if proj == 2 and pose not in ("over", "corner"):
        kw["hfov"] = deg(180.0)
    return hmrm.Camera.make(pos=tuple(v * gw for v in pos), hang=deg(hang), vang=deg(vang), **kw)


class World:
    """Maps, oracle heights and expected frames, made once and shared."""

    def __init__(self, hmrm, oracle=None):
        self.hmrm, self.oracle = hmrm, oracle
        self.maps = {k: make_maps(hmrm, k) for k in MAP_KEYS}
        self._expected = {}

    def setup(self, name):
        key, gw, pose, proj, frame, step, sampling, kernel = CASES[name]
        rgb, cmap = self.maps[key]
        params = scene_params(self.hmrm, rgb.shape, gw)
        cam = camera(self.hmrm, rgb.shape, gw, pose, proj, frame, step, sampling)
        return rgb, cmap, params, cam, kernel

    def expected(self, name):
        if name not in self._expected:
            rgb, cmap, params, cam, _ = self.setup(name)
            heights = self.oracle.update_heightmap(rgb, params)
            cfg = self.oracle.make_cfg(cam, params, rgb.shape[1], rgb.shape[0])
            fb, total, capped, steps, _ = self.oracle.render(cfg, heights, cmap, per_pixel=True)
            assert capped == 0
            self._expected[name] = (fb, total, steps, heights, cfg)
        return self._expected[name]


def count(hmrm, world, name, with_levels=False):
    """(frame, Stats counters, per-pixel steps[, per-level attempts]) of case `name` from the instrumented kernel and the
    production kernel's frame."""
    rgb, cmap, params, cam, kernel = world.setup(name)
    with env(HMRM_KERNEL=kernel, HMRM_DIAG_ITERS=None):  # (set before the scene exists: a scene reads its knobs when created)
        scene = hmrm.Scene(rgb, cmap, params)
        try:
            fb_stats, st, steps, _ = scene.render_stats(cam, per_pixel=True)
            fb = scene.render(cam)
        finally:
            scene.close()
    out = {k: int(getattr(st, k)) for k in FIELDS}
    if with_levels:
        for mode, keys in ((5, ("attempts_l0", "attempts_l1", "attempts_l2", "attempts_l3")),
                           (23, ("attempts_l3_4", "attempts_l5_6", "attempts_whole_map", "steps_leaped_whole_map"))):
            with env(HMRM_KERNEL=kernel, HMRM_DIAG_ITERS=mode):
                scene = hmrm.Scene(rgb, cmap, params)
                try:
                    _, s2, _, _ = scene.render_stats(cam)
                finally:
                    scene.close()
            out.update(dict(zip(keys, (int(s2.leap_attempts), int(s2.leaps), int(s2.groups), int(s2.leaped_steps)))))
    return fb, fb_stats, out, steps


@pytest.fixture(scope="module")
def world(hmrm, oracle):
    return World(hmrm, oracle)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_every_case(golden):
    assert set(golden["cases"]) == set(CASES)
    for name in LEVEL_CASES:
        assert "attempts_whole_map" in golden["cases"][name]


def test_recorded_frames_reach_every_level_and_clamp(golden):
    """What the cases are for, read off the recorded counters: attempts in every level bucket of the instrumented kernel
    (levels 0, 1, 2, 3, 3-4, 5-6, the whole map) and leaps at the whole-map level on the 1024 x 1024 map, steep rays that
    start below the top on the flat map, and a majority of refused attempts (height-limited descents) on the needles."""
    c = golden["cases"]
    big = [c[n] for n in LEVEL_CASES if n.startswith("sq1024")]
    for key in ("attempts_l0", "attempts_l1", "attempts_l2", "attempts_l3", "attempts_l3_4", "attempts_l5_6", "attempts_whole_map",
                "steps_leaped_whole_map"):
        assert sum(b[key] for b in big) > 0, key
    assert c["flat/sph/over"]["attempts_l5_6"] > 0 and c["flat/sph/over"]["leaps"] > 0
    assert c["flat/persp/low"]["attempts_whole_map"] > 0  # (nearly level rays from outside: the whole-map level)
    needles = c["needles/persp/front"]
    assert needles["attempts_l0"] > 0 and needles["leap_attempts"] > 2 * needles["leaps"]


@pytest.mark.parametrize("name", list(CASES))
def test_frame_steps_and_counters(gpu, world, golden, name):
    want_fb, want_total, want_steps, _, _ = world.expected(name)
    fb, fb_stats, got, steps = count(gpu, world, name, with_levels=name in LEVEL_CASES)
    assert np.array_equal(fb, want_fb), f"{name}: the production kernel's frame differs from the oracle"
    assert np.array_equal(fb_stats, want_fb), f"{name}: the instrumented kernel's frame differs from the oracle"
    assert np.array_equal(steps.astype(np.int64), want_steps), f"{name}: per-pixel step counts differ"
    assert got["steps"] == want_total and got["rays"] == want_fb.shape[0] * want_fb.shape[1]
    assert got == golden["cases"][name], f"{name}: the traversal changed"


def test_antialiased_frame(gpu, world):
    from aa_box import box_filter, super_camera
    rgb, cmap, params, cam, _ = world.setup(AA_CASE)
    sc = super_camera(gpu, cam, 2)
    heights = world.oracle.update_heightmap(rgb, params)
    ofb, _, capped, _, _ = world.oracle.render(world.oracle.make_cfg(sc, params, rgb.shape[1], rgb.shape[0]), heights, cmap)
    assert capped == 0
    scene = gpu.Scene(rgb, cmap, params)
    try:
        assert np.array_equal(scene.render_aa(cam, 2), box_filter(ofb, 2))
    finally:
        scene.close()


def test_lit_and_shaded_frame(gpu, world):
    import ray_replay
    import shade_replay
    rgb, cmap, params, cam, _ = world.setup(SHADED_CASE)
    _, _, _, heights, cfg = world.expected(SHADED_CASE)
    sun_dir, sun_step = (0.4, -0.3, 0.5), 0.5
    rays = ray_replay.camera_rays(world.oracle, cfg)
    want = shade_replay.replay(rays, heights, cmap, params, cam.step_dist, sun_dir, sun_step, bg=(cam.bg_r, cam.bg_g, cam.bg_b),
                               sampling=cam.sampling, ambient=96, diffuse=True, shadows=True)
    assert want["capped"] == 0 and int(want["shadowed"].sum()) > 0
    scene = gpu.Scene(rgb, cmap, params)
    try:
        fb = scene.render_shaded(cam, gpu.Sun.make(sun_dir, sun_step, ambient=96), diffuse=True, shadows=True)
    finally:
        scene.close()
    assert np.array_equal(fb.reshape(-1, 4), want["rgba"])


def test_ray_batch(gpu, world):
    import ray_replay
    rgb, cmap, params, cam, _ = world.setup(RAYS_CASE)
    _, _, _, heights, cfg = world.expected(RAYS_CASE)
    rays = ray_replay.camera_rays(world.oracle, cfg)
    want = ray_replay.expected_from_oracle(world.oracle, cfg, heights, cmap, rays, params)
    scene = gpu.Scene(rgb, cmap, params)
    try:
        got = scene.trace_rays(rays, cam.step_dist, bg=(cam.bg_r, cam.bg_g, cam.bg_b), sampling=cam.sampling)
    finally:
        scene.close()
    for field in ("status", "steps", "rgba", "cell_x", "cell_y"):
        assert np.array_equal(got[field], want[field]), field
    assert np.array_equal(got["entry_d"].view(np.uint64), want["entry_d"].view(np.uint64))
    assert np.array_equal(got["point"].view(np.uint64), want["point"].view(np.uint64))


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    import importlib
    hm = importlib.import_module("heightmap-ray-marcher_amd")
    hm.set_device(0)
    w = World(hm)
    cases = {}
    for name in CASES:
        cases[name] = count(hm, w, name, with_levels=name in LEVEL_CASES)[2]
        print(name, cases[name], flush=True)
    out = sys.argv[sys.argv.index("--record") + 1] if len(sys.argv) > sys.argv.index("--record") + 1 else GOLDEN
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"what": "instrumented march kernel counters per frame (hmrm_render_stats; per-level attempts: HMRM_DIAG_ITERS 5 and 23)",
                   "recorded_with": "the build of commit e2d4f14", "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
