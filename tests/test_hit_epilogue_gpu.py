"""A hit lane's colour is fetched behind the march loop (csrc/march.hpp DEFER, hcell): the lane leaves the loop with its hit
cell and the epilogue makes the pixel, the diffuse level and the record from it.  Small frames (40 x 24: partial 8 x 8 wave
tiles on the right, three tile rows) over the 64 x 48 map of tests/segment_cases.py (oblong, a block of alpha-0 texels, a patch
of zero-height cells), compared EXACTLY with the oracle and the numpy replays: pixels, records, per-pixel step counts.

What the cases are chosen for, each asserted from the oracle / the replays so that a scene change cannot drop it quietly:
  * hits on alpha-0 texels (the background-colour rule, hmap.cpp:1020) among the hit cells;
  * hits at every position of a speculative group: under HMRM_KERNEL=group a hit ray's position in its group of 6 is
    (step count - 1) mod 6; in the production kernel a ray that never leaped hits at (step count - 1) mod 4;
  * step caps and per-ray limits under which rays hit inside the near-the-cap literal path (budget < U on entry to a group),
    are stopped exactly where they would have hit, leave the grid inside that path, and enter a group with budget 0;
  * the three sampling modes, grid widths 1, 0.5 and 0.05 (grid modes 0, 1, 2), the four kernels (default, group, rec, simple),
    and every family once: plain, antialiased, lit, shaded, lit + shaded (also antialiased), ray batches, segments, interior."""
import numpy as np
import pytest

import gpu_support as gs
import segment_cases as sc
import segment_replay as sr
import shade_cases as shc
from aa_box import box_filter, super_camera
from gpu_support import env, gpu, same_frame, same_records, samplings_of
from segment_cases import BG, GRID_WIDTHS, GW_IDS, MAP_H, MAP_W

pytestmark = pytest.mark.gpu

W, H = 40, 24
KERNELS = (None, "group", "rec", "simple")  # None: the scene's own choice, the production kernel
KERNEL_IDS = ["default", "group", "rec", "simple"]
SUN = shc.SUNS[0]
# (step cap, inside camera): what the cap leaves over of a group of 4 and of 6 -- 0 and 0 (budget 0 on entry to a group), 3 and 3,
# 1 and 5, 2 and 0 for the outside camera (rays of 1 .. 150 loads); 3 and 5, 0 and 0, 2 and 2 for the inside one (hits from 19 loads on)
CAPS = ((12, False), (15, False), (53, False), (54, False), (23, True), (24, True), (26, True))
CAP_IDS = [f"cap{c}{'in' if i else 'out'}" for c, i in CAPS]


class World(gs.Scenes, shc.Replays):
    """Scenes per grid width, the oracle's frames, and the replays' caches (computed once, read-only)."""

    def __init__(self, gpu, oracle):
        super().__init__(gpu, oracle)
        self._oracle, self._seg = {}, {}

    def cam(self, gw, sampling=0, inside=False, proj=1):
        return sc.camera(self.gpu, gw, proj, inside, sampling, width=W, height=H)

    def oracle_frame(self, gw, sampling, n=1):
        """(frame, per-pixel steps) of the outside perspective camera, n x n samples per pixel."""
        key = (gw, sampling, n)
        if key not in self._oracle:
            cam = super_camera(self.gpu, self.cam(gw, sampling), n)
            fb, _total, capped, steps, _ = self.oracle.render(self.oracle.make_cfg(cam, self.params[gw], MAP_W, MAP_H), self.heights[gw],
                                                              self.cmap, per_pixel=True)
            assert capped == 0
            fb.setflags(write=False)
            steps.setflags(write=False)
            self._oracle[key] = (fb, steps)
        return self._oracle[key]

    def records(self, gw, sampling=0, inside=False, **kw):
        """segment_replay.replay of the camera's rays (interior rule for the inside camera)."""
        key = (gw, sampling, inside, tuple(sorted((k, v if not isinstance(v, np.ndarray) else v.tobytes()) for k, v in kw.items())))
        if key not in self._seg:
            r = sr.replay(self.rays(gw, 1, inside, W, H), self.heights[gw], self.cmap, self.params[gw], 0.2 * gw, bg=BG,
                          sampling=sampling, interior=inside, **kw)
            r.setflags(write=False)
            self._seg[key] = r
        return self._seg[key]


world = gs.world_fixture(World)


def sun_of(gpu, gw, **kw):
    return gpu.Sun.make(SUN, 0.3 * gw, ambient=shc.AMBIENT, **kw)


# ---- what the scenes cover ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
def test_hits_cover_alpha_zero_texels_and_every_group_position(world, gw):
    for inside in (False, True):
        rec = world.records(gw, 0, inside)
        hit = rec["status"] == sr.HIT
        assert hit.sum() > (300 if inside else 150)
        alpha = world.cmap[rec["cell_y"][hit], rec["cell_x"][hit], 3]
        assert (alpha == 0).sum() >= 20 and (alpha == 255).sum() >= 100, "hits on alpha-0 texels and on opaque ones"
        pos6 = (rec["steps"][hit].astype(np.int64) - 1) % 6
        assert set(pos6.tolist()) == set(range(6)), "HMRM_KERNEL=group: a hit at every position of a group of 6"
    # the production kernel: rays that never leap (instrumented kernel, per pixel: attempts << 16 | leaps) march groups of 4
    _fb, steps = world.oracle_frame(gw, 0)
    rec = world.records(gw, 0)
    with env(HMRM_KERNEL=None, HMRM_DIAG_ITERS=19):
        _, _st, word, _ = world.scenes[gw].render_stats(world.cam(gw), per_pixel=True)
    unleaped_hit = ((word.reshape(-1) & 0xffff) == 0) & (rec["status"] == sr.HIT)
    pos4 = (steps.reshape(-1)[unleaped_hit].astype(np.int64) - 1) % 4
    assert set(pos4.tolist()) == set(range(4)), "the production kernel: an unleaped hit at every position of a group of 4"


@pytest.mark.parametrize("cap,inside", CAPS, ids=CAP_IDS)
def test_caps_cover_the_literal_path(world, cap, inside):
    """Read off the uncapped replay (no leaps: the plain groups, and the production kernel's unleaped rays): with `cap` loads
    allowed, a ray whose group starts at load k * U + 1 enters it with budget cap - k * U."""
    free = world.records(0.5, 0, inside)
    s = free["steps"].astype(np.int64)
    hit, miss = free["status"] == sr.HIT, (free["status"] == sr.MISS) & (s > 0)
    for U in (4, 6):
        left = cap % U
        if left == 0:
            assert (s > cap).sum() >= 50, "rays that enter a group with budget 0"
            continue
        last = (s > cap - left) & (s <= cap)  # the ray's last load is one of the cap's last `left`: made by the literal path
        assert (hit & last).sum() >= 3, f"hits inside the literal path (U = {U})"
        assert (hit & (s == cap + 1)).sum() >= 1, "rays stopped exactly where they would have hit"
        if not inside:  # (s loads, then the range test fails: the ray leaves the grid with budget left, inside the path)
            assert (miss & last).sum() >= 1, f"rays that leave the grid inside the literal path (U = {U})"


# ---- plain frames, instrumented frames, ray batches ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_plain_frames_and_ray_batches(world, kernel, gw):
    scene = world.scenes[gw]
    with env(HMRM_KERNEL=kernel, HMRM_DIAG_ITERS=None):
        for sampling in samplings_of(kernel):
            cam = world.cam(gw, sampling)
            want_fb, want_steps = world.oracle_frame(gw, sampling)
            what = f"{kernel} gw {gw} sampling {sampling}"
            same_frame(scene.render(cam), want_fb, "render " + what)
            fb, st, steps, _ = scene.render_stats(cam, per_pixel=True)
            same_frame(fb, want_fb, "render_stats " + what)
            assert np.array_equal(steps.astype(np.int64), want_steps), "per-pixel step counts " + what
            want = world.records(gw, sampling)
            assert st.hits == (want["status"] == sr.HIT).sum() and st.steps == want_steps.sum()
            assert np.array_equal(want["rgba"].reshape(H, W, 4), want_fb), "the replay is the oracle's frame"
            same_records(scene.trace_rays(world.rays(gw, 1, False, W, H), 0.2 * gw, bg=BG, sampling=sampling), want, "trace_rays " + what)


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_antialiased_frames(world, kernel):
    with env(HMRM_KERNEL=kernel):
        for gw in GRID_WIDTHS:
            for sampling in samplings_of(kernel):
                want = box_filter(world.oracle_frame(gw, sampling, 2)[0], 2)
                same_frame(world.scenes[gw].render_aa(world.cam(gw, sampling), 2), want, f"render_aa {kernel} gw {gw} sampling {sampling}")


# ---- segments and interior frames ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_segments_and_interior_frames(world, kernel, gw):
    scene = world.scenes[gw]
    with env(HMRM_KERNEL=kernel):
        for sampling in samplings_of(kernel):
            want = world.records(gw, sampling, True)
            what = f"{kernel} gw {gw} sampling {sampling}"
            same_records(scene.trace_segments(world.rays(gw, 1, True, W, H), 0.2 * gw, bg=BG, sampling=sampling, interior=True), want,
                         "trace_segments " + what)
            same_frame(scene.render_interior(world.cam(gw, sampling, True)), want["rgba"], "render_interior " + what)


# ---- step caps and per-ray limits around the hit ----
@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("cap,inside", CAPS, ids=CAP_IDS)
def test_step_caps(world, cap, inside, kernel):
    gw = 0.5
    scene = world.scenes[gw]
    rays = world.rays(gw, 1, inside, W, H)
    with env(HMRM_KERNEL=kernel, HMRM_STEP_CAP=cap):
        for sampling in samplings_of(kernel):
            want = world.records(gw, sampling, inside, step_cap=cap)
            capped = int((want["status"] == sr.CAPPED).sum())
            assert capped >= 50 and (want["status"] == sr.HIT).sum() >= 100
            what = f"cap {cap} {kernel} sampling {sampling} inside {inside}"
            got, st = scene.trace_segments(rays, 0.2 * gw, bg=BG, sampling=sampling, interior=inside, stats=True, allow_capped=True)
            same_records(got, want, "trace_segments " + what)
            assert st.capped == capped
            same_frame(scene.render_interior(world.cam(gw, sampling, inside), allow_capped=True), want["rgba"], "render_interior " + what)
            if not inside:  # (the entries without the rules: ray batches and the instrumented kernel)
                same_records(scene.trace_rays(rays, 0.2 * gw, bg=BG, sampling=sampling, allow_capped=True), want, "trace_rays " + what)
                fb, st, _steps, _ = scene.render_stats(world.cam(gw, sampling), per_pixel=True, allow_capped=True)
                same_frame(fb, want["rgba"], "render_stats " + what)
                assert st.capped == capped and st.steps == want["steps"].sum()


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_per_ray_limits_around_the_hit(world, kernel):
    """Every ray's own limit is set from its free step count S: S - 1 (ended exactly where it would have hit), S (its last
    load hits, or leaves the grid, with the budget spent), S + 1 .. S + 3 (budget below the group length in the last group),
    and the multiples of 4 and 6 below S (budget 0 on entry to a group).  Whatever leaps a ray makes, its budget passes
    through the literal path's every state somewhere in the frame."""
    for gw in GRID_WIDTHS:
        scene = world.scenes[gw]
        for inside in (False, True):
            rays = world.rays(gw, 1, inside, W, H)
            s = world.records(gw, 0, inside)["steps"].astype(np.int64)
            i = np.arange(s.size)
            delta = np.array([-1, 0, 1, 2, 3, 0, -1])[i % 7]
            lim = np.where(i % 11 == 3, (s - 1) // 4 * 4, np.where(i % 11 == 7, (s - 1) // 6 * 6, s + delta))
            per = np.maximum(lim, 0).astype(np.uint32)  # (0: no limit)
            with env(HMRM_KERNEL=kernel):
                for sampling in samplings_of(kernel):
                    want = world.records(gw, sampling, inside, per_ray=per)
                    if sampling == 0:
                        assert (want["status"] == sr.END).sum() >= 100 and (want["status"] == sr.HIT).sum() >= 100
                        assert ((want["status"] == sr.HIT) & (want["steps"] == per)).sum() >= 30, "hits with the last load of the budget"
                    got = scene.trace_segments(rays, 0.2 * gw, bg=BG, sampling=sampling, interior=inside, per_ray_max_steps=per)
                    same_records(got, want, f"per-ray limits {kernel} gw {gw} sampling {sampling} inside {inside}")


# ---- lit, shaded, lit + shaded ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_lit_and_shaded_frames(world, kernel, gw):
    gpu, scene = world.gpu, world.scenes[gw]
    with env(HMRM_KERNEL=kernel):
        for sampling in samplings_of(kernel):
            for inside in ((False, True) if sampling == 0 else (False,)):
                cam = world.cam(gw, sampling, inside)
                sun = sun_of(gpu, gw, interior=inside)
                what = f"{kernel} gw {gw} sampling {sampling} inside {inside}"
                lit = world.lit(gw, 1, sampling, SUN, inside, W, H, ambient=shc.AMBIENT)
                hit = lit["primary"]["status"] == sr.HIT
                assert lit["capped"] == 0 and lit["shadowed"].sum() >= 20 and (hit & ~lit["shadowed"]).sum() >= 100
                same_frame(scene.render_lit(cam, sun), lit["rgba"], "render_lit " + what)
                for diffuse, shadows in ((True, False), (True, True)):
                    want = world.shaded(gw, 1, sampling, SUN, diffuse, shadows, inside, W, H)
                    same_frame(scene.render_shaded(cam, sun, diffuse=diffuse, shadows=shadows), want["rgba"],
                               f"render_shaded shadows {shadows} " + what)


def test_lit_frames_under_a_step_cap(world):
    """Primary and shadow rays near the cap: both marches' literal paths, the primary hit's cell kept across the second."""
    gw, cap = 0.5, 23
    with env(HMRM_STEP_CAP=cap):
        for kernel in KERNELS:
            with env(HMRM_KERNEL=kernel):
                for sampling in samplings_of(kernel):
                    cam = world.cam(gw, sampling)
                    want = world.shaded(gw, 1, sampling, SUN, True, True, False, W, H, step_cap=cap)
                    assert want["capped"] >= 50
                    fb = world.scenes[gw].render_shaded(cam, sun_of(world.gpu, gw), diffuse=True, shadows=True, allow_capped=True)
                    same_frame(fb, want["rgba"], f"render_shaded cap {cap} {kernel} sampling {sampling}")
                    lit = world.lit(gw, 1, sampling, SUN, False, W, H, step_cap=cap, ambient=shc.AMBIENT)
                    same_frame(world.scenes[gw].render_lit(cam, sun_of(world.gpu, gw), allow_capped=True), lit["rgba"],
                               f"render_lit cap {cap} {kernel} sampling {sampling}")


@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
def test_antialiased_lit_and_shaded_frames(world, kernel):
    """The sun-lit families' antialiased kernels: each sample lit and shaded on its own, then filtered."""
    gw = 0.05
    with env(HMRM_KERNEL=kernel):
        for sampling in samplings_of(kernel):
            cam = world.cam(gw, sampling)
            sun = sun_of(world.gpu, gw)
            lit = world.lit(gw, 1, sampling, SUN, False, 2 * W, 2 * H, ambient=shc.AMBIENT)
            same_frame(world.scenes[gw].render_lit(cam, sun, aa=2), box_filter(lit["rgba"].reshape(2 * H, 2 * W, 4), 2),
                       f"render_lit aa {kernel} sampling {sampling}")
            for shadows in (False, True):
                want = world.shaded(gw, 1, sampling, SUN, True, shadows, False, 2 * W, 2 * H)
                same_frame(world.scenes[gw].render_shaded(cam, sun, diffuse=True, shadows=shadows, aa=2),
                           box_filter(want["rgba"].reshape(2 * H, 2 * W, 4), 2), f"render_shaded aa shadows {shadows} {kernel} sampling {sampling}")
