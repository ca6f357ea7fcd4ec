"""The family-scale cases (tests/family_scale.py) on the GPU: ray and segment batches, interior, sun-lit and shaded frames, cell
maps, geometry planes, water and haze on every member of every sweep -- world magnitudes 2^-900 .. 2^900, decimal scales, grid
widths an ulp off a power of two, relief on top of 1e9, suns of magnitude 2^+-600 -- under every kernel variant, and their
compositions on each sweep's ends and middle, all BYTEWISE against the numpy replays, whose conditions
tests/test_family_scale_cpu.py asserts.  The kernels carry absolute magnitudes (slab_points_away's moderate-exponent test and
slab_classify's 2^+-500 gate with a different origin in every lane, the binades axis_refresh declines, scaled Newton sequences
for the divisions and the root of diffuse_level, float casts of the range and the slope); the replays carry none.

The module's name sorts it behind tests/test_parity_gpu.py on purpose: that module's two heaviest cases run only while the
suite is inside its time budget (conftest.skip_if_over_budget), and these tests in front of them made both skip.

One gpu.Scene per distinct scene of the sweeps, shared by the module's tests and closed behind the last one; each is first
checked against the oracle's heights, bit for bit.  One line per case is printed (`pytest -rP` shows them)."""
import numpy as np
import pytest

import aa_box
import family_scale as fs
import gpu_support as gs
import haze_replay as hr
import lit_replay as lr
import world_scale as ws
from family_scale import AMBIENT, BG, FRAME_H, FRAME_W
from gpu_support import KERNEL_VARIANTS, env, gpu, kernel_variant, same_cells, same_frame, same_records  # noqa: F401  (gpu: the fixture)

pytestmark = pytest.mark.gpu

PROJ_NAME = dict(fs.PROJECTIONS)
SWEEP_PROJ = [(s, p) for s in fs.SWEEPS for p in (1, 2, 3)]
SWEEP_PROJ_IDS = [f"{s}-{PROJ_NAME[p]}" for s, p in SWEEP_PROJ]
LITERAL_NEAREST = ("rec", "simple")  # the families whose literal loop is nearest-only too (cell maps, geometry, haze)


class World:
    def __init__(self, gpu, oracle):
        self.gpu, self.oracle, self.R = gpu, oracle, fs.Replays(gpu, oracle)
        self._scenes = {}

    def scene(self, c):
        key = (c.rgb.ctypes.data, bytes(c.params))
        if key not in self._scenes:
            s = self.gpu.Scene(c.rgb, c.cmap, c.params)
            self._scenes[key] = s
            got, want = s.read_heights(), self.R.heights(c)
            assert got.tobytes() == np.ascontiguousarray(want).tobytes(), f"{c}: UpdateHeightmap"
        return self._scenes[key]

    def close(self):
        for s in self._scenes.values():
            s.close()


world = gs.world_fixture(World)


def samplings(c, variant, nearest_only=("rec",)):
    """NEAREST everywhere; BILINEAR and NEAREST_F32 as gpu_support.samplings_of has them, on the P2 and OFFSET sweeps."""
    return gs.samplings_of(variant, nearest_only) if c.sweep in ("P2", "OFFSET") else (0,)


def frame_is(fb, want_rgba, what):
    same_frame(np.ascontiguousarray(fb), want_rgba, what)


def records_are(got, want, what):
    """same_records, a NaN equal to a NaN (the sign and payload of a generated NaN are the machine's)."""
    got, want = got.copy(), np.array(want)
    for f in ("point", "entry_d"):
        both = np.isnan(got[f]) & np.isnan(want[f])
        got[f][both] = 0.0
        want[f][both] = 0.0
    same_records(got, want, what)


def floats_are(got, want, what):
    """float32 planes as bits, a NaN equal to a NaN."""
    g = np.ascontiguousarray(got, dtype=np.float32).reshape(-1)
    w = np.ascontiguousarray(want, dtype=np.float32).reshape(-1)
    bad = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.size} floats differ; first {i}: got {g[i]!r}, want {w[i]!r}")


def members(sweep, proj):
    out = fs.sweep(sweep, proj)
    assert out
    return out


# ---- the core families: every member of every sweep, outside and inside, every kernel variant ----
@pytest.mark.parametrize("sweep,proj", SWEEP_PROJ, ids=SWEEP_PROJ_IDS)
def test_trace_rays(world, sweep, proj):
    """The outside camera's rays and the rays no camera makes (interior origins miss: the rule is off), whole records."""
    R = world.R
    for c in members(sweep, proj):
        scene = world.scene(c)
        for variant in KERNEL_VARIANTS:
            with kernel_variant(variant):
                for sampling in samplings(c, variant):
                    got, st = scene.trace_rays(R.rays(c, False), c.cam_step, bg=BG, sampling=sampling, stats=True)
                    want = R.primary(c, False, sampling)
                    records_are(got, want, f"{c} {variant} sampling {sampling}: camera rays")
                    assert (st.rays, st.steps, st.capped) == (want.shape[0], int(want["steps"].sum()), 0), (c, variant)
                    with env(HMRM_STEP_CAP=fs.ODD_CAP):
                        odd = scene.trace_rays(R.odd_rays(c), c.cam_step, bg=BG, sampling=sampling, allow_capped=True)
                    records_are(odd, R.odd_records(c, sampling, False), f"{c} {variant} sampling {sampling}: odd rays")


@pytest.mark.parametrize("sweep,proj", SWEEP_PROJ, ids=SWEEP_PROJ_IDS)
def test_trace_segments(world, sweep, proj):
    """Both cameras' rays under the interior rule with max_steps = 25 and per-ray limits; the odd rays under the rule."""
    R = world.R
    for c in members(sweep, proj):
        scene = world.scene(c)
        for variant in KERNEL_VARIANTS:
            with kernel_variant(variant):
                for sampling in samplings(c, variant):
                    for inside in (False, True):
                        got = scene.trace_segments(R.rays(c, inside), c.cam_step, bg=BG, sampling=sampling, interior=True, max_steps=25,
                                                   per_ray_max_steps=R.limits(c, inside))
                        records_are(got, R.segments(c, inside, sampling), f"{c} {variant} sampling {sampling} inside {inside}: segments")
                    with env(HMRM_STEP_CAP=fs.ODD_CAP):
                        odd = scene.trace_segments(R.odd_rays(c), c.cam_step, bg=BG, sampling=sampling, interior=True, allow_capped=True)
                    records_are(odd, R.odd_records(c, sampling, True), f"{c} {variant} sampling {sampling}: odd rays, interior")


@pytest.mark.parametrize("sweep,proj", SWEEP_PROJ, ids=SWEEP_PROJ_IDS)
def test_render_and_render_interior(world, sweep, proj):
    """The inside camera under hmrm_render_interior, the outside one under both entries (its origins are outside: one frame)."""
    R = world.R
    for c in members(sweep, proj):
        scene = world.scene(c)
        for variant in KERNEL_VARIANTS:
            with kernel_variant(variant):
                for sampling in samplings(c, variant):
                    what = f"{c} {variant} sampling {sampling}"
                    frame_is(scene.render_interior(c.camera(True, sampling)), R.primary(c, True, sampling)["rgba"], what + " interior")
                    frame_is(scene.render_interior(c.camera(False, sampling)), R.primary(c, False, sampling)["rgba"], what + " interior, outside")
                    fb, st, _steps, _entry = scene.render_stats(c.camera(False, sampling))
                    want = R.primary(c, False, sampling)
                    frame_is(fb, want["rgba"], what + " render, instrumented")
                    frame_is(scene.render(c.camera(False, sampling)), want["rgba"], what + " render")
                    assert (st.rays, st.steps, st.capped) == (want.shape[0], int(want["steps"].sum()), 0), what
                    if variant == "leap" and sampling == 0:
                        r, hit = R.ranges(c, False)
                        print(f"{c.name:24s} steps {st.steps:7d} leap_attempts {st.leap_attempts:6d} leaps {st.leaps:6d} groups {st.groups:6d} "
                              f"leaped_steps {st.leaped_steps:7d} shadowed {fs.lit_counts(R.lit(c, False))[0]:4d} "
                              f"wet {fs.water_counts(R.water(c, False))[0]:4d} levels {fs.level_count(R.shaded(c, False)):3d} "
                              f"non-finite ranges {int((~np.isfinite(r[hit])).sum()):4d}")


@pytest.mark.parametrize("sweep,proj", SWEEP_PROJ, ids=SWEEP_PROJ_IDS)
def test_render_lit(world, sweep, proj):
    R = world.R
    for c in members(sweep, proj):
        scene = world.scene(c)
        for variant in KERNEL_VARIANTS:
            with kernel_variant(variant):
                for sampling in samplings(c, variant):
                    for inside in (False, True):
                        fb = scene.render_lit(c.camera(inside, sampling), c.sun(inside))
                        frame_is(fb, R.lit(c, inside, sampling)["rgba"], f"{c} {variant} sampling {sampling} inside {inside}: lit")


@pytest.mark.parametrize("sweep,proj", SWEEP_PROJ, ids=SWEEP_PROJ_IDS)
def test_render_shaded(world, sweep, proj):
    """HMRM_SHADE_DIFFUSE, and HMRM_SHADE_DIFFUSE | HMRM_SHADE_NO_SHADOWS."""
    R = world.R
    for c in members(sweep, proj):
        scene = world.scene(c)
        for variant in KERNEL_VARIANTS:
            with kernel_variant(variant):
                for sampling in samplings(c, variant):
                    for inside in (False, True):
                        for shadows in (True, False):
                            fb = scene.render_shaded(c.camera(inside, sampling), c.sun(inside), diffuse=True, shadows=shadows)
                            frame_is(fb, R.shaded(c, inside, sampling, shadows)["rgba"],
                                     f"{c} {variant} sampling {sampling} inside {inside} shadows {shadows}: shaded")


@pytest.mark.parametrize("sweep", fs.SWEEPS)
def test_cell_map(world, sweep):
    """One direction and one point target, status bytes and HMRM_MAP_WEIGHT | HMRM_MAP_DIFFUSE (a cell map has no camera: the
    orthographic members are every member of the sweep)."""
    R = world.R
    for c in members(sweep, 3):
        scene = world.scene(c)
        for variant in KERNEL_VARIANTS:
            with kernel_variant(variant):
                for sampling in samplings(c, variant, LITERAL_NEAREST):
                    for point in (False, True):
                        target, step, lift, limit = R.cell_target(c, point)
                        what = f"{c} {variant} sampling {sampling} point {point}"
                        got = scene.cell_map(target, step, lift=lift, max_steps=limit, point=point, sampling=sampling, ambient=AMBIENT)
                        same_cells(got, R.cell_status(c, point, sampling), what + ": status", np.uint8)
                        got = scene.cell_map(target, step, lift=lift, max_steps=limit, point=point, weight=True, diffuse=True,
                                             sampling=sampling, ambient=AMBIENT)
                        same_cells(got, R.cell_weight(c, point, sampling), what + ": weight", np.uint8)


@pytest.mark.parametrize("sweep,proj", SWEEP_PROJ, ids=SWEEP_PROJ_IDS)
def test_render_geometry(world, sweep, proj):
    """All four planes; the float planes as bits."""
    R = world.R
    for c in members(sweep, proj):
        scene = world.scene(c)
        for variant in KERNEL_VARIANTS:
            with kernel_variant(variant):
                for sampling in samplings(c, variant, LITERAL_NEAREST):
                    for inside in (False, True):
                        want = R.planes(c, inside, sampling)
                        got = scene.render_geometry(c.camera(inside, sampling), interior=inside)
                        what = f"{c} {variant} sampling {sampling} inside {inside}: plane "
                        frame_is(got["rgba"], want["rgba"], what + "rgba")
                        assert got["cell"].reshape(-1).tobytes() == want["cell"].tobytes(), what + "cell"
                        floats_are(got["range"], want["range"], what + "range")
                        floats_are(got["slope"], want["slope"], what + "slope")


@pytest.mark.parametrize("sweep,proj", SWEEP_PROJ, ids=SWEEP_PROJ_IDS)
def test_render_water(world, sweep, proj):
    R = world.R
    for c in members(sweep, proj):
        scene = world.scene(c)
        for variant in KERNEL_VARIANTS:
            with kernel_variant(variant):
                for sampling in samplings(c, variant):
                    for inside in (False, True):
                        fb = scene.render_water(c.camera(inside, sampling), R.water_of(c, inside))
                        frame_is(fb, R.water(c, inside, sampling)["rgba"], f"{c} {variant} sampling {sampling} inside {inside}: water")


@pytest.mark.parametrize("sweep,proj", SWEEP_PROJ, ids=SWEEP_PROJ_IDS)
def test_render_haze(world, sweep, proj):
    """Plain, and with HMRM_HAZE_SKY."""
    R = world.R
    for c in members(sweep, proj):
        scene = world.scene(c)
        for variant in KERNEL_VARIANTS:
            with kernel_variant(variant):
                for sampling in samplings(c, variant, LITERAL_NEAREST):
                    for inside in (False, True):
                        for sky in (False, True):
                            fb = scene.render_haze(c.camera(inside, sampling), R.haze_of(c, inside, sky), R.table)
                            frame_is(fb, R.haze(c, inside, sampling, sky)["rgba"], f"{c} {variant} sampling {sampling} inside {inside} sky {sky}: haze")


@pytest.mark.parametrize("k", [-145, -140, 123])
@pytest.mark.parametrize("proj", [2, 3], ids=["sph", "ortho"])
def test_plain_frame_on_denormal_and_huge_float_tables(world, proj, k):
    """hmrm_render under HMRM_NEAREST_F32 where every float threshold is a denormal (2^-140, 2^-145) and just below the float
    maximum (2^123): frame, steps and distance() against the replay's records.  tests/world_scale.py's sweep jumps over this band."""
    R, c = world.R, fs.p2(proj, k)
    scene, cam, want = world.scene(c), c.camera(False, 2), R.primary(c, False, 2)
    assert (want["status"] == lr.HIT).sum() >= 100
    for variant in ("leap", "group", "simple"):
        with kernel_variant(variant):
            fb, st, steps, entry = scene.render_stats(cam, per_pixel=True)
            frame_is(fb, want["rgba"], f"{c} {variant}")
            assert np.array_equal(steps.reshape(-1).astype(np.int64), want["steps"].astype(np.int64)), (c, variant)
            e, w = np.ascontiguousarray(entry, dtype=np.float64).reshape(-1), want["entry_d"]
            assert ((e.view(np.uint64) == w.view(np.uint64)) | (np.isnan(e) & np.isnan(w))).all(), (c, variant)
            assert st.steps == int(want["steps"].sum()) and st.capped == 0


# ---- the compositions: the production kernel, each sweep's ends and middle ----
def special(sweep, proj):
    return ws.ends_and_middle(members(sweep, proj))


@pytest.mark.parametrize("sweep,proj", SWEEP_PROJ, ids=SWEEP_PROJ_IDS)
def test_lit_sum_baked_and_water_lit(world, sweep, proj):
    """hmrm_render_lit_sum with K = 3 (both planes), hmrm_render_baked under a hillshade baked by hmrm_scene_bake_light, and
    hmrm_render_water_lit."""
    R = world.R
    with kernel_variant("leap"):
        for c in special(sweep, proj):
            scene = world.scene(c)
            for inside in (False, True):
                cam, what = c.camera(inside), f"{c} inside {inside}"
                want = R.lit_sum(c, inside)
                fb, light = scene.render_lit_sum(cam, c.sun(inside), R.sum_dirs(c), diffuse=True, shadows=True, light=True)
                frame_is(fb, want["rgba"], what + ": lit sum")
                assert light.reshape(-1).tobytes() == want["light"].tobytes(), what + ": light plane"
                fb = scene.render_water_lit(cam, R.water_of(c, inside), c.sun(inside), diffuse=True, shadows=True)
                frame_is(fb, R.water_lit(c, inside)["rgba"], what + ": water lit")
            try:
                scene.bake_light([c.cell_dir], c.cell_step, weight=True, diffuse=True, ambient=AMBIENT)
                plane, full_scale = scene.light()
                assert full_scale == 255 and plane.tobytes() == R.baked_plane(c).tobytes(), f"{c}: the baked plane"
                for inside in (False, True):
                    frame_is(scene.render_baked(c.camera(inside), interior=inside), R.baked(c, inside)["rgba"], f"{c} inside {inside}: baked")
            finally:
                scene.clear_light()


@pytest.mark.parametrize("sweep,proj", SWEEP_PROJ, ids=SWEEP_PROJ_IDS)
def test_antialiased_factor_2(world, sweep, proj):
    """hmrm_render_shaded_aa, hmrm_render_water_aa and hmrm_render_haze with factor 2: the 80 x 60 super frame's replay, every
    sample shaded, mirrored or hazed on its own, box-filtered."""
    R = world.R
    with kernel_variant("leap"):
        for c in special(sweep, proj):
            scene = world.scene(c)
            for inside in (False, True):
                cam, what = c.camera(inside), f"{c} inside {inside}"
                sup = lambda want: aa_box.box_filter(np.ascontiguousarray(want["rgba"]).reshape(2 * FRAME_H, 2 * FRAME_W, 4), 2)
                frame_is(scene.render_shaded(cam, c.sun(inside), diffuse=True, shadows=True, aa=2),
                         sup(R.shaded(c, inside, width=2 * FRAME_W, height=2 * FRAME_H)), what + ": shaded aa")
                frame_is(scene.render_water_aa(cam, R.water_of(c, inside), factor=2),
                         sup(R.water(c, inside, width=2 * FRAME_W, height=2 * FRAME_H)), what + ": water aa")
                frame_is(scene.render_haze(cam, R.haze_of(c, inside, True), R.table, factor=2),
                         hr.filtered(R.haze(c, inside, sky=True, factor=2), FRAME_W, FRAME_H, 2), what + ": haze aa")


@pytest.mark.parametrize("sweep,proj", SWEEP_PROJ, ids=SWEEP_PROJ_IDS)
def test_views_and_device_forms(world, sweep, proj):
    """hmrm_render_views of the case's two cameras and a third under the interior rule; hmrm_render_haze_device and
    hmrm_render_water_device into torch tensors on a caller stream."""
    import torch
    R = world.R
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    d_table = torch.from_numpy(np.array(R.table)).cuda()
    with kernel_variant("leap"):
        for c in special(sweep, proj):
            scene = world.scene(c)
            got = scene.render_views(R.view_cameras(c), interior=True)
            want = R.views(c)
            for v in range(3):
                frame_is(got[v], want[v], f"{c}: view {v}")
            for inside in (False, True):
                cam = c.camera(inside)
                t = torch.zeros((FRAME_H, FRAME_W), dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                scene.render_haze_device(cam, R.haze_of(c, inside), d_table.data_ptr(), t.data_ptr(), FRAME_W * 4, stream=stream.cuda_stream)
                assert scene.take_capped(stream.cuda_stream) == 0  # (waits for the stream)
                frame_is(t.cpu().numpy().view(np.uint8).reshape(FRAME_H, FRAME_W, 4), R.haze(c, inside)["rgba"], f"{c} inside {inside}: haze, device")
                t.zero_()
                torch.cuda.synchronize()
                scene.render_water_device(cam, R.water_of(c, inside), t.data_ptr(), FRAME_W * 4, stream=stream.cuda_stream)
                assert scene.take_capped(stream.cuda_stream) == 0
                frame_is(t.cpu().numpy().view(np.uint8).reshape(FRAME_H, FRAME_W, 4), R.water(c, inside)["rgba"], f"{c} inside {inside}: water, device")
