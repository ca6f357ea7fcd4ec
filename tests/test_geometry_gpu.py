"""Geometry frames on the GPU (hmrm_render_geometry, hmrm_render_geometry_device; include/hmrm.h).  Every plane is compared
BYTEWISE with tests/geometry_replay.py, the definition in numpy, which tests/test_geometry_cpu.py pins to a scalar loop and to a
ramp's analytic gradient; one test pins the kernels to hmrm_trace_rays / hmrm_trace_segments records and the device's own
threshold table without the replay's march.  Map, grid widths and cameras are those of tests/segment_cases.py at 40 x 30 unless
said otherwise."""
import functools

import numpy as np
import pytest

import geometry_cases as gc
import geometry_replay as gr
import gpu_support as gs
import segment_cases as sc
from gpu_support import KERNEL_VARIANTS, PROJ_IDS, env, gpu, kernel_variant
from segment_cases import BG, GRID_WIDTHS, GW_IDS, MAP_H, MAP_W

pytestmark = pytest.mark.gpu

PLANES = ("rgba", "cell", "range", "slope")
ELEM = dict(rgba=4, cell=4, range=4, slope=8)
samplings_of = functools.partial(gs.samplings_of, nearest_only=("rec", "simple"))  # (the literal loop too: nearest sampling only)


class World(gs.Scenes, gc.Replays):
    pass


world = gs.world_fixture(World)


def same_planes(got, want, width, what, names=PLANES):
    """Every plane of `got` ((H, W[, k]) arrays) against the replay's flat ones, byte for byte."""
    for name in names:
        g = np.ascontiguousarray(got[name])
        h = g.shape[0]
        w = np.ascontiguousarray(want[name]).reshape(g.shape)
        if g.tobytes() != w.tobytes():
            diff = (g.reshape(h, width, -1).view(np.uint8) != w.reshape(h, width, -1).view(np.uint8)).any(axis=2)
            y, x = np.argwhere(diff)[0]
            raise AssertionError(f"{what}: plane {name}: {int(diff.sum())} of {h * width} pixels differ; first ({x}, {y}): got {g[y, x]}, want {w[y, x]}")


# ---- 1. the base cases: outside and inside x 3 projections x 3 grid widths x 4 variants x their samplings ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_geometry_frame_is_the_replay(world, proj, variant, gw):
    gpu, scene = world.gpu, world.scenes[gw]
    with kernel_variant(variant):
        for inside in (False, True):
            for sampling in samplings_of(variant):
                want, prim = world.planes(gw, proj, sampling, inside)
                hits, misses, capped, ranges, cells = gr.counts(want, prim)
                assert hits >= 100 and misses >= 100 and capped == 0 and ranges >= 80 and cells >= 100, (hits, misses, capped, ranges, cells)
                got = scene.render_geometry(sc.camera(gpu, gw, proj, inside, sampling), interior=inside)
                same_planes(got, want, 40, f"proj {proj} {variant} gw {gw} sampling {sampling} inside {inside}")


# ---- 2. ragged tiles ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_geometry_odd_frame(world, proj, variant):
    """101 x 67: no multiple of the 8 x 16 tile, more than one workgroup each way."""
    gw = 0.5
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            want, prim = world.planes(gw, proj, sampling, False, 101, 67)
            hits, misses, capped, _ranges, _cells = gr.counts(want, prim)
            assert hits >= 800 and misses >= 3900 and capped == 0, (hits, misses, capped)
            got = world.scenes[gw].render_geometry(sc.camera(world.gpu, gw, proj, False, sampling, width=101, height=67))
            same_planes(got, want, 101, f"101 x 67 proj {proj} {variant} sampling {sampling}")


# ---- 3. identities, byte for byte ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_rgba_plane_is_the_frame(world, variant):
    """The rgba plane is hmrm_render's frame; with the flag and the inside camera hmrm_render_interior's."""
    gpu = world.gpu
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            gw = GRID_WIDTHS[proj - 1]
            scene = world.scenes[gw]
            for sampling in samplings_of(variant):
                cam, icam = sc.camera(gpu, gw, proj, False, sampling), sc.camera(gpu, gw, proj, True, sampling)
                assert scene.render_geometry(cam)["rgba"].tobytes() == scene.render(cam).tobytes(), (proj, sampling)
                assert scene.render_geometry(icam, interior=True)["rgba"].tobytes() == scene.render_interior(icam).tobytes(), (proj, sampling)
                # (without the flag an inside perspective / spherical camera misses everything, as hmrm_render's does)
                assert scene.render_geometry(icam)["rgba"].tobytes() == scene.render(icam).tobytes(), (proj, sampling)


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_planes_are_trace_records_plus_numpy(world, proj, variant):
    """hmrm_trace_rays / hmrm_trace_segments of the oracle's camera rays (cell and point of every hit, from the GPU), the
    threshold table read back from the device, the planes in numpy: no march of the replay's."""
    gpu = world.gpu
    gw = GRID_WIDTHS[proj - 1]
    scene, params = world.scenes[gw], world.params[gw]
    _recs, thr = scene.read_records()
    assert params.min_height == 0.0 and thr.shape == (MAP_H, MAP_W)  # (thr + 0.0 is thr: it stands in for heightmap_buf below)
    with kernel_variant(variant):
        for inside in (False, True):
            rays = world.rays(gw, proj, inside)
            for sampling in samplings_of(variant):
                if inside:
                    primary = scene.trace_segments(rays, 0.2 * gw, bg=BG, sampling=sampling, interior=True)
                else:
                    primary = scene.trace_rays(rays, 0.2 * gw, bg=BG, sampling=sampling)
                want = gr.planes(primary, rays, thr, params, sampling)
                assert (primary["status"] == gr.HIT).sum() >= 100
                got = scene.render_geometry(sc.camera(gpu, gw, proj, inside, sampling), interior=inside)
                same_planes(got, want, 40, f"records + table proj {proj} {variant} sampling {sampling} inside {inside}")


@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_one_plane_alone_and_padded_rows(world, variant):
    """A call with one plane alone writes that plane's same bytes; rows with a stride larger than the width keep their padding
    bytes; a poisoned device buffer handed over for no plane stays untouched."""
    import torch
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    with kernel_variant(variant):
        for proj, inside, sampling in ((1, False, 0), (3, True, samplings_of(variant)[-1]), (2, False, samplings_of(variant)[len(samplings_of(variant)) // 2])):
            cam = sc.camera(gpu, gw, proj, inside, sampling)
            want, _prim = world.planes(gw, proj, sampling, inside)
            for name in PLANES:
                got = scene.render_geometry(cam, interior=inside, **{k: k == name for k in PLANES})
                assert list(got) == [name]
                same_planes(got, want, 40, f"{name} alone, proj {proj} {variant}", names=(name,))
            padded = scene.render_geometry(cam, interior=inside, pad_px=5)
            for name in PLANES:
                rows = padded[name].reshape(30, 45, -1)
                assert (rows[:, 40:].view(np.uint8) == 0xA5).all(), name
                same_planes({name: np.ascontiguousarray(rows[:, :40])}, want, 40, f"padded rows, proj {proj} {variant}", names=(name,))
            # device entry, two planes of four: the poisoned buffers of the other two are never written
            bufs = {k: torch.full((30 * 40 * ELEM[k] + 64,), 0xA5, dtype=torch.uint8, device="cuda") for k in PLANES}
            torch.cuda.synchronize()
            scene.render_geometry_device(cam, cell=(bufs["cell"].data_ptr(), 160), slope=(bufs["slope"].data_ptr(), 320), interior=inside)
            assert scene.take_capped(0) == 0
            torch.cuda.synchronize()
            host = {k: v.cpu().numpy() for k, v in bufs.items()}
            assert (host["rgba"] == 0xA5).all() and (host["range"] == 0xA5).all()
            for k in ("cell", "slope"):
                assert (host[k][30 * 40 * ELEM[k]:] == 0xA5).all()
                assert host[k][:30 * 40 * ELEM[k]].tobytes() == np.ascontiguousarray(want[k]).tobytes(), (k, proj, variant)


# ---- 4. the step cap ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_capped_rays_are_no_hits_in_any_plane(world, variant):
    """One frame under a small HMRM_STEP_CAP: the rays it stops are non-hits in every plane -- cell -1, range +inf, slope +0, the
    miss shade -- and the host entry returns HMRM_E_NOTERM with valid planes."""
    gpu, gw, proj, cap = world.gpu, 0.5, 1, 60
    scene = world.scenes[gw]
    with kernel_variant(variant), env(HMRM_STEP_CAP=cap):
        for sampling in samplings_of(variant):
            want, prim = world.planes(gw, proj, sampling, False, step_cap=cap)
            hits, _misses, capped, _ranges, _cells = gr.counts(want, prim)
            assert capped >= 20 and hits >= 100, (capped, hits)
            stopped = prim["status"] == 2
            assert (want["cell"][stopped] == -1).all() and (want["range"][stopped].view(np.uint32) == gr.INF_BITS).all()
            assert (want["slope"][stopped].view(np.uint32) == 0).all()
            cam = sc.camera(gpu, gw, proj, False, sampling)
            with pytest.raises(gpu.HmrmError) as e:
                scene.render_geometry(cam)
            assert e.value.code == gpu.HMRM_E_NOTERM and f"{capped} ray(s)" in str(e.value)
            same_planes(scene.render_geometry(cam, allow_capped=True), want, 40, f"capped frame {variant} sampling {sampling}")


# ---- 5. the device entry ----
def test_device_entry_on_a_stream(world):
    """Planes in torch tensors, a non-default torch stream, take_capped for that stream; hmrm_debug_kernel_choice and a
    following plain frame are as they would have been."""
    import torch
    gpu, gw = world.gpu, 0.05
    scene = world.scenes[gw]
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    for proj, inside, sampling in ((1, False, 0), (2, True, 1), (3, True, 2)):
        cam = sc.camera(gpu, gw, proj, inside, sampling)
        want, _prim = world.planes(gw, proj, sampling, inside)
        plain = sc.camera(gpu, gw, proj, False, sampling)
        before, choice = scene.render(plain).tobytes(), scene.kernel_choice()
        t = dict(rgba=torch.zeros((30, 48), dtype=torch.int32, device="cuda"), cell=torch.zeros((30, 40), dtype=torch.int32, device="cuda"),
                 range=torch.zeros((30, 44), dtype=torch.float32, device="cuda"), slope=torch.zeros((30, 40, 2), dtype=torch.float32, device="cuda"))
        torch.cuda.synchronize()
        scene.render_geometry_device(cam, rgba=(t["rgba"].data_ptr(), 48 * 4), cell=(t["cell"].data_ptr(), 160), range=(t["range"].data_ptr(), 44 * 4),
                                     slope=(t["slope"].data_ptr(), 320), interior=inside, stream=stream.cuda_stream)
        assert scene.take_capped(stream.cuda_stream) == 0  # (waits for the stream)
        got = dict(rgba=t["rgba"].cpu().numpy()[:, :40].copy().view(np.uint8).reshape(30, 40, 4), cell=t["cell"].cpu().numpy(),
                   range=np.ascontiguousarray(t["range"].cpu().numpy()[:, :40]), slope=t["slope"].cpu().numpy())
        same_planes(got, want, 40, f"device entry proj {proj} sampling {sampling}")
        assert (t["rgba"].cpu().numpy()[:, 40:] == 0).all() and (t["range"].cpu().numpy()[:, 40:] == 0).all()
        assert scene.kernel_choice() == choice and scene.render(plain).tobytes() == before
    # capped rays of a device call: reported through take_capped for its stream
    want, prim = world.planes(0.5, 1, 0, False, step_cap=60)
    capped = int((prim["status"] == 2).sum())
    d_range = torch.zeros((30, 40), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with env(HMRM_STEP_CAP=60):
        world.scenes[0.5].render_geometry_device(sc.camera(gpu, 0.5, 1, False, 0), range=(d_range.data_ptr(), 160), stream=stream.cuda_stream)
        assert world.scenes[0.5].take_capped(stream.cuda_stream, allow_capped=True) == capped >= 20
    assert d_range.cpu().numpy().tobytes() == want["range"].tobytes()


# ---- 6. CLI ----
def test_cli_range_map_key(world, tmp_path):
    """`range_map out.pfm`: a file that a PFM reader opens as the replay's range plane, outside and, with `interior on`, inside."""
    gpu, gw = world.gpu, 0.5
    rangep = str(tmp_path / "range.pfm")
    for inside in (False, True):
        cfgp, _, _ = gs.cli_config(gpu, world, tmp_path, gw, inside, f"range_map {rangep}\n" + ("interior on\n" if inside else ""))
        r = gs.run_hmap(gpu, cfgp)
        assert f"range_map {rangep}\n" in r.stdout and f"Saved range map at {rangep}\n" in r.stdout
        want, _prim = world.planes(gw, 1, 0, inside)
        back = gr.read_pfm(rangep)
        assert back.shape == (30, 40) and back.tobytes() == want["range"].tobytes(), inside
