"""Haze frames on the GPU (hmrm_render_haze, hmrm_render_haze_device; include/hmrm.h).  Every frame is compared BYTEWISE with
tests/haze_replay.py, the definition in numpy, which tests/test_haze_cpu.py pins to a scalar loop; one test pins the kernels to
hmrm_trace_rays / hmrm_trace_segments records without the replay's march.  Map, grid widths and cameras are those of
tests/segment_cases.py at 40 x 30 unless said otherwise; every camera's haze is picked from its own replay (tests/haze_cases.py),
and every replay-based case first asserts that replay's conditions: both kinds of pixel, hits on both clamps of the table and in
between, a haze that shows."""
import functools

import numpy as np
import pytest

import gpu_support as gs
import haze_cases as hc
import haze_replay as hr
import segment_cases as sc
from gpu_support import KERNEL_VARIANTS, PROJ_IDS, env, gpu, kernel_variant, same_frame
from haze_cases import COLOR, ENTRIES
from segment_cases import BG, GRID_WIDTHS, GW_IDS

pytestmark = pytest.mark.gpu

samplings_of = functools.partial(gs.samplings_of, nearest_only=("rec", "simple"))  # (the literal loop too: nearest sampling only)


class World(gs.Scenes, hc.Replays):
    def filtered(self, gw, proj, sampling, n, inside=False, sky=False, width=20, height=15, **kw):
        """The replayed antialiased frame: the haze frame of the n x n larger camera, every sample hazed, box-filtered."""
        want = self.haze(gw, proj, sampling, inside, width, height, sky=sky, factor=n, **kw)
        return hr.filtered(want, width, height, n), want


world = gs.world_fixture(World)


def sky_of(*keys):
    """The sky flag alternates over the cases."""
    return sum(int(k) if isinstance(k, (bool, int)) else int(k * 20) for k in keys) % 2 == 1


# ---- 1. the base cases: outside and inside x 3 projections x 3 grid widths x 4 variants x their samplings ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_haze_frame_is_the_replay(world, proj, variant, gw):
    gpu, scene = world.gpu, world.scenes[gw]
    with kernel_variant(variant):
        for inside in (False, True):
            for sampling in samplings_of(variant):
                sky = sky_of(proj, sampling, inside, gw)
                want = world.haze(gw, proj, sampling, inside, sky=sky)
                hc.check(want)
                got = scene.render_haze(sc.camera(gpu, gw, proj, inside, sampling), world.haze_of(gw, proj, sampling, inside, sky), world.table)
                same_frame(got, want["rgba"], f"proj {proj} {variant} gw {gw} sampling {sampling} inside {inside} sky {sky}")


# ---- 2. ragged tiles ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_haze_odd_frame(world, proj, variant):
    """101 x 67: no multiple of the 8 x 16 tile, more than one workgroup each way."""
    gw = 0.5
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            sky = sky_of(proj, sampling)
            want = world.haze(gw, proj, sampling, False, 101, 67, sky=sky)
            hc.check(want)
            got = world.scenes[gw].render_haze(sc.camera(world.gpu, gw, proj, False, sampling, width=101, height=67),
                                               world.haze_of(gw, proj, sampling, False, sky), world.table)
            same_frame(got, want["rgba"], f"101 x 67 proj {proj} {variant} sampling {sampling}")


# ---- 3. antialiasing: every sample hazed on its own, then the box filter ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("factor", [2, 4])
def test_antialiased_frame_is_the_filtered_replay(world, factor, variant):
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            for inside in (False, True):
                for sampling in samplings_of(variant):
                    sky = sky_of(proj, sampling, inside, factor)
                    frame, want = world.filtered(gw, proj, sampling, factor, inside, sky)
                    hc.check(want)
                    cam = sc.camera(gpu, gw, proj, inside, sampling, width=20, height=15)
                    same_frame(scene.render_haze(cam, world.haze_of(gw, proj, sampling, inside, sky), world.table, factor=factor), frame,
                               f"aa {factor} {variant} proj {proj} sampling {sampling} inside {inside} sky {sky}")


@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_factor_eight(world, proj):
    """Factor 8, one camera per projection (bilinear, nearest f32, and nearest through the literal loop)."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    sampling, inside, variant = ((1, False, None), (2, True, None), (0, False, "simple"))[proj - 1]
    frame, want = world.filtered(gw, proj, sampling, 8, inside, True)
    hc.check(want)
    with kernel_variant(variant):
        cam = sc.camera(gpu, gw, proj, inside, sampling, width=20, height=15)
        same_frame(scene.render_haze(cam, world.haze_of(gw, proj, sampling, inside, True), world.table, factor=8), frame, f"aa 8 proj {proj}")
        with pytest.raises(gpu.HmrmError) as e:
            scene.render_haze(cam, world.haze_of(gw, proj, sampling, inside), world.table, factor=3)
        assert e.value.code == gpu.HMRM_E_ARG and "antialias factor" in str(e.value)


# ---- 4. identities, byte for byte ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_identities(world, variant):
    """A table of zeros is hmrm_render / hmrm_render_interior / hmrm_render_aa, with and without the sky flag; a table of 255s with
    the sky flag is a frame of the haze colour; without the flag the pixels that did not hit are hmrm_render's and the hits are
    the haze colour."""
    gpu = world.gpu
    zeros, full = np.zeros(ENTRIES, dtype=np.uint8), np.full(ENTRIES, 255, dtype=np.uint8)
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            gw = GRID_WIDTHS[proj - 1]
            scene = world.scenes[gw]
            for sampling in samplings_of(variant):
                cam, icam = sc.camera(gpu, gw, proj, False, sampling), sc.camera(gpu, gw, proj, True, sampling)
                small = sc.camera(gpu, gw, proj, False, sampling, width=20, height=15)
                for sky in (False, True):
                    hz, ihz = world.haze_of(gw, proj, sampling, False, sky), world.haze_of(gw, proj, sampling, True, sky)
                    assert scene.render_haze(cam, hz, zeros).tobytes() == scene.render(cam).tobytes(), (proj, sampling, sky)
                    assert scene.render_haze(icam, ihz, zeros).tobytes() == scene.render_interior(icam).tobytes(), (proj, sampling, sky)
                    assert scene.render_haze(small, hz, zeros, factor=2).tobytes() == scene.render_aa(small, 2).tobytes(), (proj, sampling, sky)
                uniform = np.empty((30, 40, 4), dtype=np.uint8)
                uniform[:] = COLOR + (255,)
                assert scene.render_haze(cam, world.haze_of(gw, proj, sampling, False, True), full).tobytes() == uniform.tobytes()
                want = world.haze(gw, proj, sampling, False)
                hc.check(want)
                hit = want["hit"].reshape(30, 40)
                got, plain = scene.render_haze(cam, world.haze_of(gw, proj, sampling, False, False), full), scene.render(cam)
                assert got[~hit].tobytes() == plain[~hit].tobytes() and got[hit].tobytes() == uniform[hit].tobytes(), (proj, sampling)
                # (and with the real table the non-hit pixels are hmrm_render's)
                got = scene.render_haze(cam, world.haze_of(gw, proj, sampling, False, False), world.table)
                assert got[~hit].tobytes() == plain[~hit].tobytes() and got[hit].tobytes() != plain[hit].tobytes()


# ---- 5. no march of the replay's ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_frame_is_trace_records_plus_numpy(world, proj, variant):
    """hmrm_trace_rays / hmrm_trace_segments of the oracle's camera rays (point and pixel of every ray as doubles and bytes, from
    the GPU), then the range, the index and the blend in numpy."""
    gpu = world.gpu
    gw = GRID_WIDTHS[proj - 1]
    scene = world.scenes[gw]
    with kernel_variant(variant):
        for inside in (False, True):
            rays = world.rays(gw, proj, inside)
            for sampling in samplings_of(variant):
                if inside:
                    primary = scene.trace_segments(rays, 0.2 * gw, bg=BG, sampling=sampling, interior=True)
                else:
                    primary = scene.trace_rays(rays, 0.2 * gw, bg=BG, sampling=sampling)
                sky = sky_of(proj, sampling, inside)
                hz = world.haze_of(gw, proj, sampling, inside, sky)
                want = hr.frame(primary, rays, hz.start, hz.scale, world.table, COLOR, sky)
                assert want["hit"].sum() >= 100 and np.unique(want["index"][want["hit"]]).size >= 10
                got = scene.render_haze(sc.camera(gpu, gw, proj, inside, sampling), hz, world.table)
                same_frame(got, want["rgba"], f"records + numpy proj {proj} {variant} sampling {sampling} inside {inside}")


# ---- 6. the table's edges ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_table_edges(world, variant):
    """n = 1 and n = 4096; a start beyond every range (all hits at entry 0); a huge scale (all hits at entry n - 1); a NaN scale
    (entry 0); a negative scale.  The entries are told apart by their bytes."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    ramp = (np.arange(ENTRIES) * 4 + 3).astype(np.uint8)  # (entry 0: 3, entry 63: 255)
    with kernel_variant(variant):
        for proj, inside in ((1, False), (2, True), (3, False)):
            for sampling in samplings_of(variant):
                hc.check(world.haze(gw, proj, sampling, inside))
                cam = sc.camera(gpu, gw, proj, inside, sampling)
                base = world.haze_of(gw, proj, sampling, inside, proj == 2)
                flags = int(base.flags)
                fine = gpu.Haze.make(base.start, base.start + (ENTRIES / base.scale), 4096, COLOR, sky=proj == 2, interior=inside)
                cases = [("n = 1", gpu.Haze.raw(base.start, base.scale, 1, COLOR, flags), np.array([77], dtype=np.uint8), None),
                         ("n = 4096", fine, gpu.haze_table(gpu.HAZE_EXP2, 2.0, 4096), None),
                         ("start beyond", gpu.Haze.raw(1e9, base.scale, ENTRIES, COLOR, flags), ramp, 0),
                         ("huge scale", gpu.Haze.raw(0.0, 1e300, ENTRIES, COLOR, flags), ramp, ENTRIES - 1),
                         ("NaN scale", gpu.Haze.raw(base.start, float("nan"), ENTRIES, COLOR, flags), ramp, 0),
                         ("negative scale", gpu.Haze.raw(base.start + 1.0, -base.scale, ENTRIES, COLOR, flags), ramp, None)]
                for name, hz, table, everywhere in cases:
                    want = world.haze(gw, proj, sampling, inside, haze=hz, table=table)
                    if everywhere is not None:
                        assert (want["index"][want["hit"]] == everywhere).all(), name
                    same_frame(scene.render_haze(cam, hz, table), want["rgba"], f"{name}: proj {proj} {variant} sampling {sampling}")
                # (a camera's ranges are a step apart along each ray, so a few dozen of the 4096 entries are used: far ones among them)
                used = np.unique(world.haze(gw, proj, sampling, inside, haze=fine, table=cases[1][2])["index"])
                assert used.size >= 30 and (used > 1024).sum() >= 10 and used.max() == 4095


# ---- 7. padded rows ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_padded_rows_stay_poisoned(world, variant):
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    with kernel_variant(variant):
        for proj, inside, factor in ((1, False, 1), (3, True, 1), (2, False, 2)):
            sampling = samplings_of(variant)[-1]
            w, h = (40, 30) if factor == 1 else (20, 15)
            cam = sc.camera(gpu, gw, proj, inside, sampling, width=w, height=h)
            hz = world.haze_of(gw, proj, sampling, inside, True)
            if factor == 1:
                want = world.haze(gw, proj, sampling, inside, sky=True)
                frame = want["rgba"]
            else:
                frame, want = world.filtered(gw, proj, sampling, factor, inside, True)
            hc.check(want)
            rows = scene.render_haze(cam, hz, world.table, factor=factor, pad_px=5)
            assert rows.shape == (h, w + 5, 4) and (rows[:, w:] == 0xA5).all()
            same_frame(np.ascontiguousarray(rows[:, :w]), frame, f"padded rows proj {proj} {variant} factor {factor}")


# ---- 8. the device entry ----
def test_device_entry_on_a_stream(world):
    """The frame in a torch tensor with a wide stride, the table in device memory, a non-default torch stream, take_capped for
    that stream; hmrm_debug_kernel_choice and a following plain frame are as they would have been."""
    import torch
    gpu, gw = world.gpu, 0.05
    scene = world.scenes[gw]
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    d_table = torch.from_numpy(np.array(world.table)).cuda()
    for proj, inside, sampling, factor in ((1, False, 0, 1), (2, True, 1, 1), (3, True, 2, 1), (1, False, 1, 2), (3, True, 0, 4)):
        w, h = (40, 30) if factor == 1 else (20, 15)
        cam = sc.camera(gpu, gw, proj, inside, sampling, width=w, height=h)
        hz = world.haze_of(gw, proj, sampling, inside, proj != 2)
        if factor == 1:
            want = world.haze(gw, proj, sampling, inside, sky=proj != 2)
            frame = want["rgba"]
        else:
            frame, want = world.filtered(gw, proj, sampling, factor, inside, proj != 2)
        hc.check(want)
        plain = sc.camera(gpu, gw, proj, False, sampling)
        before, choice = scene.render(plain).tobytes(), scene.kernel_choice()
        t = torch.full((h, w + 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        scene.render_haze_device(cam, hz, d_table.data_ptr(), t.data_ptr(), (w + 8) * 4, factor=factor, stream=stream.cuda_stream)
        assert scene.take_capped(stream.cuda_stream) == 0  # (waits for the stream)
        host = t.cpu().numpy()
        same_frame(host[:, :w].copy().view(np.uint8).reshape(h, w, 4), frame, f"device entry proj {proj} sampling {sampling} factor {factor}")
        assert (host[:, w:] == 0x5A5A5A5A).all()
        assert scene.kernel_choice() == choice and scene.render(plain).tobytes() == before
    # the stride rule of the device form
    cam = sc.camera(gpu, gw, 1, False, 0)
    t = torch.zeros((30, 48), dtype=torch.int32, device="cuda")
    for stride in (40 * 4 - 4, 40 * 4 + 2):
        with pytest.raises(gpu.HmrmError) as e:
            scene.render_haze_device(cam, world.haze_of(gw, 1, 0), d_table.data_ptr(), t.data_ptr(), stride)
        assert e.value.code == gpu.HMRM_E_ARG and "stride_bytes" in str(e.value)
    with pytest.raises(gpu.HmrmError) as e:
        scene.render_haze(cam, world.haze_of(gw, 1, 0), world.table, pad_px=-1)
    assert e.value.code == gpu.HMRM_E_ARG and "stride_bytes" in str(e.value)


# ---- 9. the step cap ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_capped_rays_are_hazed_only_as_sky(world, variant):
    """One frame under HMRM_STEP_CAP=60: the rays it stops are non-hits -- untouched without the sky flag, blended at the table's
    last entry with it -- the host entry returns HMRM_E_NOTERM with the replayed count, the frame is the replay's; the device
    entry reports the count through take_capped."""
    import torch
    gpu, gw, proj, cap = world.gpu, 0.5, 1, 60
    scene = world.scenes[gw]
    with kernel_variant(variant), env(HMRM_STEP_CAP=cap):
        for sampling in samplings_of(variant):
            cam = sc.camera(gpu, gw, proj, False, sampling)
            prim = world.primary(gw, proj, sampling, False, step_cap=cap)
            stopped = prim["status"] == hr.CAPPED
            for sky in (False, True):
                want = world.haze(gw, proj, sampling, False, step_cap=cap, sky=sky)
                hc.check(want, capped_ok=True)
                assert want["capped"] == int(stopped.sum()) >= 20 and not want["hit"][stopped].any()
                if sky:
                    assert want["rgba"][stopped].tobytes() == hr.blend(prim["rgba"][stopped], COLOR, np.full(int(stopped.sum()), world.table[-1])).tobytes()
                    assert (want["rgba"][stopped] != prim["rgba"][stopped]).any()
                else:
                    assert want["rgba"][stopped].tobytes() == prim["rgba"][stopped].tobytes()
                hz = world.haze_of(gw, proj, sampling, False, sky)
                with pytest.raises(gpu.HmrmError) as e:
                    scene.render_haze(cam, hz, world.table)
                assert e.value.code == gpu.HMRM_E_NOTERM and f"{want['capped']} ray(s)" in str(e.value)
                same_frame(scene.render_haze(cam, hz, world.table, allow_capped=True), want["rgba"], f"capped frame {variant} sampling {sampling} sky {sky}")
        d_table = torch.from_numpy(np.array(world.table)).cuda()
        t = torch.zeros((30, 40), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        want = world.haze(gw, proj, 0, False, step_cap=cap, sky=True)
        scene.render_haze_device(sc.camera(gpu, gw, proj, False, 0), world.haze_of(gw, proj, 0, False, True), d_table.data_ptr(), t.data_ptr(), 160)
        assert scene.take_capped(0, allow_capped=True) == want["capped"]
        same_frame(t.cpu().numpy().view(np.uint8).reshape(30, 40, 4), want["rgba"], f"capped device frame {variant}")


# ---- 10. CLI ----
def test_cli_haze_keys(world, tmp_path):
    """`haze on` with the haze keys writes the replay's frame, with `antialias 2` and `interior on` the filtered one; beside
    `water on` and `shadows on` the key is ignored with its warning."""
    gpu, gw = world.gpu, 0.5
    cfgp, _, outp = gs.cli_config(gpu, world, tmp_path, gw, output=False)

    def run(body):
        cfgp.write_text(body)
        return gs.run_hmap(gpu, cfgp)

    def keys(hz, far, sky):
        return (f"haze on\nhaze_start {hz.start:.17g}\nhaze_far {far:.17g}\nhaze_law exp\nhaze_density {hc.DENSITY:.17g}\nhaze_entries {ENTRIES}\n"
                f"haze_color {COLOR[0]} {COLOR[1]} {COLOR[2]}\nhaze_sky {'on' if sky else 'off'}\n")

    def far_of(key):
        return world._params[key][1]

    hz = world.haze_of(gw, 1, 0, False, True)
    want = world.haze(gw, 1, 0, False, sky=True)
    hc.check(want)
    text = gs.cli_preamble(gw, tmp_path / "h.ppm", tmp_path / "c.png")
    r = run(text + f"output {outp}\n" + keys(hz, far_of((gw, 1, 0, False)), True))
    assert "haze on\n" in r.stdout and "rays with haze" in r.stdout and "ignored" not in r.stderr
    assert open(outp, "rb").read() == gpu.png_encode(np.ascontiguousarray(want["rgba"]).reshape(30, 40, 4))
    # antialias 2 and interior on, the inside camera, no sky
    ihz = world.haze_of(gw, 1, 0, True, False)
    frame, iwant = world.filtered(gw, 1, 0, 2, True, False)
    hc.check(iwant)
    text = gs.cli_preamble(gw, tmp_path / "h.ppm", tmp_path / "c.png", inside=True, proj=1, width=20, height=15)
    r = run(text + f"output {outp}\nantialias 2\ninterior on\n" + keys(ihz, far_of((gw, 1, 0, True)), False))
    assert "at antialias 2 under the interior rule" in r.stdout and "ignored" not in r.stderr
    assert open(outp, "rb").read() == gpu.png_encode(frame)
    # the warnings
    text = gs.cli_preamble(gw, tmp_path / "h.ppm", tmp_path / "c.png")
    plain = gpu.png_encode(np.ascontiguousarray(world.primary(gw, 1, 0)["rgba"].reshape(30, 40, 4)))
    r = run(text + f"output {outp}\n" + keys(hz, far_of((gw, 1, 0, False)), True) + "water on\nwater_level -1\n")
    assert "WARNING: haze is ignored with water\n" in r.stderr and "rays with haze" not in r.stdout
    assert open(outp, "rb").read() == plain  # (a level below every threshold: hmrm_render's frame)
    r = run(text + f"output {outp}\n" + keys(hz, far_of((gw, 1, 0, False)), True) + "shadows on\n")
    assert "WARNING: haze is ignored with shadows\n" in r.stderr and "rays with haze" not in r.stdout and "with sun shadows" in r.stdout
