"""View batches on the GPU (hmrm_render_views, hmrm_render_views_device; include/hmrm.h).  Every comparison is BYTEWISE.  The
expected frame of a plain view is the C oracle's, that of a view under the interior rule tests/segment_replay.py's
(tests/views_cases.py caches both); the same batches are also compared with N calls of hmrm_render / hmrm_render_interior on the
same scene.  Map and grid widths are those of tests/segment_cases.py; the seven cameras, which differ in everything a batch lets
differ, are described in tests/views_cases.py.  No case but the dedicated one produces a capped ray: views_cases.Expected.batch
asserts it of every expected batch."""
import functools

import numpy as np
import pytest

import gpu_support as gs
import views_cases as vc
from gpu_support import KERNEL_VARIANTS, PROJ_IDS, env, gpu, kernel_variant
from segment_cases import GRID_WIDTHS, GW_IDS
from views_cases import COUNTS, SIZES

pytestmark = pytest.mark.gpu

samplings_of = functools.partial(gs.samplings_of, nearest_only=("rec", "simple"))  # (the literal loop too: nearest sampling only)


class World(gs.Scenes, vc.Expected):
    def __init__(self, gpu, oracle):
        super().__init__(gpu, oracle)
        self._single = {}

    def singles(self, gw, proj, sampling, indices, width, height, interior):
        """The N single renders of the same cameras on the same scene (each rendered once, with whatever kernel was current)."""
        out = []
        for k in indices:
            key = (gw, proj, sampling, k, width, height, interior)
            if key not in self._single:
                cam = vc.camera(self.gpu, gw, proj, k, sampling, width, height)
                fb = self.scenes[gw].render_interior(cam) if interior else self.scenes[gw].render(cam)
                fb.setflags(write=False)
                self._single[key] = fb
            out.append(self._single[key])
        return np.stack(out)


world = gs.world_fixture(World)


def same_batch(got, want, what, named=()):
    """(n, H, W, 4) against (n, H, W, 4); the message names the first view that differs, and whether each of `named` does."""
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    bad = np.nonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0]
    k = int(bad[0])
    px = np.argwhere((got[k] != want[k]).any(axis=2))
    y, x = px[0]
    extra = "".join(f"; view {v}: {'differs' if v in set(bad.tolist()) else 'same'}" for v in named)
    raise AssertionError(f"{what}: {bad.size} of {got.shape[0]} views differ; first view {k}, {px.shape[0]} pixels, first ({x}, {y}): "
                         f"got {got[k, y, x]}, want {want[k, y, x]}{extra}")


# ---- 1. the base cases: 3 projections x 4 variants x 3 grid widths, their samplings, both rules, 4 view sizes x 4 batch sizes ----
@pytest.mark.parametrize("gw", GRID_WIDTHS, ids=GW_IDS)
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_batch_is_the_single_frames(world, proj, variant, gw):
    """Views of 8 x 16 (one tile), 9 x 17 (four tiles, mostly dead lanes), 1 x 1 and 24 x 33 (three tile rows per view, the last
    partial) in batches of 1, 2, 3 and 7 cameras, which start at another camera for every shape: the batch of 7 holds the camera
    inside the box, the one that sees only sky and -- spherical -- views that share column tables, row tables, both and neither."""
    scene = world.scenes[gw]
    with kernel_variant(variant):
        for sampling in samplings_of(variant):
            for interior in (False, True):
                for si, (w, h) in enumerate(SIZES):
                    for n in COUNTS:
                        idx = vc.batch_indices(n, first=(3 * si + n) % vc.N_CAMS)
                        what = f"proj {proj} {variant} gw {gw} sampling {sampling} interior {interior} {w} x {h} cameras {idx}"
                        want = world.batch(gw, proj, sampling, idx, w, h, interior)
                        got = scene.render_views(world.cameras(gw, proj, sampling, idx, w, h), interior=interior)
                        same_batch(got, want, what)
                        same_batch(world.singles(gw, proj, sampling, idx, w, h, interior), want, "single renders: " + what)


# ---- 2. a padded target ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_padded_target_is_left_alone(world, variant):
    """stride_bytes larger than a row and view_stride_bytes larger than a view, host form and device form: the frames are right
    and every byte of the padding keeps what it was prefilled with."""
    import torch
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    idx = vc.batch_indices(3, first=5)
    with kernel_variant(variant):
        for proj in (1, 2, 3):
            for w, h in ((9, 17), (24, 33)):
                cams = world.cameras(gw, proj, 0, idx, w, h)
                want = world.batch(gw, proj, 0, idx, w, h, True)
                got = scene.render_views(cams, interior=True, pad_px=3, pad_rows=2)
                assert got.shape == (3, h + 2, w + 3, 4)
                same_batch(np.ascontiguousarray(got[:, :h, :w]), want, f"padded host target {variant} proj {proj} {w} x {h}")
                assert (got[:, h:] == 0xA5).all() and (got[:, :, w:] == 0xA5).all()
                t = torch.full((3, h + 2, w + 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                scene.render_views_device(cams, t.data_ptr(), (w + 3) * 4, (h + 2) * (w + 3) * 4, interior=True)
                assert scene.take_capped(0) == 0  # (waits for the stream)
                host = t.cpu().numpy()
                same_batch(np.ascontiguousarray(host[:, :h, :w]).view(np.uint8).reshape(3, h, w, 4), want,
                           f"padded device target {variant} proj {proj} {w} x {h}")
                assert (host[:, h:] == 0x5A5A5A5A).all() and (host[:, :, w:] == 0x5A5A5A5A).all()


# ---- 3. the row fold ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_row_fold_beyond_32768_grid_rows(world, variant):
    """32 770 perspective views of 8 x 1 pixels cycling through four cameras: one tile row per view, so the batch's grid rows
    reach blockIdx.z = 1.  The expected batch is four single renders, tiled."""
    gpu, gw, n = world.gpu, 1.0, 32770
    scene = world.scenes[gw]
    idx = (0, 3, 4, 5)
    four = world.cameras(gw, 1, 0, idx, 8, 1)
    want4 = world.batch(gw, 1, 0, idx, 8, 1, False)
    assert len({want4[k].tobytes() for k in range(4)}) == 4  # (four distinct frames: a view at the wrong index shows)
    cams = (gpu.Camera * n)(*[four[k % 4] for k in range(n)])
    want = np.ascontiguousarray(np.tile(want4, (n // 4 + 1, 1, 1, 1))[:n])
    with kernel_variant(variant):
        same_batch(world.singles(gw, 1, 0, idx, 8, 1, False), want4, f"single renders, row fold {variant}")
        same_batch(scene.render_views(cams), want, f"row fold {variant}", named=(0, 32767, 32768, 32769))


# ---- 4. staging reuse: two device batches back to back on one caller stream ----
@pytest.mark.parametrize("proj", [1, 2, 3], ids=PROJ_IDS)
def test_two_device_batches_back_to_back(world, proj):
    """Different cameras, no host wait between the two calls, then one synchronize: both batches are right -- the second batch's
    records and tables did not overwrite what the first batch's upload had yet to read.  Then four more without a wait (the ring
    of staging blocks goes round), the last of them checked."""
    import torch
    gpu, gw, w, h = world.gpu, 0.05, 24, 33
    scene = world.scenes[gw]
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    first, second = vc.batch_indices(7, 0), [6, 2, 5, 1]
    for sampling, interior in ((0, False), (1, True), (2, True)):
        a = torch.zeros((7, h, w), dtype=torch.int32, device="cuda")
        b = torch.zeros((4, h, w), dtype=torch.int32, device="cuda")
        cams_a, cams_b = world.cameras(gw, proj, sampling, first, w, h), world.cameras(gw, proj, sampling, second, w, h)
        want_a, want_b = world.batch(gw, proj, sampling, first, w, h, interior), world.batch(gw, proj, sampling, second, w, h, interior)
        torch.cuda.synchronize()
        scene.render_views_device(cams_a, a.data_ptr(), w * 4, h * w * 4, interior=interior, stream=stream.cuda_stream)
        scene.render_views_device(cams_b, b.data_ptr(), w * 4, h * w * 4, interior=interior, stream=stream.cuda_stream)
        stream.synchronize()
        what = f"proj {proj} sampling {sampling} interior {interior}"
        same_batch(a.cpu().numpy().view(np.uint8).reshape(7, h, w, 4), want_a, "first of two batches " + what)
        same_batch(b.cpu().numpy().view(np.uint8).reshape(4, h, w, 4), want_b, "second of two batches " + what)
        for _ in range(3):
            scene.render_views_device(cams_b, b.data_ptr(), w * 4, h * w * 4, interior=interior, stream=stream.cuda_stream)
        scene.render_views_device(cams_a, a.data_ptr(), w * 4, h * w * 4, interior=interior, stream=stream.cuda_stream)
        assert scene.take_capped(stream.cuda_stream) == 0  # (waits for the stream)
        same_batch(a.cpu().numpy().view(np.uint8).reshape(7, h, w, 4), want_a, "sixth batch " + what)


# ---- 5. a height update between two batches ----
def test_height_update_between_batches(world, oracle):
    """The second batch is rendered from the new heights: its records carry the scene's new box and bound."""
    gpu, gw, w, h = world.gpu, 0.5, 24, 33
    idx = vc.batch_indices(7)
    after = vc.Expected(gpu, oracle)
    after.params[gw] = gpu.SceneParams.make(0.0, 5.0 * gw, grid_width=gw)
    after.heights[gw] = oracle.update_heightmap(after.rgb, after.params[gw])
    scene = gpu.Scene(world.rgb, world.cmap, world.params[gw])
    try:
        for proj in (1, 2, 3):
            cams = world.cameras(gw, proj, 0, idx, w, h)
            same_batch(scene.render_views(cams), world.batch(gw, proj, 0, idx, w, h, False), f"before the update, proj {proj}")
            scene.update(after.params[gw])
            want = after.batch(gw, proj, 0, idx, w, h, False)
            assert want.tobytes() != world.batch(gw, proj, 0, idx, w, h, False).tobytes()
            same_batch(scene.render_views(cams), want, f"after the update, proj {proj}")
            same_batch(scene.render_views(cams, interior=True), after.batch(gw, proj, 0, idx, w, h, True), f"after the update, interior, proj {proj}")
            scene.update(world.params[gw])
    finally:
        scene.close()


# ---- 6. the step cap: the one case with capped rays ----
@pytest.mark.parametrize("variant", KERNEL_VARIANTS)
def test_capped_rays_are_the_batch_s(world, variant):
    """HMRM_STEP_CAP=60: the host form returns HMRM_E_NOTERM with valid frames and the batch's count, the device form reports the
    same count through take_capped -- the sum of the single renders' counts."""
    import torch
    gpu, gw, w, h, cap = world.gpu, 0.5, 24, 33, 60
    scene = world.scenes[gw]
    idx = vc.batch_indices(7)
    with kernel_variant(variant), env(HMRM_STEP_CAP=cap):
        for proj in (1, 2, 3):
            for interior in (False, True):
                cams = world.cameras(gw, proj, 0, idx, w, h)
                want = world.batch(gw, proj, 0, idx, w, h, interior, step_cap=cap, capped_ok=True)
                counts = [world.frame(gw, proj, 0, k, w, h, interior, cap)[2] for k in idx]
                total = sum(counts)
                assert total >= 10 and sum(1 for c in counts if c) >= 2, counts  # (more than one view has some)
                if not interior:  # (the single renders' own counts: hmrm_render_stats')
                    assert [scene.render_stats(c, allow_capped=True)[1].capped for c in cams] == counts
                with pytest.raises(gpu.HmrmError) as e:
                    scene.render_views(cams, interior=interior)
                assert e.value.code == gpu.HMRM_E_NOTERM and f"{total} ray(s)" in str(e.value)
                what = f"capped {variant} proj {proj} interior {interior}"
                same_batch(scene.render_views(cams, interior=interior, allow_capped=True), want, what)
                t = torch.zeros((7, h, w), dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                scene.render_views_device(cams, t.data_ptr(), w * 4, h * w * 4, interior=interior)
                assert scene.take_capped(0, allow_capped=True) == total
                same_batch(t.cpu().numpy().view(np.uint8).reshape(7, h, w, 4), want, "device form, " + what)


# ---- 7. the device form's own refusals, with a live scene ----
def test_device_form_refusals(world):
    import torch
    gpu, gw = world.gpu, 1.0
    scene = world.scenes[gw]
    cams = world.cameras(gw, 1, 0, [0, 3], 24, 33)
    t = torch.zeros((2, 33, 24), dtype=torch.int32, device="cuda")
    for stride, view_stride, text in ((24 * 4 - 4, 33 * 24 * 4, "stride_bytes"), (24 * 4 + 2, 33 * 26 * 4, "stride_bytes"),
                                      (24 * 4, 33 * 24 * 4 - 4, "view_stride_bytes"), (24 * 4, 33 * 24 * 4 + 2, "view_stride_bytes")):
        with pytest.raises(gpu.HmrmError) as e:
            scene.render_views_device(cams, t.data_ptr(), stride, view_stride)
        assert e.value.code == gpu.HMRM_E_ARG and text in str(e.value)
    mixed = world.cameras(gw, 1, 0, [0, 3], 24, 33)
    mixed[1].sampling = 1
    with pytest.raises(gpu.HmrmError) as e:
        scene.render_views(mixed)
    assert e.value.code == gpu.HMRM_E_ARG and "view 1 differs from view 0 in sampling" in str(e.value)
    with pytest.raises(gpu.HmrmError) as e:
        scene.render_views([])
    assert e.value.code == gpu.HMRM_E_ARG and "n must be 1 .. 65536" in str(e.value)


# ---- 8. CLI ----
def test_cli_view_lines(world, tmp_path):
    """Three `view` lines and a `views_output` prefix: three PNGs, each hmrm_render's frame of that camera; with `interior on`,
    hmrm_render_interior's; one key without the other warns and writes nothing."""
    gpu, gw = world.gpu, 0.5
    scene = world.scenes[gw]
    cfgp, text, outp = gs.cli_config(gpu, world, tmp_path, gw, width=24, height=33)
    prefix = str(tmp_path / "view_")
    lines = ""
    for k in (3, 1, 5):
        pos, hang, vang = vc._CAMS[k][0], vc._CAMS[k][1], vc._CAMS[k][2]
        lines += f"view {pos[0] * gw:.17g} {pos[1] * gw:.17g} {pos[2] * gw:.17g} {hang} {vang}\n"
    for interior in (False, True):
        cfgp.write_text(text + lines + f"views_output {prefix}\n" + ("interior on\n" if interior else ""))
        cfg = gpu.Config()
        cfg.consume_file(str(cfgp))
        cams = cfg.views()
        assert len(cams) == 3 and cfg.views_output == prefix
        r = gs.run_hmap(gpu, cfgp)
        assert "rendered 3 views" in r.stdout and "WARNING: view" not in r.stderr
        for k, cam in enumerate(cams):
            want = scene.render_interior(cam) if interior else scene.render(cam)
            assert open(f"{prefix}{k:03d}.png", "rb").read() == gpu.png_encode(want), (interior, k)
            assert f"Saved view at {prefix}{k:03d}.png" in r.stdout
        # (the views differ from each other and from the main frame)
        assert len({open(f"{prefix}{k:03d}.png", "rb").read() for k in range(3)}) == 3
        assert not (tmp_path / "view_003.png").exists()
    for k in range(3):
        (tmp_path / f"view_{k:03d}.png").unlink()
    cfgp.write_text(text + lines)
    r = gs.run_hmap(gpu, cfgp)
    assert "WARNING: view is ignored without views_output\n" in r.stderr and "rendered 3 views" not in r.stdout
    cfgp.write_text(text + f"views_output {prefix}\n")
    r = gs.run_hmap(gpu, cfgp)
    assert "WARNING: views_output is ignored without a view\n" in r.stderr and "rendered" not in r.stdout.split("Saved screenshot")[1]
    assert not (tmp_path / "view_000.png").exists()
