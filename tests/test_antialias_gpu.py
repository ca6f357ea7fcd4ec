"""Antialiased rendering on the GPU (hmrm_render_aa, HMRM_AA): every frame is compared bit for bit with the CPU oracle's
frame at n times the resolution, box-filtered in numpy (tests/aa_box.py) -- the definition in include/hmrm.h."""
import numpy as np
import pytest

import gpu_support as gs
import scenes
from aa_box import box_filter, super_camera
from gpu_support import env, gpu

pytestmark = pytest.mark.gpu

CASES = {c[0]: c for c in scenes.cases()}
FEW = ("persp_outside_pow2", "sph_min_height", "ortho_default_grid")
EIGHT = ("persp_outside_pow2", "sph_grazing", "ortho_lowside_exit", "persp_width1", "sph_height1")


def _expected(gpu, oracle, heights, cmap, params, cam, n, step_cap=None):
    sc = super_camera(gpu, cam, n)
    kw = {} if step_cap is None else {"step_cap": step_cap}
    ofb, total, capped, *_ = oracle.render(oracle.make_cfg(sc, params, cmap.shape[1], cmap.shape[0], **kw), heights, cmap)
    return box_filter(ofb, n), total, capped


@pytest.mark.parametrize("case", scenes.cases(), ids=scenes.case_ids())
def test_scene_antialiased_bit_exact(gpu, oracle, case):
    name, rgb, cmap, params, cam = scenes.build_case(case)
    scene = gpu.Scene(rgb, cmap, params)
    heights = oracle.update_heightmap(rgb, params)
    for n in (2, 4, 8) if name in EIGHT else (2, 4):
        want, *_ = _expected(gpu, oracle, heights, cmap, params, cam, n)
        got = scene.render_aa(cam, n)
        assert got.shape == (cam.height, cam.width, 4)
        assert np.array_equal(got, want), f"{name} n={n}: {int((got != want).any(axis=2).sum())} pixels differ"
    scene.close()


@pytest.mark.parametrize("name", FEW)
def test_kernel_variants_and_samplings(gpu, oracle, name):
    _, rgb, cmap, params, cam = scenes.build_case(CASES[name])
    scene = gpu.Scene(rgb, cmap, params)
    heights = oracle.update_heightmap(rgb, params)
    for sampling in (gpu.NEAREST, gpu.BILINEAR, gpu.NEAREST_F32):
        c = gpu.Camera.from_buffer_copy(cam)
        c.sampling = sampling
        want, *_ = _expected(gpu, oracle, heights, cmap, params, c, 2)
        for variant in ("leap", "group", "simple", "rec"):
            with env(HMRM_KERNEL=variant):
                assert np.array_equal(scene.render_aa(c, 2), want), (name, sampling, variant)
                fb, st = scene.render_aa(c, 2, stats=True)
                assert np.array_equal(fb, want), (name, sampling, variant, "instrumented")
    scene.close()


def test_factor_one_is_render(gpu):
    for name in ("persp_outside_pow2", "sph_upward", "ortho_top_down", "persp_width1"):
        _, rgb, cmap, params, cam = scenes.build_case(CASES[name])
        scene = gpu.Scene(rgb, cmap, params)
        plain = scene.render(cam)
        assert np.array_equal(scene.render_aa(cam, 1), plain), name
        fb, st = scene.render_aa(cam, 1, stats=True)
        _, st0, _, _ = scene.render_stats(cam)
        assert np.array_equal(fb, plain) and (st.rays, st.steps, st.hits) == (st0.rays, st0.steps, st0.hits)
        scene.close()


def test_stats_count_samples(gpu, oracle):
    for name in ("persp_min_height", "sph_outside_pow2", "ortho_lowside_exit"):
        _, rgb, cmap, params, cam = scenes.build_case(CASES[name])
        scene = gpu.Scene(rgb, cmap, params)
        heights = oracle.update_heightmap(rgb, params)
        for n in (2, 4):
            fb, st = scene.render_aa(cam, n, stats=True)
            _, sst, _, _ = scene.render_stats(super_camera(gpu, cam, n))
            want, total, capped = _expected(gpu, oracle, heights, cmap, params, cam, n)
            assert np.array_equal(fb, want)
            assert st.rays == n * n * cam.width * cam.height == sst.rays
            assert (st.steps, st.hits, st.capped) == (sst.steps, sst.hits, sst.capped)
            assert st.steps == total and st.capped == capped == 0
        scene.close()


def test_step_cap_reported_over_samples(gpu, oracle):
    """step_dist 0 straight up (the endless loop of hmap.cpp:1000): every sample is capped; HMRM_E_NOTERM says so."""
    rgb = np.zeros((8, 8, 3), dtype=np.uint8)
    cmap = np.full((8, 8, 4), 255, dtype=np.uint8)
    params = gpu.SceneParams.make(0.0, 4.0, grid_width=1.0)
    cam = gpu.Camera.make(width=4, height=4, projection=3, hang=0.0, vang=0.0, pos=(4.0, -4.0, -3.0),
                          ortho_width=0.5, step_dist=0.0, bg=(9, 8, 7))
    with env(HMRM_STEP_CAP=1000):
        scene = gpu.Scene(rgb, cmap, params)
        fb, st = scene.render_aa(cam, 2, stats=True, allow_capped=True)
        assert st.capped == 64 and st.rays == 64 and st.steps == 64 * 1000
        with pytest.raises(gpu.HmrmError) as e:
            scene.render_aa(cam, 2)
        assert e.value.code == gpu.HMRM_E_NOTERM
        heights = oracle.update_heightmap(rgb, params)
        want, _, capped = _expected(gpu, oracle, heights, cmap, params, cam, 2, step_cap=1000)
        assert capped == 64 and np.array_equal(fb, want)
        scene.close()


@pytest.mark.parametrize("wl_name", ["C2", "C3"])
def test_full_size_against_plain_super_frame(gpu, wl_name):
    """C2 at 960x540 with n = 2 is C2's 1920x1080 frame filtered; C3's map at 1920x1080 with n = 2 is the 3840x2160
    headline frame filtered (Scene.render of those frames is itself tested against the oracle elsewhere)."""
    wl = gpu.synth.WORKLOADS[wl_name]
    rgb, cmap = gpu.synth.synth_maps(wl.map_size)
    scene = gpu.Scene(rgb, cmap, wl.scene_params())
    big = wl.camera()
    cam = gpu.Camera.from_buffer_copy(big)
    cam.width, cam.height = big.width // 2, big.height // 2
    want = box_filter(scene.render(big), 2)
    assert np.array_equal(scene.render_aa(cam, 2), want)
    fb, st = scene.render_aa(cam, 2, stats=True)
    assert np.array_equal(fb, want) and st.rays == big.width * big.height
    scene.close()


def test_host_and_device_tickets_mixed_factors(gpu, oracle):
    torch = pytest.importorskip("torch")
    _, rgb, cmap, params, cam = scenes.build_case(CASES["persp_outside_pow2"])
    scene = gpu.Scene(rgb, cmap, params)
    heights = oracle.update_heightmap(rgb, params)
    want = {n: _expected(gpu, oracle, heights, cmap, params, cam, n)[0] for n in (1, 2, 4, 8)}
    order = [1, 2, 4, 8, 2, 8, 1, 4]
    tickets = [(n, scene.render_begin(cam, aa=n)) for n in order]
    for n, t in tickets:
        got = scene.render_wait(t, (cam.height, cam.width))
        scene.render_release(t)
        assert np.array_equal(got, want[n]), n
    bufs = [(n, torch.zeros((cam.height, cam.width, 4), dtype=torch.uint8, device="cuda")) for n in order]
    torch.cuda.synchronize()
    dt = [(n, b, scene.render_device_begin(cam, b.data_ptr(), cam.width * 4, aa=n)) for n, b in bufs]
    for n, b, t in dt:
        scene.render_device_wait(t)
        assert np.array_equal(b.cpu().numpy(), want[n]), n
    scene.close()


def test_record_orbit_antialiased(gpu, oracle, tmp_path):
    rgb, cmap = scenes.small_maps(64, 64, 41)
    params = gpu.SceneParams.make(0.0, 8.0, grid_width=1.0)
    base = gpu.Camera.make(width=80, height=45, projection=1, hfov=gpu.degrees_to_rads(80), hang=0.0,
                           vang=gpu.degrees_to_rads(112), pos=(-20.0, 20.0, 30.0), step_dist=0.5, bg=(4, 5, 6))
    scene = gpu.Scene(rgb, cmap, params)
    heights = oracle.update_heightmap(rgb, params)
    frames, cx, cy, radius, hang0 = 4, 32.0, -32.0, 70.0, gpu.degrees_to_rads(-45.0)
    out = tmp_path / "rec"
    out.mkdir()
    gpu.record_orbit(scene, base, cx, cy, radius, hang0, frames, str(out), 77, encoder_threads=2, aa=2)
    assert sorted(p.name for p in out.iterdir()) == [f"hmap_77_{k}.png" for k in range(frames)]
    for k in range(frames):
        cam = gpu.orbit_camera(base, cx, cy, radius, hang0, k, frames)
        want, *_ = _expected(gpu, oracle, heights, cmap, params, cam, 2)
        assert (out / f"hmap_77_{k}.png").read_bytes() == gpu.png_encode(want), k
    scene.close()


def test_cli_antialias_key(gpu, oracle, tmp_path):
    wl = gpu.synth.WORKLOADS["C1"]
    rgb, cmap = gpu.synth.synth_maps(wl.map_size)
    hp, cp = str(tmp_path / "h.ppm"), str(tmp_path / "c.png")
    gpu.write_ppm(hp, rgb)
    gpu.write_png(cp, cmap)
    params, cam = wl.scene_params(), wl.camera()
    heights = oracle.update_heightmap(rgb, params)
    want, total, _ = _expected(gpu, oracle, heights, cmap, params, cam, 2)
    outp = str(tmp_path / "frame.png")
    cfgp = tmp_path / "c.txt"
    cfgp.write_text(gpu.synth.config_text(wl, hp, cp, outp) + "antialias 2\n")
    r = gs.run_hmap(gpu, cfgp)
    assert "antialias 2\n" in r.stdout
    assert f"rendered {4 * cam.width * cam.height} rays, {total} ray-steps" in r.stdout
    assert open(outp, "rb").read() == gpu.png_encode(want)


def _orbit(gpu, cam, k):
    c = gpu.Camera.from_buffer_copy(cam)
    c.hang += 1e-3 * (k + 1)
    return c


@pytest.mark.parametrize("kind,proj", [("needles", 2), ("smooth", 1)])
def test_calibration_and_both_probes_under_antialiasing(gpu, oracle, kind, proj, capfd):
    """An antialiased frame shares the cache record, the launch-order calibration and the kernel probes with the plain frame of
    its super camera (api_frames.cpp check_antialias -> api_launch.cpp prepare_frame) but runs another kernel instantiation into a W x H buffer.  A
    camera whose 4x super frame has 15 tile rows: rendered 16 times (first launch, measured trials of either kernel, settled
    launches), then 14 cameras that never repeat through device tickets (the sixth unprobed frame is launched twice), each
    interleaved with the plain frame of the super camera itself; on a map where the groups may win and on a smooth one; with
    the probe on and off (HMRM_TRY_GROUP=0) and under an explicit pieced order.  Every frame is the oracle's, box-filtered
    where antialiased; the library's own report (HMRM_ORDER_VERBOSE) shows that the calibration settled and the shadow probe
    ran on these records."""
    torch = pytest.importorskip("torch")
    n = 4
    rgb, cmap = gpu.synth.content_maps(256, kind)
    params = gpu.SceneParams.make(0.0, 40.0, grid_width=1.0)
    heights = oracle.update_heightmap(rgb, params)
    cam = gpu.Camera.make(width=80, height=60, projection=proj, hfov=gpu.degrees_to_rads(150 if proj == 2 else 90), hang=gpu.degrees_to_rads(-45),
                          vang=gpu.degrees_to_rads(118), pos=(-40.0, 40.0, 90.0), step_dist=0.5, bg=(3, 4, 5))
    assert (cam.height * n + 15) // 16 >= 12

    def both(c):
        ofb, _, capped, *_ = oracle.render(oracle.make_cfg(super_camera(gpu, c, n), params, 256, 256), heights, cmap)
        assert capped == 0
        return box_filter(ofb, n), ofb
    want, want_super = both(cam)
    for try_group in (None, "0"):
        capfd.readouterr()
        with env(HMRM_ORDER_VERBOSE=1, **({} if try_group is None else {"HMRM_TRY_GROUP": try_group})):
            scene = gpu.Scene(rgb, cmap, params)
            for k in range(16):
                assert np.array_equal(scene.render_aa(cam, n), want), (kind, try_group, k)
                if k % 3 == 1:
                    assert np.array_equal(scene.render(super_camera(gpu, cam, n)), want_super), (kind, try_group, k)
            choice = scene.kernel_choice()
            assert choice in (0, 1, 3) and (try_group is None or choice == 0) and (kind != "smooth" or choice == 0)
            scene.update(params)  # (the verdict is forgotten: the moving cameras below are probed by themselves)
            buf = torch.zeros((cam.height, cam.width, 4), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            for k in range(14):
                c = _orbit(gpu, cam, k)
                w, ws = both(c)
                t = scene.render_device_begin(c, buf.data_ptr(), cam.width * 4, aa=n)
                scene.render_device_wait(t)
                assert np.array_equal(buf.cpu().numpy(), w), (kind, try_group, k)
                if k % 4 == 2:
                    assert np.array_equal(scene.render(super_camera(gpu, c, n)), ws), (kind, try_group, k)
            assert scene.kernel_choice() in (0, 1, 3)
            with env(HMRM_TILE_SEGMENTS="9:5,2:3"):
                assert np.array_equal(scene.render_aa(cam, n), want), (kind, try_group, "pieces")
            scene.close()
        err = capfd.readouterr().err
        assert err.count("hmrm order: settled") >= 1, err
        assert (err.count("hmrm probe:") >= 1) == (try_group is None), err


def test_capped_sample_in_a_doubled_antialiased_frame_is_counted_once(gpu, oracle, capfd):
    """HMRM_STEP_CAP=60 over needles, antialiased cameras that never repeat: the scene's sixth full frame is launched twice
    (shadow probe) and still reports each capped sample once -- the count of the instrumented launch and the oracle's.  Every
    one of the nine frames has capped samples, the doubled one among them, and the library's own report (HMRM_ORDER_VERBOSE)
    shows that the probe did run on these antialiased frames."""
    n = 4
    rgb, cmap = gpu.synth.content_maps(256, "needles")
    params = gpu.SceneParams.make(0.0, 40.0, grid_width=1.0)
    heights = oracle.update_heightmap(rgb, params)
    cam = gpu.Camera.make(width=80, height=60, projection=2, hfov=gpu.degrees_to_rads(150), hang=gpu.degrees_to_rads(-45),
                          vang=gpu.degrees_to_rads(118), pos=(-40.0, 40.0, 90.0), step_dist=0.5, bg=(3, 4, 5))
    capfd.readouterr()
    with env(HMRM_STEP_CAP=60, HMRM_ORDER_VERBOSE=1):
        scene = gpu.Scene(rgb, cmap, params)
        for k in range(9):
            c = _orbit(gpu, cam, k)
            ofb, total, capped, *_ = oracle.render(oracle.make_cfg(super_camera(gpu, c, n), params, 256, 256, step_cap=60), heights, cmap)
            fb, st = scene.render_aa(c, n, stats=True, allow_capped=True)
            assert np.array_equal(fb, box_filter(ofb, n)) and (st.capped, st.steps) == (capped, total), k
            try:
                scene.render_aa(c, n)
                got = 0
            except gpu.HmrmError as e:
                assert e.code == gpu.HMRM_E_NOTERM
                got = int(e.message.split()[0])
            assert got == capped > 0, (k, got, capped)   # (the cap does stop samples of every frame, whichever is doubled)
        scene.close()
    assert capfd.readouterr().err.count("hmrm probe:") == 1


@pytest.mark.parametrize("kind", ["white", "needles"])
def test_hostile_content_full_size_factor_four(gpu, kind):
    """The 1920x1080 frames of test_hostile_content_full_frames_match_oracle (test_parity_gpu.py checks them against the
    oracle) as the super frames of 480x270 at n = 4, under all four HMRM_KERNEL values.  The reference here is the plain
    kernel's frame, box-filtered in numpy -- not the oracle."""
    wl = gpu.synth.content_workload("C2", kind)
    rgb, cmap = wl.maps()
    scene = gpu.Scene(rgb, cmap, wl.scene_params())
    big = wl.camera()
    assert (big.width, big.height) == (1920, 1080)
    cam = gpu.Camera.from_buffer_copy(big)
    cam.width, cam.height = 480, 270
    want = box_filter(scene.render(big), 4)
    for variant in ("leap", "group", "simple", "rec"):
        with env(HMRM_KERNEL=variant):
            assert np.array_equal(scene.render_aa(cam, 4), want), (kind, variant)
            fb, st = scene.render_aa(cam, 4, stats=True)
            assert np.array_equal(fb, want) and st.rays == 1920 * 1080, (kind, variant)
    scene.close()


def test_headline_frame_factor_eight(gpu):
    """C3's 3840x2160 headline frame as the super frame of 480x270 at n = 8, against the plain kernel's frame box-filtered in
    numpy (that frame against the oracle: test_baseline_config_full_size_subsampled_and_properties) -- not the oracle."""
    wl = gpu.synth.WORKLOADS["C3"]
    rgb, cmap = gpu.synth.synth_maps(wl.map_size)
    scene = gpu.Scene(rgb, cmap, wl.scene_params())
    big = wl.camera()
    assert (big.width, big.height) == (3840, 2160)
    cam = gpu.Camera.from_buffer_copy(big)
    cam.width, cam.height = 480, 270
    want = box_filter(scene.render(big), 8)
    assert np.array_equal(scene.render_aa(cam, 8), want)
    fb, st = scene.render_aa(cam, 8, stats=True)
    assert np.array_equal(fb, want) and st.rays == 3840 * 2160
    scene.close()


def test_strides_wider_than_the_row(gpu, oracle):
    """hmrm_render_aa into host memory and antialiased device tickets into device memory whose stride exceeds 4 W: the frame
    is the oracle's, every byte of padding keeps what it held."""
    import ctypes
    torch = pytest.importorskip("torch")
    _, rgb, cmap, params, cam = scenes.build_case(CASES["sph_outside_pow2"])
    scene = gpu.Scene(rgb, cmap, params)
    heights = oracle.update_heightmap(rgb, params)
    W, H = cam.width, cam.height
    for n, pad in ((1, 4), (2, 4), (4, 52), (8, 1024)):
        want, *_ = _expected(gpu, oracle, heights, cmap, params, cam, n)
        stride = W * 4 + pad
        host = np.full((H, stride), 0x5A, dtype=np.uint8)
        rc = gpu.lib.lib.hmrm_render_aa(scene._h, ctypes.byref(cam), n, host.ctypes.data_as(ctypes.c_void_p), stride, None)
        assert rc == gpu.HMRM_OK, gpu.last_error()
        assert np.array_equal(host[:, :W * 4].reshape(H, W, 4), want) and (host[:, W * 4:] == 0x5A).all(), (n, pad)
        dev = torch.full((H, stride), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t = scene.render_device_begin(cam, dev.data_ptr(), stride, aa=n)
        scene.render_device_wait(t)
        got = dev.cpu().numpy()
        assert np.array_equal(got[:, :W * 4].reshape(H, W, 4), want) and (got[:, W * 4:] == 0x5A).all(), (n, pad)
    with pytest.raises(gpu.HmrmError):   # (a device stride must be a multiple of 4)
        scene.render_device_begin(cam, dev.data_ptr(), W * 4 + 2, aa=2)
    scene.close()
