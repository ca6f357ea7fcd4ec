"""Antialiased rendering on the GPU (hmrm_render_aa, HMRM_AA): every frame is compared bit for bit with the CPU oracle's
frame at n times the resolution, box-filtered in numpy (tests/aa_box.py) -- the definition in include/hmrm.h."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import scenes
from aa_box import box_filter, super_camera

pytestmark = pytest.mark.gpu

CASES = {c[0]: c for c in scenes.cases()}
FEW = ("persp_outside_pow2", "sph_min_height", "ortho_default_grid")
EIGHT = ("persp_outside_pow2", "sph_grazing", "ortho_lowside_exit", "persp_width1", "sph_height1")


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def gpu(hmrm):
    assert hmrm.device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    hmrm.set_device(0)
    return hmrm


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
    exe = os.path.join(os.path.dirname(gpu.LIB_PATH), "hmap")
    r = subprocess.run([exe, str(cfgp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "antialias 2\n" in r.stdout
    assert f"rendered {4 * cam.width * cam.height} rays, {total} ray-steps" in r.stdout
    assert open(outp, "rb").read() == gpu.png_encode(want)
