"""The world-scale cases (tests/world_scale.py) on the GPU: every case of every family under every kernel variant
against the CPU oracle, bit for bit -- frame, per-ray steps, distance(), totals.  The kernels carry absolute magnitudes
(slab_classify's 2^+-500 gate, 0x1p40 as "no constraint", the 2^-20 near-integer test of the general grid width, float
window maxima, binade bookkeeping); the reference's loop carries none, and whatever its loop does the kernels must do too.

The traversal counters (leap attempts / leaps / groups / leaped steps) are printed per case, `pytest -rP` shows them;
they legitimately differ between scales and are not compared, only the base case must leap at all."""
import numpy as np
import pytest

import world_scale as ws
from aa_box import box_filter, super_camera
from test_parity_gpu import KERNEL_VARIANTS, _bits, gpu, kernel_variant  # noqa: F401  (gpu: the module-scoped fixture)

pytestmark = pytest.mark.gpu

PROJ_IDS = [p[1] for p in ws.PROJECTIONS]
PROJS = [p[0] for p in ws.PROJECTIONS]

_oracle_frames = {}


def _same_doubles(a, b):
    """Bit for bit; a NaN equals a NaN (the sign and payload of a generated NaN are the machine's, x86 and gfx950 differ)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _oracle_frame(oracle, case):
    name, fam, rgb, cmap, params, cam, exempt = case
    if name not in _oracle_frames:
        heights = oracle.update_heightmap(rgb, params)
        cfg = oracle.make_cfg(cam, params, rgb.shape[1], rgb.shape[0])
        _oracle_frames[name] = (heights, cfg) + tuple(oracle.render(cfg, heights, cmap, per_pixel=True))
    return _oracle_frames[name]


def _with_sampling(gpu, cam, sampling):
    c = gpu.Camera.from_buffer_copy(cam)
    c.sampling = sampling
    return c


def _check_case(gpu, oracle, case, extras):
    """-> (GPU frame, GPU steps, Stats under `leap`)"""
    import torch
    name, fam, rgb, cmap, params, cam, exempt = case
    mh, mw = rgb.shape[:2]
    heights, cfg, ofb, total, capped, osteps, oentry = _oracle_frame(oracle, case)
    assert capped == 0, name
    scene = gpu.Scene(rgb, cmap, params)
    assert np.array_equal(_bits(scene.read_heights()), _bits(heights)), f"{name}: UpdateHeightmap"
    kept = None
    for variant in KERNEL_VARIANTS:
        with kernel_variant(variant):
            fb, st, steps, entry = scene.render_stats(cam, per_pixel=True)
            assert _same_doubles(entry, oentry), f"{name} {variant}: distance(), {int((_bits(entry) != _bits(oentry)).sum())} rays differ"
            assert np.array_equal(steps.astype(np.int64), osteps), f"{name} {variant}: steps of {int((steps != osteps).sum())} rays differ"
            assert np.array_equal(fb, ofb), f"{name} {variant}: {int((fb != ofb).any(axis=2).sum())} pixels differ"
            assert (st.rays, st.steps, st.capped) == (cam.width * cam.height, total, 0), (name, variant)
            assert np.array_equal(scene.render(cam), ofb), f"{name} {variant}: the un-instrumented kernel"
            if variant == "leap":
                kept = (fb, steps, st)
                print(f"{name:34s} steps {st.steps:8d} leap_attempts {st.leap_attempts:7d} leaps {st.leaps:7d} "
                      f"groups {st.groups:8d} leaped_steps {st.leaped_steps:8d}")
    if extras:
        for sampling in (gpu.BILINEAR, gpu.NEAREST_F32):
            c = _with_sampling(gpu, cam, sampling)
            sfb, stotal, scapped, ssteps, sentry = oracle.render(oracle.make_cfg(c, params, mw, mh), heights, cmap, per_pixel=True)
            assert scapped == 0, (name, sampling)
            # (under the production kernel and the plain groups only: "simple" and "rec" have no bilinear loop of their
            # own -- "group" serves them, test_bilinear_mode_bit_exact -- and all four ran the nearest frame above)
            for variant in ("leap", "group"):
                with kernel_variant(variant):
                    fb, st, steps, entry = scene.render_stats(c, per_pixel=True)
                    assert _same_doubles(entry, sentry), (name, sampling, variant)
                    assert np.array_equal(steps.astype(np.int64), ssteps) and st.steps == stotal and st.capped == 0, (name, sampling, variant)
                    assert np.array_equal(fb, sfb) and np.array_equal(scene.render(c), sfb), (name, sampling, variant)
        super_fb, *_ = oracle.render(oracle.make_cfg(super_camera(gpu, cam, 2), params, mw, mh), heights, cmap)
        assert np.array_equal(scene.render_aa(cam, 2), box_filter(super_fb, 2)), f"{name}: antialiased 2x2"
        out = torch.zeros((cam.height, cam.width, 4), dtype=torch.uint8, device="cuda")
        scene.render_device_wait(scene.render_device_begin(cam, out.data_ptr(), cam.width * 4))
        assert np.array_equal(out.cpu().numpy(), ofb), f"{name}: device ticket"
        for px, py in ((0, 0), (cam.width - 1, 0), (0, cam.height - 1), (cam.width - 1, cam.height - 1), (cam.width // 2, cam.height // 2)):
            pos, d, dist = scene.debug_ray(cam, px, py)
            opos, od, odist = oracle.probe_ray(cfg, px, py)
            assert _same_doubles(pos, opos) and _same_doubles(d, od) and _same_doubles(dist, odist), (name, px, py)
    scene.close()
    return kept


def _run_family(gpu, oracle, fam, proj):
    members = ws.family(fam, proj)
    assert members
    # (OFFSET and RATIO are two short sweeps each -- above / below zero, step / height: every member is an end or a middle)
    special = {c[0] for c in (members if fam in ("OFFSET", "RATIO") else ws.ends_and_middle(members))}
    return {c[0]: _check_case(gpu, oracle, c, c[0] in special) for c in members}


@pytest.mark.parametrize("proj", PROJS, ids=PROJ_IDS)
def test_p2_exact_rescale(gpu, oracle, proj):
    """2^-900 .. 2^900 (perspective up to 2^24, and 2^60 whose every direction is NaN and whose frame is background).
    +-490 / +-510 straddle slab_classify's gate; from about 2^-895 down and 2^877 up axis_refresh declines a binade."""
    got = _run_family(gpu, oracle, "P2", proj)
    base = next(n for n in got if n.endswith("_k0"))
    assert got[base][2].leaped_steps > 0, "the base scene does not exercise the leap path: fix the scene"
    if proj != 1:
        for name, (fb, steps, st) in got.items():
            assert np.array_equal(fb, got[base][0]) and np.array_equal(steps, got[base][1]), f"{name} differs from the GPU's own k = 0"


@pytest.mark.parametrize("proj", PROJS, ids=PROJ_IDS)
def test_dec_decimal_rescale(gpu, oracle, proj):
    _run_family(gpu, oracle, "DEC", proj)


@pytest.mark.parametrize("proj", PROJS, ids=PROJ_IDS)
def test_gw_grid_widths_next_to_the_specialisations(gpu, oracle, proj):
    _run_family(gpu, oracle, "GW", proj)


@pytest.mark.parametrize("proj", PROJS, ids=PROJ_IDS)
def test_far_telephoto(gpu, oracle, proj):
    _run_family(gpu, oracle, "FAR", proj)


@pytest.mark.parametrize("proj", PROJS, ids=PROJ_IDS)
def test_offset_relief_below_float_resolution(gpu, oracle, proj):
    _run_family(gpu, oracle, "OFFSET", proj)


@pytest.mark.parametrize("proj", PROJS, ids=PROJ_IDS)
def test_ratio_step_and_height_to_grid_width(gpu, oracle, proj):
    _run_family(gpu, oracle, "RATIO", proj)
