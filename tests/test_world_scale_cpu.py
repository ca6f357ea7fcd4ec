"""The world-scale cases (tests/world_scale.py) on the CPU alone: the conditions every case must meet for the GPU
comparison to mean something, the two restatements of the reference against each other at these magnitudes, the
power-of-two invariance of the reference's loop, and the host's per-frame record."""
import numpy as np
import pytest

import np_marcher
import world_scale as ws

CASES = ws.cases()
IDS = [c[0] for c in CASES]
MAX_EXEMPT = 4
NP_MARCHER_MAX_STEPS = 2_000_000  # frames above this take the vectorised restatement seconds

_rendered = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _oracle_frame(oracle, case, opt="O2"):
    """(heights, frame, total, capped, steps, entry_d) of a case, rendered once per optimisation level."""
    name, fam, rgb, cmap, params, cam, exempt = case
    if (name, opt) not in _rendered:
        heights = oracle.update_heightmap(rgb, params, opt=opt)
        cfg = oracle.make_cfg(cam, params, rgb.shape[1], rgb.shape[0])
        _rendered[(name, opt)] = (heights,) + tuple(oracle.render(cfg, heights, cmap, per_pixel=True, opt=opt))
    return _rendered[(name, opt)]


def test_generator_shape():
    assert len(set(IDS)) == len(IDS)
    assert {c[1] for c in CASES} == set(ws.FAMILIES)
    for fam in ws.FAMILIES:
        assert {c[5].projection for c in ws.family(fam)} == {1, 2, 3}, fam
    for name, fam, rgb, cmap, params, cam, exempt in CASES:
        assert (cam.width, cam.height) == (ws.FRAME_W, ws.FRAME_H), name
    exempt = [c[0] for c in CASES if c[6]]
    assert len(exempt) <= MAX_EXEMPT and exempt == [f"P2_persp_k{ws.P2_PERSP_EXEMPT_K}"]
    # the sweeps the cases are built from
    assert ws.P2_K == (-900, -510, -490, -300, -60, -24, -1, 0, 1, 24, 60, 300, 490, 510, 900)
    assert ws.DEC_S == (1e-12, 1e-9, 1e-6, 1e-3, 30.0, 1e3, 1e6, 1e9, 1e12)
    for proj in (1, 2, 3):
        assert len(ws.family("DEC", proj)) == len(ws.DEC_S)
    for proj in (2, 3):
        assert len(ws.family("P2", proj)) == len(ws.P2_K)
        assert len(ws.family("FAR", proj)) == 4 and len(ws.family("GW", proj)) == 25
    assert len(ws.family("P2", 1)) == sum(k <= 24 for k in ws.P2_K) + 1 and len(ws.family("FAR", 1)) == 3
    for e in ws.GW_E:
        p = 2.0 ** e
        got = [gw for _, gw in ws.gw_members(e)]
        assert got == [p, np.nextafter(p, 0.0), np.nextafter(p, np.inf), 0.75 * p, p / 3.0]
    assert len(ws.family("OFFSET")) == 18 and len(ws.family("RATIO")) == 18 and len(CASES) == 190
    # the generator is deterministic
    again = ws.cases()
    assert [bytes(c[4]) + bytes(c[5]) for c in again] == [bytes(c[4]) + bytes(c[5]) for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conditions_on_the_oracle(oracle, case):
    """No ray capped under the default step cap, a quarter of the rays take a step, 40 colours -- or, for the cases the
    generator marks exempt, what makes them degenerate.  Conditions on the inputs: a pose that misses them is tuned in
    world_scale.py."""
    name, fam, rgb, cmap, params, cam, exempt = case
    heights, fb, total, capped, steps, entry = _oracle_frame(oracle, case)
    colours = len(np.unique(fb.reshape(-1, 4), axis=0))
    assert capped == 0, name
    if exempt:
        cfg = oracle.make_cfg(cam, params, rgb.shape[1], rgb.shape[0])
        for px, py in ((0, 0), (cam.width - 1, 0), (0, cam.height - 1), (cam.width - 1, cam.height - 1), (31, 24), (17, 40)):
            pos, d, dist = oracle.probe_ray(cfg, px, py)
            assert np.isnan(d).all(), (name, px, py)
        assert total == 0 and (fb == np.array([cam.bg_r, cam.bg_g, cam.bg_b, 255], dtype=np.uint8)).all(), name
        return
    assert (steps > 0).mean() >= 0.25, (name, (steps > 0).mean())
    assert colours >= 40, (name, colours)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_o0_equals_o2(oracle, case):
    a, b = _oracle_frame(oracle, case), _oracle_frame(oracle, case, "O0")
    assert np.array_equal(_bits(a[0]), _bits(b[0])), "heights"
    assert np.array_equal(a[1], b[1]) and a[2:4] == b[2:4], "frame / total / capped"
    assert np.array_equal(a[4], b[4]) and np.array_equal(_bits(a[5]), _bits(b[5])), "steps / distance()"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_numpy_restatement_agrees(oracle, case):
    """The vectorised restatement and the C one had only met at unit scale."""
    name, fam, rgb, cmap, params, cam, exempt = case
    heights, fb, total, capped, steps, entry = _oracle_frame(oracle, case)
    if total > NP_MARCHER_MAX_STEPS:
        assert fam == "RATIO" and "step0p001" in name  # (only these three are that long)
        return
    nfb, nsteps, ndist = np_marcher.render(cam, params, heights, cmap)
    assert np.array_equal(_bits(ndist), _bits(entry)), name
    assert np.array_equal(nsteps, steps), name
    assert np.array_equal(nfb, fb), name


@pytest.mark.parametrize("proj", [2, 3], ids=["sph", "ortho"])
def test_power_of_two_invariance_on_the_oracle(oracle, proj):
    """Scaling every length by 2^k scales every intermediate of the reference's loop by 2^k exactly (no over- or
    underflow in this sweep): same frame, same steps, distance() times 2^k with its infinities in place.  The one
    expectation here that does not come from the oracle's own arithmetic at that scale."""
    members = ws.family("P2", proj)
    base = next(c for c in members if c[0].endswith("_k0"))
    _, bfb, btotal, _, bsteps, bentry = _oracle_frame(oracle, base)
    assert len(members) == len(ws.P2_K)
    for case, k in zip(members, ws.P2_K):
        _, fb, total, capped, steps, entry = _oracle_frame(oracle, case)
        assert np.array_equal(fb, bfb) and np.array_equal(steps, bsteps) and total == btotal, case[0]
        assert np.array_equal(_bits(entry), _bits(np.ldexp(bentry, k))), case[0]
        assert np.array_equal(np.isinf(entry), np.isinf(bentry)), case[0]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_frame_record(hmrm, oracle, case):
    """hmrm_debug_frame at these magnitudes: the record equals the oracle's, and nothing in it has overflowed,
    underflowed to zero or become NaN where the reference's value has not."""
    name, fam, rgb, cmap, params, cam, exempt = case
    mh, mw = rgb.shape[:2]
    rec = hmrm.debug_frame(cam, params, mw, mh)
    o = oracle.frame_record(oracle.make_cfg(cam, params, mw, mh))
    fields = [("cam", 0), ("c0", 15), ("c1", 18)]
    if cam.projection in (1, 3):
        fields += [("upper_left", 3), ("plane_right", 6), ("plane_down", 9)]
    if cam.projection == 3:
        fields += [("look", 12)]
    for key, at in fields:
        got, want = np.asarray(rec[key]), o[at:at + 3]
        assert np.array_equal(_bits(got), _bits(want)), (name, key)
        assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.array_equal(got != 0.0, want != 0.0), (name, key)
    assert _bits(rec["nudge"]) == _bits(o[21]) and np.isfinite(rec["nudge"]) and rec["nudge"] != 0.0, name
    assert rec["step_dist"] == cam.step_dist and np.isfinite(rec["step_dist"]) and rec["step_dist"] != 0.0, name
    inv = rec["inv_grid_width"]
    assert np.isfinite(inv) and inv != 0.0, name
    gw = params.grid_width
    pow2 = np.frexp(gw)[0] == 0.5
    assert rec["grid_pow2"] == int(pow2), (name, gw)
    assert inv == 1.0 / gw, (name, gw)  # (exact for a power of two, the correctly rounded reciprocal otherwise)
    if cam.projection == 2:
        cfg = oracle.make_cfg(cam, params, mw, mh)
        for px, py in ((0, 0), (cam.width - 1, cam.height - 1), (31, 24), (5, 40)):
            _, d, _ = oracle.probe_ray(cfg, px, py)
            got = [rec["row_sin_va"][py] * rec["col_cos_ha"][px], rec["row_sin_va"][py] * rec["col_sin_ha"][px], rec["row_cos_va"][py]]
            assert np.array_equal(_bits(got), _bits(d)), (name, px, py)
