"""The family-scale cases (tests/family_scale.py) on the CPU alone: the generator's shape, the conditions every case must meet on
the replay for the GPU comparison (tests/test_world_scale_families_gpu.py) to mean something, the power-of-two invariance of every
replay -- and what happens instead where a product over- or underflows --, the scalar segment loop against the vectorised replay
at the ends of the sweep, and the host's per-frame record for both cameras."""
import numpy as np
import pytest

import cell_map_replay as cmr
import family_scale as fs
import haze_cases as hc
import lit_replay as lr
import ray_replay
import segment_replay as sr

CASES = fs.cases()
IDS = [c.name for c in CASES]
P2_ENDS = (fs.P2_K[0], fs.P2_K[-1])
N = fs.HAZE_ENTRIES


@pytest.fixture(scope="module")
def replays(hmrm, oracle):
    return fs.Replays(hmrm, oracle)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_generator_shape():
    assert len(set(IDS)) == len(IDS) and {c.sweep for c in CASES} == set(fs.SWEEPS)
    assert fs.P2_K == (-900, -530, -510, -490, -154, -145, -140, 0, 5, 7, 24, 123, 490, 510, 900)
    assert fs.DEC_S == (1e-12, 1e-3, 30.0, 1e12) and fs.GW_E == (-40, 0, 40) and fs.OFFSET_H == (1e6, 1e9)
    assert fs.SUN_M == (-600, -535, -520, 3, 512, 520, 600)
    for proj in (1, 2, 3):
        assert len(fs.sweep("DEC", proj)) == 4 and len(fs.sweep("GW", proj)) == 9
        assert len(fs.sweep("OFFSET", proj)) == 4 and len(fs.sweep("SUN", proj)) == 7
        assert len(fs.sweep("P2", proj)) == (sum(k <= fs.P2_PERSP_MAX_K for k in fs.P2_K) if proj == 1 else len(fs.P2_K))
    assert len(CASES) == 113
    for e in fs.GW_E:
        p = 2.0 ** e
        assert [c.unit for c in fs.sweep("GW", 2) if c.member.startswith(f"e{fs._tag(e)}_")] == [np.nextafter(p, 0.0), np.nextafter(p, np.inf), p / 3.0]
    for c in CASES:
        for inside in (False, True):
            cam = c.camera(inside)
            assert (cam.width, cam.height, cam.projection) == (fs.FRAME_W, fs.FRAME_H, c.proj), c
            assert cam.step_dist == c.cam_step == 0.2 * c.unit and c.params.grid_width == (1.0 if c.sweep in ("OFFSET", "SUN") else c.unit)
        if c.sweep != "OFFSET":
            assert (c.params.min_height, c.params.max_height, c.base) == (0.0, 8.0 * c.unit, 0.0)
        else:
            assert c.base in (1e6, 1e9, -2e6 + 128.0 / 255.0 * 2e6, -2e9 + 128.0 / 255.0 * 2e9) and c.params.grid_width == 1.0
    # every length of a P2 member is the unit one times 2^k, exactly
    for proj in (1, 2, 3):
        u = fs.unit_case(proj)
        for c in fs.sweep("P2", proj):
            for inside in (False, True):
                a, b = c.camera(inside), u.camera(inside)
                assert list(a.pos) == [np.ldexp(v, c.k) for v in b.pos] and a.ortho_width == np.ldexp(b.ortho_width, c.k)
            assert (c.sun_step, c.mirror_step, c.cell_step, c.cell_lift) == tuple(np.ldexp(v, c.k) for v in (u.sun_step, u.mirror_step, u.cell_step, u.cell_lift))
            assert c.cell_point == tuple(np.ldexp(v, c.k) for v in u.cell_point) and c.sun_dir == fs.SUN_DIR
    # SUN: the shadow and cell rays' step vectors are the unit ones
    for c in fs.sweep("SUN"):
        u = fs.unit_case(c.proj)
        assert [c.sun_step * v for v in c.sun_dir] == [u.sun_step * v for v in u.sun_dir]
        assert [c.cell_step * v for v in c.cell_dir] == [u.cell_step * v for v in u.cell_dir]
        assert bytes(c.params) == bytes(u.params) and bytes(c.camera(True)) == bytes(u.camera(True))
    # the generator is deterministic
    again = fs._build()
    assert [(bytes(c.params), bytes(c.camera(False)), bytes(c.camera(True)), c.sun_dir, c.sun_step) for c in again] == \
           [(bytes(c.params), bytes(c.camera(False)), bytes(c.camera(True)), c.sun_dir, c.sun_step) for c in CASES]


def _is_clamped(c):
    return c.sweep == "P2" and abs(c.k) >= 510 and c.k != -510 and c.k != -530


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_conditions_on_the_replay(replays, c):
    """Conditions on the inputs, per case and family: a pose that misses one is tuned in family_scale.py, and what the extreme
    members give instead of a condition is asserted, not skipped."""
    R = replays
    hits = misses = 0
    for inside in (False, True):
        prim = R.primary(c, inside)
        h, m, capped = fs.hit_counts(prim)
        hits, misses = hits + h, misses + m
        assert capped == 0, (c, inside)
        # lit
        shadowed, unshadowed, capped = fs.lit_counts(R.lit(c, inside))
        assert capped == 0
        if c.sweep == "SUN" and c.sun_pow >= 512:
            assert shadowed == 0 and (R.lit(c, inside)["shadow"]["steps"] == 0).all(), "the first position is off the grid: no shadow ray takes a load"
        elif c.sweep == "SUN" and c.sun_pow == 3:
            # a first position 0.08 |dir| grid widths along the ray: neither the unit one nor off the grid
            other = (R.lit(c, inside)["shadowed"] != R.lit(fs.unit_case(c.proj), inside)["shadowed"]).sum()
            assert shadowed >= 30 and unshadowed >= 30 and other >= 1, (c, inside, shadowed, unshadowed, int(other))
        else:
            assert shadowed >= 30 and unshadowed >= 30, (c, inside, shadowed, unshadowed)
        # shaded
        want = R.shaded(c, inside)
        q = np.unique(want["q"][prim["status"] == lr.HIT]).tolist()
        if c.sweep != "SUN":
            assert len(q) >= 40, (c, inside, len(q))
        elif c.sun_pow == 512:
            # s.s is finite, (n.n) * (s.s) overflows on every slope with n.n > 1.36: 0 there, the unit level on flatter ground
            uq = R.shaded(fs.unit_case(c.proj), inside)["q"][prim["status"] == lr.HIT]
            cq = want["q"][prim["status"] == lr.HIT]
            assert len(q) >= 40 and ((cq == uq) | (cq == 0)).all() and (cq != uq).sum() >= 50, (c, inside, len(q))
        elif c.sun_pow >= 520:
            assert q == [0]
        elif c.sun_pow == -600:
            assert q == [0, 255]
        elif c.sun_pow == -535:
            # s.s keeps 4 bits, the product is rounded to that grid before the root
            uq = R.shaded(fs.unit_case(c.proj), inside)["q"]
            assert len(q) >= 40 and (want["q"] != uq)[prim["status"] == lr.HIT].sum() >= 50, (c, inside, len(q))
        else:
            uq = R.shaded(fs.unit_case(c.proj), inside)["q"]
            assert len(q) >= 40 and np.array_equal(want["q"], uq), "2^-520, 2^3: the unit levels (at 2^-520 through a denormal s.s)"
        assert R.shaded(c, inside, shadows=False)["capped"] == 0
        # water
        wet, dry, mirror_hits, capped = fs.water_counts(R.water(c, inside))
        assert wet >= 30 and dry >= 30 and mirror_hits >= 20 and capped == 0, (c, inside, wet, dry, mirror_hits, capped)
        # haze
        for sky in (False, True):
            want = R.haze(c, inside, sky=sky)
            own = R.haze_bounds(c, inside)[2]
            idx = want["index"][want["hit"]]
            if _is_clamped(c):
                r, hit = R.ranges(c, inside)
                assert not own and want["capped"] == 0
                if c.k > 0:
                    # (at 2^510 a few squares stay finite -- 7 of the inside spherical camera's 809 hits, the nearest hits of the
                    # orthographic planes -- and at 2^900 none)
                    far = np.isinf(r[hit])
                    assert (idx[far] == N - 1).all() and far.sum() >= 0.6 * far.size and (c.k == 510 or far.all()), (c, inside, int(far.sum()))
                else:
                    assert (r[hit] == 0.0).all() and (idx == 0).all()
            else:
                assert own
                # (the outside and the inside camera together see 100 of each kind; haze_cases.check asks it of every frame)
                hc.check(want)
        # geometry: the planes exist for every case; what the float range plane holds at the members picked for it
        if c.sweep == "P2":
            r, hit = R.ranges(c, inside)
            zeros, denormals, normals, infs = fs.float_classes(R.planes(c, inside)["range"], hit)
            if c.k == 123 and c.proj != 1:
                assert (infs, infs + normals) == {(2, False): (58, 164), (2, True): (3, 809), (3, False): (445, 631), (3, True): (9, 130)}[(c.proj, inside)]
            if c.k == -154:
                assert zeros >= 1 and denormals >= 1 and normals == infs == 0, (c, inside, zeros, denormals)
            if c.k == -140:
                assert denormals == h and h >= 100
            if c.k == -145:
                assert denormals >= 99 and zeros + denormals == h  # (the inside orthographic camera's nearest 31 hits: zero)
            if c.k == -530:
                assert (r[hit] != 0.0).all() and (r[hit] < 2.0 ** -1000 * 2.0 ** 480).all()
    assert hits >= 100 and misses >= 100, (c, hits, misses)


CELL_CASES = [c for c in CASES if c.proj == 3]  # (a cell map has no camera: one projection's members are every member)


@pytest.mark.parametrize("c", CELL_CASES, ids=[c.name for c in CELL_CASES])
def test_cell_map_conditions(replays, c):
    """Both statuses in at least a tenth of the cells -- or what the first position, pos + (0.01 * grid_width) * dir, does instead.
    In point mode dir = O - pos, so a ray starts the fraction 0.01 * grid_width of the way to O: a viewshed means what it says
    while grid_width < 100.  2^5 is on the near side (the ray starts 0.32 of the way: still hits and visible cells, a tenth of
    each), 2^7 on the far side (it starts 1.28 of the way, beyond O, and marches on away from it: no cell is hidden, those that
    end inside the grid and those that leave it make a tenth each); from 2^15 every ray has left the grid before its first load.
    A direction map has the same first position: every ray towards a sun of magnitude 2^512 or more starts off the grid."""
    tenth = fs.MAP_W * fs.MAP_H // 10
    for point in (False, True):
        status = replays.cell_status(c, point)
        n = {k: int((status == v).sum()) for k, v in (("miss", cmr.MISS), ("hit", cmr.HIT), ("capped", cmr.CAPPED), ("end", cmr.END))}
        assert n["capped"] == 0
        assert c.params.grid_width <= 32.0 or c.params.grid_width >= 128.0  # (the members next to 100: 32 and 128)
        beyond = point and c.params.grid_width >= 128.0
        gone = (c.unit >= 2.0 ** 15) if point else (c.sun_pow >= 512)
        if gone:
            assert n["miss"] == status.size, (c, point, n)
        elif beyond:
            assert c.k == 7 and n["hit"] == 0 and n["miss"] >= tenth and n["end"] >= tenth, (c, n)
        else:
            assert n["hit"] >= tenth and n["miss"] + n["end"] >= tenth, (c, point, n)
        weights = np.unique(replays.cell_weight(c, point)).size
        if not gone and not (c.sweep == "SUN" and not point and c.sun_pow == -600) and not (point and c.k == -900):
            assert weights >= 40, (c, point, weights)


def _same_records_scaled(a, b, k):
    """Records a of the 2^k member against the unit member's b: everything but the lengths equal, the lengths times 2^k."""
    for f in ("steps", "cell_x", "cell_y", "rgba", "status"):
        assert np.array_equal(a[f], b[f]), f
    assert np.array_equal(_bits(a["point"]), _bits(np.ldexp(b["point"], k)))
    assert np.array_equal(_bits(a["entry_d"]), _bits(np.ldexp(b["entry_d"], k)))


@pytest.mark.parametrize("proj", [2, 3], ids=["sph", "ortho"])
def test_p2_invariance_of_every_replay(replays, proj):
    """Scaling every length by 2^k scales every intermediate of every replay by 2^k exactly while nothing over- or underflows:
    NEAREST and BILINEAR frames, statuses, levels and weights are the unit ones at every k of the sweep; points and entry
    distances are the unit ones times 2^k; the range's doubles are for |k| <= 490.  Where invariance breaks, what happens
    instead (perspective is left out: its image plane lies a unit `look` from the camera at every scale): the float table (HMRM_NEAREST_F32) holds from 2^-140 to 2^123 only, the range is 0 or inf at the far ends."""
    R, u = replays, fs.unit_case(proj)
    for c in fs.sweep("P2", proj):
        k = c.k
        for inside in (False, True):
            for sampling in (0, 1):
                _same_records_scaled(R.primary(c, inside, sampling), R.primary(u, inside, sampling), k)
                for f in ("rgba", "shadowed"):
                    assert np.array_equal(R.lit(c, inside, sampling)[f], R.lit(u, inside, sampling)[f]), (c, f)
                for shadows in (True, False):
                    for f in ("rgba", "q", "w"):
                        assert np.array_equal(R.shaded(c, inside, sampling, shadows)[f], R.shaded(u, inside, sampling, shadows)[f]), (c, f)
                for f in ("rgba", "water"):
                    assert np.array_equal(R.water(c, inside, sampling)[f], R.water(u, inside, sampling)[f]), (c, f)
                a, b = R.planes(c, inside, sampling), R.planes(u, inside, sampling)
                assert np.array_equal(a["cell"], b["cell"]) and a["slope"].tobytes() == b["slope"].tobytes(), c
                r, hit = R.ranges(c, inside, sampling)
                r0, _ = R.ranges(u, inside, sampling)
                if abs(k) <= 490:
                    assert np.array_equal(_bits(r[hit]), _bits(np.ldexp(r0[hit], k))), c
                    assert np.array_equal(R.haze(c, inside, sampling)["rgba"], R.haze(u, inside, sampling)["rgba"]), c
                elif k in (-510, -530):
                    assert (r[hit] != 0.0).all() and np.isfinite(r[hit]).all()
                elif k > 0:
                    assert np.isinf(r[hit]).sum() >= 0.6 * hit.sum() and (k == 510 or np.isinf(r[hit]).all())
                else:
                    assert (r[hit] == 0.0).all()
            # the float table
            f32, f32u = R.primary(c, inside, 2), R.primary(u, inside, 2)
            same = all(np.array_equal(f32[f], f32u[f]) for f in ("steps", "cell_x", "cell_y", "rgba", "status"))
            pixels = int((f32["rgba"] != f32u["rgba"]).any(axis=1).sum())
            if 0 <= k <= 123:
                assert same, c
            elif k == -140:
                # every threshold is a float denormal with 12 bits left: the frame is the unit one (none of the two orthographic
                # and of the outside spherical camera's pixels differs), a few rays take another step
                assert pixels == 0 and int((f32["steps"] != f32u["steps"]).sum()) <= 1, c
            elif k == -145:
                assert 1 <= pixels <= 12, (c, pixels)
            elif k >= 490:
                # every threshold is +inf or, over the zero-height cells, 0: a ray that enters over any other cell hits at once
                assert not same and (f32["status"] == lr.HIT).sum() > (f32u["status"] == lr.HIT).sum(), c
                assert (f32["steps"][f32["status"] == lr.HIT] == 1).mean() > 0.9, c
            else:
                # (from -154 down) every threshold is 0: a ray hits only where it has left the box through its floor, over the grid
                assert k <= -154 and not same and (f32["point"][f32["status"] == lr.HIT, 2] < 0.0).all(), c
    for c in fs.sweep("P2", 3):
        for sampling in (0, 1):
            assert np.array_equal(R.cell_status(c, False, sampling), R.cell_status(fs.unit_case(3), False, sampling)), c
            assert np.array_equal(R.cell_weight(c, False, sampling), R.cell_weight(fs.unit_case(3), False, sampling)), c


@pytest.mark.parametrize("k", P2_ENDS)
def test_scalar_loop_agrees_at_the_ends(replays, k):
    """segment_replay.scalar_ray against the vectorised replay on 64 rays: the two had only met at unit scale."""
    c = fs.p2(2, k)
    rays = replays.odd_rays(c)
    pick = np.random.RandomState(11).permutation(rays.shape[0])[:64]
    per = np.random.RandomState(9).choice([0, 0, 3, 11, 60], size=64)
    vec = sr.replay(rays[pick], replays.heights(c), c.cmap, c.params, c.cam_step, bg=fs.BG, interior=True, step_cap=700, per_ray=per)
    assert len(set(vec["status"].tolist())) >= 3
    for i, ray in enumerate(rays[pick]):
        status, steps, point, cell, rgba, dist = sr.scalar_ray(ray, replays.heights(c), c.cmap, c.params, c.cam_step, fs.BG, 700, True, int(per[i]))
        one = np.zeros(1, dtype=sr.RAY_HIT_DTYPE)
        one["point"], one["entry_d"], one["steps"], one["cell_x"], one["cell_y"] = point, dist, steps, cell[0], cell[1]
        one["rgba"], one["status"] = rgba, status
        if np.isnan(dist) and np.isnan(vec["entry_d"][i]):
            one["entry_d"] = vec["entry_d"][i]  # (a generated NaN's sign is the machine's)
        assert one.tobytes() == vec[i:i + 1].tobytes(), (i, ray, one, vec[i])


@pytest.mark.parametrize("inside", [False, True], ids=["outside", "inside"])
@pytest.mark.parametrize("proj,k", [(1, fs.P2_K[0]), (1, fs.P2_PERSP_MAX_K)] + [(p, k) for p in (2, 3) for k in P2_ENDS],
                         ids=lambda v: str(v))
def test_host_frame_record_at_the_ends(hmrm, oracle, proj, k, inside):
    """hmrm_debug_frame at 2^-900 and 2^900 (perspective: 2^24) for both cameras against the oracle's record, as
    tests/test_world_scale_cpu.py does for the plain frame's pose."""
    c = fs.p2(proj, k)
    cam = c.camera(inside)
    rec = hmrm.debug_frame(cam, c.params, fs.MAP_W, fs.MAP_H)
    o = oracle.frame_record(oracle.make_cfg(cam, c.params, fs.MAP_W, fs.MAP_H))
    fields = [("cam", 0), ("c0", 15), ("c1", 18)] + ([("upper_left", 3), ("plane_right", 6), ("plane_down", 9)] if proj != 2 else [])
    fields += [("look", 12)] if proj == 3 else []
    for key, at in fields:
        got, want = np.asarray(rec[key]), o[at:at + 3]
        assert np.array_equal(_bits(got), _bits(want)), key
        assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.array_equal(got != 0.0, want != 0.0), key
    assert _bits(rec["nudge"]) == _bits(o[21]) and np.isfinite(rec["nudge"]) and rec["nudge"] != 0.0
    assert rec["step_dist"] == cam.step_dist and rec["grid_pow2"] == 1 and rec["inv_grid_width"] == 1.0 / c.params.grid_width
    if proj == 2:
        cfg = oracle.make_cfg(cam, c.params, fs.MAP_W, fs.MAP_H)
        for px, py in ((0, 0), (cam.width - 1, cam.height - 1), (21, 14), (5, 27)):
            _, d, _ = oracle.probe_ray(cfg, px, py)
            got = [rec["row_sin_va"][py] * rec["col_cos_ha"][px], rec["row_sin_va"][py] * rec["col_sin_ha"][px], rec["row_cos_va"][py]]
            assert np.array_equal(_bits(got), _bits(d)), (px, py)


@pytest.mark.parametrize("sweep", fs.SWEEPS)
def test_compositions_on_the_replay(replays, sweep):
    """The compositions the GPU module runs on each sweep's ends and middle: no capped ray, a light plane and a baked frame with
    content, three views that differ -- and for P2 the unit member's bytes."""
    import world_scale as ws
    R = replays
    for proj in (1, 2, 3):
        for c in ws.ends_and_middle(fs.sweep(sweep, proj)):
            for inside in (False, True):
                hit = R.primary(c, inside)["status"] == lr.HIT
                want = R.lit_sum(c, inside)
                assert want["capped"] == 0 and (want["light"][~hit] == 0xFFFF).all()
                if c.sweep != "SUN":
                    assert np.unique(want["light"][hit]).size >= 40, c
                elif c.sun_pow == -600:
                    assert np.unique(want["light"][hit]).size >= 3, c  # (levels 0 and 255 alone, and the shadows)
                baked = R.baked(c, inside)
                assert np.unique(baked["L"][hit]).size >= (1 if c.sweep == "SUN" and c.sun_pow in (520, 600) else 2), c
                assert R.water_lit(c, inside)["capped"] == 0
                if c.sweep == "P2" and proj != 1:
                    u = fs.unit_case(proj)
                    assert np.array_equal(want["rgba"], R.lit_sum(u, inside)["rgba"]) and np.array_equal(want["light"], R.lit_sum(u, inside)["light"])
                    assert np.array_equal(baked["rgba"], R.baked(u, inside)["rgba"]), c
                    assert np.array_equal(R.water_lit(c, inside)["rgba"], R.water_lit(u, inside)["rgba"]), c
            v = R.views(c)
            assert v.shape == (3, fs.FRAME_W * fs.FRAME_H, 4) and v[0].tobytes() != v[2].tobytes() != v[1].tobytes()
            if c.sweep == "P2" and proj != 1:
                assert v.tobytes() == R.views(fs.unit_case(proj)).tobytes(), c
