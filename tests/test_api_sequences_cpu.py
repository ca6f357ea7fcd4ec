"""The sequence fuzzer's plan and model without a GPU (tests/deep_fuzz_api.py): the op stream of the GPU slice's seed is
deterministic and reaches, within its first F ops, everything the slice is there for -- so the slice's floor of F ops is a
coverage condition --; and the model's own rules are checked against the oracle, by running the fuzzer's checker over a stand-in
for the library that is written here, straight from include/hmrm.h, on top of the oracle alone."""
import collections
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import deep_fuzz_api as fz
from aa_box import box_filter, super_camera

HERE = os.path.dirname(os.path.abspath(__file__))
SLICE_SEED = 20260000
F = 300   # the GPU slice's floor (test_api_sequences_gpu.py imports it)


def _plan_only(seed, ops):
    r = subprocess.run([sys.executable, os.path.join(HERE, "deep_fuzz_api.py"), str(seed), str(ops), "--plan-only"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_plan_is_deterministic_and_needs_no_torch():
    a, b = _plan_only(SLICE_SEED, F), _plan_only(SLICE_SEED, F)
    assert a == b and a.count("\n") == F + 2
    assert "skipped 0" in a and "torch imported: False" in a
    assert _plan_only(SLICE_SEED + 1, F) != a


def test_first_F_ops_reach_everything_the_slice_is_for():
    plan = fz.Plan(SLICE_SEED)
    ops = [plan.next_op() for _ in range(F)]
    cov = plan.coverage()
    assert fz.coverage_gaps(cov) == [], cov
    ev = cov["events"]
    assert ev["updates_with_a_ticket_in_flight"] >= 1 and ev["arena_regrowths"] >= 1 and ev["evictions"] >= 1
    assert ev["max_repeats_of_an_eligible_record_on_one_stream"] >= 12 and ev["longest_run_of_fresh_probeable_frames"] >= 8
    assert ev["eligible_antialiased_launches"] >= 12 and ev["donor_col_halves"] >= 1 and ev["donor_row_halves"] >= 1
    assert 4 <= plan.n_streams <= 8 and max(op.get("st", 0) for op in ops) < plan.n_streams
    # every op can run: a wait names a ticket in flight, a release a lent frame (skipped ops = 0 by construction)
    host, lent, dev, owner = set(), set(), set(), {}
    for op in ops:
        k = op["k"]
        if k in ("begin", "dev_begin"):
            (host if k == "begin" else dev).add(op["h"])
            owner[op["h"]] = op["s"]
        elif k == "wait":
            host.remove(op["h"])
            lent.add(op["h"])
        elif k == "release":
            lent.remove(op["h"])
        elif k == "dev_wait":
            dev.remove(op["h"])
        elif k in ("env", "reopen"):   # (both collect what is in flight first: all of it, or the scene's)
            for x in (host, lent, dev):
                x -= {h for h in x if k == "env" or owner[h] == op["s"]}


def test_mirror_of_the_record_cache():
    """The coverage bookkeeping itself: 64 records per stream, least recently used out first; a wider spherical camera
    regrows the arena and drops the spherical records only."""
    ev = collections.Counter()
    m = fz.CtxMirror()
    cams = [fz.hm.Camera.make(width=8 + i, height=8, projection=1) for i in range(70)]
    for i, c in enumerate(cams[:64]):
        m.launch(i, c, ev)
    m.launch(0, cams[0], ev)                 # touched: the oldest is now record 1
    m.launch(64, cams[64], ev)
    assert ev["evictions"] == 1 and 0 in m.slots and 1 not in m.slots
    s1 = fz.hm.Camera.make(width=16, height=16, projection=2)
    s2 = fz.hm.Camera.make(width=64, height=16, projection=2)
    m.launch("s1", s1, ev)
    assert ev["arena_regrowths"] == 0 and m.arena == 64
    m.launch("s2", s2, ev)
    assert ev["arena_regrowths"] == 1 and "s1" not in m.slots and 0 in m.slots and m.arena == 160


# ---------------------------------------------------------------- the model's rules against the oracle
def _write(ptr, arr):
    ctypes.memmove(ptr, np.ascontiguousarray(arr).ctypes.data, arr.nbytes)


class OracleScene:
    """include/hmrm.h on top of the oracle, no GPU: what a correct library returns.  Launches "run" when they are enqueued,
    which the contract allows (a ticket begun before an update finishes with the old heights)."""
    new_heights_for_tickets = False   # the deliberate error of test_checker_notices_...: tickets finish with the heights at wait time

    def __init__(self, oracle, rgb, cmap, params):
        self.o, self.rgb, self.cmap, self.params = oracle, rgb, cmap, params
        self.tickets, self.dev, self.capped = {}, {}, collections.Counter()
        self.lane, self.lane_seen, self.lane_cum = 0, [0, 0, 0], [0, 0, 0]

    def _render(self, cam, n=1, rows=None, params=None):
        params = params or self.params
        cap = int(os.environ.get("HMRM_STEP_CAP", self.o.DEFAULT_STEP_CAP))
        cfg = self.o.make_cfg(super_camera(fz.hm, cam, n), params, self.cmap.shape[1], self.cmap.shape[0], step_cap=cap)
        fb, total, capped, steps, entry = self.o.render(cfg, self.o.update_heightmap(self.rgb, params), self.cmap, per_pixel=True, rows=rows)
        return (box_filter(fb, n) if n > 1 else fb), total, capped, steps, entry

    def _report(self, capped):
        if capped:
            raise fz.hm.HmrmError(fz.hm.HMRM_E_NOTERM, f"{capped} ray(s) reached the step cap")

    def _stats(self, cam, n, total, capped):
        s = fz.hm.Stats()
        s.rays, s.steps, s.capped, s.hits = n * n * cam.width * cam.height, total, capped, 1
        return s

    def render(self, cam):
        fb, _, capped, *_ = self._render(cam)
        self._report(capped)
        return fb

    def render_aa(self, cam, n, stats=False, allow_capped=False):
        fb, total, capped, *_ = self._render(cam, n)
        if not allow_capped:
            self._report(capped)
        return (fb, self._stats(cam, n, total, capped)) if stats else fb

    def render_stats(self, cam, per_pixel=False, allow_capped=False):
        fb, total, capped, steps, entry = self._render(cam)
        return fb, self._stats(cam, 1, total, capped), np.abs(np.where(steps < 0, steps + 1, steps)).astype(np.uint32), entry

    def render_cycle(self, cam, framebuf, cycle, period):
        fb, _, capped, *_ = self._render(cam)
        flat, src = framebuf.reshape(-1, 4), fb.reshape(-1, 4)
        for p in range(cycle, cam.width * cam.height, period):
            flat[p] = src[p]
        self._report(capped)

    def _begin(self, cam, aa):
        fb, _, capped, *_ = self._render(cam, aa)
        lane = self.lane % 3
        self.lane += 1
        self.lane_cum[lane] += capped
        return fb, lane, self.lane_cum[lane]

    def render_begin(self, cam, no_probe=False, aa=1):
        t = len(self.tickets)
        self.tickets[t] = self._begin(cam, aa) + (fz.hm.Camera.from_buffer_copy(cam), aa)
        return t

    def render_wait(self, t, shape, allow_capped=False, copy=True):
        fb, lane, cum, cam, aa = self.tickets[t]
        if self.new_heights_for_tickets:
            fb = self._render(cam, aa)[0]
        n = max(0, cum - self.lane_seen[lane])
        self.lane_seen[lane] += n
        self._report(n)
        return fb.copy()

    def render_release(self, t):
        pass

    def render_device_begin(self, cam, ptr, stride, no_probe=False, aa=1):
        fb, lane, cum = self._begin(cam, aa)
        for y in range(cam.height):
            _write(ptr + y * stride, fb[y])
        self.dev[len(self.dev)] = (lane, cum)
        return len(self.dev) - 1

    def render_device_wait(self, t):
        lane, cum = self.dev[t]
        n = max(0, cum - self.lane_seen[lane])
        self.lane_seen[lane] += n
        self._report(n)

    def render_rows_device(self, cam, ptr, stride, row_begin=0, row_end=0, band_rows=0, band_index=0, band_count=1, stream=0):
        if band_rows > 0:
            starts = list(range(band_index * band_rows, cam.height, band_count * band_rows))
            spans = [(r0, min(r0 + band_rows, cam.height), j * band_rows) for j, r0 in enumerate(starts)]
        else:
            spans = [(row_begin, row_end, 0)]
        for r0, r1, at in spans:
            fb, _, capped, *_ = self._render(cam, rows=(r0, r1))
            self.capped[stream] += capped
            for y in range(r0, r1):
                _write(ptr + (at + y - r0) * stride, fb[y])

    def take_capped(self, stream=0, allow_capped=False):
        n = self.capped.pop(stream, 0)
        if not allow_capped:
            self._report(n)
        return n

    def kernel_choice(self):
        return {"group": 1, "simple": 2, "rec": 3}.get(os.environ.get("HMRM_KERNEL"), 0)

    def update(self, params):
        self.params = params

    def close(self):
        pass


class HostBackend:
    def __init__(self, oracle, cls=OracleScene):
        self.oracle, self.cls = oracle, cls

    def scene(self, rgb, cmap, params):
        return self.cls(self.oracle, rgb, cmap, params)

    def stream_handle(self, k):
        return k + 1

    def sync_stream(self, k):
        pass

    def buffer(self, rows, nbytes, stream=None):
        return np.full((max(rows, 1), nbytes), fz.SENTINEL, dtype=np.uint8)

    def ptr(self, b):
        return b.ctypes.data

    def read(self, b, rows):
        return b[:rows]


@pytest.fixture
def clean_env():
    old = {k: os.environ.pop(k, None) for k in ("HMRM_KERNEL", "HMRM_STEP_CAP")}
    yield
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _hand_made_ops(plan):
    """begin, update, wait: the old heights; two progressive refreshes out of sequence; a strip of packed bands on a caller's
    stream into a buffer wider than the row, checked after the sync."""
    cam = ("p", 0, 0)
    return [{"k": "begin", "s": 0, "cam": cam, "n": 2, "h": 1, "no_probe": False},
            {"k": "update", "s": 0, "p": (plan.scenes[0].pidx + 1) % fz.N_PARAMS},
            {"k": "wait", "s": 0, "h": 1},
            {"k": "cycle", "s": 0, "cam": ("p", 0, 1), "n": 1, "period": 7, "cycle": 5},
            {"k": "cycle", "s": 0, "cam": ("p", 0, 1), "n": 1, "period": 3, "cycle": -1},
            {"k": "rows", "s": 0, "cam": ("p", 0, 1), "n": 1, "st": 2, "pad": 3, "h": 2, "rb": 0, "re": 37,
             "band": (5, 1, 3)},
            {"k": "sync", "st": 2}, {"k": "release", "s": 0, "h": 1}]


def _run(oracle, ops_of, cls=OracleScene, seed=7):
    plan = fz.Plan(seed)
    runner = fz.Runner(plan, fz.Expect(oracle, seed), HostBackend(oracle, cls))
    for op in ops_of(plan):
        runner.run(plan._emit(op) if "i" not in op else op)
    runner.finish()
    return runner


def test_model_rules_on_a_hand_made_sequence(oracle, clean_env, capsys):
    runner = _run(oracle, _hand_made_ops)
    assert sum(runner.bad.values()) == 0, capsys.readouterr().out
    # ... and what the model expected is what the contract says, computed here once more from the oracle
    plan = fz.Plan(7)
    p0, p1 = plan.scenes[0].pidx, (plan.scenes[0].pidx + 1) % fz.N_PARAMS
    rgb, cmap = fz.build_map(0, 7)
    cam = fz.camera_pool(0, 7)[1]
    assert (cam.width, cam.height) == (53, 37)
    fb, *_ = oracle.render(oracle.make_cfg(cam, fz.scene_params(p1), 64, 64), oracle.update_heightmap(rgb, fz.scene_params(p1)), cmap)
    (buf, want, nxt), = runner.cycles.values()
    p = np.arange(53 * 37).reshape(37, 53)
    touched = (p % 7 == 5) | (p % 3 == 0)      # (after cycle 5 the next one in sequence is 6 mod 3 = 0)
    assert np.array_equal(want[touched], fb[touched]) and (want[~touched] == fz.SENTINEL).all() and nxt == 1
    strip, capped = fz.expected_strip(fz.Frame(fb, 0, 0, np.zeros((37, 53), dtype=np.int64), None), 53, 56, 0, 37, (5, 1, 3))
    assert strip.shape == (fz.hm.band_local_rows(37, 5, 1, 3), 56 * 4) == (15, 224) and capped == 0
    rows = [5, 6, 7, 8, 9, 20, 21, 22, 23, 24, 35, 36]   # bands 1, 4, 7 of five rows; the last one is cut by the frame's end
    assert np.array_equal(strip[:12, :212], fb[rows].reshape(12, 212))
    assert (strip[12:] == fz.SENTINEL).all() and (strip[:, 212:] == fz.SENTINEL).all()
    old = oracle.render(oracle.make_cfg(super_camera(fz.hm, fz.camera_pool(0, 7)[0], 2), fz.scene_params(p0), 64, 64),
                        oracle.update_heightmap(rgb, fz.scene_params(p0)), cmap)[0]
    new = oracle.render(oracle.make_cfg(super_camera(fz.hm, fz.camera_pool(0, 7)[0], 2), fz.scene_params(p1), 64, 64),
                        oracle.update_heightmap(rgb, fz.scene_params(p1)), cmap)[0]
    assert not np.array_equal(old, new)   # (the update does change this frame, so the rule is really tested)


def test_checker_notices_a_ticket_finished_with_the_new_heights(oracle, clean_env, capsys):
    class Wrong(OracleScene):
        new_heights_for_tickets = True
    runner = _run(oracle, _hand_made_ops, Wrong)
    out = capsys.readouterr().out
    assert dict(runner.bad) == {"wait": 1} and "MISMATCH seed 7 op 2" in out and "host ticket" in out


def test_checker_notices_a_frame_record_that_outlives_an_update(oracle, clean_env, capsys):
    """A stand-in whose frames keep the parameters the camera was first rendered under on that map -- a record that survives
    every hmrm_scene_update and every reopen -- is caught within the slice's first F ops: the cameras do not depend on the
    scene's parameters, so the same camera bytes come back after an update, on the own stream, the lanes and caller streams."""
    first_params = {}

    class Stale(OracleScene):
        def _render(self, cam, n=1, rows=None, params=None):
            key = (self.rgb.tobytes(), bytes(super_camera(fz.hm, cam, n)))
            return super()._render(cam, n, rows, first_params.setdefault(key, self.params))

    def first(plan):
        for _ in range(F):
            yield plan.next_op()
    runner = _run(oracle, first, Stale, seed=SLICE_SEED)
    out = capsys.readouterr().out
    assert sum(runner.bad.values()) >= 3 and "MISMATCH seed" in out
    assert {"render", "render_aa"} & set(runner.bad) and {"wait", "dev_wait"} & set(runner.bad) and "rows" in runner.bad, dict(runner.bad)


def test_generated_stream_passes_on_the_oracle_backed_stand_in(oracle, clean_env, capsys):
    """The fuzzer's first ops, every kind among them and step caps of 60 and 200, over the stand-in: the checker and the
    contract agree (capped counts per call, per launch lane and per caller stream included)."""
    def first(plan):
        for _ in range(130):
            yield plan.next_op()
    runner = _run(oracle, first, seed=SLICE_SEED)
    assert sum(runner.bad.values()) == 0, capsys.readouterr().out[-3000:]
    assert runner.plan.cover["kinds"]["env"] >= 2 and runner.exp.computed >= 40
