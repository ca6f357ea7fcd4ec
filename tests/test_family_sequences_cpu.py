"""The family fuzzer's plan and model without a GPU (tests/deep_fuzz_families.py): the op stream of the GPU test's seed is
deterministic and reaches, within its first F ops, everything that test is there for; and the model's rules are checked by running
the fuzzer's checker over a stand-in for lib.Scene that is written here, from include/hmrm.h, on top of the numpy replays and the
oracle alone -- a correct one passes, three deliberately wrong ones are each reported at the op kinds one expects.

The stand-in owns its state (parameters, light plane, tickets, lanes, capped counters per stream, what each call stages) and asks a
deep_fuzz_families.Calc of its OWN for the replayed bytes of that state: the arithmetic is the replays' on both sides (each family's
test_*_cpu.py pins it), what is compared here is the bookkeeping around it."""
import collections
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import deep_fuzz_families as ff

HERE = os.path.dirname(os.path.abspath(__file__))
hm = ff.hm
SUITE_SEED = 20260000
F = 200   # the GPU test's op count (test_family_sequences_gpu.py imports it): the smallest multiple of 50 without a coverage gap


def _plan_only(script, seed, ops):
    r = subprocess.run([sys.executable, os.path.join(HERE, script), str(seed), str(ops), "--plan-only"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_plan_is_deterministic_and_needs_no_torch():
    a, b = _plan_only("deep_fuzz_families.py", SUITE_SEED, F), _plan_only("deep_fuzz_families.py", SUITE_SEED, F)
    assert a == b and a.count("\n") == F + 2
    assert "skipped 0" in a and "torch imported: False" in a and "plan: missing []" in a
    assert _plan_only("deep_fuzz_families.py", SUITE_SEED + 1, F) != a


def test_the_older_fuzzers_plan_is_untouched():
    """deep_fuzz_api.Plan's stream for its suite seed, by its digest: importing from that module must not have moved it."""
    import hashlib
    out = _plan_only("deep_fuzz_api.py", 20260000, 300)
    assert hashlib.sha256(out.encode()).hexdigest() == API_PLAN_SHA256


API_PLAN_SHA256 = "c496b4cc5826fece78df9e2cd70b749ffdcc1161dbb7bbc4a7b1c32bdc19b00c"


def test_F_is_the_smallest_multiple_of_50_without_a_gap():
    gaps = {}
    for f in range(50, F + 1, 50):
        plan = ff.Plan(SUITE_SEED)
        for _ in range(f):
            plan.next_op()
        gaps[f] = ff.coverage_gaps(plan.coverage())
    assert gaps[F] == [] and all(gaps[f] for f in gaps if f < F), {f: len(g) for f, g in gaps.items()}
    assert F <= 600


def test_first_F_ops_reach_everything_and_every_op_can_run():
    plan = ff.Plan(SUITE_SEED)
    ops = [plan.next_op() for _ in range(F)]
    cov = plan.coverage()
    assert ff.coverage_gaps(cov) == [], cov
    assert set(cov["kinds"]) == set(ff.OP_KINDS)
    assert 4 <= plan.n_streams <= 8 and max(op.get("st", 0) for op in ops) < plan.n_streams
    host, lent, dev, owner, plane, whole = set(), set(), set(), {}, collections.defaultdict(bool), {}
    for op in ops:
        k, s = op["k"], op.get("s")
        if k in ff.BEGIN_KINDS:
            assert not k.startswith("baked") or plane[s], op       # no baked begin without a plane
            (dev if "dev" in k else host).add(op["h"])
            owner[op["h"]] = s
        elif k == "wait":
            host.remove(op["h"])
            lent.add(op["h"])
        elif k == "release":
            lent.remove(op["h"])
        elif k == "dev_wait":
            dev.remove(op["h"])
        elif k == "baked":
            assert plane[s], op
        elif k == "refuse_baked":
            assert not plane[s], op                                  # a planned refusal, and only then
        elif k in ("set_light", "bake_light"):
            plane[s] = True
        elif k == "cell_map_sum_dev" and op.get("whole"):
            whole[s] = (op["i"], op["st"])
        elif k == "set_light_device":
            assert whole[s] == (op["src"], op["st"]) and op["src"] == op["i"] - 1, op   # the header's recipe, on the same stream
            plane[s] = True
        elif k == "clear_light":
            plane[s] = False
        if k in ("env", "reopen"):
            for x in (host, lent, dev):
                x -= {h for h in x if k == "env" or owner[h] == s}
            if k == "reopen":
                plane[s] = False
                whole.pop(s, None)
        if "rect" in op:
            x0, y0, w, h = op["rect"]
            _, mw, mh = ff.MAPS[s]
            assert 0 <= x0 and 0 <= y0 and x0 + w <= mw and y0 + h <= mh and w >= 1 and h >= 1, op
            assert (w <= 20 and h <= 12) or (op.get("whole") and s == ff.BAKE_SLOT), op
        if "cam" in op:
            c = ff.camera_of(op["cam"], SUITE_SEED)
            assert (c.width, c.height) in ff.FRAMES and op["n"] in ff.factors_of(c.width, c.height), op


# ---------------------------------------------------------------- the stand-in
def _write_rows(ptr, rows, stride):
    rows = np.ascontiguousarray(rows)
    for y in range(rows.shape[0]):
        ctypes.memmove(ptr + y * stride, rows[y].ctypes.data, rows[y].nbytes)


def _read(ptr, nbytes):
    return np.frombuffer(ctypes.string_at(ptr, nbytes), dtype=np.uint8).copy()


def _poisoned(rows, stride):
    return ff.padded(np.ascontiguousarray(rows), stride)


class ReplayScene:
    """include/hmrm.h on top of the replays, no GPU: what a correct library returns.  Launches "run" when they are enqueued, which
    the contract allows: a ticket finishes with the heights and the plane of its begin."""
    baked_tickets_read_the_plane_at_wait = False     # the three deliberate errors
    lit_sum_reuses_staged_targets = False
    lit_tickets_finish_with_the_new_heights = False

    def __init__(self, calc, slot, params):
        self.calc, self.slot, self.params = calc, slot, params
        self.map_w, self.map_h = ff.MAPS[slot][1], ff.MAPS[slot][2]
        self.plane = None
        self.tickets, self.dev, self.capped = {}, {}, collections.Counter()
        self.lane, self.lane_seen, self.lane_cum = 0, [0, 0, 0], [0, 0, 0]
        self.staged_targets = None

    # -- helpers
    @staticmethod
    def _cap():
        v = os.environ.get("HMRM_STEP_CAP")
        return int(v) if v else None

    @staticmethod
    def _report(capped, allow=False):
        if capped and not allow:
            raise hm.HmrmError(hm.HMRM_E_NOTERM, f"{capped} ray(s) reached the step cap")

    @staticmethod
    def _refuse(text):
        raise hm.HmrmError(hm.HMRM_E_ARG, text)

    @staticmethod
    def _sun(sun):
        return (tuple(sun.dir), sun.step_dist, sun.max_steps, sun.ambient, bool(sun.flags & hm.TRACE_INTERIOR))

    def _world(self):
        return self.calc.world(self.slot, self.params)

    # -- plain frames
    def render(self, cam):
        fr = self.calc.frame(self.slot, self.params, cam, 1, self._cap())
        self._report(fr.capped)
        return fr.fb

    def render_stats(self, cam, per_pixel=False, allow_capped=False):
        fr = self.calc.frame(self.slot, self.params, cam, 1, self._cap())
        s = hm.Stats()
        s.rays, s.steps, s.capped, s.hits = cam.width * cam.height, fr.total, fr.capped, 1
        return fr.fb, s, np.where(fr.steps < 0, -1 - fr.steps, fr.steps).astype(np.uint32), fr.entry

    def kernel_choice(self):
        return {"group": 1, "simple": 2, "rec": 3}.get(os.environ.get("HMRM_KERNEL"), 0)

    # -- the families' host calls
    def render_interior(self, cam, allow_capped=False):
        fb, capped = self.calc.interior(self.slot, self.params, cam, self._cap())
        self._report(capped, allow_capped)
        return fb

    def render_lit(self, cam, sun, allow_capped=False, aa=1):
        return self.render_shaded(cam, sun, diffuse=False, shadows=True, allow_capped=allow_capped, aa=aa)

    def render_shaded(self, cam, sun, diffuse=True, shadows=True, allow_capped=False, aa=1):
        fb, capped = self.calc.shaded(self.slot, self.params, cam, aa, self._sun(sun), diffuse, shadows, self._cap())
        self._report(capped, allow_capped)
        return fb

    def render_geometry(self, cam, rgba=True, cell=True, range=True, slope=True, interior=False, allow_capped=False, pad_px=0):
        want, capped = self.calc.geometry(self.slot, self.params, cam, interior, self._cap())
        self._report(capped, allow_capped)
        return {name: _poisoned(ff._rows(want[name], cam.height), (cam.width + pad_px) * elem)
                for name, elem in (("rgba", 4), ("cell", 4), ("range", 4), ("slope", 8))}

    def _lit_sum(self, cam, sun, dirs, diffuse, shadows):
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        if not 1 <= len(dirs) <= 256:
            self._refuse("n_dirs outside 1 .. 256")
        if self.lit_sum_reuses_staged_targets and self.staged_targets is not None and len(self.staged_targets) == len(dirs):
            dirs = self.staged_targets
        return self.calc.lit_sum(self.slot, self.params, cam, self._sun(sun), dirs, diffuse, shadows, self._cap())

    def render_lit_sum(self, cam, sun, dirs, diffuse=False, shadows=True, light=False, allow_capped=False, rgba=True, pad_px=0):
        fb, lp, capped = self._lit_sum(cam, sun, dirs, diffuse, shadows)
        self.staged_targets = None     # (the directions went where the targets were)
        self._report(capped, allow_capped)
        return (_poisoned(ff._rows(fb, cam.height), (cam.width + pad_px) * 4), _poisoned(ff._rows(lp, cam.height), (cam.width + pad_px) * 2))

    def _baked(self, cam, interior, factor, plane=None):
        plane = plane or self.plane
        if plane is None:
            self._refuse("hmrm_render_baked: the scene has no light plane")
        return self.calc.baked(self.slot, self.params, cam, factor, interior, plane[0], plane[1], self._cap())

    def render_baked(self, cam, interior=False, factor=1, pad_px=0, allow_capped=False):
        fb, capped = self._baked(cam, interior, factor)
        self._report(capped, allow_capped)
        return _poisoned(ff._rows(fb, cam.height), (cam.width + pad_px) * 4)

    def pick(self, cam, px, py, allow_capped=False):
        rec = self.calc.pick(self.slot, self.params, cam, px, py, self._cap())
        self._report(int(rec["status"][0] == 2), allow_capped)
        return rec[0]

    def _trace(self, rays, step_dist, bg, sampling, interior=None, max_steps=0, per_ray=None):
        heights, cmap = self._world()
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        if interior is None:
            return self.calc.rr.replay(rays, heights, cmap, self.params, step_dist, bg=bg, sampling=sampling, step_cap=self._cap() or 1 << 26)
        return self.calc.sr.replay(rays, heights, cmap, self.params, step_dist, bg=bg, sampling=sampling, step_cap=self._cap() or 1 << 26,
                                   interior=interior, max_steps=max_steps, per_ray=per_ray)

    def _batch_result(self, rec, stats, allow_capped):
        s = hm.Stats()
        s.rays, s.steps, s.hits, s.capped = rec.shape[0], int(rec["steps"].sum()), int((rec["status"] == 1).sum()), int((rec["status"] == 2).sum())
        self._report(s.capped, allow_capped)
        return (rec, s) if stats else rec

    def trace_rays(self, rays, step_dist, bg=(0, 0, 0), sampling=0, stats=False, allow_capped=False):
        return self._batch_result(self._trace(rays, step_dist, bg, sampling), stats, allow_capped)

    def trace_segments(self, rays, step_dist, bg=(0, 0, 0), sampling=0, interior=False, max_steps=0, per_ray_max_steps=None, stats=False,
                       allow_capped=False):
        return self._batch_result(self._trace(rays, step_dist, bg, sampling, interior, max_steps, per_ray_max_steps), stats, allow_capped)

    def _cells(self, target, rect, step_dist, lift, max_steps, point, weight, diffuse, shadows, sampling, ambient, many):
        flags = hm.map_flags(point, weight, diffuse, shadows)
        if (diffuse or not shadows) and not weight:
            self._refuse("DIFFUSE or NO_SHADOWS without WEIGHT")
        rect = tuple(int(v) for v in rect) if rect is not None else (0, 0, self.map_w, self.map_h)
        if many:
            t = np.ascontiguousarray(target, dtype=np.float64).reshape(-1, 3)
            if not 1 <= len(t) <= 256:
                self._refuse("cell map sum: n_targets outside 1 .. 256")
            self.staged_targets = t
            return self.calc.cell_sum(self.slot, self.params, rect, t, step_dist, lift, max_steps, flags, sampling, ambient, self._cap())
        return self.calc.cells(self.slot, self.params, rect, tuple(float(v) for v in target), step_dist, lift, max_steps, flags, sampling, ambient,
                               self._cap())

    def cell_map(self, target, step_dist, lift=0.0, max_steps=0, point=False, weight=False, diffuse=False, shadows=True, sampling=0, ambient=128,
                 rect=None, allow_capped=False, stride_bytes=None):
        out, capped = self._cells(target, rect, step_dist, lift, max_steps, point, weight, diffuse, shadows, sampling, ambient, False)
        self._report(capped, allow_capped)
        return _poisoned(out, stride_bytes or out.shape[1])

    def cell_map_sum(self, targets, step_dist, lift=0.0, max_steps=0, point=False, weight=False, diffuse=False, shadows=True, sampling=0,
                     ambient=128, rect=None, allow_capped=False, stride_bytes=None):
        out, capped = self._cells(targets, rect, step_dist, lift, max_steps, point, weight, diffuse, shadows, sampling, ambient, True)
        self._report(capped, allow_capped)
        return _poisoned(ff._rows(out, out.shape[0]), stride_bytes or 2 * out.shape[1]).view(np.uint16)

    # -- device forms: the launch "runs" at once, its capped rays go to the caller stream's counter
    def trace_rays_device(self, d_rays, n, d_hits, step_dist, bg=(0, 0, 0), sampling=0, stream=0):
        rec = self._trace(_read(d_rays, 48 * n).view(np.float64), step_dist, bg, sampling)
        self.capped[stream] += int((rec["status"] == 2).sum())
        _write_rows(d_hits, ff._rows(rec, 1), 0)

    def trace_segments_device(self, d_rays, n, d_hits, step_dist, bg=(0, 0, 0), sampling=0, interior=False, max_steps=0, d_max_steps_ptr=0,
                              stream=0):
        lim = _read(d_max_steps_ptr, 4 * n).view(np.uint32) if d_max_steps_ptr else None
        rec = self._trace(_read(d_rays, 48 * n).view(np.float64), step_dist, bg, sampling, interior, max_steps, lim)
        self.capped[stream] += int((rec["status"] == 2).sum())
        _write_rows(d_hits, ff._rows(rec, 1), 0)

    def cell_map_device(self, d_ptr, stride_bytes, target, step_dist, lift=0.0, max_steps=0, point=False, weight=False, diffuse=False,
                        shadows=True, sampling=0, ambient=128, rect=None, stream=0):
        out, capped = self._cells(target, rect, step_dist, lift, max_steps, point, weight, diffuse, shadows, sampling, ambient, False)
        self.capped[stream] += capped
        _write_rows(d_ptr, out, stride_bytes)

    def cell_map_sum_device(self, d_ptr, stride_bytes, d_targets, n_targets, step_dist, lift=0.0, max_steps=0, point=False, weight=False,
                            diffuse=False, shadows=True, sampling=0, ambient=128, rect=None, stream=0):
        staged = self.staged_targets    # (the device entry reads the caller's targets: nothing is staged)
        t = _read(d_targets, 24 * n_targets).view(np.float64).reshape(-1, 3)
        out, capped = self._cells(t, rect, step_dist, lift, max_steps, point, weight, diffuse, shadows, sampling, ambient, True)
        self.staged_targets = staged
        self.capped[stream] += capped
        _write_rows(d_ptr, ff._rows(out, out.shape[0]), stride_bytes)

    def render_geometry_device(self, cam, rgba=(0, 0), cell=(0, 0), range=(0, 0), slope=(0, 0), interior=False, stream=0):
        want, capped = self.calc.geometry(self.slot, self.params, cam, interior, self._cap())
        self.capped[stream] += capped
        for name, (ptr, stride) in (("rgba", rgba), ("cell", cell), ("range", range), ("slope", slope)):
            if ptr:
                _write_rows(ptr, ff._rows(want[name], cam.height), stride)

    def render_lit_sum_device(self, cam, sun, d_dirs, n_dirs, rgba=(0, 0), light=(0, 0), diffuse=False, shadows=True, stream=0):
        staged, self.staged_targets = self.staged_targets, None
        fb, lp, capped = self._lit_sum(cam, sun, _read(d_dirs, 24 * n_dirs).view(np.float64).reshape(-1, 3), diffuse, shadows)
        self.staged_targets = staged
        self.capped[stream] += capped
        if rgba[0]:
            _write_rows(rgba[0], ff._rows(fb, cam.height), rgba[1])
        if light[0]:
            _write_rows(light[0], ff._rows(lp, cam.height), light[1])

    def take_capped(self, stream=0, allow_capped=False):
        n = self.capped.pop(stream, 0)
        self._report(n, allow_capped)
        return n

    # -- the light plane
    def set_light(self, plane, full_scale, stride_bytes=None):
        a = np.ascontiguousarray(plane)
        stride = a.strides[0] if stride_bytes is None else int(stride_bytes)
        if not 1 <= int(full_scale) <= 65535:
            self._refuse("full_scale outside 1 .. 65535")
        if stride < self.map_w * a.itemsize or (a.dtype == np.uint16 and stride % 2):
            self._refuse("hmrm_scene_set_light: a stride below a row, or odd for 16-bit light")
        self.plane = (a[:self.map_h, :self.map_w].astype(np.uint16), int(full_scale))

    def set_light_device(self, d_ptr, stride_bytes, full_scale, u16=True, stream=0):
        rows = [_read(d_ptr + y * stride_bytes, 2 * self.map_w).view(np.uint16) for y in range(self.map_h)]
        self.plane = (np.stack(rows), int(full_scale))

    def bake_light(self, targets, step_dist, lift=0.0, max_steps=0, point=False, weight=False, diffuse=False, shadows=True, sampling=0,
                   ambient=128, allow_capped=False):
        out, capped = self._cells(targets, None, step_dist, lift, max_steps, point, weight, diffuse, shadows, sampling, ambient, True)
        self.plane = (out.copy(), (255 if weight else 1) * len(np.asarray(targets).reshape(-1, 3)))
        self._report(capped, allow_capped)

    def clear_light(self):
        self.plane = None

    def light(self):
        return (None, 0) if self.plane is None else (self.plane[0].copy(), self.plane[1])

    # -- tickets: one ring, one rotation of three lanes, capped rays per lane
    def _begin(self, make, later):
        fb, capped = make()
        lane = self.lane % 3
        self.lane += 1
        self.lane_cum[lane] += capped
        return [fb, lane, self.lane_cum[lane], later]

    def _finish(self, t, allow_capped):
        fb, lane, cum, later = t
        if later:
            fb = later()[0]
        n = max(0, cum - self.lane_seen[lane])
        self.lane_seen[lane] += n
        return fb, n

    def _host_ticket(self, make, later=None):
        self.tickets[len(self.tickets)] = self._begin(make, later)
        return len(self.tickets) - 1

    def _dev_ticket(self, make, ptr, stride, later=None):
        t = self._begin(make, later)
        if not later:
            _write_rows(ptr, ff._rows(t[0], t[0].shape[0]), stride)
        self.dev[len(self.dev)] = t + [ptr, stride]
        return len(self.dev) - 1

    def _plain(self, cam, aa):
        params, cap = self.params, self._cap()

        def make():
            fr = self.calc.frame(self.slot, params, cam, aa, cap)
            return fr.fb, fr.capped
        return make, None

    def _lit(self, cam, sun, diffuse, shadows, aa):
        params, cap, sun = self.params, self._cap(), self._sun(sun)
        make = lambda: self.calc.shaded(self.slot, params, cam, aa, sun, diffuse, shadows, cap)
        later = lambda: self.calc.shaded(self.slot, self.params, cam, aa, sun, diffuse, shadows, cap)
        return make, later if self.lit_tickets_finish_with_the_new_heights else None

    def _baked_ticket(self, cam, interior, aa):
        if self.plane is None:
            self._refuse("the scene has no light plane")
        params, cap, plane = self.params, self._cap(), self.plane
        make = lambda: self.calc.baked(self.slot, params, cam, aa, interior, plane[0], plane[1], cap)
        later = lambda: self.calc.baked(self.slot, params, cam, aa, interior, *(self.plane or plane), cap)
        return make, later if self.baked_tickets_read_the_plane_at_wait else None

    def render_begin(self, cam, no_probe=False, aa=1):
        return self._host_ticket(*self._plain(hm.Camera.from_buffer_copy(cam), aa))

    def render_shaded_begin(self, cam, sun, diffuse=True, shadows=True, aa=1, no_probe=False):
        return self._host_ticket(*self._lit(hm.Camera.from_buffer_copy(cam), sun, diffuse, shadows, aa))

    def render_baked_begin(self, cam, interior=False, aa=1, no_probe=False):
        return self._host_ticket(*self._baked_ticket(hm.Camera.from_buffer_copy(cam), interior, aa))

    def render_device_begin(self, cam, d_ptr, stride_bytes, no_probe=False, aa=1):
        return self._dev_ticket(*self._plain(hm.Camera.from_buffer_copy(cam), aa)[:1], d_ptr, stride_bytes)

    def render_shaded_device_begin(self, cam, sun, d_ptr, stride_bytes, diffuse=True, shadows=True, aa=1, no_probe=False):
        make, later = self._lit(hm.Camera.from_buffer_copy(cam), sun, diffuse, shadows, aa)
        return self._dev_ticket(make, d_ptr, stride_bytes, later)

    def render_baked_device_begin(self, cam, d_ptr, stride_bytes, interior=False, aa=1, no_probe=False):
        make, later = self._baked_ticket(hm.Camera.from_buffer_copy(cam), interior, aa)
        return self._dev_ticket(make, d_ptr, stride_bytes, later)

    def render_wait(self, t, shape, allow_capped=False, copy=True):
        fb, n = self._finish(self.tickets[t], allow_capped)
        self.tickets[t][3] = None
        self.tickets[t][0] = fb
        self._report(n, allow_capped)
        return fb.copy()

    def render_release(self, t):
        pass

    def render_device_wait(self, t, allow_capped=False):
        fb, n = self._finish(self.dev[t][:4], allow_capped)
        if self.dev[t][3]:
            _write_rows(self.dev[t][4], ff._rows(fb, fb.shape[0]), self.dev[t][5])
        self._report(n, allow_capped)

    def update(self, params):
        self.params = params

    def close(self):
        pass


class HostBackend:
    def __init__(self, oracle, seed, cls=ReplayScene):
        self.calc, self.cls = ff.Calc(oracle, seed), cls

    def scene(self, rgb, cmap, params):
        slot = [i for i, (_, w, h) in enumerate(ff.MAPS) if (h, w) == rgb.shape[:2]][0]
        return self.cls(self.calc, slot, params)

    def stream_handle(self, k):
        return k + 1

    def sync_stream(self, k):
        pass

    def buffer(self, rows, nbytes, stream=None):
        return np.full((max(rows, 1), nbytes), ff.SENTINEL, dtype=np.uint8)

    def upload(self, a, stream):
        return np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()

    def ptr(self, b):
        return b.ctypes.data

    def read(self, b, rows):
        return b[:rows]


class Recorder(ff.Runner):
    def __init__(self, *a):
        self.flagged = []
        super().__init__(*a)

    def mismatch(self, op, what):
        self.flagged.append(op)
        super().mismatch(op, what)


@pytest.fixture
def clean_env():
    old = {k: os.environ.pop(k, None) for k in ("HMRM_KERNEL", "HMRM_STEP_CAP")}
    yield
    for k, v in old.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def _run(oracle, cls=ReplayScene, ops=F, seed=SUITE_SEED):
    plan = ff.Plan(seed)
    runner = Recorder(plan, ff.Calc(oracle, seed), HostBackend(oracle, seed, cls))
    done = []
    for _ in range(ops):
        done.append(plan.next_op())
        runner.run(done[-1])
    runner.finish()
    return runner, done


def test_generated_stream_passes_on_the_replay_backed_stand_in(oracle, clean_env, capsys):
    """The first F ops over the correct stand-in: 0 mismatches, and the run-time half of the coverage list -- every device form
    with a NON-ZERO capped count taken on two caller streams -- is reached too.  Prints the wall time, which bounds the
    expectation side of the GPU test (both sides of this run compute the replays, so it is about twice that)."""
    t0 = time.time()
    runner, _ = _run(oracle)
    out = capsys.readouterr().out
    assert sum(runner.bad.values()) == 0, out[-4000:]
    assert ff.coverage_gaps(runner.plan.coverage(), runner.capped_taken) == [], dict(runner.capped_taken)
    print(f"stand-in run of {F} ops: {time.time() - t0:.1f} s, replays {runner.calc.computed}, oracle frames {runner.calc.plain.computed}")


def _begin_kind(done, flagged):
    """The begin kinds of the tickets whose waits were flagged."""
    begun = {op["h"]: op["k"] for op in done if op["k"] in ff.BEGIN_KINDS}
    return collections.Counter(begun[op["h"]] for op in flagged if op["k"] in ("wait", "dev_wait") and op["h"] in begun)


def test_checker_notices_a_baked_ticket_finished_with_the_plane_at_wait_time(oracle, clean_env, capsys):
    class Wrong(ReplayScene):
        baked_tickets_read_the_plane_at_wait = True
    runner, done = _run(oracle, Wrong)
    capsys.readouterr()
    kinds = _begin_kind(done, runner.flagged)
    assert set(runner.bad) <= {"wait", "dev_wait"} and kinds["baked_begin"] >= 1 and kinds["baked_dev_begin"] >= 1, (dict(runner.bad), kinds)
    assert set(kinds) <= {"baked_begin", "baked_dev_begin"}


def test_checker_notices_a_lit_sum_that_reuses_staged_targets(oracle, clean_env, capsys):
    class Wrong(ReplayScene):
        lit_sum_reuses_staged_targets = True
    runner, _ = _run(oracle, Wrong)
    capsys.readouterr()
    assert set(runner.bad) == {"lit_sum"}, dict(runner.bad)


def test_checker_notices_a_sun_lit_ticket_finished_with_the_new_heights(oracle, clean_env, capsys):
    class Wrong(ReplayScene):
        lit_tickets_finish_with_the_new_heights = True
    runner, done = _run(oracle, Wrong)
    capsys.readouterr()
    kinds = _begin_kind(done, runner.flagged)
    assert set(runner.bad) <= {"wait", "dev_wait"} and kinds["shaded_begin"] >= 1 and kinds["shaded_dev_begin"] >= 1, (dict(runner.bad), kinds)
    assert set(kinds) <= {"shaded_begin", "shaded_dev_begin"}
