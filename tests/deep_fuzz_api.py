"""Model-based fuzz of whole API call sequences against the CPU oracle (the host state of csrc/api_*.cpp: per-stream caches of
frame records, the spherical-table arena and donor halves, launch-order calibration and both kernel probes, ticket rings and
launch lanes, capped counters per stream, hmrm_scene_update with frames in flight, antialiased frames sharing a record with the
plain frame of the super camera).  Test infrastructure, not collected by pytest:

    python tests/deep_fuzz_api.py <seed> <ops> [seconds] [--plan-only]

One seeded stream of operations drives the library and a model side by side; every byte that comes back from any entry point is
compared with what the model expects from the oracle (antialiased frames: the oracle's super frame through tests/aa_box.py).
Prints one line per mismatch with what is needed to replay it (seed, op index, the last 40 ops) and the summary line
`api: ops N, mismatches M, per-kind {...}`; exit status 1 on any mismatch, 2 when the library reports a device error (nothing
is run after that).  --plan-only prints the op stream and the model's bookkeeping without torch or a GPU.

What the model knows (include/hmrm.h): a ticket begun before an update finishes with the OLD heights; hmrm_render_cycle rewrites
pixels p = cycle (mod period) and nothing else; strips hold rows [row_begin, row_end) or the packed cyclic bands; bytes between
width*4 and the stride and rows outside a strip keep the sentinel they were filled with; rays = n^2 W H, steps / capped are the
oracle's sums, per-pixel steps and distance() bits the oracle's; a step cap is reported (HMRM_E_NOTERM with the count) by the
call that rendered the frame, by a wait on a ticket of its launch lane (hmrm_render_wait in include/hmrm.h: at the latest by
the frame's own ticket, maybe by an earlier wait on the lane; under a cap the `render` op compares the count only, the
instrumented calls the pixels too) or by hmrm_scene_take_capped for the caller's stream it was enqueued on.
Two things the oracle does not pin: kernel_choice() depends on timing and is only required to be 0, 1 or 3 (or the forced
HMRM_KERNEL), and `hits` is not reported by the oracle, so it is only required to be the same for every render of the same
frame under the same cap.

The fuzzer obeys the ABI itself: caller streams with strips of a scene in flight are synchronised before that scene is updated
or closed, host-pixel calls are made one at a time, and the environment knobs change only while nothing is in flight (the `env`
op drains every ticket and stream first -- checking what they deliver -- and is one op).  The generator only emits ops that can
run (no wait without a ticket): no op is ever skipped."""
import collections
import importlib
import os
import sys
import time

if __name__ == "__main__" and "--plan-only" in sys.argv:
    os.environ.setdefault("HMRM_NO_TORCH_PRELOAD", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

hm = importlib.import_module("heightmap-ray-marcher_amd")
import scenes
from aa_box import box_filter, super_camera

OP_KINDS = ("render", "render_aa", "render_aa_stats", "render_stats", "begin", "wait", "release", "dev_begin", "dev_wait", "rows",
            "sync", "take_capped", "cycle", "update", "env", "reopen")
KERNELS = (None, "leap", "group", "simple", "rec")
CAPS = (None, 60, None, 200, None)
# every PERIOD ops the stream is made to hold what a slice must reach whatever the dice say: (op index mod PERIOD, what)
PERIOD = 300
MILESTONES = {12: "burst", 40: "update", 70: "orbit", 100: "reopen", 120: "sweep", 215: "burst", 260: "orbit"}
ENV_EVERY = 36            # ... and the knobs move on: five kernel settings and the step caps within one period
SENTINEL = 0xA5
MAX_IN_FLIGHT = 12
FRAME_SLOTS = 64          # api_internal.hpp kFrameSlots: cached frame records per stream
ELIGIBLE_ROWS = 177       # 12 tile rows of 16 pixels: the smallest frame whose launch order is calibrated (api_launch.cpp launch_frame)
MAX_SUPER_PX = 40000      # keeps one oracle frame cheap
MEMO_FRAMES = 1000        # oracle frames kept (tickets in flight hold their own)
# (width, height): few distinct sizes so that records collide; some tall enough for calibration by themselves, some under a factor
SIZES = ((64, 48), (53, 37), (48, 192), (64, 208), (24, 24), (48, 48), (32, 96), (160, 40), (96, 200), (24, 24), (48, 192), (40, 30))
MAPS = (("smooth", 64, 64), ("smooth", 50, 37), ("hostile", 96, 96))   # 50 x 37 clips the last windows of every pyramid level
N_PARAMS = 4


def scene_params(pidx):
    gw = (1.0, 0.5, 0.7, 1.0)[pidx]   # (powers of two and a general width; close enough that one camera sees every box)
    lo, hi = ((0.0, 10.0), (-1.5, 6.0), (2.0, 14.0), (-1.5, 6.0))[pidx]
    lum = ((0.299, 0.587, 0.114), (1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.299, 0.587, 0.114))[pidx]
    return hm.SceneParams.make(lo * gw, hi * gw, lum=lum, grid_width=gw)


def build_map(slot, seed):
    kind, w, h = MAPS[slot]
    if kind == "smooth":
        return scenes.small_maps(w, h, seed * 8 + slot, color_heights=(slot == 1))
    # needles on a plateau or white noise: rays cannot jump over whole windows, the probes may pick the groups
    return hm.synth.content_maps(w, "needles" if seed % 2 == 0 else "white", seed)


def allowed_factors(w, h):
    return [n for n in (1, 2, 4, 8) if w * h * n * n <= MAX_SUPER_PX]


_pools = {}


NOMINAL_PIDX = 2          # the parameter set the cameras are laid out around


def camera_pool(slot, seed):
    """~100 cameras of scene `slot`, the SAME whatever the scene's parameters are -- so one camera is rendered before and after
    a height update, and a record that outlived the update would return the old frame --, built to collide: spherical ones share width + hfov + hang or
    height + vang (donor halves of the tables), widths differ so that the arena regrows, every projection and sampling mode."""
    key = (slot, seed)
    if key in _pools:
        return _pools[key]
    rng = np.random.RandomState((seed * 1000 + slot * 10) % (1 << 32))
    p = scene_params(NOMINAL_PIDX)
    gw = p.grid_width
    _, mw, mh = MAPS[slot]
    ex, ey = mw * gw, mh * gw
    span = p.max_height - p.min_height
    poses = []
    for k in range(3):
        ang = rng.uniform(0, 2 * np.pi)
        dist = (0.8 + 0.3 * k) * max(ex, ey)
        pos = (ex / 2 + dist * np.cos(ang), -ey / 2 + dist * np.sin(ang), p.max_height + p.min_height + (0.4 + 0.5 * k) * span)
        poses.append((pos, float(np.arctan2(-ey / 2 - pos[1], ex / 2 - pos[0]))))
    cams = []
    for i in range(100):
        w, h = SIZES[i % len(SIZES)]
        proj = (2, 1, 2, 3, 2, 1)[(i // len(SIZES) + i) % 6]
        pos, hang0 = poses[int(rng.randint(0, 3))]
        hfov = hm.degrees_to_rads((150.0, 120.0)[int(rng.randint(0, 2))] if proj == 2 else (80.0, 60.0)[int(rng.randint(0, 2))])
        cams.append(hm.Camera.make(width=w, height=h, projection=proj, hfov=hfov, hang=hang0 + (0.0, 0.15, -0.2)[int(rng.randint(0, 3))],
                                   vang=hm.degrees_to_rads((105.0, 120.0, 135.0)[int(rng.randint(0, 3))]), pos=pos,
                                   ortho_width=1.5 * max(ex, ey) / max(w, h), step_dist=float(rng.choice([0.25, 0.5, 0.37])) * gw,
                                   bg=tuple(int(v) for v in rng.randint(0, 256, size=3)), sampling=int((0, 0, 1, 2, 0)[int(rng.randint(0, 5))])))
    _pools[key] = cams
    return cams


# hot cameras (index into the pool, antialias factor): rendered again and again, so their records are calibrated -- by
# themselves (48 x 192, 64 x 208) or as the super frame of a small antialiased one (24 x 24 at 8, 48 x 48 at 4, 32 x 96 at 2)
HOT = ((2, 1), (4, 8), (5, 4), (3, 1), (6, 2), (14, 1), (16, 8))


def camera_of(spec, seed):
    """('p', slot, i) a pool camera; ('o', slot, i, k) frame k of a never-repeating orbit around pool camera i;
    ('S', spec, n) the super camera of another one (same cache record as its antialiased frame)."""
    if spec[0] == "p":
        return camera_pool(spec[1], seed)[spec[2]]
    if spec[0] == "o":
        c = hm.Camera.from_buffer_copy(camera_pool(spec[1], seed)[spec[2]])
        c.hang += 1e-3 * (spec[3] + 1)
        return c
    return super_camera(hm, camera_of(spec[1], seed), spec[2])


class CtxMirror:
    """What one stream context of api_launch.cpp caches (prepare_frame): 64 records, least recently used first out; the arena of
    spherical tables, regrown -- every spherical record dropped -- when a wider camera arrives.  Bookkeeping for the coverage
    report only: expected pixels never depend on it."""

    def __init__(self):
        self.slots = collections.OrderedDict()
        self.arena = 0
        self.params_of = {}   # camera bytes -> parameter sets it was rendered under on this stream (a record must not outlive an update)

    def launch(self, key, cam, ev, pidx=None, where=""):
        if pidx is not None:
            under = self.params_of.setdefault(bytes(cam), set())
            if pidx not in under:
                under.add(pidx)
                ev["cameras_under_two_parameter_sets_on_" + where] += int(len(under) == 2)
        if key in self.slots:
            self.slots.move_to_end(key)
            return
        if cam.projection == hm.SPHERICAL:
            n = 2 * cam.width + 2 * cam.height
            if n > self.arena:
                if self.arena:
                    ev["arena_regrowths"] += 1
                for k in [k for k, c in self.slots.items() if c.projection == hm.SPHERICAL]:
                    del self.slots[k]
                self.arena = (n + 31) & ~31
            for o in self.slots.values():
                if o.projection == hm.SPHERICAL and o.width == cam.width and o.hfov == cam.hfov:
                    ev["donor_col_halves"] += int(o.hang == cam.hang)
                    ev["donor_row_halves"] += int(o.height == cam.height and o.vang == cam.vang)
        self.slots[key] = cam
        if len(self.slots) > FRAME_SLOTS:
            self.slots.popitem(last=False)
            ev["evictions"] += 1


class PScene:
    def __init__(self, slot, pidx):
        self.slot, self.pidx, self.epoch = slot, pidx, 0
        self.reset()

    def reset(self):
        self.host, self.lent, self.dev = [], [], []   # handles: begun, waited but not released, device tickets in flight
        self.strips = collections.Counter()           # caller stream -> strips not yet checked
        self.ctx = collections.defaultdict(CtxMirror)
        self.lane_next = 0
        self.seen = collections.Counter()             # eligible full-frame launches per (stream context, record, knob setting)
        self.met = set()                              # records the scene has launched as eligible full frames
        self.fresh_run = 0


class Plan:
    """The seeded op stream.  Depends on the seed alone (never on what the GPU or the oracle return), so --plan-only shows exactly
    what a run will do."""

    def __init__(self, seed):
        self.seed = seed
        self.rng = np.random.RandomState(seed % (1 << 32))
        self.n_streams = 4 + seed % 5
        self.scenes = [PScene(slot, (slot + seed) % N_PARAMS) for slot in range(len(MAPS))]
        self.kernel, self.cap = None, None
        self.script = collections.deque()
        self.n = 0
        self.handle = 0
        self.orbit = 0
        self.envs = 0
        self.milestone_at = -1
        self.milestones_done = set()
        self.next_env_at = ENV_EVERY - 1
        self.cover = {"kinds": collections.Counter(), "kernels": collections.Counter(), "projections": collections.Counter(),
                      "samplings": collections.Counter(), "factors": collections.Counter()}
        self.ev = collections.Counter()

    # -- choosing
    def _cam_spec(self, sc, want_aa):
        r = self.rng.rand()
        if r < 0.3:
            i, n = HOT[int(self.rng.randint(0, len(HOT)))]
            return ("p", sc.slot, i), (n if want_aa else 1)
        i = int(self.rng.randint(0, 100))
        w, h = SIZES[i % len(SIZES)]
        fs = allowed_factors(w, h)
        return ("p", sc.slot, i), (int(fs[int(self.rng.randint(0, len(fs)))]) if want_aa else 1)

    def _frame_op(self, kind, sc, spec, n, may_probe=False):
        """The op of `kind` that renders the frame (spec, n); may_probe: a ticket never carries HMRM_NO_PROBE."""
        rng = self.rng
        if kind in ("render", "render_stats") and n > 1:
            spec, n = ("S", spec, n), 1  # the plain frame of the super camera: the antialiased frame's own record
        op = {"k": kind, "s": sc.slot, "cam": spec, "n": n}
        if kind in ("begin", "dev_begin"):
            self.handle += 1
            op.update(h=self.handle, no_probe=bool(rng.rand() < 0.25) and not may_probe)
        if kind == "dev_begin":
            op["pad"] = int(rng.choice([0, 1, 5, 16]))
        return op

    def _burst(self, sc, orbit):
        """Calibration + kernel probe (one camera 13 times on the scene's own stream -- a record and its calibration belong to one
        stream --, then up to 6 more times through tickets too) or the shadow probe (10-14 frames that never repeat, none flagged
        HMRM_NO_PROBE), through the host calls and tickets in turn; antialiased frames and the plain frame of their super camera
        share the record."""
        i, n = HOT[int(self.rng.randint(0, len(HOT)))]
        for j in range(int(self.rng.randint(10, 15)) if orbit else int(self.rng.randint(14, 20))):
            if orbit:
                self.orbit += 1
                spec = ("o", sc.slot, i, self.orbit)
            else:
                spec = ("p", sc.slot, i)
            kind = ("render", "render_aa", "render", "dev_begin", "begin", "render_aa")[int(self.rng.randint(0, 6))]
            if not orbit and j < 13 and kind in ("dev_begin", "begin"):
                kind = "render_aa"
            if kind == "render_aa" and n == 1:
                kind = "render"
            if kind in ("begin", "dev_begin") and len(sc.host) + len(sc.dev) + len([s for s in self.script if s[0] == "frame"]) >= MAX_IN_FLIGHT:
                kind = "render"
            self.script.append(("frame", kind, sc.slot, spec, n, True))
            if kind == "begin":
                self.script.extend([("wait_last", sc.slot), ("release_last", sc.slot)])
            elif kind == "dev_begin":
                self.script.append(("dev_wait_last", sc.slot))

    def _sweep(self, sc):
        """More distinct cameras than a stream caches records (eviction), on the scene's own stream."""
        pool = camera_pool(sc.slot, self.seed)
        widest = max((i for i in range(100) if pool[i].projection == hm.SPHERICAL), key=lambda i: pool[i].width + pool[i].height)
        self.script.append(("frame", "render", sc.slot, ("p", sc.slot, widest), 1))  # (the arena grows once, in front)
        i0 = int(self.rng.randint(0, 100))
        for j in range(FRAME_SLOTS + 6):
            self.script.append(("frame", "render" if j % 5 else "render_stats", sc.slot, ("p", sc.slot, (i0 + j) % 100), 1))

    def _env_op(self, kernel=False):
        self.envs += 1
        return {"k": "env", "kernel": KERNELS[(self.envs + self.seed) % len(KERNELS)] if kernel is False else kernel,
                "step_cap": CAPS[(3 * self.envs + self.seed) % len(CAPS)]}

    def _update_script(self, sc):
        """One camera on the scene's own stream, on all three launch lanes and on a caller's stream; the heights changed with the
        three tickets still in flight (they finish with the old heights); the same camera on every one of those streams again:
        a record, a table or a calibration that outlived the update would show the old frame."""
        spec, n = self._cam_spec(sc, True)
        st = int(self.rng.randint(0, self.n_streams))
        self.script.append(("frame", "render_aa" if n > 1 else "render", sc.slot, spec, n))
        self.script.extend([("frame", "begin", sc.slot, spec, n)] * 3)
        self.script.extend([("rows", sc.slot, spec, st), ("update", sc.slot, (sc.pidx + 1 + int(self.rng.randint(0, N_PARAMS - 1))) % N_PARAMS)])
        self.script.append(("frame", "render_aa" if n > 1 else "render", sc.slot, spec, n))
        self.script.extend([("frame", "dev_begin", sc.slot, spec, n)] * 3)
        self.script.append(("rows", sc.slot, spec, st))
        self.script.extend([("wait_last", sc.slot), ("release_last", sc.slot)] * 3 + [("dev_wait_last", sc.slot)] * 3)

    def next_op(self):
        rng = self.rng
        while True:
            if not self.script and self.n != self.milestone_at:
                self.milestone_at = self.n
                # (a milestone whose op index passed while a burst was running is made up for as soon as the burst ends)
                due = [(self.n // PERIOD, pos) for pos in sorted(MILESTONES) if pos <= self.n % PERIOD and (self.n // PERIOD, pos) not in self.milestones_done]
                what = None
                if due and (self.kernel == "simple" if MILESTONES[due[0][1]] == "burst" else
                            MILESTONES[due[0][1]] == "orbit" and self.kernel not in (None, "leap")):
                    self.milestone_at = -1   # (the literal loop is never calibrated, a forced kernel never probed: move the knob first)
                    return self._emit(self._env_op(kernel=None))
                if due:
                    self.milestones_done = {d for d in self.milestones_done if d[0] == due[0][0]} | {due[0]}
                    what = MILESTONES[due[0][1]]
                    self.milestone_at = -1 if len(due) > 1 else self.n
                sc = self.scenes[(self.n // 7) % len(self.scenes)]
                if what == "sweep":
                    self._sweep(sc)
                elif what == "update":
                    self._update_script(sc)
                elif what == "reopen":
                    return self._emit({"k": "reopen", "s": sc.slot, "p": int(rng.randint(0, N_PARAMS))})
                elif what:
                    self._burst(sc, what == "orbit")
                elif self.n >= self.next_env_at:
                    self.next_env_at = self.n + ENV_EVERY
                    return self._emit(self._env_op())
            if self.script:
                item = self.script.popleft()
                sc = self.scenes[item[1] if item[0] != "frame" else item[2]]
                if item[0] == "frame":
                    op = self._frame_op(item[1], sc, item[3], item[4], len(item) > 5)
                elif item[0] == "rows":
                    self.handle += 1
                    op = {"k": "rows", "s": sc.slot, "cam": item[2], "n": 1, "st": item[3], "pad": 3, "h": self.handle, "rb": 0,
                          "re": camera_of(item[2], self.seed).height, "band": None}
                elif item[0] == "update":
                    op = {"k": "update", "s": sc.slot, "p": item[2]}
                elif item[0] == "wait_last":
                    op = {"k": "wait", "s": sc.slot, "h": sc.host[-1]}
                elif item[0] == "release_last":
                    op = {"k": "release", "s": sc.slot, "h": sc.lent[-1]}
                else:
                    op = {"k": "dev_wait", "s": sc.slot, "h": sc.dev[-1]}
                return self._emit(op)
            sc = self.scenes[int(rng.randint(0, len(self.scenes)))]
            room = len(sc.host) + len(sc.dev) < MAX_IN_FLIGHT
            cand = [("render", 10), ("render_aa", 10), ("render_aa_stats", 5), ("render_stats", 6), ("rows", 9), ("sync", 4),
                    ("take_capped", 3), ("cycle", 6), ("update", 1.6), ("env", 0.4), ("reopen", 0.5), ("burst", 0.6), ("orbit", 0.6)]
            if room:
                cand += [("begin", 11), ("dev_begin", 11)]
            if sc.host:
                cand.append(("wait", 7))
            if sc.lent:
                cand.append(("release", 6))
            if sc.dev:
                cand.append(("dev_wait", 7))
            w = np.array([c[1] for c in cand], dtype=np.float64)
            kind = cand[int(rng.choice(len(cand), p=w / w.sum()))][0]
            if kind in ("burst", "orbit"):
                self._burst(sc, kind == "orbit")
                continue
            if kind in ("render", "render_stats", "begin", "dev_begin", "render_aa", "render_aa_stats"):
                aa = kind.startswith("render_aa") or (kind in ("begin", "dev_begin", "render") and rng.rand() < 0.5)
                spec, n = self._cam_spec(sc, aa)
                op = self._frame_op(kind, sc, spec, n)
            elif kind == "wait":
                op = {"k": kind, "s": sc.slot, "h": sc.host[int(rng.randint(0, len(sc.host)))]}
            elif kind == "release":
                op = {"k": kind, "s": sc.slot, "h": sc.lent[int(rng.randint(0, len(sc.lent)))]}
            elif kind == "dev_wait":
                op = {"k": kind, "s": sc.slot, "h": sc.dev[int(rng.randint(0, len(sc.dev)))]}
            elif kind == "rows":
                spec, _ = self._cam_spec(sc, False)
                H = camera_of(spec, self.seed).height
                self.handle += 1
                op = {"k": kind, "s": sc.slot, "cam": spec, "n": 1, "st": int(rng.randint(0, self.n_streams)), "pad": int(rng.choice([0, 3, 16])),
                      "h": self.handle, "rb": 0, "re": H, "band": None}
                mode = int(rng.randint(0, 4))
                if mode == 1:     # (never an empty strip: nothing would come back to compare)
                    a = int(rng.randint(0, H))
                    op.update(rb=a, re=int(rng.randint(a + 1, H + 1)))
                elif mode >= 2:
                    cnt, rows = int(rng.randint(1, 5)), int(rng.choice([1, 5, 16]))
                    op["band"] = (rows, int(rng.randint(0, min(cnt, (H + rows - 1) // rows))), cnt)
            elif kind == "sync":
                op = {"k": kind, "st": int(rng.randint(0, self.n_streams))}
            elif kind == "take_capped":
                op = {"k": kind, "s": sc.slot, "st": int(rng.randint(0, self.n_streams))}
            elif kind == "cycle":
                i, _ = HOT[int(rng.randint(0, 3))] if rng.rand() < 0.5 else (int(rng.randint(0, 100)), 1)
                period = int(rng.choice([1, 3, 7, 47]))
                op = {"k": kind, "s": sc.slot, "cam": ("p", sc.slot, i), "n": 1, "period": period,
                      "cycle": int(rng.randint(0, period)) if rng.rand() < 0.4 else -1}  # (-1: the next one in sequence)
            elif kind in ("update", "reopen"):
                op = {"k": kind, "s": sc.slot, "p": int(rng.randint(0, N_PARAMS))}
            else:
                op = self._env_op()
            return self._emit(op)

    # -- bookkeeping
    def _note_launch(self, sc, ctx, op, full, stats=False):
        cam = camera_of(op["cam"], self.seed)
        sup = super_camera(hm, cam, op["n"])
        key = (bytes(sup), sc.epoch)
        where = "the_own_stream" if ctx == "own" else "a_launch_lane" if ctx[0] == "lane" else "a_caller_stream"
        sc.ctx[ctx].launch(key, sup, self.ev, sc.pidx, where)
        self.cover["kernels"][self.kernel or "unset"] += 1
        self.cover["projections"][cam.projection] += 1
        self.cover["samplings"][cam.sampling] += 1
        self.cover["factors"][op["n"]] += 1
        # what api_launch.cpp launch_frame calls eligible: a full frame of >= 12 tile rows, not instrumented, not the literal loop
        if full and not stats and sup.height >= ELIGIBLE_ROWS and self.kernel != "simple":
            # a record and its calibration live in ONE stream context, and re-reading the knobs resets them
            rec = (ctx, key, self.envs)
            sc.seen[rec] += 1
            self.ev["max_repeats_of_an_eligible_record_on_one_stream"] = max(self.ev["max_repeats_of_an_eligible_record_on_one_stream"], sc.seen[rec])
            self.ev["eligible_antialiased_launches"] += int(op["n"] > 1)
            # the shadow probe: frames the scene has not met, the kernel left to the scene, no HMRM_NO_PROBE
            fresh = key not in sc.met and self.kernel in (None, "leap") and not op.get("no_probe")
            sc.met.add(key)
            sc.fresh_run = sc.fresh_run + 1 if fresh else 0
            self.ev["longest_run_of_fresh_probeable_frames"] = max(self.ev["longest_run_of_fresh_probeable_frames"], sc.fresh_run)

    def _emit(self, op):
        k = op["k"]
        op["i"] = self.n
        self.n += 1
        self.cover["kinds"][k] += 1
        sc = self.scenes[op["s"]] if "s" in op else None
        if "cam" in op:
            op["step_cap"] = self.cap  # (every call that takes a camera re-reads the knobs first)
        if k in ("render", "render_aa", "render_aa_stats", "render_stats", "cycle"):
            self._note_launch(sc, "own", op, True, stats=k in ("render_aa_stats", "render_stats"))
        elif k in ("begin", "dev_begin"):
            op["lane"] = sc.lane_next % 3
            sc.lane_next += 1
            self._note_launch(sc, ("lane", op["lane"]), op, True)
            (sc.host if k == "begin" else sc.dev).append(op["h"])
        elif k == "wait":
            sc.host.remove(op["h"])
            sc.lent.append(op["h"])
        elif k == "release":
            sc.lent.remove(op["h"])
        elif k == "dev_wait":
            sc.dev.remove(op["h"])
        elif k == "rows":
            H = camera_of(op["cam"], self.seed).height
            self._note_launch(sc, ("caller", op["st"]), op, op["band"] is None and op["rb"] == 0 and op["re"] == H)
            sc.strips[op["st"]] += 1
        elif k == "sync":
            for s in self.scenes:
                s.strips.pop(op["st"], None)
        elif k == "update":
            self.ev["updates_with_a_ticket_in_flight"] += int(bool(sc.host or sc.dev))
            self.ev["updates_with_a_lent_frame"] += int(bool(sc.lent))
            sc.strips.clear()  # (the caller's streams are synchronised -- and their strips checked -- first)
            sc.pidx = op["p"]
            sc.epoch += 1
            for c in sc.ctx.values():
                c.slots.clear()
        elif k == "reopen":
            sc.reset()
            sc.pidx = op["p"]
            sc.epoch += 1
        elif k == "env":
            self.kernel, self.cap = op["kernel"], op["step_cap"]
            for s in self.scenes:
                s.host, s.lent, s.dev = [], [], []
                s.strips.clear()
        self.ev["max_in_flight"] = max(self.ev["max_in_flight"], max(len(s.host) + len(s.dev) for s in self.scenes))
        return op

    def coverage(self):
        out = {k: dict(sorted(v.items(), key=lambda kv: str(kv[0]))) for k, v in self.cover.items()}
        out["events"] = dict(sorted(self.ev.items()))
        out["records_on_the_busiest_stream"] = max(len(c.slots) for s in self.scenes for c in s.ctx.values()) if any(s.ctx for s in self.scenes) else 0
        return out


def coverage_gaps(cov):
    """What the issue wants every slice to reach -> list of what is missing (empty = all there)."""
    gaps = [f"op kind {k}" for k in OP_KINDS if not cov["kinds"].get(k)]
    gaps += [f"kernel {k}" for k in ("unset", "leap", "group", "simple", "rec") if not cov["kernels"].get(k)]
    gaps += [f"projection {p}" for p in (1, 2, 3) if not cov["projections"].get(p)]
    gaps += [f"sampling {m}" for m in (0, 1, 2) if not cov["samplings"].get(m)]
    gaps += [f"factor {n}" for n in (1, 2, 4, 8) if not cov["factors"].get(n)]
    ev = cov["events"]
    for name, least in (("updates_with_a_ticket_in_flight", 1), ("arena_regrowths", 1), ("evictions", 1),
                        ("max_repeats_of_an_eligible_record_on_one_stream", 12), ("longest_run_of_fresh_probeable_frames", 8),
                        ("cameras_under_two_parameter_sets_on_the_own_stream", 1), ("cameras_under_two_parameter_sets_on_a_launch_lane", 1),
                        ("cameras_under_two_parameter_sets_on_a_caller_stream", 1)):
        if ev.get(name, 0) < least:
            gaps.append(f"{name} {ev.get(name, 0)} < {least}")
    return gaps


def fmt_op(op):
    return "{" + ", ".join(f"{k}: {v}" for k, v in op.items()) + "}"


# ------------------------------------------------------------------------------------------------ expected values
Frame = collections.namedtuple("Frame", "fb total capped steps entry")


class Expect:
    """The oracle, memoised per (map, parameters, camera bytes, factor, step cap)."""

    def __init__(self, oracle, seed):
        self.oracle, self.seed = oracle, seed
        self.maps = {}
        self.heights = {}
        self.memo = collections.OrderedDict()   # (bounded: a long run meets hundreds of thousands of distinct frames)
        self.filtered = {}
        self.computed = 0

    def map_of(self, slot):
        if slot not in self.maps:
            self.maps[slot] = build_map(slot, self.seed)
        return self.maps[slot]

    def frame(self, slot, params, cam, n, step_cap):
        sup = super_camera(hm, cam, n)
        key = (slot, bytes(params), bytes(sup), step_cap)
        if key not in self.memo:
            rgb, cmap = self.map_of(slot)
            hk = (slot, bytes(params))
            if hk not in self.heights:
                self.heights[hk] = self.oracle.update_heightmap(rgb, params)
            cfg = self.oracle.make_cfg(sup, params, cmap.shape[1], cmap.shape[0], step_cap=step_cap or self.oracle.DEFAULT_STEP_CAP)
            self.memo[key] = Frame(*self.oracle.render(cfg, self.heights[hk], cmap, per_pixel=True))
            self.computed += 1
            if len(self.memo) > MEMO_FRAMES:
                old, _ = self.memo.popitem(last=False)
                for f in (1, 2, 4, 8):
                    self.filtered.pop((old, f), None)
        self.memo.move_to_end(key)
        fr = self.memo[key]
        if n > 1 and (key, n) not in self.filtered:
            self.filtered[(key, n)] = fr._replace(fb=box_filter(fr.fb, n), steps=None, entry=None)
        return self.filtered[(key, n)] if n > 1 else fr


def apply_cycle(buf, frame, cycle, period):
    """hmrm_render_cycle on the caller's frame `buf` (H x W x 4, in place): pixels p = x + y W with p = cycle (mod period)."""
    h, w = frame.shape[:2]
    sel = (np.arange(w * h).reshape(h, w) % period) == cycle
    buf[sel] = frame[sel]


def strip_rows(height, rb, re, band):
    """Frame row of every row of a strip (-1: a row of the strip the launch does not write) for hmrm_render_rows_device."""
    if band is None:
        return np.arange(rb, re)
    rows, idx, cnt = band
    local = hm.band_local_rows(height, rows, idx, cnt)
    out = np.full(local, -1, dtype=np.int64)
    for b in range(local // rows):
        r0 = (idx + b * cnt) * rows
        m = max(0, min(rows, height - r0))
        out[b * rows: b * rows + m] = np.arange(r0, r0 + m)
    return out


def expected_strip(fr, width, stride_px, rb, re, band):
    """-> (bytes of the strip buffer filled with SENTINEL before the launch, capped rays among the rows it renders)."""
    rows = strip_rows(fr.fb.shape[0], rb, re, band)
    out = np.full((len(rows), stride_px * 4), SENTINEL, dtype=np.uint8)
    live = rows >= 0
    out[live, :width * 4] = fr.fb[rows[live]].reshape(-1, width * 4)
    return out, int((fr.steps[rows[live]] < 0).sum())


# ------------------------------------------------------------------------------------------------ running
class TorchBackend:
    """The real library: scenes of lib.py, torch streams and device buffers."""

    def __init__(self, n_streams):
        import torch
        self.torch = torch
        hm.set_device(0)
        self.streams = [torch.cuda.Stream() for _ in range(n_streams)]
        self.fill = torch.cuda.Stream()

    def scene(self, rgb, cmap, params):
        return hm.Scene(rgb, cmap, params)

    def stream_handle(self, k):
        return self.streams[k].cuda_stream

    def sync_stream(self, k):
        self.streams[k].synchronize()

    def buffer(self, rows, nbytes, stream=None):
        """rows x nbytes bytes of device memory filled with SENTINEL, the fill ordered in front of what follows on `stream`
        (None: finished before this returns)."""
        t = self.torch
        if stream is None:  # (on a stream of its own: the scene's frames in flight stay in flight)
            with t.cuda.stream(self.fill):
                b = t.full((max(rows, 1), nbytes), SENTINEL, dtype=t.uint8, device="cuda")
            self.fill.synchronize()
            return b
        with t.cuda.stream(self.streams[stream]):
            return t.full((max(rows, 1), nbytes), SENTINEL, dtype=t.uint8, device="cuda")

    def ptr(self, b):
        return b.data_ptr()

    def read(self, b, rows):
        return b.cpu().numpy()[:rows]


class Runner:
    def __init__(self, plan, expect, backend, verbose=False):
        self.plan, self.exp, self.be, self.seed = plan, expect, backend, plan.seed
        self.scenes = {}
        self.bad = collections.Counter()
        self.recent = collections.deque(maxlen=40)
        self.hits = {}
        self.cycles = {}
        self.choices = collections.Counter()
        self.verbose = verbose
        for ps in plan.scenes:
            self._open(ps.slot, ps.pidx)

    def _open(self, slot, pidx):
        rgb, cmap = self.exp.map_of(slot)
        params = scene_params(pidx)
        self.scenes[slot] = {"scene": self.be.scene(rgb, cmap, params), "params": params, "host": {}, "lent": {}, "dev": {}, "strips": [],
                             "lane_cum": [0, 0, 0], "lane_cums": [{0}, {0}, {0}], "lane_seen": [0, 0, 0], "pending_capped": collections.Counter()}

    def mismatch(self, op, what):
        self.bad[op["k"]] += 1
        print(f"MISMATCH seed {self.seed} op {op['i']} {fmt_op(op)}: {what}; replay: python tests/deep_fuzz_api.py {self.seed} {op['i'] + 1}; "
              f"last ops: {' '.join(fmt_op(o) for o in self.recent)}", flush=True)

    def _same(self, op, got, want, what):
        if got.shape != want.shape or not np.array_equal(got, want):
            d = np.argwhere(got != want) if got.shape == want.shape else []
            self.mismatch(op, f"{what}: {len(d)} bytes differ, first at {d[:3].tolist() if len(d) else (got.shape, want.shape)}")
            return False
        return True

    def _frame(self, st, op):
        return self.exp.frame(op["s"], st["params"], camera_of(op["cam"], self.seed), op["n"], op["step_cap"])

    def _call(self, op, fn, want_capped):
        """A call that reports capped rays with HMRM_E_NOTERM and their number in the message -> whether the count was right."""
        got = 0
        try:
            fn()
        except hm.HmrmError as e:
            if e.code != hm.HMRM_E_NOTERM:
                raise
            got = int(e.message.split()[0])
        if want_capped is not None and got != want_capped:
            self.mismatch(op, f"{got} capped rays reported, the oracle has {want_capped}")
        return got

    def _lane_wait(self, op, st, lane, cum_j, got, exact):
        """hmrm_render_wait / hmrm_render_device_wait report what the lane's counter held beyond what was reported before: a device
        ticket reads it in stream order (exactly through its own launch), a host ticket on the copy stream (its own launch, maybe
        later ones of the lane)."""
        seen = st["lane_seen"][lane] + got
        last = st["lane_cum"][lane]
        if exact:
            ok = seen == max(st["lane_seen"][lane], cum_j)
        else:   # (the counter after this launch or after a later one of the lane)
            ok = seen >= cum_j and seen in st["lane_cums"][lane]
        if not ok:
            self.mismatch(op, f"lane {lane}: {got} capped rays reported; reported so far {st['lane_seen'][lane]}, through this launch {cum_j}, "
                              f"through the lane's last {last}")
        st["lane_seen"][lane] = seen if ok else min(max(seen, cum_j), last)

    def _check_strip(self, rec):
        op, buf, want = rec
        self._same(op, self.be.read(buf, want.shape[0]), want, "strip")

    def _drain_streams(self, st, streams=None):
        """Synchronise the caller streams that hold strips of this scene and check them."""
        for k in sorted({r[0]["st"] for r in st["strips"]} if streams is None else streams):
            self.be.sync_stream(k)
        keep = []
        for r in st["strips"]:
            if streams is None or r[0]["st"] in streams:
                self._check_strip(r)
            else:
                keep.append(r)
        st["strips"] = keep

    def _wait(self, op, st):
        fr, lane, cum_j = st["host"].pop(op["h"])
        sc = st["scene"]
        ticket = fr[1]
        got = self._call(op, lambda: sc.render_wait(ticket, fr[0].fb.shape[:2], copy=False), None)
        frame = sc.render_wait(ticket, fr[0].fb.shape[:2])   # (the frame stays lent until it is released; nothing is left to report)
        self._lane_wait(op, st, lane, cum_j, got, False)
        self._same(op, frame, fr[0].fb, "host ticket")
        st["lent"][op["h"]] = ticket

    def _dev_wait(self, op, st):
        fr, ticket, buf, want, lane, cum_j = st["dev"].pop(op["h"])
        got = self._call(op, lambda: st["scene"].render_device_wait(ticket), None)
        self._lane_wait(op, st, lane, cum_j, got, True)
        self._same(op, self.be.read(buf, want.shape[0]), want, "device ticket")

    def quiesce(self, st):
        for h in list(st["host"]):
            self._wait({"k": "wait", "s": -1, "h": h, "i": self.plan.n}, st)
        for h in list(st["lent"]):
            st["scene"].render_release(st["lent"].pop(h))
        for h in list(st["dev"]):
            self._dev_wait({"k": "dev_wait", "s": -1, "h": h, "i": self.plan.n}, st)
        self._drain_streams(st)

    def run(self, op):
        self.recent.append(op)
        k = op["k"]
        if k == "env":
            for st in self.scenes.values():
                self.quiesce(st)
            for name, v in (("HMRM_KERNEL", op["kernel"]), ("HMRM_STEP_CAP", op["step_cap"])):
                if v is None:
                    os.environ.pop(name, None)
                else:
                    os.environ[name] = str(v)
            return
        if k == "sync":
            for st in self.scenes.values():
                self._drain_streams(st, {op["st"]})
            return
        st = self.scenes[op["s"]]
        sc = st["scene"]
        if "cam" in op:
            cam = camera_of(op["cam"], self.seed)
            fr = self._frame(st, op)
            n = op["n"]
        if k == "render":
            got = []
            self._call(op, lambda: got.append(sc.render(cam) if n == 1 else sc.render_aa(cam, n)), fr.capped)
            if got:
                self._same(op, got[0], fr.fb, "frame")
            choice = sc.kernel_choice()
            self.choices[choice] += 1
            forced = {"group": 1, "simple": 2, "rec": 3}.get(os.environ.get("HMRM_KERNEL"))
            if choice != forced if forced else choice not in (0, 1, 3):
                self.mismatch(op, f"kernel_choice() {choice} under HMRM_KERNEL={os.environ.get('HMRM_KERNEL')}")
        elif k == "render_aa":
            got = []
            self._call(op, lambda: got.append(sc.render_aa(cam, n)), fr.capped)
            if got:
                self._same(op, got[0], fr.fb, "antialiased frame")
        elif k in ("render_aa_stats", "render_stats"):
            if k == "render_stats":
                fb, s, steps, entry = sc.render_stats(cam, per_pixel=True, allow_capped=True)
                self._same(op, steps.astype(np.int64), np.where(fr.steps < 0, -1 - fr.steps, fr.steps), "per-pixel steps")
                self._same(op, entry.view(np.uint64), fr.entry.view(np.uint64), "distance() bits")
            else:
                fb, s = sc.render_aa(cam, n, stats=True, allow_capped=True)
            self._same(op, fb, fr.fb, "instrumented frame")
            if (s.rays, s.steps, s.capped) != (n * n * cam.width * cam.height, fr.total, fr.capped):
                self.mismatch(op, f"stats rays {s.rays} steps {s.steps} capped {s.capped}, oracle {n * n * cam.width * cam.height} {fr.total} {fr.capped}")
            hk = (op["s"], bytes(st["params"]), bytes(cam), n, op["step_cap"])
            if self.hits.setdefault(hk, s.hits) != s.hits:
                self.mismatch(op, f"hits {s.hits}, an earlier render of the same frame had {self.hits[hk]}")
        elif k in ("begin", "dev_begin"):
            lane = op["lane"]
            cum_j = st["lane_cum"][lane] = st["lane_cum"][lane] + fr.capped
            st["lane_cums"][lane].add(cum_j)
            if k == "begin":
                st["host"][op["h"]] = ((fr, sc.render_begin(cam, no_probe=op["no_probe"], aa=n)), lane, cum_j)
            else:
                stride_px = cam.width + op["pad"]
                buf = self.be.buffer(cam.height, stride_px * 4)
                want = np.full((cam.height, stride_px * 4), SENTINEL, dtype=np.uint8)
                want[:, :cam.width * 4] = fr.fb.reshape(cam.height, -1)
                t = sc.render_device_begin(cam, self.be.ptr(buf), stride_px * 4, no_probe=op["no_probe"], aa=n)
                st["dev"][op["h"]] = (fr, t, buf, want, lane, cum_j)
        elif k == "wait":
            self._wait(op, st)
        elif k == "release":
            sc.render_release(st["lent"].pop(op["h"]))
        elif k == "dev_wait":
            self._dev_wait(op, st)
        elif k == "rows":
            stride_px = cam.width + op["pad"]
            want, capped = expected_strip(fr, cam.width, stride_px, op["rb"], op["re"], op["band"])
            buf = self.be.buffer(want.shape[0], stride_px * 4, stream=op["st"])
            band = op["band"] or (0, 0, 1)
            sc.render_rows_device(cam, self.be.ptr(buf), stride_px * 4, op["rb"], op["re"], band[0], band[1], band[2],
                                  stream=self.be.stream_handle(op["st"]))
            st["strips"].append((op, buf, want))
            st["pending_capped"][op["st"]] += capped
        elif k == "take_capped":
            got = sc.take_capped(self.be.stream_handle(op["st"]), allow_capped=True)
            want = st["pending_capped"].pop(op["st"], 0)
            if got != want:
                self.mismatch(op, f"take_capped {got}, the launches enqueued on stream {op['st']} since the last call hold {want}")
            if got:  # (taken: a second call has nothing left to report)
                self._call(op, lambda: sc.take_capped(self.be.stream_handle(op["st"])), 0)
        elif k == "cycle":
            ck = (op["s"], op["cam"][2], cam.width, cam.height)
            if ck not in self.cycles:
                self.cycles[ck] = [np.full((cam.height, cam.width, 4), SENTINEL, dtype=np.uint8), np.full((cam.height, cam.width, 4), SENTINEL, dtype=np.uint8), 0]
            buf, want, nxt = self.cycles[ck]
            cycle = op["cycle"] if op["cycle"] >= 0 else nxt % op["period"]
            self.cycles[ck][2] = cycle + 1
            apply_cycle(want, fr.fb, cycle, op["period"])
            self._call(op, lambda: sc.render_cycle(cam, buf, cycle, op["period"]), fr.capped)
            if not self._same(op, buf, want, f"progressive frame after cycle {cycle} of {op['period']}"):
                buf[...] = want
        elif k == "update":
            self._drain_streams(st)
            st["params"] = scene_params(op["p"])
            sc.update(st["params"])
        elif k == "reopen":
            self.quiesce(st)
            sc.close()
            self._open(op["s"], op["p"])

    def finish(self):
        for st in self.scenes.values():
            self.quiesce(st)
            for k, want in list(st["pending_capped"].items()):
                got = st["scene"].take_capped(self.be.stream_handle(k), allow_capped=True)
                if got != want:
                    self.mismatch({"k": "take_capped", "i": self.plan.n, "st": k}, f"at the end: take_capped {got}, expected {want}")
            st["scene"].close()


def main(argv):
    args = [a for a in argv if not a.startswith("--")]
    seed = int(args[0]) if args else 1
    ops = int(args[1]) if len(args) > 1 else 300
    budget_s = float(args[2]) if len(args) > 2 else 600.0
    plan = Plan(seed)
    if "--plan-only" in argv:
        for _ in range(ops):
            print(fmt_op(plan.next_op()))
        cov = plan.coverage()
        print(f"plan: seed {seed}, ops {plan.n}, skipped 0, streams {plan.n_streams}, coverage {cov}")
        print(f"plan: missing {coverage_gaps(cov)}; torch imported: {'torch' in sys.modules}")
        return 0
    for name in ("HMRM_KERNEL", "HMRM_STEP_CAP"):
        os.environ.pop(name, None)
    from oracle import oracle_py as oracle
    t0 = time.time()
    runner = Runner(plan, Expect(oracle, seed), TorchBackend(plan.n_streams))
    try:
        while plan.n < ops and time.time() - t0 < budget_s and sum(runner.bad.values()) < 20:
            runner.run(plan.next_op())
            if plan.n % 50000 == 0:
                print(f"... {plan.n} ops, {sum(runner.bad.values())} mismatches, {time.time() - t0:.0f} s", flush=True)
        runner.finish()
    except hm.HmrmError as e:
        print(f"ERROR seed {seed} after op {plan.n - 1}: {e}; last ops: {' '.join(fmt_op(o) for o in runner.recent)}", flush=True)
        print(f"api: ops {plan.n}, mismatches {sum(runner.bad.values()) + 1}, per-kind {dict(runner.bad)}, stopped by an error of the library")
        return 2
    cov = plan.coverage()
    bad = sum(runner.bad.values())
    print(f"api: ops {plan.n}, mismatches {bad}, per-kind {dict(runner.bad)}, seed {seed}, streams {plan.n_streams}, oracle frames {runner.exp.computed}, "
          f"kernel_choice() seen {dict(runner.choices)}, {time.time() - t0:.0f} s")
    print(f"api: coverage {cov}")
    print(f"api: missing {coverage_gaps(cov)}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
