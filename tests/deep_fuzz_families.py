"""Model-based fuzz of call sequences that MIX the entry-point families added after tests/deep_fuzz_api.py: ray and segment
batches, hmrm_pick, interior frames, sun-lit frames and their tickets, cell maps and their sums, geometry frames, accumulated lit
frames, the scene's light plane and the baked frames and tickets -- host and device forms -- next to the plain frames whose
staging buffers they share (d_frame, d_entry, d_cells, d_targets, one ticket pool, three launch lanes).  Test
infrastructure, not collected by pytest:

    python tests/deep_fuzz_families.py <seed> <ops> [seconds] [--plan-only]

One seeded stream of operations drives the library and a model side by side, over live scenes, with tickets in flight, across
height updates, changes of the light plane and HMRM_KERNEL / HMRM_STEP_CAP changes.  Every byte that comes back is compared with
what the numpy replays of tests/ give for the model's state (ray_replay, segment_replay, lit_replay, shade_replay, cell_map_replay,
geometry_replay, the compositions of lit_sum_cases, baked_cases and aa_box; plain frames: the oracle) -- nothing that calls the
library.  Prints one line per mismatch with what is needed to replay it and the summary lines `fam: ops N, mismatches M, per-kind
{...}`, `fam: coverage {...}`, `fam: missing [...]`; exit status 1 on any mismatch, 2 when the library reports a device error
(nothing is run after that).  --plan-only prints the op stream and the plan's bookkeeping without torch or a GPU.

What the model knows (include/hmrm.h): a ticket of any kind finishes with the heights AND the light plane of the moment it was
begun (the expected frame is computed at the begin); hmrm_scene_update leaves the plane; after hmrm_scene_clear_light every baked
entry point is refused with "the scene has no light plane" and nothing else changes; hmrm_scene_bake_light writes hmrm_cell_map_sum's
words with D = 255 K or K; capped rays give HMRM_E_NOTERM with valid output -- host calls report their own count (shadow rays per
ray), tickets per launch lane, device forms per caller stream through hmrm_scene_take_capped --; bytes beyond a row, outside a rect
or behind a batch keep the sentinel; a refused call (a baked frame without a plane, K = 0, an odd 16-bit stride) returns HMRM_E_ARG
and leaves every later result unchanged.  Not pinned: kernel_choice() and `hits`, as in deep_fuzz_api.py.

The fuzzer obeys the ABI itself: caller streams with launches of a scene in flight are synchronised (and checked) before that
scene is updated or closed, host-memory calls are made one at a time, the knobs change only while nothing is in flight.  The
generator only emits ops that can run, planned refusals apart: no op is ever skipped."""
import collections
import hashlib
import os
import sys
import time

if __name__ == "__main__" and "--plan-only" in sys.argv:
    os.environ.setdefault("HMRM_NO_TORCH_PRELOAD", "1")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import deep_fuzz_api as fz
from deep_fuzz_api import MAPS, N_PARAMS, SENTINEL, TorchBackend, build_map, fmt_op, scene_params  # noqa: F401
from aa_box import box_filter, super_camera

hm = fz.hm

FRAME_KINDS = ("render", "render_stats", "interior", "lit", "shaded", "shaded_aa", "geometry", "lit_sum", "baked", "pick")
QUERY_KINDS = ("rays", "segments", "cell_map", "cell_map_sum")
DEV_KINDS = ("rays_dev", "segments_dev", "cell_map_dev", "cell_map_sum_dev", "geometry_dev", "lit_sum_dev")
BEGIN_KINDS = ("begin", "dev_begin", "shaded_begin", "shaded_dev_begin", "baked_begin", "baked_dev_begin")
LIGHT_KINDS = ("set_light", "set_light_device", "bake_light", "clear_light", "light")
REFUSALS = ("refuse_baked", "refuse_k0", "refuse_stride")
OP_KINDS = (FRAME_KINDS + QUERY_KINDS + DEV_KINDS + BEGIN_KINDS + ("wait", "release", "dev_wait") + LIGHT_KINDS
            + ("take_capped", "update", "env", "reopen", "sync") + REFUSALS)
KERNELS = fz.KERNELS
CAPS = (None, 60, 200)
PERIOD = 250
# (op index mod PERIOD, what): every period holds what a slice must reach whatever the dice say
MILESTONES = {5: "ring", 30: "kset", 45: "scratch", 65: "kset", 80: "swap", 105: "kset", 120: "devs", 155: "kset", 170: "reopen",
              185: "kset", 200: "ring", 225: "swap"}
MAX_IN_FLIGHT = 9
FRAMES = ((8, 8), (12, 9), (20, 15), (24, 16))
BATCHES = (1, 63, 65, 300)       # straddle a wave and a 256-lane workgroup
KS = (1, 3, 4)
N_CAMS = 24
SUN_DIRS = ((0.6, 0.5, 0.35), (-0.7, 0.2, 0.15), (0.3, -0.8, 0.6), (0.5, -0.4, -0.1))   # (the last one: below the horizon)
GW0 = 0.7                        # the nominal grid width the pools are laid out around (deep_fuzz_api.NOMINAL_PIDX)
SUN_STEP = 0.3 * GW0
RAY_STEP = 0.2 * GW0
SLOW = 0.05                      # step factor of the ops that are meant to reach a step cap of 60
BAKE_SLOT = 1                    # whole-map light (bake_light, set_light_device) on the 50 x 37 map only: the replay's cost
MODES = (0, 2, 6, 14)            # HMRM_MAP_*: status, WEIGHT, WEIGHT + DIFFUSE, WEIGHT + DIFFUSE + NO_SHADOWS
BG = (12, 34, 56)


def factors_of(w, h):
    return [n for n in (1, 2, 4) if w * n <= 48 and h * n <= 32]


_pools = {}


def camera_pool(slot, seed):
    """24 small cameras of scene `slot`, the same whatever the scene's parameters are: every frame size under every projection,
    the sampling modes rotating; 0..11 look at the map from outside, 12..23 stand strictly inside the box of every parameter set
    (z = 2.5, a fifth of the map in) and look about level, so that no interior ray climbs for long."""
    key = (slot, seed)
    if key in _pools:
        return _pools[key]
    rng = np.random.RandomState((seed * 1000 + slot * 10 + 3) % (1 << 32))
    p = scene_params(fz.NOMINAL_PIDX)
    _, mw, mh = MAPS[slot]
    ex, ey = mw * GW0, mh * GW0
    span = p.max_height - p.min_height
    cams = []
    for i in range(N_CAMS):
        w, h = FRAMES[i % 4]
        proj = (1, 2, 3)[(i // 4) % 3]
        inside = i >= 12
        ang = rng.uniform(0, 2 * np.pi)
        if inside:
            pos = (0.2 * mw, -0.2 * mh, 2.5)
            hang, vang = float(rng.uniform(-1.2, -0.2)), hm.degrees_to_rads(float(rng.choice([95.0, 105.0])))
            hfov = hm.degrees_to_rads(100.0 if proj == 2 else 80.0)
            ortho = 3.0 * GW0 / w
        else:
            dist = float(rng.choice([0.8, 1.1])) * max(ex, ey)
            pos = (ex / 2 + dist * np.cos(ang), -ey / 2 + dist * np.sin(ang), p.max_height + p.min_height + 0.6 * span)
            hang = float(np.arctan2(-ey / 2 - pos[1], ex / 2 - pos[0])) + float(rng.choice([0.0, 0.15, -0.2]))
            vang = hm.degrees_to_rads(float(rng.choice([105.0, 120.0, 135.0])))
            hfov = hm.degrees_to_rads(150.0 if proj == 2 else 80.0)
            ortho = 1.5 * max(ex, ey) / max(w, h)
        cams.append(hm.Camera.make(width=w, height=h, projection=proj, hfov=hfov, hang=hang, vang=vang, pos=pos, ortho_width=ortho,
                                   step_dist=float(rng.choice([0.25, 0.5, 0.37])) * GW0, bg=tuple(int(v) for v in rng.randint(0, 256, size=3)),
                                   sampling=(i + i // 4 + i // 12) % 3))
    _pools[key] = cams
    return cams


def camera_of(spec, seed):
    """('c', slot, i) a pool camera; ('q', slot, i) the same with SLOW times its step: most of its rays reach a cap of 60."""
    c = camera_pool(spec[1], seed)[spec[2]]
    if spec[0] == "q":
        c = hm.Camera.from_buffer_copy(c)
        c.step_dist *= SLOW
    return c


def directions(k, variant):
    """k directions above the horizon, none alike (tests/test_scratch_growth_gpu.py's)."""
    a = np.arange(k, dtype=np.float64) + 5.0 * variant
    return np.ascontiguousarray(np.stack([np.cos(0.7 * a + 0.3), np.sin(0.7 * a + 0.3), 0.25 + 0.02 * a], axis=1))


def batch_rays(slot, n, bid):
    """n rays: from above the map down into it, every seventh one upwards, every fifth one from inside the box (a miss
    without the interior rule), none with a horizontal component too small to leave the grid soon."""
    _, mw, mh = MAPS[slot]
    rng = np.random.RandomState((bid * 7919 + slot * 31 + n) % (1 << 32))
    r = np.empty((n, 6), dtype=np.float64)
    r[:, 0] = rng.uniform(0.05, 0.95, n) * mw * 0.5
    r[:, 1] = -rng.uniform(0.05, 0.95, n) * mh * 0.5
    r[:, 2] = 12.0
    r[:, 3:5] = rng.uniform(-1.0, 1.0, (n, 2))
    r[:, 3] = np.where(np.abs(r[:, 3]) < 0.2, np.where(r[:, 3] < 0, -0.2, 0.2), r[:, 3])
    r[:, 5] = -1.0
    r[3::7, 5] = 1.0
    r[2::5, 2] = 2.5
    r[2::5, 5] = rng.uniform(-0.3, 0.3, len(r[2::5]))
    return r


def batch_limits(slot, n, bid):
    return np.random.RandomState((bid * 104729 + slot + n) % (1 << 32)).randint(0, 40, n).astype(np.uint32)


def light_plane(slot, pid, u16):
    """The host plane of a set_light op -> ((map_h, map_w) uint8 or uint16, full scale)."""
    _, mw, mh = MAPS[slot]
    rng = np.random.RandomState((pid * 2654435761 + slot) % (1 << 32))
    if u16:
        d = int(rng.choice([1000, 65535, 300]))
        return rng.randint(0, d + d // 4 + 1, size=(mh, mw)).clip(0, 65535).astype(np.uint16), d
    d = int(rng.choice([255, 200]))
    return rng.randint(0, 256, size=(mh, mw)).astype(np.uint8), d


def point_target(slot):
    _, mw, mh = MAPS[slot]
    return (0.31 * mw * 0.5, -0.27 * mh * 0.5, 9.0)


# ------------------------------------------------------------------------------------------------ the plan
class PScene:
    def __init__(self, slot, pidx):
        self.slot, self.pidx = slot, pidx
        self.reset()

    def reset(self):
        self.host, self.lent, self.dev = {}, [], {}      # handle -> kind of ticket; lent handles
        self.plane = False
        self.lane_next = 0
        self.whole = None                                  # (op index, stream) of the last whole-map cell_map_sum_dev
        self.users = collections.defaultdict(list)         # scratch member -> [(user kind, bytes)]
        self.pending = collections.defaultdict(set)        # caller stream -> device forms enqueued under a cap, not yet taken


class Plan:
    """The seeded op stream.  Depends on the seed alone (never on what the GPU or the replays return)."""

    def __init__(self, seed):
        self.seed = seed
        self.rng = np.random.RandomState((seed * 3 + 1) % (1 << 32))
        self.n_streams = 4 + seed % 5
        self.scenes = [PScene(slot, (slot + seed) % N_PARAMS) for slot in range(len(MAPS))]
        self.kernel, self.cap = None, None
        self.script = collections.deque()
        self.n = self.handle = self.envs = self.pid = self.bid = self.ksets = self.rings = 0
        self.milestone_at = -1
        self.milestones_done = set()
        self.cover = {k: collections.Counter() for k in ("kinds", "kernels", "projections", "samplings", "factors", "interior")}
        self.ev = collections.Counter()
        self.taken = collections.defaultdict(set)          # device form -> caller streams it was taken on under a cap

    # -- pieces of ops
    def _cam(self, sc, i=None):
        return ("c", sc.slot, int(self.rng.randint(0, N_CAMS)) if i is None else i)

    def _sun(self):
        r = self.rng
        return {"sd": int(r.randint(0, len(SUN_DIRS))), "sm": int(r.choice([0, 40])), "amb": int(r.choice([96, 128, 255])),
                "dif": bool(r.rand() < 0.5), "sh": bool(r.rand() < 0.7)}

    def _frame(self, kind, sc, cam=None, n=None, **kw):
        r = self.rng
        cam = cam or self._cam(sc)
        c = camera_pool(cam[1], self.seed)[cam[2]]
        op = {"k": kind, "s": sc.slot, "cam": cam, "n": 1}
        if kind in ("shaded_aa",) or (kind in BEGIN_KINDS + ("baked",) and n is None and r.rand() < 0.5):
            fs = [f for f in factors_of(c.width, c.height) if f > 1 or kind != "shaded_aa"]
            n = int(fs[int(r.randint(0, len(fs)))]) if fs else 1
        op["n"] = n or 1
        if kind == "shaded_aa" and op["n"] == 1:
            op["k"] = "shaded"
        if kind in ("interior", "lit", "shaded", "shaded_aa", "geometry", "geometry_dev", "lit_sum", "lit_sum_dev", "baked", "shaded_begin",
                    "shaded_dev_begin", "baked_begin", "baked_dev_begin", "refuse_baked"):
            op["int"] = kind == "interior" or bool(cam[2] >= 12 and r.rand() < 0.7)
        if kind in ("lit", "shaded", "shaded_aa", "lit_sum", "lit_sum_dev", "shaded_begin", "shaded_dev_begin"):
            op.update(self._sun())
            if kind == "lit":
                op.update(dif=False, sh=True)
        if kind in ("lit_sum", "lit_sum_dev"):
            op.update(K=int(r.choice(KS)), dv=int(r.randint(0, 3)))
        if kind in ("geometry", "lit_sum", "baked", "geometry_dev", "lit_sum_dev", "dev_begin", "shaded_dev_begin", "baked_dev_begin"):
            op["pad"] = int(r.choice([0, 1, 5]))
        if kind == "pick":
            op.update(px=int(r.randint(0, c.width)), py=int(r.randint(0, c.height)))
        if kind in ("begin", "dev_begin"):
            op["no_probe"] = bool(r.rand() < 0.25)
        if kind in DEV_KINDS:
            op["st"] = int(r.randint(0, self.n_streams))
        op.update(kw)
        return op

    def _batch(self, kind, sc, **kw):
        r = self.rng
        self.bid += 1
        op = {"k": kind, "s": sc.slot, "nr": int(r.choice(BATCHES)), "bid": self.bid, "smp": int(r.randint(0, 3)), "slow": False}
        if kind.startswith("segments"):
            op.update(int=bool(r.rand() < 0.6), ms=int(r.choice([0, 30])), per=bool(r.rand() < 0.5))
        if kind in DEV_KINDS:
            op["st"] = int(r.randint(0, self.n_streams))
        op.update(kw)
        return op

    def _cells(self, kind, sc, **kw):
        r = self.rng
        _, mw, mh = MAPS[sc.slot]
        w, h = int(r.randint(1, 21)), int(r.randint(1, 13))
        op = {"k": kind, "s": sc.slot, "rect": (int(r.randint(0, mw - w + 1)), int(r.randint(0, mh - h + 1)), w, h), "pad": int(r.choice([0, 1, 3])),
              "mode": int(r.randint(0, 4)), "point": bool(r.rand() < 0.25), "lift": float(r.choice([0.0, 0.25 * GW0])),
              "ms": int(r.choice([0, 40])), "smp": int(r.randint(0, 3)), "slow": False}
        if kind.startswith("cell_map_sum") or kind == "bake_light":
            op.update(K=int(r.choice(KS)), dv=int(r.randint(0, 3)))
        else:
            op["tg"] = int(r.randint(0, len(SUN_DIRS)))
        if kind == "bake_light":
            del op["rect"], op["pad"]
        if kind in DEV_KINDS:
            op["st"] = int(r.randint(0, self.n_streams))
        op.update(kw)
        return op

    def _set_light(self, sc, **kw):
        self.pid += 1
        return dict({"k": "set_light", "s": sc.slot, "pid": self.pid, "u16": bool(self.rng.rand() < 0.5), "pad": int(self.rng.choice([0, 1, 4]))}, **kw)

    def _env_op(self, kernel=False, cap=False):
        self.envs += 1
        return {"k": "env", "kernel": KERNELS[(self.envs + self.seed) % len(KERNELS)] if kernel is False else kernel,
                "step_cap": CAPS[(self.envs + self.seed) % len(CAPS)] if cap is False else cap}

    # -- scripts
    def _ring(self, sc):
        """A host ring and the device tickets holding a plain, a sun-lit and a baked frame at once; a host-memory call of another
        family and an update while they are in flight; then everything is collected."""
        self.rings += 1
        s = self.script
        if not sc.plane:
            s.append(self._set_light(sc))
        cams = [self._cam(sc, (self.rings * 5 + j * 7) % N_CAMS) for j in range(6)]
        for j, kind in enumerate(("begin", "shaded_begin", "baked_begin", "dev_begin", "shaded_dev_begin", "baked_dev_begin")):
            if j in (1, 5):   # (an 8 x 8 camera: the one size that takes both factors)
                s.append(self._frame(kind, sc, self._cam(sc, (self.rings * 4 + 12 * (j == 5)) % N_CAMS), n=4 if j == 1 else 2))
            else:
                s.append(self._frame(kind, sc, cams[j]))
        s.append(self._cells("cell_map", sc))
        s.append(self._batch("rays", sc))
        s.append({"k": "update", "s": sc.slot, "p": (sc.pidx + 1 + int(self.rng.randint(0, N_PARAMS - 1))) % N_PARAMS})
        s.append(self._frame("baked", sc, cams[2]))
        s.extend([("wait_first", sc.slot), ("release_last", sc.slot)] * 3 + [("dev_wait_first", sc.slot)] * 3)

    def _kset(self, sc):
        """The next kernel setting, and under it a sun-lit frame, a baked one, a cell map and a ray batch."""
        self.ksets += 1
        s = self.script
        s.append(self._env_op(kernel=KERNELS[self.ksets % len(KERNELS)]))
        if not sc.plane:
            s.append(self._set_light(sc))
        s.extend([self._frame("shaded", sc), self._frame("baked", sc), self._cells("cell_map", sc), self._batch("rays", sc)])

    def _scratch(self, sc):
        """Each shared staging buffer changes hands in both directions, small - large - small."""
        s = self.script
        small, large, sph = self._cam(sc, 0), self._cam(sc, 3), self._cam(sc, 7)
        s.extend([self._frame("lit_sum", sc, small, K=3), self._cells("cell_map_sum", sc, K=4), self._frame("lit_sum", sc, small, K=1)])
        s.extend([self._cells("cell_map_sum", sc, K=3, dv=0), self._frame("lit_sum", sc, small, K=3, dv=1)])   # (equal K, other directions)
        s.extend([self._frame("render_stats", sc, small), self._frame("pick", sc, sph), self._frame("render_stats", sc, small)])
        s.extend([self._frame("render", sc, small), self._frame("lit_sum", sc, large), self._frame("render", sc, small)])
        _, mw, mh = MAPS[sc.slot]
        s.extend([self._cells("cell_map", sc, rect=(3, 5, 4, 4)), self._cells("cell_map_sum", sc, rect=(mw - 20, mh - 12, 20, 12)),
                  self._cells("cell_map", sc, rect=(1, 2, 3, 2))])

    def _swap(self, _sc):
        """set_light, bake_light and clear_light each with a baked ticket in flight (it finishes with the old plane), the device
        recipe (cell_map_sum_device's words into set_light_device on the same stream), the planned refusals."""
        sc = self.scenes[BAKE_SLOT]
        s = self.script
        st = int(self.rng.randint(0, self.n_streams))
        if not sc.plane:
            s.append(self._set_light(sc))
        s.extend([self._frame("baked_begin", sc), self._set_light(sc), ("wait_first", sc.slot), ("release_last", sc.slot)])
        s.extend([self._frame("baked_dev_begin", sc), self._cells("bake_light", sc), ("dev_wait_first", sc.slot), {"k": "light", "s": sc.slot}])
        s.extend([self._frame("baked_begin", sc), {"k": "clear_light", "s": sc.slot}, ("wait_first", sc.slot), ("release_last", sc.slot)])
        s.extend([self._frame("refuse_baked", sc), {"k": "light", "s": sc.slot}])
        s.extend([self._cells("cell_map_sum_dev", sc, rect=(0, 0, MAPS[sc.slot][1], MAPS[sc.slot][2]), whole=True, st=st, mode=int(self.rng.choice([0, 2]))),
                  {"k": "set_light_device", "s": sc.slot}, self._frame("baked", sc), {"k": "refuse_stride", "s": sc.slot},
                  self._cells("refuse_k0", sc), self._frame("baked", sc)])

    def _devs(self, sc):
        """Every device form on two caller streams under a cap of 60, with steps so short that rays reach it, each taken per stream."""
        s = self.script
        s.append(self._env_op(kernel=self.kernel, cap=60))
        a = int(self.rng.randint(0, self.n_streams))
        for j, st in enumerate((a, (a + 1 + int(self.rng.randint(0, self.n_streams - 1))) % self.n_streams)):
            cam = ("q", sc.slot, (3 * j + 1) % 12)
            for op in (self._batch("rays_dev", sc, st=st, slow=True, nr=BATCHES[1 + j]), self._batch("segments_dev", sc, st=st, slow=True, ms=0, per=False),
                       self._cells("cell_map_dev", sc, st=st, slow=True, ms=0, mode=0, point=False, tg=j, lift=0.25 * GW0),
                       self._cells("cell_map_sum_dev", sc, st=st, slow=True, ms=0, mode=2, point=False, lift=0.25 * GW0),
                       self._frame("geometry_dev", sc, cam, st=st), self._frame("lit_sum_dev", sc, cam, st=st, sm=0, sh=True)):
                s.extend([op, {"k": "take_capped", "s": sc.slot, "st": st}])
        s.append({"k": "sync", "st": a})

    def _reopen(self, sc):
        s = self.script
        if not sc.plane:
            s.append(self._set_light(sc))
        s.extend([{"k": "reopen", "s": sc.slot, "p": int(self.rng.randint(0, N_PARAMS))}, self._frame("refuse_baked", sc)])

    def next_op(self):
        rng = self.rng
        while True:
            if not self.script and self.n != self.milestone_at:
                self.milestone_at = self.n
                due = [(self.n // PERIOD, pos) for pos in sorted(MILESTONES) if pos <= self.n % PERIOD and (self.n // PERIOD, pos) not in self.milestones_done]
                if due:
                    self.milestones_done = {d for d in self.milestones_done if d[0] == due[0][0]} | {due[0]}
                    self.milestone_at = -1 if len(due) > 1 else self.n
                    sc = self.scenes[(self.n // 7) % len(self.scenes)]
                    getattr(self, "_" + MILESTONES[due[0][1]])(sc)
            if self.script:
                item = self.script.popleft()
                if isinstance(item, dict):
                    return self._emit(item)
                sc = self.scenes[item[1]]
                if item[0] == "wait_first":
                    return self._emit({"k": "wait", "s": sc.slot, "h": next(iter(sc.host))})
                if item[0] == "release_last":
                    return self._emit({"k": "release", "s": sc.slot, "h": sc.lent[-1]})
                return self._emit({"k": "dev_wait", "s": sc.slot, "h": next(iter(sc.dev))})
            sc = self.scenes[int(rng.randint(0, len(self.scenes)))]
            cand = [("render", 4), ("render_stats", 3), ("interior", 3), ("lit", 3), ("shaded", 4), ("shaded_aa", 3), ("geometry", 4), ("lit_sum", 4),
                    ("pick", 3), ("rays", 4), ("segments", 4), ("cell_map", 4), ("cell_map_sum", 4), ("rays_dev", 3), ("segments_dev", 3),
                    ("cell_map_dev", 3), ("cell_map_sum_dev", 3), ("geometry_dev", 3), ("lit_sum_dev", 3), ("set_light", 3), ("light", 2),
                    ("take_capped", 3), ("update", 1.5), ("env", 1.2), ("reopen", 0.5), ("sync", 3), ("refuse_k0", 0.5), ("refuse_stride", 0.5),
                    ("ring", 0.4), ("swap", 0.4)]
            if len(sc.host) + len(sc.dev) < MAX_IN_FLIGHT:
                cand += [("begin", 4), ("dev_begin", 4), ("shaded_begin", 5), ("shaded_dev_begin", 5)]
                if sc.plane:
                    cand += [("baked_begin", 5), ("baked_dev_begin", 5)]
            cand += [("baked", 6), ("clear_light", 1)] if sc.plane else [("refuse_baked", 1)]
            if sc.slot == BAKE_SLOT:
                cand += [("bake_light", 2), ("light_dev", 1.5)]
            if sc.host:
                cand.append(("wait", 7))
            if sc.lent:
                cand.append(("release", 6))
            if sc.dev:
                cand.append(("dev_wait", 7))
            w = np.array([c[1] for c in cand], dtype=np.float64)
            kind = cand[int(rng.choice(len(cand), p=w / w.sum()))][0]
            if kind in ("ring", "swap"):
                getattr(self, "_" + kind)(sc)
                continue
            if kind == "light_dev":
                self.script.extend([self._cells("cell_map_sum_dev", sc, rect=(0, 0, MAPS[sc.slot][1], MAPS[sc.slot][2]), whole=True),
                                    {"k": "set_light_device", "s": sc.slot}])
                continue
            if kind in FRAME_KINDS + BEGIN_KINDS + ("geometry_dev", "lit_sum_dev", "refuse_baked"):
                op = self._frame(kind, sc)
            elif kind in ("rays", "segments", "rays_dev", "segments_dev"):
                op = self._batch(kind, sc)
            elif kind in ("cell_map", "cell_map_sum", "cell_map_dev", "cell_map_sum_dev", "bake_light", "refuse_k0"):
                op = self._cells(kind, sc)
            elif kind == "set_light":
                op = self._set_light(sc)
            elif kind == "wait":
                op = {"k": kind, "s": sc.slot, "h": list(sc.host)[int(rng.randint(0, len(sc.host)))]}
            elif kind == "release":
                op = {"k": kind, "s": sc.slot, "h": sc.lent[int(rng.randint(0, len(sc.lent)))]}
            elif kind == "dev_wait":
                op = {"k": kind, "s": sc.slot, "h": list(sc.dev)[int(rng.randint(0, len(sc.dev)))]}
            elif kind in ("sync", "take_capped"):
                op = {"k": kind, "s": sc.slot, "st": int(rng.randint(0, self.n_streams))}
                if kind == "sync":
                    del op["s"]
            elif kind in ("update", "reopen"):
                op = {"k": kind, "s": sc.slot, "p": int(rng.randint(0, N_PARAMS))}
            elif kind == "env":
                op = self._env_op()
            else:
                op = {"k": kind, "s": sc.slot}
            return self._emit(op)

    # -- bookkeeping
    def _use(self, sc, member, user, size, pattern):
        """`user` stages `size` bytes in a scratch member; counts the hand-over a - b - a with b the largest."""
        u = sc.users[member]
        u.append((user, size))
        if len(u) >= 3 and tuple(x[0] for x in u[-3:]) == pattern and u[-3][1] < u[-2][1] > u[-1][1]:
            self.ev[f"{member}_changed_hands_both_ways_with_a_grow_and_a_shrink"] += 1

    def _emit(self, op):
        k = op["k"]
        op["i"] = self.n
        self.n += 1
        self.cover["kinds"][k] += 1
        sc = self.scenes[op["s"]] if "s" in op else None
        ev = self.ev
        if k in FRAME_KINDS + QUERY_KINDS + DEV_KINDS + BEGIN_KINDS + ("bake_light",):
            op["step_cap"] = self.cap     # (every such call re-reads the knobs first)
            kn = self.kernel or "unset"
            fam = ("lit" if k in ("lit", "shaded", "shaded_aa", "shaded_begin", "shaded_dev_begin") else
                   "baked" if k.startswith("baked") else "cells" if k.startswith("cell_map") else "rays" if k in ("rays", "rays_dev", "segments", "segments_dev") else None)
            if fam:
                self.cover["kernels"][f"{kn}:{fam}"] += 1
        if "cam" in op and k not in REFUSALS:
            cam = camera_of(op["cam"], self.seed)
            self.cover["projections"][cam.projection] += 1
            self.cover["samplings"][cam.sampling] += 1
            self.cover["factors"][op["n"]] += 1
            self.cover["interior"][bool(op.get("int"))] += 1
            px = cam.width * cam.height
            if k in ("render", "render_stats", "interior", "lit", "shaded", "shaded_aa", "lit_sum", "baked", "geometry"):
                self._use(sc, "d_frame", k, px * 4, ("render", "lit_sum", "render"))
            if k == "render_stats":
                self._use(sc, "d_entry", k, px * 8, ("render_stats", "pick", "render_stats"))
            if k == "pick":
                self._use(sc, "d_entry", k, (8 + (2 * cam.width + 2 * cam.height if cam.projection == hm.SPHERICAL else 0)) * 8,
                          ("render_stats", "pick", "render_stats"))
            if k == "lit_sum":
                self._use(sc, "d_targets", k, op["K"] * 24, ("lit_sum", "cell_map_sum", "lit_sum"))
        if k in ("cell_map", "cell_map_sum"):
            self._use(sc, "d_cells", k, op["rect"][2] * op["rect"][3] * (2 if k == "cell_map_sum" else 1), ("cell_map", "cell_map_sum", "cell_map"))
        if k in ("cell_map_sum", "bake_light"):
            self._use(sc, "d_targets", "cell_map_sum" if k == "cell_map_sum" else k, op["K"] * 24, ("lit_sum", "cell_map_sum", "lit_sum"))
        if k in FRAME_KINDS + QUERY_KINDS and (sc.host or sc.dev):
            ev["host_memory_calls_with_tickets_in_flight"] += 1
            ev["host_memory_calls_of_a_new_family_with_tickets_in_flight"] += int(k not in ("render", "render_stats"))
        if k in BEGIN_KINDS:
            self.handle += 1
            op["h"] = self.handle
            op["lane"] = sc.lane_next % 3
            sc.lane_next += 1
            ring = sc.dev if "dev" in k else sc.host
            ring[op["h"]] = k.split("_")[0] if k.split("_")[0] in ("shaded", "baked") else "plain"
            if {"plain", "shaded", "baked"} <= set(ring.values()):
                ev["device_tickets_of_all_three_kinds_in_flight" if "dev" in k else "host_ring_with_all_three_kinds"] += 1
        elif k == "wait":
            del sc.host[op["h"]]
            sc.lent.append(op["h"])
        elif k == "release":
            sc.lent.remove(op["h"])
        elif k == "dev_wait":
            del sc.dev[op["h"]]
        elif k in DEV_KINDS:
            if op.get("whole"):
                sc.whole = (op["i"], op["st"])
            if self.cap is not None:
                sc.pending[op["st"]].add(k)
        elif k == "take_capped":
            for kind in sc.pending.pop(op["st"], ()):
                self.taken[kind].add(op["st"])
        elif k == "sync":
            pass
        elif k == "update":
            kinds = set(sc.host.values()) | set(sc.dev.values())
            ev["updates_with_a_shaded_and_a_baked_ticket_in_flight"] += int({"shaded", "baked"} <= kinds)
            sc.pidx = op["p"]
        elif k in ("set_light", "set_light_device", "bake_light", "clear_light"):
            if "baked" in set(sc.host.values()) | set(sc.dev.values()):
                ev[f"{k}_with_a_baked_ticket_in_flight"] += 1
            if k == "set_light_device":
                op["src"], op["st"] = sc.whole
            sc.plane = k != "clear_light"
        elif k == "reopen":
            ev["reopens_with_a_light_plane"] += int(sc.plane)
            sc.reset()
            sc.pidx = op["p"]
        elif k == "env":
            self.kernel, self.cap = op["kernel"], op["step_cap"]
            for s in self.scenes:
                s.host, s.lent, s.dev = {}, [], {}
                s.pending.clear()
        ev["max_in_flight"] = max(ev["max_in_flight"], max(len(s.host) + len(s.dev) for s in self.scenes))
        return op

    def coverage(self):
        out = {k: dict(sorted(v.items(), key=lambda kv: str(kv[0]))) for k, v in self.cover.items()}
        out["events"] = dict(sorted(self.ev.items()))
        out["device_forms_taken_under_a_cap_on_streams"] = {k: sorted(v) for k, v in sorted(self.taken.items())}
        return out


EVENTS = ("host_ring_with_all_three_kinds", "device_tickets_of_all_three_kinds_in_flight", "updates_with_a_shaded_and_a_baked_ticket_in_flight",
          "set_light_with_a_baked_ticket_in_flight", "bake_light_with_a_baked_ticket_in_flight", "clear_light_with_a_baked_ticket_in_flight",
          "host_memory_calls_of_a_new_family_with_tickets_in_flight", "reopens_with_a_light_plane") + tuple(
              f"{m}_changed_hands_both_ways_with_a_grow_and_a_shrink" for m in ("d_targets", "d_entry", "d_frame", "d_cells"))


def coverage_gaps(cov, capped_taken=None):
    """What the issue wants every slice to reach -> list of what is missing.  capped_taken (a run's, not the plan's): device form
    -> caller streams on which hmrm_scene_take_capped returned a NON-ZERO count owed to that form alone."""
    gaps = [f"op kind {k}" for k in OP_KINDS if not cov["kinds"].get(k)]
    gaps += [f"kernel {k} without {f}" for k in ("unset", "leap", "group", "simple", "rec") for f in ("lit", "baked", "cells", "rays")
             if not cov["kernels"].get(f"{k}:{f}")]
    gaps += [f"projection {p}" for p in (1, 2, 3) if not cov["projections"].get(p)]
    gaps += [f"sampling {m}" for m in (0, 1, 2) if not cov["samplings"].get(m)]
    gaps += [f"factor {n}" for n in (1, 2, 4) if not cov["factors"].get(n)]
    gaps += [f"interior rule {b}" for b in (False, True) if not cov["interior"].get(b)]
    gaps += [f"{name} 0 < 1" for name in EVENTS if cov["events"].get(name, 0) < 1]
    for k in DEV_KINDS:
        if len(cov["device_forms_taken_under_a_cap_on_streams"].get(k, ())) < 2:
            gaps.append(f"{k} taken under a cap on fewer than 2 streams")
        if capped_taken is not None and len(capped_taken.get(k, ())) < 2:
            gaps.append(f"{k}: a non-zero capped count taken on fewer than 2 streams")
    return gaps


# ------------------------------------------------------------------------------------------------ expected values
def _rows(a, h):
    """Any plane -> (h, row bytes) uint8."""
    return np.ascontiguousarray(a).view(np.uint8).reshape(h, -1)


def padded(plane_rows, stride):
    """Rows of bytes in a buffer of `stride` bytes per row that was filled with SENTINEL."""
    out = np.full((plane_rows.shape[0], stride), SENTINEL, dtype=np.uint8)
    out[:, :plane_rows.shape[1]] = plane_rows
    return out


class Calc:
    """The numpy replays of tests/ applied to a map of MAPS under given parameters and a given step cap, memoised per (map,
    parameters, arguments, step cap).  Stateless apart from the memo: it knows nothing of scenes, tickets or planes."""

    def __init__(self, oracle, seed, memo=600):
        import baked_cases
        import cell_map_replay
        import geometry_replay
        import lit_sum_cases
        import ray_replay
        import segment_replay
        import shade_replay
        self.rr, self.sr, self.shr, self.cmr, self.gr, self.lsc, self.bc = (ray_replay, segment_replay, shade_replay, cell_map_replay,
                                                                          geometry_replay, lit_sum_cases, baked_cases)
        self.o, self.seed = oracle, seed
        self.plain = fz.Expect(oracle, seed)
        self.memo = collections.OrderedDict()
        self.keep = memo
        self.computed = 0

    def _m(self, key, fn):
        if key not in self.memo:
            self.memo[key] = fn()
            self.computed += 1
            if len(self.memo) > self.keep:
                self.memo.popitem(last=False)
        self.memo.move_to_end(key)
        return self.memo[key]

    def world(self, slot, params):
        rgb, cmap = self.plain.map_of(slot)
        return self._m(("h", slot, bytes(params)), lambda: self.o.update_heightmap(rgb, params)), cmap

    def frame(self, slot, params, cam, n, cap):
        return self.plain.frame(slot, params, cam, n, cap)

    def primary(self, slot, params, cam, n, interior, cap):
        """-> (rays, records) of the super camera's pixels, row-major."""
        sup = super_camera(hm, cam, n)
        heights, cmap = self.world(slot, params)
        bg = (cam.bg_r, cam.bg_g, cam.bg_b)

        def make():
            rays = self._m(("r", slot, bytes(params), bytes(sup)),
                           lambda: self.rr.camera_rays(self.o, self.o.make_cfg(sup, params, cmap.shape[1], cmap.shape[0])))
            if interior:
                return rays, self.sr.replay(rays, heights, cmap, params, cam.step_dist, bg=bg, sampling=cam.sampling, step_cap=cap or 1 << 26, interior=True)
            return rays, self.rr.replay(rays, heights, cmap, params, cam.step_dist, bg=bg, sampling=cam.sampling, step_cap=cap or 1 << 26)
        return self._m(("p", slot, bytes(params), bytes(sup), bool(interior), cap), make)

    def _fb(self, rgba, cam, n):
        fb = np.ascontiguousarray(rgba).reshape(cam.height * n, cam.width * n, 4)
        return box_filter(fb, n) if n > 1 else fb

    def interior(self, slot, params, cam, cap):
        _, rec = self.primary(slot, params, cam, 1, True, cap)
        return self._fb(rec["rgba"], cam, 1), int((rec["status"] == 2).sum())

    def shaded(self, slot, params, cam, n, sun, diffuse, shadows, cap):
        """sun: (dir, step_dist, max_steps, ambient, interior) -> (frame, capped rays)."""
        def make():
            heights, cmap = self.world(slot, params)
            rays, rec = self.primary(slot, params, cam, n, sun[4], cap)
            w = self.shr.replay(rays, heights, cmap, params, cam.step_dist, sun[0], sun[1], bg=(cam.bg_r, cam.bg_g, cam.bg_b), sampling=cam.sampling,
                                step_cap=cap or 1 << 26, max_steps=sun[2], ambient=sun[3], interior=sun[4], diffuse=diffuse, shadows=shadows, primary=rec)
            return self._fb(w["rgba"], cam, n), int(w["capped"])
        return self._m(("s", slot, bytes(params), bytes(cam), n, repr(sun), diffuse, shadows, cap), make)

    def geometry(self, slot, params, cam, interior, cap):
        def make():
            heights, _ = self.world(slot, params)
            rays, rec = self.primary(slot, params, cam, 1, interior, cap)
            return self.gr.planes(rec, rays, heights, params, cam.sampling), int((rec["status"] == 2).sum())
        return self._m(("g", slot, bytes(params), bytes(cam), bool(interior), cap), make)

    def lit_sum(self, slot, params, cam, sun, dirs, diffuse, shadows, cap):
        """-> (rgba (H, W, 4), light (H, W) uint16, capped rays: the primary ones once, shadow rays per ray)."""
        def make():
            heights, cmap = self.world(slot, params)
            rays, rec = self.primary(slot, params, cam, 1, sun[4], cap)
            hit = rec["status"] == 1
            own = int((rec["status"] == 2).sum())
            s = np.zeros(rec.shape[0], dtype=np.int64)
            capped = own
            for d in dirs:
                one = self.shr.replay(rays, heights, cmap, params, cam.step_dist, tuple(d.tolist()), sun[1], bg=(cam.bg_r, cam.bg_g, cam.bg_b),
                                      sampling=cam.sampling, step_cap=cap or 1 << 26, max_steps=sun[2], ambient=sun[3], interior=sun[4],
                                      diffuse=diffuse, shadows=shadows, primary=rec)
                s += one["w"]
                capped += int(one["capped"]) - own
            return (self._fb(self.lsc.apply(rec["rgba"], hit, s, len(dirs)), cam, 1),
                    self.lsc.light_plane(hit, s).reshape(cam.height, cam.width), capped)
        return self._m(("ls", slot, bytes(params), bytes(cam), repr(sun), dirs.tobytes(), diffuse, shadows, cap), make)

    def baked(self, slot, params, cam, n, interior, plane, full_scale, cap):
        def make():
            _, rec = self.primary(slot, params, cam, n, interior, cap)
            hit = rec["status"] == 1
            light = self.bc.light_of(rec, plane, params, cam.sampling)
            return self._fb(self.bc.apply(rec["rgba"], hit, light, full_scale), cam, n), int((rec["status"] == 2).sum())
        return self._m(("b", slot, bytes(params), bytes(cam), n, bool(interior), hashlib.md5(plane.tobytes()).hexdigest(), full_scale, cap), make)

    def pick(self, slot, params, cam, px, py, cap):
        _, rec = self.primary(slot, params, cam, 1, False, cap)
        return rec[py * cam.width + px: py * cam.width + px + 1]

    def batch(self, slot, params, op, cap):
        """The records of a rays / segments op."""
        def make():
            heights, cmap = self.world(slot, params)
            rays = batch_rays(slot, op["nr"], op["bid"])
            step = RAY_STEP * (SLOW if op["slow"] else 1.0)
            if "ms" not in op:
                return self.rr.replay(rays, heights, cmap, params, step, bg=BG, sampling=op["smp"], step_cap=cap or 1 << 26)
            return self.sr.replay(rays, heights, cmap, params, step, bg=BG, sampling=op["smp"], step_cap=cap or 1 << 26, interior=op["int"],
                                  max_steps=op["ms"], per_ray=batch_limits(slot, op["nr"], op["bid"]) if op["per"] else None)
        return self._m(("t", slot, bytes(params), op["nr"], op["bid"], op["smp"], op["slow"], op.get("int"), op.get("ms"), op.get("per"), cap), make)

    def cells(self, slot, params, rect, target, step, lift, max_steps, flags, sampling, ambient, cap):
        """hmrm_cell_map over `rect`: cell_map_replay's rays, statuses, levels and weights for the rect's cells alone
        -> ((h, w) uint8, capped rays)."""
        def make():
            cmr, shr = self.cmr, self.shr
            heights, cmap = self.world(slot, params)
            x0, y0, w, h = rect
            rays, cx, cy = cmr.cell_rays(heights, params, sampling, target, lift, bool(flags & cmr.TOWARDS_POINT))
            idx = np.nonzero((cx >= x0) & (cx < x0 + w) & (cy >= y0) & (cy < y0 + h))[0]
            status = None
            if not flags & cmr.NO_SHADOWS:
                status = self.sr.replay(rays[idx], heights, cmap, params, step, sampling=sampling, step_cap=cap or 1 << 26, interior=True,
                                        max_steps=max_steps)["status"].astype(np.uint8)
            capped = int((status == cmr.CAPPED).sum()) if status is not None else 0
            if not flags & cmr.WEIGHT:
                return status.reshape(h, w), capped
            q = None
            if flags & cmr.DIFFUSE:
                rec = np.zeros(idx.size, dtype=self.rr.RAY_HIT_DTYPE)
                rec["status"], rec["cell_x"], rec["cell_y"], rec["point"] = cmr.HIT, cx[idx], cy[idx], rays[idx, 0:3]
                gx, gy = shr.gradients(rec, heights, params, sampling)
                q = shr.levels_of(gx, gy, (rays[idx, 3], rays[idx, 4], rays[idx, 5]))
            return cmr.weights((idx.size,), status, q, flags, ambient).reshape(h, w), capped
        return self._m(("c", slot, bytes(params), rect, repr(target), step, lift, max_steps, flags, sampling, ambient, cap), make)

    def cell_sum(self, slot, params, rect, targets, step, lift, max_steps, flags, sampling, ambient, cap):
        """hmrm_cell_map_sum: the integer sum of the K maps (status mode: 1 per target whose ray did not hit) -> ((h, w) uint16, capped)."""
        def make():
            total, capped = np.zeros((rect[3], rect[2]), dtype=np.int64), 0
            for t in targets:
                one, c = self.cells(slot, params, rect, tuple(t.tolist()), step, lift, max_steps, flags, sampling, ambient, cap)
                total += one if flags & self.cmr.WEIGHT else (one != self.cmr.HIT)
                capped += c
            return total.astype(np.uint16), capped
        return self._m(("cs", slot, bytes(params), rect, targets.tobytes(), step, lift, max_steps, flags, sampling, ambient, cap), make)


def sun_of(op):
    """(dir, step_dist, max_steps, ambient, interior) of a sun-lit op."""
    return (SUN_DIRS[op["sd"]], SUN_STEP * (SLOW if op["cam"][0] == "q" else 1.0), op["sm"], op["amb"], bool(op.get("int")))


def make_sun(t):
    return hm.Sun.make(t[0], t[1], max_steps=t[2], ambient=t[3], interior=t[4])


def cell_args(op):
    """-> (target or targets, step_dist, lift, max_steps, flags, sampling, ambient) of a cell-map op."""
    point = op["point"]
    flags = MODES[op["mode"]] | (1 if point else 0)
    step, ms = (1.0 / 64, 64) if point else (SUN_STEP * (SLOW if op["slow"] else 1.0), op["ms"])
    if "K" in op:
        tg = directions(op["K"], op["dv"])
        if point:
            tg = np.ascontiguousarray(np.asarray(point_target(op["s"]))[None, :] + 0.5 * tg)
    else:
        tg = point_target(op["s"]) if point else SUN_DIRS[op["tg"]]
    return tg, step, op["lift"], ms, flags, op["smp"], 96


def cell_kw(a):
    return dict(step_dist=a[1], lift=a[2], max_steps=a[3], point=bool(a[4] & 1), weight=bool(a[4] & 2), diffuse=bool(a[4] & 4),
                shadows=not a[4] & 8, sampling=a[5], ambient=a[6])


# ------------------------------------------------------------------------------------------------ running
class Backend(TorchBackend):
    def upload(self, a, stream):
        """A host array in device memory, the copy ordered on caller stream `stream`."""
        with self.torch.cuda.stream(self.streams[stream]):
            return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")


class Runner:
    def __init__(self, plan, calc, backend):
        self.plan, self.calc, self.be, self.seed = plan, calc, backend, plan.seed
        self.scenes = {}
        self.bad = collections.Counter()
        self.recent = collections.deque(maxlen=40)
        self.hits = {}
        self.choices = collections.Counter()
        self.capped_taken = collections.defaultdict(set)
        for ps in plan.scenes:
            self._open(ps.slot, ps.pidx)

    def _open(self, slot, pidx):
        rgb, cmap = self.calc.plain.map_of(slot)
        params = scene_params(pidx)
        self.scenes[slot] = {"scene": self.be.scene(rgb, cmap, params), "params": params, "host": {}, "lent": {}, "dev": {}, "strips": [],
                             "lane_cum": [0, 0, 0], "lane_cums": [{0}, {0}, {0}], "lane_seen": [0, 0, 0], "plane": None, "whole": None,
                             "pending": collections.defaultdict(collections.Counter)}

    def mismatch(self, op, what):
        self.bad[op["k"]] += 1
        print(f"MISMATCH seed {self.seed} op {op['i']} {fmt_op(op)}: {what}; replay: python tests/deep_fuzz_families.py {self.seed} {op['i'] + 1}; "
              f"last ops: {' '.join(fmt_op(o) for o in self.recent)}", flush=True)

    def _same(self, op, got, want, what):
        got, want = np.asarray(got), np.asarray(want)
        if got.dtype != np.uint8 or want.dtype != np.uint8:
            got, want = _rows(got, 1), _rows(want, 1)
        if got.shape != want.shape or not np.array_equal(got, want):
            d = np.argwhere(got != want) if got.shape == want.shape else []
            self.mismatch(op, f"{what}: {len(d)} bytes differ, first at {d[:3].tolist() if len(d) else (got.shape, want.shape)}")
            return False
        return True

    def _host(self, op, fn, want_capped):
        """fn(allow_capped) -> result.  Capped rays: HMRM_E_NOTERM with the count in front of the message AND valid output, which a
        second call that allows them fetches."""
        got = 0
        try:
            res = fn(False)
        except hm.HmrmError as e:
            if e.code != hm.HMRM_E_NOTERM:
                raise
            got = int(e.message.split()[0])
            res = fn(True)
        if got != want_capped:
            self.mismatch(op, f"{got} capped rays reported, the replay has {want_capped}")
        return res

    def _refused(self, op, fn, text=""):
        try:
            fn()
        except hm.HmrmError as e:
            if e.code != hm.HMRM_E_ARG or text not in e.message:
                self.mismatch(op, f"refused with {e.code} '{e.message}', expected HMRM_E_ARG '{text}'")
            return
        self.mismatch(op, "the call was accepted, expected HMRM_E_ARG")

    def _lane_wait(self, op, st, lane, cum_j, got, exact):
        """deep_fuzz_api.Runner._lane_wait: a wait reports what its lane's counter held beyond what was reported before."""
        seen = st["lane_seen"][lane] + got
        last = st["lane_cum"][lane]
        ok = seen == max(st["lane_seen"][lane], cum_j) if exact else (seen >= cum_j and seen in st["lane_cums"][lane])
        if not ok:
            self.mismatch(op, f"lane {lane}: {got} capped rays reported; reported so far {st['lane_seen'][lane]}, through this launch {cum_j}, "
                              f"through the lane's last {last}")
        st["lane_seen"][lane] = seen if ok else min(max(seen, cum_j), last)

    def _noterm(self, fn):
        try:
            fn()
        except hm.HmrmError as e:
            if e.code != hm.HMRM_E_NOTERM:
                raise
            return int(e.message.split()[0])
        return 0

    def _wait(self, op, st):
        want, ticket, lane, cum_j = st["host"].pop(op["h"])
        sc = st["scene"]
        got = self._noterm(lambda: sc.render_wait(ticket, want.shape[:2], copy=False))
        frame = sc.render_wait(ticket, want.shape[:2])
        self._lane_wait(op, st, lane, cum_j, got, False)
        self._same(op, frame, want, "host ticket")
        st["lent"][op["h"]] = ticket

    def _dev_wait(self, op, st):
        ticket, buf, want, lane, cum_j = st["dev"].pop(op["h"])
        got = self._noterm(lambda: st["scene"].render_device_wait(ticket))
        self._lane_wait(op, st, lane, cum_j, got, True)
        self._same(op, self.be.read(buf, want.shape[0]), want, "device ticket")

    def _drain_streams(self, st, streams=None):
        for k in sorted({r[0]["st"] for r in st["strips"]} if streams is None else streams):
            self.be.sync_stream(k)
        keep = []
        for r in st["strips"]:
            if streams is None or r[0]["st"] in streams:
                for name, buf, want in r[1]:
                    self._same(r[0], self.be.read(buf, want.shape[0]), want, f"device form, {name}")
            else:
                keep.append(r)
        st["strips"] = keep

    def quiesce(self, st):
        for h in list(st["host"]):
            self._wait({"k": "wait", "s": -1, "h": h, "i": self.plan.n}, st)
        for h in list(st["lent"]):
            st["scene"].render_release(st["lent"].pop(h))
        for h in list(st["dev"]):
            self._dev_wait({"k": "dev_wait", "s": -1, "h": h, "i": self.plan.n}, st)
        self._drain_streams(st)

    def _check_light(self, op, st):
        got, fs = st["scene"].light()
        if st["plane"] is None:
            if got is not None or fs != 0:
                self.mismatch(op, f"the scene reports a light plane of full scale {fs}, the model has none")
        elif got is None or fs != st["plane"][1]:
            self.mismatch(op, f"full scale {fs}, the model's plane has {st['plane'][1]}")
        else:
            self._same(op, _rows(got, got.shape[0]), _rows(st["plane"][0], got.shape[0]), "light plane read back")

    def _ticket_frame(self, op, st, cam):
        """The frame a ticket begun NOW owes, and its capped rays."""
        k, cap, n = op["k"], op["step_cap"], op["n"]
        if k in ("begin", "dev_begin"):
            fr = self.calc.frame(op["s"], st["params"], cam, n, cap)
            return fr.fb, fr.capped
        if k.startswith("shaded"):
            return self.calc.shaded(op["s"], st["params"], cam, n, sun_of(op), op["dif"], op["sh"], cap)
        return self.calc.baked(op["s"], st["params"], cam, n, op["int"], st["plane"][0], st["plane"][1], cap)

    def _dev_launched(self, op, st, outs, capped, keep=()):
        st["strips"].append((op, outs, keep))
        st["pending"][op["st"]][op["k"]] += capped

    def run(self, op):
        self.recent.append(op)
        k = op["k"]
        be, calc = self.be, self.calc
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
        sc, slot, params, cap = st["scene"], op["s"], st["params"], op.get("step_cap")
        if "cam" in op:
            cam = camera_of(op["cam"], self.seed)
            W, H, n = cam.width, cam.height, op["n"]
        if k == "render":
            fr = calc.frame(slot, params, cam, 1, cap)
            got = []
            if self._noterm(lambda: got.append(sc.render(cam))) != fr.capped:
                self.mismatch(op, f"capped rays reported differ from the oracle's {fr.capped}")
            if got:
                self._same(op, got[0], fr.fb, "frame")
            choice = sc.kernel_choice()
            self.choices[choice] += 1
            forced = {"group": 1, "simple": 2, "rec": 3}.get(os.environ.get("HMRM_KERNEL"))
            if choice != forced if forced else choice not in (0, 1, 3):
                self.mismatch(op, f"kernel_choice() {choice} under HMRM_KERNEL={os.environ.get('HMRM_KERNEL')}")
        elif k == "render_stats":
            fr = calc.frame(slot, params, cam, 1, cap)
            fb, s, steps, entry = sc.render_stats(cam, per_pixel=True, allow_capped=True)
            self._same(op, steps.astype(np.int64), np.where(fr.steps < 0, -1 - fr.steps, fr.steps), "per-pixel steps")
            self._same(op, entry.view(np.uint64), fr.entry.view(np.uint64), "distance() bits")
            self._same(op, fb, fr.fb, "instrumented frame")
            if (s.rays, s.steps, s.capped) != (W * H, fr.total, fr.capped):
                self.mismatch(op, f"stats rays {s.rays} steps {s.steps} capped {s.capped}, oracle {W * H} {fr.total} {fr.capped}")
            hk = (slot, bytes(params), bytes(cam), cap)
            if self.hits.setdefault(hk, s.hits) != s.hits:
                self.mismatch(op, f"hits {s.hits}, an earlier render of the same frame had {self.hits[hk]}")
        elif k == "interior":
            want, capped = calc.interior(slot, params, cam, cap)
            self._same(op, self._host(op, lambda a: sc.render_interior(cam, allow_capped=a), capped), want, "interior frame")
        elif k in ("lit", "shaded", "shaded_aa"):
            sun = sun_of(op)
            want, capped = calc.shaded(slot, params, cam, n, sun, op["dif"], op["sh"], cap)
            if k == "lit":
                got = self._host(op, lambda a: sc.render_lit(cam, make_sun(sun), allow_capped=a), capped)
            else:
                got = self._host(op, lambda a: sc.render_shaded(cam, make_sun(sun), diffuse=op["dif"], shadows=op["sh"], allow_capped=a, aa=n), capped)
            self._same(op, got, want, "sun-lit frame")
        elif k == "geometry":
            want, capped = calc.geometry(slot, params, cam, op["int"], cap)
            got = self._host(op, lambda a: sc.render_geometry(cam, interior=op["int"], allow_capped=a, pad_px=op["pad"]), capped)
            for name, elem in (("rgba", 4), ("cell", 4), ("range", 4), ("slope", 8)):
                self._same(op, _rows(got[name], H), padded(_rows(want[name], H), (W + op["pad"]) * elem), f"geometry plane {name}")
        elif k == "lit_sum":
            sun, dirs = sun_of(op), directions(op["K"], op["dv"])
            rgba, light, capped = calc.lit_sum(slot, params, cam, sun, dirs, op["dif"], op["sh"], cap)
            got = self._host(op, lambda a: sc.render_lit_sum(cam, make_sun(sun), dirs, diffuse=op["dif"], shadows=op["sh"], light=True, allow_capped=a,
                                                             pad_px=op["pad"]), capped)
            self._same(op, _rows(got[0], H), padded(_rows(rgba, H), (W + op["pad"]) * 4), "lit sum, rgba")
            self._same(op, _rows(got[1], H), padded(_rows(light, H), (W + op["pad"]) * 2), "lit sum, light")
        elif k == "baked":
            want, capped = calc.baked(slot, params, cam, n, op["int"], st["plane"][0], st["plane"][1], cap)
            got = self._host(op, lambda a: sc.render_baked(cam, interior=op["int"], factor=n, pad_px=op["pad"], allow_capped=a), capped)
            self._same(op, _rows(got, H), padded(_rows(want, H), (W + op["pad"]) * 4), "baked frame")
        elif k == "pick":
            want = calc.pick(slot, params, cam, op["px"], op["py"], cap)
            got = self._host(op, lambda a: sc.pick(cam, op["px"], op["py"], allow_capped=a), int(want["status"][0] == 2))
            self._same(op, np.asarray(got).reshape(1), want, "picked record")
        elif k in ("rays", "segments"):
            want = calc.batch(slot, params, op, cap)
            rays, step = batch_rays(slot, op["nr"], op["bid"]), RAY_STEP * (SLOW if op["slow"] else 1.0)
            if k == "rays":
                fn = lambda a: sc.trace_rays(rays, step, bg=BG, sampling=op["smp"], stats=True, allow_capped=a)
            else:
                lim = batch_limits(slot, op["nr"], op["bid"]) if op["per"] else None
                fn = lambda a: sc.trace_segments(rays, step, bg=BG, sampling=op["smp"], interior=op["int"], max_steps=op["ms"], per_ray_max_steps=lim,
                                                 stats=True, allow_capped=a)
            capped = int((want["status"] == 2).sum())
            got, s = self._host(op, fn, capped)
            self._same(op, got, want, "records")
            if (s.rays, s.steps, s.hits, s.capped) != (op["nr"], int(want["steps"].sum()), int((want["status"] == 1).sum()), capped):
                self.mismatch(op, f"stats rays {s.rays} steps {s.steps} hits {s.hits} capped {s.capped}")
        elif k in ("rays_dev", "segments_dev"):
            want = calc.batch(slot, params, op, cap)
            nr, step = op["nr"], RAY_STEP * (SLOW if op["slow"] else 1.0)
            d_rays = be.upload(batch_rays(slot, nr, op["bid"]), op["st"])
            buf = be.buffer(1, (nr + 2) * 56, stream=op["st"])
            keep = [d_rays]
            if k == "rays_dev":
                sc.trace_rays_device(be.ptr(d_rays), nr, be.ptr(buf), step, bg=BG, sampling=op["smp"], stream=be.stream_handle(op["st"]))
            else:
                d_lim = be.upload(batch_limits(slot, nr, op["bid"]), op["st"]) if op["per"] else None
                keep.append(d_lim)
                sc.trace_segments_device(be.ptr(d_rays), nr, be.ptr(buf), step, bg=BG, sampling=op["smp"], interior=op["int"], max_steps=op["ms"],
                                         d_max_steps_ptr=be.ptr(d_lim) if op["per"] else 0, stream=be.stream_handle(op["st"]))
            self._dev_launched(op, st, [("records", buf, padded(_rows(want, 1), (nr + 2) * 56))], int((want["status"] == 2).sum()), keep)
        elif k in ("cell_map", "cell_map_dev"):
            a = cell_args(op)
            want, capped = calc.cells(slot, params, op["rect"], a[0], *a[1:], cap)
            stride = op["rect"][2] + op["pad"]
            if k == "cell_map":
                got = self._host(op, lambda al: sc.cell_map(a[0], rect=op["rect"], allow_capped=al, stride_bytes=stride, **cell_kw(a)), capped)
                self._same(op, got, padded(want, stride), "cell map")
            else:
                buf = be.buffer(want.shape[0], stride, stream=op["st"])
                sc.cell_map_device(be.ptr(buf), stride, a[0], rect=op["rect"], stream=be.stream_handle(op["st"]), **cell_kw(a))
                self._dev_launched(op, st, [("cell map", buf, padded(want, stride))], capped)
        elif k in ("cell_map_sum", "cell_map_sum_dev"):
            a = cell_args(op)
            want, capped = calc.cell_sum(slot, params, op["rect"], a[0], *a[1:], cap)
            stride = 2 * (op["rect"][2] + op["pad"])
            if k == "cell_map_sum":
                got = self._host(op, lambda al: sc.cell_map_sum(a[0], rect=op["rect"], allow_capped=al, stride_bytes=stride, **cell_kw(a)), capped)
                self._same(op, _rows(got, want.shape[0]), padded(_rows(want, want.shape[0]), stride), "cell map sum")
            else:
                d_t = be.upload(a[0], op["st"])
                buf = be.buffer(want.shape[0], stride, stream=op["st"])
                sc.cell_map_sum_device(be.ptr(buf), stride, be.ptr(d_t), len(a[0]), rect=op["rect"], stream=be.stream_handle(op["st"]), **cell_kw(a))
                self._dev_launched(op, st, [("cell map sum", buf, padded(_rows(want, want.shape[0]), stride))], capped, [d_t])
                if op.get("whole"):
                    st["whole"] = (op["i"], buf, stride, want, (255 if a[4] & 2 else 1) * len(a[0]))
        elif k == "geometry_dev":
            want, capped = calc.geometry(slot, params, cam, op["int"], cap)
            outs, at = [], {}
            for name, elem in (("rgba", 4), ("cell", 4), ("range", 4), ("slope", 8)):
                stride = (W + op["pad"]) * elem
                buf = be.buffer(H, stride, stream=op["st"])
                outs.append((f"geometry plane {name}", buf, padded(_rows(want[name], H), stride)))
                at[name] = (be.ptr(buf), stride)
            sc.render_geometry_device(cam, interior=op["int"], stream=be.stream_handle(op["st"]), **at)
            self._dev_launched(op, st, outs, capped)
        elif k == "lit_sum_dev":
            sun, dirs = sun_of(op), directions(op["K"], op["dv"])
            rgba, light, capped = calc.lit_sum(slot, params, cam, sun, dirs, op["dif"], op["sh"], cap)
            d_dirs = be.upload(dirs, op["st"])
            b_rgba, b_light = be.buffer(H, (W + op["pad"]) * 4, stream=op["st"]), be.buffer(H, (W + op["pad"]) * 2, stream=op["st"])
            sc.render_lit_sum_device(cam, make_sun(sun), be.ptr(d_dirs), len(dirs), rgba=(be.ptr(b_rgba), (W + op["pad"]) * 4),
                                     light=(be.ptr(b_light), (W + op["pad"]) * 2), diffuse=op["dif"], shadows=op["sh"], stream=be.stream_handle(op["st"]))
            self._dev_launched(op, st, [("lit sum, rgba", b_rgba, padded(_rows(rgba, H), (W + op["pad"]) * 4)),
                                        ("lit sum, light", b_light, padded(_rows(light, H), (W + op["pad"]) * 2))], capped, [d_dirs])
        elif k in BEGIN_KINDS:
            want, capped = self._ticket_frame(op, st, cam)
            lane = op["lane"]
            cum_j = st["lane_cum"][lane] = st["lane_cum"][lane] + capped
            st["lane_cums"][lane].add(cum_j)
            if "dev" in k:
                stride = (W + op["pad"]) * 4
                buf = be.buffer(H, stride)
                if k == "dev_begin":
                    t = sc.render_device_begin(cam, be.ptr(buf), stride, no_probe=op["no_probe"], aa=n)
                elif k == "shaded_dev_begin":
                    t = sc.render_shaded_device_begin(cam, make_sun(sun_of(op)), be.ptr(buf), stride, diffuse=op["dif"], shadows=op["sh"], aa=n)
                else:
                    t = sc.render_baked_device_begin(cam, be.ptr(buf), stride, interior=op["int"], aa=n)
                st["dev"][op["h"]] = (t, buf, padded(_rows(want, H), stride), lane, cum_j)
            else:
                if k == "begin":
                    t = sc.render_begin(cam, no_probe=op["no_probe"], aa=n)
                elif k == "shaded_begin":
                    t = sc.render_shaded_begin(cam, make_sun(sun_of(op)), diffuse=op["dif"], shadows=op["sh"], aa=n)
                else:
                    t = sc.render_baked_begin(cam, interior=op["int"], aa=n)
                st["host"][op["h"]] = (want, t, lane, cum_j)
        elif k == "wait":
            self._wait(op, st)
        elif k == "release":
            sc.render_release(st["lent"].pop(op["h"]))
        elif k == "dev_wait":
            self._dev_wait(op, st)
        elif k == "set_light":
            plane, d = light_plane(slot, op["pid"], op["u16"])
            wide = np.full((plane.shape[0], plane.shape[1] + op["pad"]), 0x5A, dtype=plane.dtype)
            wide[:, :plane.shape[1]] = plane
            sc.set_light(wide, d)
            st["plane"] = (plane.astype(np.uint16), d)
        elif k == "set_light_device":
            i, buf, stride, words, d = st["whole"]
            if i != op["src"]:
                self.mismatch(op, f"the runner holds the words of op {i}, the plan names op {op['src']}")
            sc.set_light_device(be.ptr(buf), stride, d, u16=True, stream=be.stream_handle(op["st"]))
            st["plane"] = (words.copy(), d)
            self._check_light(op, st)
        elif k == "bake_light":
            a = cell_args(op)
            _, mw, mh = MAPS[slot]
            want, capped = calc.cell_sum(slot, params, (0, 0, mw, mh), a[0], *a[1:], cap)
            self._host(op, lambda al: sc.bake_light(a[0], allow_capped=al, **cell_kw(a)), capped)
            st["plane"] = (want.copy(), (255 if a[4] & 2 else 1) * len(a[0]))
            self._check_light(op, st)
        elif k == "clear_light":
            sc.clear_light()
            st["plane"] = None
        elif k == "light":
            self._check_light(op, st)
        elif k == "refuse_baked":
            self._refused(op, lambda: sc.render_baked(cam, interior=op["int"], factor=n), "the scene has no light plane")
            self._check_light(op, st)
        elif k == "refuse_k0":
            a = cell_args(op)
            self._refused(op, lambda: sc.cell_map_sum(np.zeros((0, 3)), rect=op["rect"], **cell_kw(a)))
        elif k == "refuse_stride":
            _, mw, mh = MAPS[slot]
            self._refused(op, lambda: sc.set_light(np.zeros((mh, mw + 1), dtype=np.uint16), 1000, stride_bytes=2 * mw + 1))
            self._check_light(op, st)
        elif k == "take_capped":
            got = sc.take_capped(be.stream_handle(op["st"]), allow_capped=True)
            owed = st["pending"].pop(op["st"], collections.Counter())
            want = sum(owed.values())
            if got != want:
                self.mismatch(op, f"take_capped {got}, the launches enqueued on stream {op['st']} since the last call hold {want}: {dict(owed)}")
            elif len([v for v in owed.values() if v]) == 1:   # (a non-zero count owed to one device form alone)
                self.capped_taken[[f for f, v in owed.items() if v][0]].add(op["st"])
            if got and self._noterm(lambda: sc.take_capped(be.stream_handle(op["st"]))) != 0:
                self.mismatch(op, "a second take_capped still reports capped rays")
        elif k == "update":
            self._drain_streams(st)
            st["params"] = scene_params(op["p"])
            sc.update(st["params"])
        elif k == "reopen":
            self.quiesce(st)
            sc.close()
            self._open(slot, op["p"])

    def finish(self):
        for st in self.scenes.values():
            self.quiesce(st)
            for k, owed in list(st["pending"].items()):
                got = st["scene"].take_capped(self.be.stream_handle(k), allow_capped=True)
                if got != sum(owed.values()):
                    self.mismatch({"k": "take_capped", "i": self.plan.n, "st": k}, f"at the end: take_capped {got}, expected {sum(owed.values())}")
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
    runner = Runner(plan, Calc(oracle, seed), Backend(plan.n_streams))
    try:
        while plan.n < ops and time.time() - t0 < budget_s and sum(runner.bad.values()) < 20:
            runner.run(plan.next_op())
        runner.finish()
    except hm.HmrmError as e:
        print(f"ERROR seed {seed} after op {plan.n - 1}: {e}; last ops: {' '.join(fmt_op(o) for o in runner.recent)}", flush=True)
        print(f"fam: ops {plan.n}, mismatches {sum(runner.bad.values()) + 1}, per-kind {dict(runner.bad)}, stopped by an error of the library")
        return 2
    cov = plan.coverage()
    cov["non_zero_capped_counts_taken_on_streams"] = {k: sorted(v) for k, v in sorted(runner.capped_taken.items())}
    bad = sum(runner.bad.values())
    print(f"fam: ops {plan.n}, mismatches {bad}, per-kind {dict(runner.bad)}, seed {seed}, streams {plan.n_streams}, replays {runner.calc.computed}, "
          f"oracle frames {runner.calc.plain.computed}, kernel_choice() seen {dict(runner.choices)}, {time.time() - t0:.0f} s")
    print(f"fam: coverage {cov}")
    print(f"fam: missing {coverage_gaps(cov, runner.capped_taken)}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
