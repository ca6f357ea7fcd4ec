"""What tests/test_haze_cpu.py and tests/test_haze_gpu.py share: a cache of replayed haze frames (tests/haze_replay.py) on top of
tests/lit_cases.py's primary records and camera rays -- the map, grid widths and cameras of tests/segment_cases.py -- computed
once per camera, read-only; the haze every camera is tested under, picked from the replay itself; and the conditions every
replay-based case asserts of its replay before it compares anything."""
import numpy as np

import haze_replay as hr
import lit_cases as lc
import segment_cases as sc
from lit_cases import BASE_CAP

COLOR = (200, 210, 220)
ENTRIES = 64
LAW, DENSITY = 1, 3.0  # HMRM_HAZE_EXP


class Replays(lc.Replays):
    def __init__(self, hmrm, oracle):
        super().__init__(hmrm, oracle)
        self._haze, self._params = {}, {}
        self.table = hmrm.haze_table(LAW, DENSITY, ENTRIES)
        self.table.setflags(write=False)

    def haze_of(self, gw, proj, sampling, inside=False, sky=False, n=ENTRIES):
        """The camera's haze: start the 10th and far the 90th percentile of the hit ranges of its 40 x 30 frame at step cap
        BASE_CAP (so that at least a tenth of the hits lands on either clamp), n entries."""
        key = (gw, proj, sampling, inside)
        if key not in self._params:
            prim = self.primary(gw, proj, sampling, inside)
            r = hr.ranges(prim, self.rays(gw, proj, inside))[prim["status"] == hr.HIT]
            assert r.size >= 100
            self._params[key] = (float(np.percentile(r, 10)), float(np.percentile(r, 90)))
        start, far = self._params[key]
        return self.hmrm.Haze.make(start, far, n, COLOR, sky=sky, interior=inside)

    def haze(self, gw, proj, sampling, inside=False, width=40, height=30, step_cap=BASE_CAP, sky=False, factor=1, haze=None, table=None):
        """The replayed haze frame of segment_cases.camera(gw, proj, inside, sampling, width, height) under haze_of's haze and
        the EXP table -- or under `haze` (an hmrm.Haze: start, scale, colour and sky flag are read from it) and `table`; factor:
        the frame of the factor x factor larger super camera, every sample hazed (box-filter it with haze_replay.filtered)."""
        if haze is None:
            haze = self.haze_of(gw, proj, sampling, inside, sky)
        table = self.table if table is None else np.ascontiguousarray(table, dtype=np.uint8)
        assert int(haze.n) == table.size
        key = (gw, proj, sampling, inside, width, height, step_cap, factor, repr(float(haze.start)), repr(float(haze.scale)),
               bytes(haze.color), int(haze.flags) & self.hmrm.HAZE_SKY, table.tobytes())
        if key not in self._haze:
            w, h = width * factor, height * factor
            want = hr.frame(self.primary(gw, proj, sampling, inside, w, h, step_cap), self.rays(gw, proj, inside, w, h), haze.start,
                            haze.scale, table, bytes(haze.color), bool(int(haze.flags) & self.hmrm.HAZE_SKY))
            want["plain"] = self.primary(gw, proj, sampling, inside, w, h, step_cap)["rgba"]
            for v in want.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            self._haze[key] = want
        return self._haze[key]


def counts(want, n=ENTRIES):
    """(hits, non-hits, capped, hits at index 0, hits at index n - 1, distinct indices strictly between, hit pixels that differ
    from the unhazed frame) of a replayed frame."""
    hit, idx = want["hit"], want["index"]
    between = np.unique(idx[hit & (idx > 0) & (idx < n - 1)])
    differ = (np.asarray(want["rgba"]) != np.asarray(want["plain"])).any(axis=1) & hit
    return (int(hit.sum()), int((~hit).sum()), want["capped"], int((idx[hit] == 0).sum()), int((idx[hit] == n - 1).sum()), int(between.size),
            int(differ.sum()))


def check(want, n=ENTRIES, capped_ok=False):
    """The conditions of a replay a case may rely on: both kinds of pixel, no capped ray, hits on both clamps and in between,
    and a haze that shows."""
    c = counts(want, n)
    hits, misses, capped, first, last, between, differ = c
    assert hits >= 100 and misses >= 100 and first >= 10 and last >= 10 and between >= 8 and differ >= 30, c
    assert capped_ok or capped == 0, c
    return c
