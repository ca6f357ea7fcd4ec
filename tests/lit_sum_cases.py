"""What tests/test_lit_sum_cpu.py and tests/test_lit_sum_gpu.py share: hmrm_render_lit_sum (include/hmrm.h) in numpy, a
composition of the replays that exist -- w_k is tests/shade_cases.py's replayed hmrm_render_shaded weight under direction k,
summed in int64; the pixel formula is applied to the primary records' colours; capped = the primary rays' capped + the sum of
the shadow rays' capped -- and a cache of such frames, read-only."""
import numpy as np

import lit_replay as lr
import shade_cases as shc
from lit_cases import BASE_CAP, SUNS  # noqa: F401
from shade_cases import AMBIENT  # noqa: F401

NO_HIT = 0xFFFF


def pixel(c, s, k):
    """(c * S + (255 K) // 2) // (255 K), elementwise in int64."""
    c, s = np.asarray(c, dtype=np.int64), np.asarray(s, dtype=np.int64)
    return (c * s + (255 * k) // 2) // (255 * k)


def apply(rgba, hit, s, k):
    """The rgba plane: R, G and B of the hit records under their sums, A and every other record as they are."""
    out = rgba.copy()
    out[hit, 0:3] = pixel(rgba[hit, 0:3], s[hit, None], k).astype(np.uint8)
    return out


def light_plane(hit, s):
    return np.where(hit, s, NO_HIT).astype(np.uint16)


class Replays(shc.Replays):
    def __init__(self, hmrm, oracle):
        super().__init__(hmrm, oracle)
        self._sums = {}

    def lit_sum(self, gw, proj, sampling, dirs, diffuse=False, shadows=True, inside=False, width=40, height=30, step_cap=BASE_CAP,
                max_steps=0, ambient=AMBIENT, sun_step=None):
        """The replayed hmrm_render_lit_sum planes of segment_cases.camera(gw, proj, inside, sampling, width, height) ->
        dict: rgba (n x 4), light (n uint16), S (n int64), w (K x n), shadowed (K x n bools), hit, primary, capped."""
        dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
        key = (gw, proj, sampling, dirs.tobytes(), diffuse, shadows, inside, width, height, step_cap, max_steps, ambient, sun_step)
        if key not in self._sums:
            primary = self.primary(gw, proj, sampling, inside, width, height, step_cap)
            hit = primary["status"] == lr.HIT
            primary_capped = int((primary["status"] == lr.CAPPED).sum())
            k = dirs.shape[0]
            w = np.empty((k, primary.shape[0]), dtype=np.int64)
            shadowed = np.zeros((k, primary.shape[0]), dtype=bool)
            capped = primary_capped
            for i, d in enumerate(dirs):
                one = self.shaded(gw, proj, sampling, tuple(d.tolist()), diffuse, shadows, inside, width, height, step_cap, max_steps,
                                  ambient, sun_step)
                w[i] = one["w"]
                shadowed[i] = one["shadowed"]
                capped += one["capped"] - primary_capped
            s = w.sum(axis=0, dtype=np.int64)
            want = dict(rgba=apply(primary["rgba"], hit, s, k), light=light_plane(hit, s), S=s, w=w, shadowed=shadowed, hit=hit,
                        primary=primary, capped=capped)
            for v in want.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            self._sums[key] = want
        return self._sums[key]
