"""What tests/test_baked_cpu.py and tests/test_baked_gpu.py share: hmrm_render_baked (include/hmrm.h) in numpy, a composition of
the replays that exist -- the primary records are tests/lit_cases.py's; the light of a record that hit is the plane's word of its
hit cell or, bilinear sampling, the four neighbours of tests/ray_replay.py's _bil at ((P.x - c0.x) / gw, -(P.y - c0.y) / gw) mixed
in float64 (tests/shade_replay.py's set-up for its gradients); the pixel formula is applied in int64 -- the test plane, given by
formula, and a cache of such frames, read-only.  numpy's float64 ufuncs are plain IEEE operations, no contraction."""
import numpy as np

import lit_replay as lr
import lit_sum_cases as lsc
from lit_cases import BASE_CAP  # noqa: F401
from ray_replay import _bil, box
from segment_cases import MAP_H, MAP_W

FULL_SCALE = 1000


def formula_plane():
    """L[y, x] = (37 x + 101 y + 29 ((x y) mod 13)) mod 1001, full scale 1000 -> (MAP_H, MAP_W) uint16."""
    y, x = np.mgrid[0:MAP_H, 0:MAP_W].astype(np.int64)
    return ((37 * x + 101 * y + 29 * ((x * y) % 13)) % 1001).astype(np.uint16)


def u8_twin(plane):
    """The plane in bytes: L * 255 // 1000, full scale 255."""
    return (plane.astype(np.int64) * 255 // FULL_SCALE).astype(np.uint8)


def pixel(c, light, full_scale):
    """min(255, (c * L + D // 2) // D), elementwise in int64."""
    c, light = np.asarray(c, dtype=np.int64), np.asarray(light, dtype=np.int64)
    return np.minimum(255, (c * light + full_scale // 2) // full_scale)


def nearest_light(primary, plane):
    """The plane's word of every record's hit cell (0 where the ray did not hit) -> n int64."""
    hit = primary["status"] == lr.HIT
    cx = np.where(hit, primary["cell_x"].astype(np.int64), 0)
    cy = np.where(hit, primary["cell_y"].astype(np.int64), 0)
    return np.where(hit, plane.reshape(-1).astype(np.int64)[cy * plane.shape[1] + cx], 0)


def bilinear_light(primary, plane, params):
    """The four neighbours' words mixed at every record's hit point, rounded with floor(m + 0.5) and clamped -> n int64."""
    mh, mw = plane.shape
    c0, _c1 = box(params, mw, mh)
    gw = params.grid_width
    hit = primary["status"] == lr.HIT
    f = plane.reshape(-1).astype(np.float64)
    with np.errstate(all="ignore"):
        qx = np.where(hit, (primary["point"][:, 0] - c0[0]) / gw, 0.0)
        qy = np.where(hit, -(primary["point"][:, 1] - c0[1]) / gw, 0.0)
        (c00, c10, c01, c11), tx, ty = _bil(qx, qy, mw, mh)
        a = f[c00] + tx * (f[c10] - f[c00])
        c = f[c01] + tx * (f[c11] - f[c01])
        m = a + ty * (c - a)
        v = np.clip(m + 0.5, 0.0, 65535.0)
    return np.where(hit, np.floor(v).astype(np.int64), 0)


def light_of(primary, plane, params, sampling):
    plane = np.asarray(plane)
    return bilinear_light(primary, plane, params) if sampling == 1 else nearest_light(primary, plane)


def apply(rgba, hit, light, full_scale):
    """The frame: R, G and B of the hit records under their light, A and every other record as they are."""
    out = rgba.copy()
    out[hit, 0:3] = pixel(rgba[hit, 0:3], light[hit, None], full_scale).astype(np.uint8)
    return out


class Replays(lsc.Replays):
    def __init__(self, hmrm, oracle):
        super().__init__(hmrm, oracle)
        self._baked = {}
        self.plane = formula_plane()
        self.plane.setflags(write=False)
        self.plane8 = u8_twin(self.plane)
        self.plane8.setflags(write=False)

    def baked(self, gw, proj, sampling, plane=None, full_scale=FULL_SCALE, inside=False, width=40, height=30, step_cap=BASE_CAP):
        """The replayed hmrm_render_baked frame of segment_cases.camera(gw, proj, inside, sampling, width, height) under `plane`
        (None: the formula plane) -> dict: rgba (n x 4), L (n int64), hit, primary, capped."""
        plane = self.plane if plane is None else np.asarray(plane)
        key = (gw, proj, sampling, plane.dtype.str, plane.tobytes(), full_scale, inside, width, height, step_cap)
        if key not in self._baked:
            primary = self.primary(gw, proj, sampling, inside, width, height, step_cap)
            hit = primary["status"] == lr.HIT
            light = light_of(primary, plane, self.params[gw], sampling)
            want = dict(rgba=apply(primary["rgba"], hit, light, full_scale), L=light, hit=hit, primary=primary,
                        capped=int((primary["status"] == lr.CAPPED).sum()))
            for v in want.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            self._baked[key] = want
        return self._baked[key]


def content(replays, gw, proj, sampling, inside):
    """The four figures the tests ask of a replayed frame under the formula plane: hit pixels, distinct light values among them,
    hit pixels that differ from the plain frame and -- bilinear sampling, else None -- hit pixels whose interpolated light differs
    from the nearest cell's."""
    want = replays.baked(gw, proj, sampling, inside=inside)
    hit, primary = want["hit"], want["primary"]
    changed = (want["rgba"] != primary["rgba"]).any(axis=1) & hit
    other = None
    if sampling == 1:
        other = int((want["L"][hit] != nearest_light(primary, replays.plane)[hit]).sum())
    return int(hit.sum()), int(np.unique(want["L"][hit]).size), int(changed.sum()), other
