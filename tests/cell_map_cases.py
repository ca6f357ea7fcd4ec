"""What tests/test_cell_map_cpu.py and tests/test_cell_map_gpu.py share: map A -- tests/segment_cases.py's 64 x 48 map, which
has zero-height cells, with a block at luminance 255 so that some cells sit at max_height --, its scene parameters and grid
widths, the three suns of tests/lit_cases.py with step_dist 0.3 grid widths, the two observer points, map B (37 x 21: partial
tiles on both sides), and a cache of replayed maps (tests/cell_map_replay.py), computed once and read-only."""
import numpy as np

import cell_map_replay as cmr
import scenes
import segment_cases as sc
from lit_cases import AMBIENT, SUN_IDS, SUNS  # noqa: F401
from segment_cases import GRID_WIDTHS, GW_IDS, MAP_H, MAP_W  # noqa: F401

SAMPLINGS = (0, 1, 2)
BASE_CAP = 4096  # no ray of the base cases comes near it
B_W, B_H, B_SEED = 37, 21, 41
# (lift in grid widths, max_steps): on the surface without a limit, an eye height above it with one
SETTINGS = ((0.0, 0), (0.25, 40))
# the four bytes a cell can be asked for: status, WEIGHT, WEIGHT + DIFFUSE, WEIGHT + DIFFUSE + NO_SHADOWS
MODES = (0, cmr.WEIGHT, cmr.WEIGHT | cmr.DIFFUSE, cmr.WEIGHT | cmr.DIFFUSE | cmr.NO_SHADOWS)
POINT_STEP, POINT_STEPS = 1.0 / 64, 64  # a ray that ends at about O


def maps_a():
    rgb, cmap = sc.maps()
    rgb[20:23, 10:14] = 255  # cells at max_height
    return rgb, cmap


def maps_b():
    return scenes.small_maps(B_W, B_H, B_SEED)


def point_above(gw):
    return (20.3 * gw, -17.7 * gw, 9.0 * gw)


def point_inside(gw):
    return (20.3 * gw, -17.7 * gw, 6.0 * gw)


def flags_kw(flags):
    """HMRM_MAP_* -> Scene.cell_map's keywords."""
    return dict(point=bool(flags & cmr.TOWARDS_POINT), weight=bool(flags & cmr.WEIGHT), diffuse=bool(flags & cmr.DIFFUSE),
                shadows=not flags & cmr.NO_SHADOWS)


class Replays:
    def __init__(self, hmrm, oracle):
        self.hmrm, self.oracle = hmrm, oracle
        self.rgb, self.cmap = maps_a()
        self.rgb_b, self.cmap_b = maps_b()
        self.params = {gw: sc.scene_params(hmrm, gw) for gw in GRID_WIDTHS}
        self.heights = {gw: oracle.update_heightmap(self.rgb, p) for gw, p in self.params.items()}
        self.heights_b = {gw: oracle.update_heightmap(self.rgb_b, p) for gw, p in self.params.items()}
        self._status, self._level = {}, {}

    def _maps(self, which, gw):
        return (self.heights[gw], self.cmap) if which == "A" else (self.heights_b[gw], self.cmap_b)

    def status(self, gw, sampling, target, step_dist, lift=0.0, max_steps=0, point=False, step_cap=BASE_CAP, which="A"):
        key = (which, gw, sampling, tuple(repr(float(v)) for v in target), step_dist, lift, max_steps, point, step_cap)
        if key not in self._status:
            heights, cmap = self._maps(which, gw)
            s = cmr.statuses(heights, cmap, self.params[gw], sampling, target, step_dist, lift, max_steps, point, step_cap)
            s.setflags(write=False)
            self._status[key] = s
        return self._status[key]

    def level(self, gw, sampling, target, lift=0.0, point=False, which="A"):
        key = (which, gw, sampling, tuple(repr(float(v)) for v in target), lift if point else 0.0, point)
        if key not in self._level:
            q = cmr.levels(self._maps(which, gw)[0], self.params[gw], sampling, target, lift, point)
            q.setflags(write=False)
            self._level[key] = q
        return self._level[key]

    def bytes(self, gw, sampling, target, step_dist, flags, lift=0.0, max_steps=0, ambient=AMBIENT, step_cap=BASE_CAP, which="A"):
        """The (H, W) uint8 map hmrm_cell_map must write."""
        point = bool(flags & cmr.TOWARDS_POINT)
        status = None
        if not flags & cmr.NO_SHADOWS:
            status = self.status(gw, sampling, target, step_dist, lift, max_steps, point, step_cap, which)
        if not flags & cmr.WEIGHT:
            return status
        q = self.level(gw, sampling, target, lift, point, which) if flags & cmr.DIFFUSE else None
        return cmr.weights(self._maps(which, gw)[0].shape, status, q, flags, ambient)


def counts(status):
    return {k: int((status == v).sum()) for k, v in (("miss", cmr.MISS), ("hit", cmr.HIT), ("capped", cmr.CAPPED), ("end", cmr.END))}
