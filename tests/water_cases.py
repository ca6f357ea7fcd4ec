"""What tests/test_water_cpu.py and tests/test_water_gpu.py share: the lake map -- tests/segment_cases.py's height image clamped
from below at luminance LAKE_LUM, np.maximum(rgb, 110): 1039 of its 3072 cells flooded, all at one threshold -- with its grid
widths and cameras, the water level a quarter of a luminance step above the lake's threshold, and a cache of replayed water
frames (tests/water_replay.py) -- primary records once per camera, mirror rays once per water, read-only."""
import numpy as np

import lit_cases as lc
import water_replay as wr
from segment_cases import BG, GRID_WIDTHS, MAP_H, MAP_W, MAX_HEIGHT_GW  # noqa: F401

LAKE_LUM = 110
FLOODED = 1039
BASE_CAP = lc.BASE_CAP  # no ray of the base cases comes near it
REFLECTIVITY = 128


def flood(rgb, lum=LAKE_LUM):
    return np.maximum(rgb, np.uint8(lum))


class Replays(lc.Replays):
    """lit_cases.Replays over the lake map: rays() and primary() are its own."""

    def __init__(self, hmrm, oracle):
        super().__init__(hmrm, oracle)
        self.dry_rgb = self.rgb
        self.flooded = (self.dry_rgb <= LAKE_LUM).all(axis=2)  # the cells whose pixel is (110, 110, 110) afterwards
        self.rgb = flood(self.dry_rgb)
        self.heights = {gw: oracle.update_heightmap(self.rgb, p) for gw, p in self.params.items()}
        self._water = {}

    def lake_threshold(self, gw, sampling=0):
        """t of a flooded cell: its height plus min_height, float-rounded for sampling 2."""
        y, x = np.argwhere(self.flooded)[0]
        t = float(self.heights[gw][y, x]) + float(self.params[gw].min_height)
        return float(np.float32(t)) if sampling == 2 else t

    def level(self, gw):
        """The lake's threshold plus a quarter of a luminance step: float rounding and the next luminance are both far away."""
        return self.lake_threshold(gw) + MAX_HEIGHT_GW * gw / 255.0 / 4.0

    def water(self, gw, proj, sampling, level=None, inside=False, width=40, height=30, step_cap=BASE_CAP, max_steps=0,
              reflectivity=REFLECTIVITY, color=None, mirror_step=None):
        """The replayed water frame of segment_cases.camera(gw, proj, inside, sampling, width, height); inside: the primary rays
        under the interior rule.  level: self.level(gw) unless given; mirror step_dist: 0.2 * gw unless given."""
        level = self.level(gw) if level is None else level
        mirror_step = 0.2 * gw if mirror_step is None else mirror_step
        key = (gw, proj, sampling, repr(float(level)), inside, width, height, step_cap, max_steps, reflectivity,
               None if color is None else tuple(color), mirror_step)
        if key not in self._water:
            want = wr.replay(self.rays(gw, proj, inside, width, height), self.heights[gw], self.cmap, self.params[gw], 0.2 * gw,
                             level, mirror_step, bg=BG, sampling=sampling, step_cap=step_cap, max_steps=max_steps,
                             reflectivity=reflectivity, color=color, interior=inside,
                             primary=self.primary(gw, proj, sampling, inside, width, height, step_cap))
            for v in want.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            self._water[key] = want
        return self._water[key]


def counts(want):
    """(water pixels, mirror rays that hit, mirror rays that miss, capped rays) of a replayed frame."""
    status = want["mirror"]["status"]
    return int(want["water"].sum()), int((status == wr.HIT).sum()), int((status == wr.MISS).sum()), want["capped"]
