"""What tests/test_lit_cpu.py and tests/test_lit_gpu.py share: the map, grid widths and cameras of tests/segment_cases.py, the
suns, and a cache of replayed lit frames (tests/lit_replay.py) -- primary records once per camera, shadow rays once per sun,
read-only."""
import numpy as np

import lit_replay as lr
import ray_replay
import segment_cases as sc
import segment_replay as sr
from segment_cases import BG, GRID_WIDTHS, MAP_H, MAP_W

SUNS = ((0.6, 0.5, 0.35), (-0.7, 0.2, 0.15), (0.3, -0.8, 0.6))
SUN_IDS = ["sun_ne", "sun_low_w", "sun_high_s"]
BASE_CAP = 4096  # no ray of the base cases comes near it: the frames are those of any larger cap
AMBIENT = 128


class Replays:
    def __init__(self, hmrm, oracle):
        self.hmrm, self.oracle = hmrm, oracle
        self.rgb, self.cmap = sc.maps()
        self.params = {gw: sc.scene_params(hmrm, gw) for gw in GRID_WIDTHS}
        self.heights = {gw: oracle.update_heightmap(self.rgb, p) for gw, p in self.params.items()}
        self._primary, self._lit = {}, {}

    def rays(self, gw, proj, inside=False, width=40, height=30):
        return sc.camera_rays(self.hmrm, self.oracle, gw, proj, inside, width, height)

    def primary(self, gw, proj, sampling, inside=False, width=40, height=30, step_cap=BASE_CAP):
        key = (gw, proj, sampling, inside, width, height, step_cap)
        if key not in self._primary:
            rays = self.rays(gw, proj, inside, width, height)
            if inside:
                r = sr.replay(rays, self.heights[gw], self.cmap, self.params[gw], 0.2 * gw, bg=BG, sampling=sampling,
                              step_cap=step_cap, interior=True)
            else:
                r = ray_replay.replay(rays, self.heights[gw], self.cmap, self.params[gw], 0.2 * gw, bg=BG, sampling=sampling,
                                      step_cap=step_cap)
            r.setflags(write=False)
            self._primary[key] = r
        return self._primary[key]

    def lit(self, gw, proj, sampling, sun, inside=False, width=40, height=30, step_cap=BASE_CAP, max_steps=0, ambient=AMBIENT,
            sun_step=None):
        """The replayed lit frame of segment_cases.camera(gw, proj, inside, sampling, width, height); inside: the primary rays
        under the interior rule.  Shadow step_dist: 0.3 * gw unless given."""
        sun_step = 0.3 * gw if sun_step is None else sun_step
        key = (gw, proj, sampling, tuple(repr(float(v)) for v in sun), inside, width, height, step_cap, max_steps, ambient, sun_step)
        if key not in self._lit:
            want = lr.replay(self.rays(gw, proj, inside, width, height), self.heights[gw], self.cmap, self.params[gw], 0.2 * gw, sun,
                             sun_step, bg=BG, sampling=sampling, step_cap=step_cap, max_steps=max_steps, ambient=ambient,
                             interior=inside, primary=self.primary(gw, proj, sampling, inside, width, height, step_cap))
            for v in want.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            self._lit[key] = want
        return self._lit[key]


def counts(want):
    """(shadowed, lit) hit pixels and capped rays of a replayed frame."""
    hit = want["primary"]["status"] == lr.HIT
    return int(want["shadowed"].sum()), int((hit & ~want["shadowed"]).sum()), want["capped"]
