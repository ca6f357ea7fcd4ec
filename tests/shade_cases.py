"""What tests/test_shaded_cpu.py and tests/test_shaded_gpu.py share: tests/lit_cases.py's map, cameras, suns and cache of
replayed lit frames, and on top of it a cache of replayed shaded frames (tests/shade_replay.py), read-only."""
import numpy as np

import lit_cases as lc
import shade_replay as shr
from lit_cases import BASE_CAP, SUNS, SUN_IDS  # noqa: F401
from segment_cases import BG

AMBIENT = 96


class Replays(lc.Replays):
    def __init__(self, hmrm, oracle):
        super().__init__(hmrm, oracle)
        self._shaded = {}

    def shaded(self, gw, proj, sampling, sun, diffuse=True, shadows=True, inside=False, width=40, height=30, step_cap=BASE_CAP,
               max_steps=0, ambient=AMBIENT, sun_step=None):
        """The replayed hmrm_render_shaded frame of segment_cases.camera(gw, proj, inside, sampling, width, height)."""
        key = (gw, proj, sampling, tuple(repr(float(v)) for v in sun), diffuse, shadows, inside, width, height, step_cap, max_steps,
               ambient, sun_step)
        if key not in self._shaded:
            primary = self.primary(gw, proj, sampling, inside, width, height, step_cap)
            lit = None
            if shadows:
                lit = self.lit(gw, proj, sampling, sun, inside, width, height, step_cap, max_steps, ambient, sun_step)
            want = shr.replay(None, self.heights[gw], self.cmap, self.params[gw], 0.2 * gw, sun, None, bg=BG, sampling=sampling,
                              step_cap=step_cap, max_steps=max_steps, ambient=ambient, interior=inside, diffuse=diffuse,
                              shadows=shadows, primary=primary, lit=lit)
            for v in want.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            self._shaded[key] = want
        return self._shaded[key]


def down_camera(hmrm, gw, sampling=0, width=56, height=72, map_w=64, map_h=48):
    """An orthographic camera straight above the map's centre, looking down (hang = 0: the frame's rows run along world x, its
    columns along world y; ortho_width is per pixel), its plane a tenth larger than the map: every border line and every
    corner cell is some pixel's hit."""
    per_pixel = 1.1 * gw * max(map_w / height, map_h / width)
    return hmrm.Camera.make(width=width, height=height, projection=3, hfov=hmrm.degrees_to_rads(80), hang=0.0,
                            vang=hmrm.degrees_to_rads(180), pos=(0.5 * map_w * gw, -0.5 * map_h * gw, 20.0 * gw),
                            ortho_width=per_pixel, step_dist=0.2 * gw, bg=BG, sampling=sampling)
