"""What tests/test_water_lit_cpu.py and tests/test_water_lit_gpu.py share: tests/water_cases.py's lake map, cameras and level, the
suns chosen on the CPU so that every base camera shows lit and shadowed hits on both sides of the mirror (the floors and the counts
found are in tests/test_water_lit_cpu.py), and a cache of replayed sun-lit water frames (tests/water_lit_replay.py) -- the water
frame once per water, the shadow rays once per sun, read-only."""
import numpy as np

import ray_replay
import segment_cases as sc
import water_cases as wc
import water_lit_replay as wl
from segment_cases import BG, GRID_WIDTHS, MAP_H, MAP_W, MAX_HEIGHT_GW  # noqa: F401
from water_cases import BASE_CAP, REFLECTIVITY  # noqa: F401

# A low sun across the relief per projection (directions as given, not normalised): 15 degrees above the horizon, from two azimuths.
SUNS = {1: (0.837, 0.483, 0.259), 2: (0.483, 0.837, 0.259), 3: (0.837, 0.483, 0.259)}
AMBIENT = 96


def sun_of(proj):
    return SUNS[proj]


INSIDE_ORTHO_WIDTH_GW = 1.5


def inside_camera(hmrm, gw, proj, sampling=0):
    """The camera inside the box of the interior cases.  Perspective and spherical: segment_cases.camera's.  Orthographic: that
    camera with a plane half as wide -- segment_cases' own shows 24 water pixels whatever the sun, below the floor of 34; this one
    shows 82 (66 bilinear), and 177 of its 1200 origins are strictly inside the box, the others are not."""
    if proj != 3:
        return sc.camera(hmrm, gw, proj, True, sampling)
    deg = hmrm.degrees_to_rads
    return hmrm.Camera.make(width=40, height=30, projection=3, hfov=deg(sc.hfov_deg(3)), hang=deg(sc.HANG_DEG), vang=deg(sc.VANG_DEG),
                            pos=sc.camera_pos(gw, True), ortho_width=INSIDE_ORTHO_WIDTH_GW * gw, step_dist=sc.STEP_DIST_GW * gw, bg=BG,
                            sampling=sampling)


class Replays(wc.Replays):
    """water_cases.Replays with the sun-lit frames: rays(), primary() and water() are its own."""

    def __init__(self, hmrm, oracle):
        super().__init__(hmrm, oracle)
        self._lit_water = {}

    def frame(self, gw, proj, sampling, sun=None, diffuse=True, shadows=True, level=None, inside=False, width=40, height=30,
              step_cap=BASE_CAP, max_steps=0, reflectivity=REFLECTIVITY, color=None, mirror_step=None, sun_step=None, sun_max_steps=0,
              ambient=AMBIENT):
        """The replayed sun-lit water frame of segment_cases.camera(gw, proj, inside, sampling, width, height) under `sun`
        (sun_of(proj) unless given); shadow step_dist: 0.3 * gw unless given; the rest as water_cases.Replays.water."""
        sun = sun_of(proj) if sun is None else sun
        level = self.level(gw) if level is None else level
        mirror_step = 0.2 * gw if mirror_step is None else mirror_step
        sun_step = 0.3 * gw if sun_step is None else sun_step
        key = (gw, proj, sampling, tuple(repr(float(v)) for v in sun), diffuse, shadows, repr(float(level)), inside, width, height,
               step_cap, max_steps, reflectivity, None if color is None else tuple(color), mirror_step, sun_step, sun_max_steps, ambient)
        if key not in self._lit_water:
            wet = self.water(gw, proj, sampling, level, inside, width, height, step_cap, max_steps, reflectivity, color, mirror_step)
            want = wl.replay(self.rays(gw, proj, inside, width, height), self.heights[gw], self.cmap, self.params[gw], 0.2 * gw,
                             level, mirror_step, sun, sun_step, bg=BG, sampling=sampling, step_cap=step_cap, max_steps=max_steps,
                             reflectivity=reflectivity, color=color, sun_max_steps=sun_max_steps, ambient=ambient, diffuse=diffuse,
                             shadows=shadows, interior=inside, wet=wet)
            for v in want.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            self._lit_water[key] = want
        return self._lit_water[key]

    def inside_frame(self, gw, proj, sampling):
        """The replayed frame of inside_camera(gw, proj, sampling) under sun_of(proj), the primary rays under the interior rule."""
        if proj != 3:
            return self.frame(gw, proj, sampling, inside=True)
        key = ("inside ortho", gw, sampling)
        if key not in self._lit_water:
            cam = inside_camera(self.hmrm, gw, 3, sampling)
            rays = ray_replay.camera_rays(self.oracle, self.oracle.make_cfg(cam, self.params[gw], MAP_W, MAP_H))
            self._lit_water[key] = wl.replay(rays, self.heights[gw], self.cmap, self.params[gw], 0.2 * gw, self.level(gw), 0.2 * gw,
                                             sun_of(3), 0.3 * gw, bg=BG, sampling=sampling, step_cap=BASE_CAP, ambient=AMBIENT,
                                             interior=True)
        return self._lit_water[key]


def counts(want, width=40):
    """Of a replayed frame: (water pixels, mirror hits, mirror hits shadowed, mirror hits lit, wet pixels whose primary hit is
    shadowed, ... lit, dry hits shadowed, waves -- 8 x 8 tiles -- that hold a wet lane, a dry hit and a miss at once, mirror hits
    whose weight differs from their primary hit's)."""
    hit = want["primary"]["status"] == wl.HIT
    wet, idx = want["water"], want["mirror_index"]
    mhit = want["mirror"]["status"] == wl.HIT
    shadowed = want["shadowed"]
    n = hit.shape[0]
    tile = (np.arange(n) // width // 8) * ((width + 7) // 8) + (np.arange(n) % width) // 8
    mixed = sum(1 for k in np.unique(tile) if wet[tile == k].any() and (hit & ~wet)[tile == k].any() and (~hit)[tile == k].any())
    return (int(wet.sum()), int(mhit.sum()), int((mhit & want["mirror_shadowed"]).sum()), int((mhit & ~want["mirror_shadowed"]).sum()),
            int((wet & shadowed).sum()), int((wet & ~shadowed).sum()), int((hit & ~wet & shadowed).sum()), int(mixed),
            int((mhit & (want["mirror_w"] != want["w"][idx])).sum()))


FLOORS = (34, 5, 2, 2, 2, 2, 2, 1, 1)
