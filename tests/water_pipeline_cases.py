"""What tests/test_water_pipeline_cpu.py and tests/test_water_pipeline_gpu.py share: hmrm_render_water_aa (include/hmrm.h) in
numpy, a composition of the replays that exist and no marching code of its own -- tests/water_cases.py's replayed water frame
(tests/water_replay.py: the primary and the mirror records), tests/baked_cases.py's light of a record (light_of) and its pixel
formula under the formula plane over the lake map, and tests/aa_box.py's filter and super camera.  The baked water frame weights
the primary records that hit (a wet one's base is the water's own colour when it has one) and the HIT rows of the mirror records,
each under the light of its own hit, then calls water_replay.blend.  A cache of such frames, read-only."""
import numpy as np

import aa_box
import baked_cases as bc
import ray_replay
import water_cases as wc
import water_replay as wr
from baked_cases import FULL_SCALE
from segment_cases import BG, MAP_H, MAP_W
from water_cases import BASE_CAP, REFLECTIVITY

# (the formula plane makes a mix-up visible on the lake map: test_water_pipeline_cpu.py counts the mirror hits whose light
# differs from their primary hit's -- more than nine in ten)
formula_plane = bc.formula_plane


def weigh(want, plane, full_scale, params, sampling, reflectivity=REFLECTIVITY, color=None):
    """The baked water frame of a replayed water frame `want` (water_replay.replay's dict) -> n x 4 uint8, and the lights of the
    primary and of the mirror records (0 where a ray did not hit)."""
    primary, mirror, idx = want["primary"], want["mirror"], want["mirror_index"]
    hit, mhit = primary["status"] == wr.HIT, mirror["status"] == wr.HIT
    light = bc.light_of(primary, plane, params, sampling)
    mlight = bc.light_of(mirror, plane, params, sampling)
    base = primary["rgba"].copy()
    if color is not None:
        base[idx] = np.array([color[0], color[1], color[2], 255], dtype=np.uint8)
    base = bc.apply(base, hit, light, full_scale)          # b': every hit pixel, wet or dry
    m = bc.apply(mirror["rgba"], mhit, mlight, full_scale)  # m': HIT rows only; MISS, END and CAPPED keep the miss shade
    rgba = base.copy()
    rgba[idx] = wr.blend(base[idx], m, reflectivity)
    return rgba, light, mlight


class Replays(wc.Replays):
    def __init__(self, hmrm, oracle):
        super().__init__(hmrm, oracle)
        self.plane = formula_plane()
        self.plane.setflags(write=False)
        self._baked_water = {}

    def frame(self, gw, proj, sampling, baked, plane=None, full_scale=FULL_SCALE, reflectivity=REFLECTIVITY, color=None, **kw):
        """The replayed water frame (baked: under `plane`, None: the formula plane) of water_cases.Replays.water's camera and
        water -> dict: rgba, water (the plain replay's dict), light and mirror_light (baked only)."""
        want = self.water(gw, proj, sampling, reflectivity=reflectivity, color=color, **kw)
        if not baked:
            return dict(rgba=want["rgba"], water=want)
        plane = self.plane if plane is None else np.asarray(plane)
        key = (gw, proj, sampling, plane.dtype.str, plane.tobytes(), full_scale, reflectivity, None if color is None else tuple(color),
               tuple(sorted((k, repr(v)) for k, v in kw.items())))
        if key not in self._baked_water:
            rgba, light, mlight = weigh(want, plane, full_scale, self.params[gw], sampling, reflectivity, color)
            for v in (rgba, light, mlight):
                v.setflags(write=False)
            self._baked_water[key] = dict(rgba=rgba, water=want, light=light, mirror_light=mlight)
        return self._baked_water[key]

    def filtered(self, gw, proj, sampling, n, baked, width=20, height=15, **kw):
        """The replayed antialiased frame: the (baked) water frame of the n x n larger camera, box-filtered."""
        want = self.frame(gw, proj, sampling, baked, width=width * n, height=height * n, **kw)
        return aa_box.box_filter(want["rgba"].reshape(height * n, width * n, 4), n)

    def of_camera(self, cam, gw, level, n=1, baked=False, plane=None, full_scale=FULL_SCALE, interior=False, mirror_step=None, **kw):
        """The replayed (antialiased, baked) water frame of any camera, from the oracle's rays of its super camera -> the filtered
        frame and the replay's dict."""
        sup = aa_box.super_camera(self.hmrm, cam, n)
        rays = ray_replay.camera_rays(self.oracle, self.oracle.make_cfg(sup, self.params[gw], MAP_W, MAP_H))
        reflectivity, color = kw.pop("reflectivity", REFLECTIVITY), kw.pop("color", None)
        want = wr.replay(rays, self.heights[gw], self.cmap, self.params[gw], cam.step_dist, level,
                         cam.step_dist if mirror_step is None else mirror_step, bg=BG, sampling=cam.sampling,
                         step_cap=kw.pop("step_cap", BASE_CAP), reflectivity=reflectivity, color=color, interior=interior, **kw)
        rgba = want["rgba"]
        if baked:
            rgba = weigh(want, self.plane if plane is None else np.asarray(plane), full_scale, self.params[gw], cam.sampling,
                         reflectivity, color)[0]
        return aa_box.box_filter(rgba.reshape(sup.height, sup.width, 4), n), want


def light_differs(got):
    """How many mirror rays that HIT have a light word other than their primary hit's (a baked frame of Replays.frame)."""
    want = got["water"]
    mhit = want["mirror"]["status"] == wr.HIT
    return int((got["mirror_light"][mhit] != got["light"][want["mirror_index"]][mhit]).sum())


def block_mixes(want, width, height, n):
    """(output pixels whose n x n block of samples mixes wet and dry ones, ... mixes primary hits and misses) of a replayed
    width * n x height * n super frame (water_replay.replay's dict)."""
    def mixed(flag):
        per = flag.reshape(height, n, width, n).sum(axis=(1, 3))
        return int(((per > 0) & (per < n * n)).sum())
    return mixed(want["water"]), mixed(want["primary"]["status"] == wr.HIT)
