"""Family-scale cases: the scene of tests/segment_cases.py -- its 64 x 48 map and its outside and inside cameras at 40 x 30, in
all three projections -- at world magnitudes other than the unit one, for the families that carry arithmetic of their own on
top of the plain frame: ray and segment batches, interior frames, sun-lit and shaded frames, cell maps, geometry planes, water,
haze and the compositions of them.  Plain module, not collected; deterministic, no GPU, and nothing here calls the library for
an expected value: every expectation is a composition of the numpy replays (tests/*_replay.py), which carry no magnitudes.
tests/test_family_scale_cpu.py asserts the conditions every case must meet on the replay alone,
tests/test_world_scale_families_gpu.py runs the kernels against it, bytewise.

A case is a descriptor (Case) from which scene, parameters, cameras and family parameters follow; `unit` is the length every
number segment_cases.py gives in grid widths is multiplied with, `base` what OFFSET adds to every absolute height.

Sweeps
  P2      every length times 2^k: grid_width 2^k, max_height 8 * 2^k, the camera's pos, ortho_width and step_dist, the sun,
          mirror and cell step distances (0.3, 0.2, 0.3 grid widths), the cell lift (0.25) and point target, the water level and
          the haze bounds.  Perspective takes k <= 24 only (beyond, cam_pos + look loses the unit `look`, tests/world_scale.py).
  DEC     the same times a power of ten: fl(1 / grid_width) is inexact, the gradient divisions round differently at every scale.
  GW      grid widths an ulp below and above 2^e and 2^e / 3 (world_scale.gw_members), every other length times that width.
  OFFSET  world_scale.offset_scene's construction on this map: relief 8 on top of an absolute height H, plain (box 0 .. 2H) and
          mirrored (box -H .. H); camera heights, the point target, the water level raised by the base.  At 1e9 the float table
          quantises the relief to multiples of 64.
  SUN     the unit scene with the sun direction (and the cell map's direction target) times 2^m and the sun's step_dist times
          2^-m: the shadow rays' step vectors are the unit ones, bit for bit (asserted), while diffuse_level's products under-
          or overflow.

What the replay gives at these members, measured and pinned by tests/test_family_scale_cpu.py:
  * SUN.  The shadow ray's first position is origin + (0.01 * grid_width) * dir: that nudge scales with the sun's magnitude, so
    the shadow march is NOT the unit one although its steps are.  A shadow ray leaves the grid before its first load once
    0.01 * |dir| exceeds the grid's extent in grid widths: at 2^512, 2^520 and 2^600 no pixel is shadowed.  At 2^3 the nudge is
    0.08 |dir| grid widths, neither the unit one nor off the grid (18 of the outside orthographic camera's 631 hits change
    sides).  At 2^-520, 2^-535 and 2^-600 it vanishes (the ray starts at the hit point itself).  The level: 0 everywhere at
    2^520 and 2^600 (dot / inf); the unit levels at 2^3 and, through a denormal s.s, at 2^-520; only 0 and 255 at 2^-600
    (s.s == 0: dot / 0 is +-inf or NaN).  None of those can tell the root of the product from the product of two roots
    (measured: a library built that way passes them); two members can: at 2^-535 s.s keeps 4 bits and (n.n) * (s.s) is
    rounded to that grid before the root (386 of the outside orthographic camera's 631 levels differ from the unit ones), and
    at 2^512 s.s = 1.465 * 2^1023 is finite while (n.n) * (s.s) overflows for every slope with n.n > 1.36 (q = 0 there, the
    unit level on flatter ground).
  * Point-mode cell maps.  dir = O - pos is a length there, so the first position lies the fraction 0.01 * grid_width of the way
    to O: a viewshed means what it says while grid_width < 100.  Cells hidden from the point, of 3072: 1818 at 2^0, 1039 at 2^5
    (the ray starts 0.32 of the way), none at 2^7 (it starts 1.28 of the way, beyond O, and marches on away from it: 1891 rays
    leave the grid, 1181 end inside it), and from 2^15 every ray has left the grid before its first load.  2^5 and 2^7 are in
    the sweep for the two sides of that limit.
  * Range.  ex * ex overflows from k = 508 (every hit's r is inf at 900, all but the nearest at 510) and is zero at -900; at -530
    it is denormal for every hit and r stays non-zero; at -510 it is still normal.  So the haze of |k| <= 490, of -510 and of
    -530 is picked from the case's own ranges; at 510 and +-900 it is the k = 0 haze times 2^k, and every hit with an infinite
    or zero range sits on one clamp.
  * The float planes: at k = 123 the range plane mixes finite and infinite floats, at -140 every range is a float denormal, at
    -154 it mixes zeros and denormals.
"""
import math

import numpy as np

import baked_cases as bkc
import cell_map_cases as cc
import cell_map_replay as cmr
import geometry_replay as gr
import haze_replay as hr
import lit_cases
import lit_replay as lr
import lit_sum_cases as lsc
import ray_replay
import scenes
import segment_cases as sc
import segment_replay as sr
import shade_replay as shr
import water_lit_replay as wlr
import water_replay as wr
import world_scale as ws
from segment_cases import BG, MAP_H, MAP_W

hmrm = scenes.hmrm

PROJECTIONS = ws.PROJECTIONS
SWEEPS = ("P2", "DEC", "GW", "OFFSET", "SUN")
P2_K = (-900, -530, -510, -490, -154, -145, -140, 0, 5, 7, 24, 123, 490, 510, 900)
P2_PERSP_MAX_K = ws.P2_PERSP_MAX_K
DEC_S = (1e-12, 1e-3, 30.0, 1e12)
GW_E = (-40, 0, 40)
GW_MEMBERS = ("below", "above", "third")
OFFSET_H = (1e6, 1e9)
SUN_M = (-600, -535, -520, 3, 512, 520, 600)
OFFSET_ORTHO_WIDTH = 1.6  # the outside orthographic camera's pixel in OFFSET (1.3 elsewhere)
RELIEF = sc.MAX_HEIGHT_GW  # 8, in grid widths

SUN_DIR = (0.6, 0.5, 0.35)  # not a unit vector, used as given
SUN_STEP_GW, MIRROR_STEP_GW, CELL_STEP_GW, CELL_LIFT_GW = 0.3, sc.STEP_DIST_GW, 0.3, 0.25
AMBIENT = 96
REFLECTIVITY = 128
HAZE_COLOR, HAZE_ENTRIES, HAZE_LAW, HAZE_DENSITY = (200, 210, 220), 64, 1, 3.0
BASE_CAP = 4096  # no camera, shadow, mirror or cell ray of any case comes near it
ODD_CAP = 4096   # the step cap the rays no camera makes are traced under (some never leave the grid)
FRAME_W, FRAME_H = 40, 30
SAMPLINGS = (0, 1, 2)


def _tag(v):
    return ("%g" % v).replace("+", "").replace("-", "m").replace(".", "p")


class Case:
    """One member of a sweep in one projection.  rgb, cmap: the maps (shared: do not write to them); params: SceneParams;
    unit, base: see the module's docstring; sun_dir, sun_step: the sun; cell_dir: the cell map's direction target."""

    def __init__(self, sweep, proj, member, unit=1.0, grid_width=None, offset=None, sun_pow=0, k=None):
        pname = dict(PROJECTIONS)[proj]
        self.sweep, self.proj, self.member, self.k = sweep, proj, member, k
        self.name = f"{sweep}_{pname}_{member}"
        self.unit = float(unit)
        gw = self.unit if grid_width is None else float(grid_width)
        self.rgb, self.cmap = _maps()
        self.base = 0.0
        if offset is None:
            self.params = hmrm.SceneParams.make(0.0, RELIEF * self.unit, grid_width=gw)
        else:
            self.rgb, self.params, self.base = _offset_scene(*offset)
        self.sun_pow = sun_pow
        self.sun_dir = tuple(math.ldexp(v, sun_pow) for v in SUN_DIR)
        self.sun_step = math.ldexp(SUN_STEP_GW * self.unit, -sun_pow)
        self.cam_step = sc.STEP_DIST_GW * self.unit
        self.mirror_step = MIRROR_STEP_GW * self.unit
        self.cell_dir, self.cell_step = self.sun_dir, math.ldexp(CELL_STEP_GW * self.unit, -sun_pow)
        p = cc.point_above(self.unit)
        self.cell_point, self.cell_lift = (p[0], p[1], p[2] + self.base), CELL_LIFT_GW * self.unit

    def camera(self, inside, sampling=0, width=FRAME_W, height=FRAME_H):
        cam = sc.camera(hmrm, self.unit, self.proj, inside, sampling, width, height)
        cam.pos[2] += self.base
        if self.sweep == "OFFSET" and self.proj == 3 and not inside:
            # (the red channel's relief alone leaves the 1.3-wide plane 95 pixels that do not hit: haze_cases.check asks for 100)
            cam.ortho_width = OFFSET_ORTHO_WIDTH
        return cam

    def sun(self, inside=False, ambient=AMBIENT):
        return hmrm.Sun.make(self.sun_dir, self.sun_step, ambient=ambient, interior=inside)

    def __repr__(self):
        return self.name


_map_cache = {}


def _maps():
    if "m" not in _map_cache:
        rgb, cmap = sc.maps()
        rgb.setflags(write=False)
        cmap.setflags(write=False)
        _map_cache["m"] = (rgb, cmap)
    return _map_cache["m"]


def _offset_scene(h, mirrored):
    """world_scale.offset_scene's construction on segment_cases' map with relief 8: blue 128, red keeps the map, value =
    eps * red + 128, threshold = value / 255 * (max - min) + 2 * min.  -> (rgb, params, lowest threshold)"""
    key = ("offset", h, mirrored)
    if key not in _map_cache:
        rgb = _maps()[0].copy()
        rgb[:, :, 2] = 128
        rgb.setflags(write=False)
        lo, hi = (-h, h) if mirrored else (0.0, h * 255.0 / 128.0)
        eps = RELIEF / (hi - lo)
        params = hmrm.SceneParams.make(lo, hi, lum=(eps, 0.0, 1.0), grid_width=1.0)
        _map_cache[key] = (rgb, params, 128.0 / 255.0 * (hi - lo) + 2.0 * lo)
    return _map_cache[key]


def _build():
    out = []
    for proj, _pname in PROJECTIONS:
        for k in P2_K:
            if proj == 1 and k > P2_PERSP_MAX_K:
                continue
            out.append(Case("P2", proj, f"k{_tag(k)}", unit=math.ldexp(1.0, k), k=k))
        for s in DEC_S:
            out.append(Case("DEC", proj, f"s{_tag(s)}", unit=s))
        for e in GW_E:
            widths = dict(ws.gw_members(e))
            for m in GW_MEMBERS:
                out.append(Case("GW", proj, f"e{_tag(e)}_{m}", unit=widths[m]))
        for mirrored in (False, True):
            for h in OFFSET_H:
                out.append(Case("OFFSET", proj, f"{'neg' if mirrored else 'pos'}{_tag(h)}", offset=(h, mirrored)))
        for m in SUN_M:
            out.append(Case("SUN", proj, f"m{_tag(m)}", sun_pow=m))
    assert len({c.name for c in out}) == len(out)
    return out


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = _build()
    return _cases


def sweep(name, proj=None):
    return [c for c in cases() if c.sweep == name and (proj is None or c.proj == proj)]


def case(name):
    return next(c for c in cases() if c.name == name)


def p2(proj, k):
    return case(f"P2_{dict(PROJECTIONS)[proj]}_k{_tag(k)}")


def unit_case(proj):
    return p2(proj, 0)


def _freeze(v):
    if isinstance(v, np.ndarray):
        v.setflags(write=False)
    elif isinstance(v, dict):
        for x in v.values():
            _freeze(x)
    elif isinstance(v, tuple):
        for x in v:
            _freeze(x)
    return v


class Replays:
    """What the replays give for a case, computed once and read-only; keyed by the case's name."""

    def __init__(self, hmrm_, oracle):
        self.hmrm, self.oracle = hmrm_, oracle
        self._c = {}
        self.table = hmrm_.haze_table(HAZE_LAW, HAZE_DENSITY, HAZE_ENTRIES)  # (host arithmetic, the same bytes at every scale)
        self.table.setflags(write=False)

    def _get(self, key, make):
        if key not in self._c:
            self._c[key] = _freeze(make())
        return self._c[key]

    # ---- the scene ----
    def heights(self, c):
        return self._get(("heights", c.rgb.ctypes.data, bytes(c.params)), lambda: self.oracle.update_heightmap(c.rgb, c.params))

    def rays(self, c, inside, width=FRAME_W, height=FRAME_H):
        """The oracle's GetRay for every pixel of the case's camera."""
        return self._get(("rays", bytes(c.camera(inside, 0, width, height)), bytes(c.params)),
                         lambda: ray_replay.camera_rays(self.oracle, self.oracle.make_cfg(c.camera(inside, 0, width, height), c.params, MAP_W, MAP_H)))

    def primary(self, c, inside, sampling=0, width=FRAME_W, height=FRAME_H):
        def make():
            rays, h = self.rays(c, inside, width, height), self.heights(c)
            if inside:
                return sr.replay(rays, h, c.cmap, c.params, c.cam_step, bg=BG, sampling=sampling, step_cap=BASE_CAP, interior=True)
            return ray_replay.replay(rays, h, c.cmap, c.params, c.cam_step, bg=BG, sampling=sampling, step_cap=BASE_CAP)
        return self._get(("primary", bytes(c.camera(inside, 0, width, height)), bytes(c.params), c.rgb.ctypes.data, sampling), make)

    def odd_rays(self, c):
        """segment_cases.odd_rays at the case's scale, raised by its base, mixed with every eighth ray of the outside camera."""
        def make():
            rays = sc.odd_rays(c.unit, np.zeros((0, 6)))
            rays[:, 2] += c.base
            rays = np.concatenate([rays, self.rays(c, False)[::8]])
            return np.ascontiguousarray(rays[np.random.RandomState(5).permutation(rays.shape[0])])
        return self._get(("odd", c.unit, c.base, c.proj), make)

    def odd_records(self, c, sampling, interior):
        def make():
            if interior:
                return sr.replay(self.odd_rays(c), self.heights(c), c.cmap, c.params, c.cam_step, bg=BG, sampling=sampling, step_cap=ODD_CAP,
                                 interior=True)
            return ray_replay.replay(self.odd_rays(c), self.heights(c), c.cmap, c.params, c.cam_step, bg=BG, sampling=sampling, step_cap=ODD_CAP)
        return self._get(("oddrec", c.name, sampling, interior), make)

    def limits(self, c, inside):
        """Per-ray step limits for the camera rays: 0 (none), 3, 9 and 40, a fixed draw."""
        n = self.rays(c, inside).shape[0]
        return np.random.RandomState(4).choice([0, 3, 9, 40], size=n).astype(np.uint32)

    def segments(self, c, inside, sampling=0):
        """The camera rays as segments: interior rule on, per-ray limits and max_steps = 25."""
        return self._get(("segments", c.name, inside, sampling),
                         lambda: sr.replay(self.rays(c, inside), self.heights(c), c.cmap, c.params, c.cam_step, bg=BG, sampling=sampling,
                                           step_cap=BASE_CAP, interior=True, max_steps=25, per_ray=self.limits(c, inside)))

    # ---- the families ----
    def lit(self, c, inside, sampling=0, width=FRAME_W, height=FRAME_H, ambient=AMBIENT):
        return self._get(("lit", c.name, inside, sampling, width, height, ambient),
                         lambda: lr.replay(self.rays(c, inside, width, height), self.heights(c), c.cmap, c.params, c.cam_step, c.sun_dir,
                                           c.sun_step, bg=BG, sampling=sampling, step_cap=BASE_CAP, ambient=ambient, interior=inside,
                                           primary=self.primary(c, inside, sampling, width, height)))

    def shaded(self, c, inside, sampling=0, shadows=True, width=FRAME_W, height=FRAME_H, ambient=AMBIENT):
        return self._get(("shaded", c.name, inside, sampling, shadows, width, height, ambient),
                         lambda: shr.replay(None, self.heights(c), c.cmap, c.params, c.cam_step, c.sun_dir, None, bg=BG, sampling=sampling,
                                            step_cap=BASE_CAP, ambient=ambient, interior=inside, diffuse=True, shadows=shadows,
                                            primary=self.primary(c, inside, sampling, width, height),
                                            lit=self.lit(c, inside, sampling, width, height, ambient) if shadows else None))

    def cell_target(self, c, point):
        """(target, step_dist, lift, max_steps) of the case's direction or point map."""
        if point:
            return c.cell_point, cc.POINT_STEP, c.cell_lift, cc.POINT_STEPS
        return c.cell_dir, c.cell_step, 0.0, 0

    def cell_status(self, c, point, sampling=0):
        target, step, lift, limit = self.cell_target(c, point)
        return self._get(("cellstatus", c.name, point, sampling),
                         lambda: cmr.statuses(self.heights(c), c.cmap, c.params, sampling, target, step, lift, limit, point, BASE_CAP))

    def cell_weight(self, c, point, sampling=0):
        """The bytes of HMRM_MAP_WEIGHT | HMRM_MAP_DIFFUSE."""
        target, _step, lift, _limit = self.cell_target(c, point)

        def make():
            q = cmr.levels(self.heights(c), c.params, sampling, target, lift, point)
            return cmr.weights((MAP_H, MAP_W), self.cell_status(c, point, sampling), q, cmr.WEIGHT | cmr.DIFFUSE, AMBIENT)
        return self._get(("cellweight", c.name, point, sampling), make)

    def planes(self, c, inside, sampling=0):
        return self._get(("planes", c.name, inside, sampling),
                         lambda: gr.planes(self.primary(c, inside, sampling), self.rays(c, inside), self.heights(c), c.params, sampling))

    def ranges(self, c, inside, sampling=0):
        """(r as doubles, hit)"""
        return self._get(("ranges", c.name, inside, sampling),
                         lambda: (hr.ranges(self.primary(c, inside, sampling), self.rays(c, inside)),
                                  self.primary(c, inside, sampling)["status"] == hr.HIT))

    def water_level(self, c, inside):
        """The median threshold of the camera's nearest-sampled hits."""
        def make():
            prim = self.primary(c, inside, 0)
            t = lr.hit_thresholds(prim, self.heights(c), c.params, 0)[prim["status"] == lr.HIT]
            return float(np.sort(t)[t.size // 2])
        return self._get(("level", c.name, inside), make)

    def water_of(self, c, inside):
        return self.hmrm.Water.make(self.water_level(c, inside), c.mirror_step, reflectivity=REFLECTIVITY, interior=inside)

    def water(self, c, inside, sampling=0, width=FRAME_W, height=FRAME_H):
        return self._get(("water", c.name, inside, sampling, width, height),
                         lambda: wr.replay(self.rays(c, inside, width, height), self.heights(c), c.cmap, c.params, c.cam_step,
                                           self.water_level(c, inside), c.mirror_step, bg=BG, sampling=sampling, step_cap=BASE_CAP,
                                           reflectivity=REFLECTIVITY, interior=inside, primary=self.primary(c, inside, sampling, width, height)))

    def water_lit(self, c, inside, sampling=0):
        return self._get(("waterlit", c.name, inside, sampling),
                         lambda: wlr.replay(self.rays(c, inside), self.heights(c), c.cmap, c.params, c.cam_step, self.water_level(c, inside),
                                            c.mirror_step, c.sun_dir, c.sun_step, bg=BG, sampling=sampling, step_cap=BASE_CAP,
                                            reflectivity=REFLECTIVITY, ambient=AMBIENT, diffuse=True, shadows=True, interior=inside,
                                            primary=self.primary(c, inside, sampling), wet=self.water(c, inside, sampling)))

    def haze_bounds(self, c, inside):
        """(start, far, own): the 10th and 90th percentile of the camera's nearest-sampled hit ranges where they all are finite
        and not all equal (own = True); else the unit case's bounds times the case's unit -- every hit then sits on one clamp."""
        def make():
            r, hit = self.ranges(c, inside, 0)
            r = r[hit]
            if np.isfinite(r).all() and r.min() > 0.0:
                return float(np.percentile(r, 10)), float(np.percentile(r, 90)), True
            assert c.sweep == "P2"
            start, far, own = self.haze_bounds(unit_case(c.proj), inside)
            assert own
            return start * c.unit, far * c.unit, False
        return self._get(("hazebounds", c.name, inside), make)

    def haze_of(self, c, inside, sky=False):
        start, far, _own = self.haze_bounds(c, inside)
        with np.errstate(all="ignore"):
            scale = float(np.float64(HAZE_ENTRIES) / (np.float64(far) - np.float64(start)))
        return self.hmrm.Haze.raw(start, scale, HAZE_ENTRIES, HAZE_COLOR,
                                  (self.hmrm.TRACE_INTERIOR if inside else 0) | (self.hmrm.HAZE_SKY if sky else 0))

    def haze(self, c, inside, sampling=0, sky=False, factor=1):
        def make():
            hz = self.haze_of(c, inside, sky)
            w, h = FRAME_W * factor, FRAME_H * factor
            prim = self.primary(c, inside, sampling, w, h)
            want = hr.frame(prim, self.rays(c, inside, w, h), hz.start, hz.scale, self.table, bytes(hz.color), sky)
            want["plain"] = prim["rgba"]
            return want
        return self._get(("haze", c.name, inside, sampling, sky, factor), make)

    # ---- the compositions ----
    def sum_dirs(self, c):
        """K = 3 directions of hmrm_render_lit_sum: tests/lit_cases.py's suns at the case's sun magnitude."""
        return np.array([[math.ldexp(v, c.sun_pow) for v in s] for s in lit_cases.SUNS], dtype=np.float64)

    def lit_sum(self, c, inside, sampling=0):
        """tests/lit_sum_cases.py's composition, HMRM_SHADE_DIFFUSE with shadows -> dict: rgba, light."""
        def make():
            prim = self.primary(c, inside, sampling)
            hit = prim["status"] == lr.HIT
            dirs = self.sum_dirs(c)
            s = np.zeros(prim.shape[0], dtype=np.int64)
            capped = 0
            for d in dirs:
                one = shr.replay(self.rays(c, inside), self.heights(c), c.cmap, c.params, c.cam_step, tuple(d.tolist()), c.sun_step, bg=BG,
                                 sampling=sampling, step_cap=BASE_CAP, ambient=AMBIENT, interior=inside, diffuse=True, shadows=True, primary=prim)
                s += one["w"]
                capped += one["capped"]
            return dict(rgba=lsc.apply(prim["rgba"], hit, s, dirs.shape[0]), light=lsc.light_plane(hit, s), capped=capped)
        return self._get(("litsum", c.name, inside, sampling), make)

    def baked_plane(self, c, sampling=0):
        """What hmrm_scene_bake_light leaves for one direction with WEIGHT | DIFFUSE: the cell map's bytes, full scale 255."""
        return self._get(("bakedplane", c.name, sampling), lambda: self.cell_weight(c, False, sampling).astype(np.uint16))

    def baked(self, c, inside, sampling=0, factor=1):
        def make():
            prim = self.primary(c, inside, sampling, FRAME_W * factor, FRAME_H * factor)
            hit = prim["status"] == lr.HIT
            light = bkc.light_of(prim, self.baked_plane(c, sampling), c.params, sampling)
            return dict(rgba=bkc.apply(prim["rgba"], hit, light, 255), L=light, hit=hit)
        return self._get(("baked", c.name, inside, sampling, factor), make)

    def view_cameras(self, c):
        """The case's outside and inside camera and the outside one turned by 25 degrees."""
        third = c.camera(False)
        third.hang += self.hmrm.degrees_to_rads(25.0)
        return [c.camera(False), c.camera(True), third]

    def views(self, c):
        """The frames of view_cameras under the interior rule -> (3, n, 4) uint8."""
        def make():
            out = []
            for cam in self.view_cameras(c):
                rays = ray_replay.camera_rays(self.oracle, self.oracle.make_cfg(cam, c.params, MAP_W, MAP_H))
                rec = sr.replay(rays, self.heights(c), c.cmap, c.params, c.cam_step, bg=BG, step_cap=BASE_CAP, interior=True)
                assert (rec["status"] != sr.CAPPED).all()
                out.append(rec["rgba"])
            return np.stack(out)
        return self._get(("views", c.name), make)


# ---- counts the conditions are written in ----
def hit_counts(prim):
    """(hits, non-hits, capped)"""
    s = prim["status"]
    return int((s == lr.HIT).sum()), int((s != lr.HIT).sum()), int((s == lr.CAPPED).sum())


def lit_counts(want):
    """(shadowed hit pixels, unshadowed hit pixels, capped rays)"""
    hit = want["primary"]["status"] == lr.HIT
    return int(want["shadowed"].sum()), int((hit & ~want["shadowed"]).sum()), want["capped"]


def level_count(want):
    """Distinct diffuse levels among the hits."""
    hit = want["primary"]["status"] == lr.HIT
    return int(np.unique(want["q"][hit]).size)


def water_counts(want):
    """(wet pixels, dry hits, mirror rays that hit, capped rays)"""
    hit = want["primary"]["status"] == lr.HIT
    return int(want["water"].sum()), int((hit & ~want["water"]).sum()), int((want["mirror"]["status"] == wr.HIT).sum()), want["capped"]


def float_classes(plane, hit):
    """(zeros, denormals, normals, infinities) among the hits of a float32 plane."""
    v = np.ascontiguousarray(plane, dtype=np.float32).reshape(-1)[hit.reshape(-1)]
    tiny = float(np.finfo(np.float32).tiny)
    a = np.abs(v.astype(np.float64))
    return int((a == 0.0).sum()), int(((a > 0.0) & (a < tiny)).sum()), int(((a >= tiny) & np.isfinite(a)).sum()), int(np.isinf(a).sum())
