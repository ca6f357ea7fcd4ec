"""World-scale cases: one scene family per way the MAGNITUDE of a world's numbers can differ from the unit-scale
scenes of scenes.py (grid_width 0.01..3, heights below 1e3, camera a few map extents away).  Plain module, not
collected; deterministic, no GPU.  tests/test_world_scale_cpu.py checks the conditions every case must meet on the
oracle (no capped ray, a quarter of the rays march, 40 colours), tests/test_world_scale_gpu.py renders them.

Every case is (name, family, rgb, cmap, SceneParams, Camera, exempt); frames are 64x48 (the hazards are per-ray
arithmetic, not frame size), every family comes in all three projections.

Base pose: the camera looks at the centre (96, -80, 5) of small_maps(192, 160, 78) from D = 300 away, hang -48 deg,
30 deg below the horizon (vang 120), hfov = 2 atan(0.75 * 192 / D) (the map about fills the frame's width), heights
0..24, grid_width 1, step_dist 0.25; the orthographic pixel is 2 * 0.75 * 192 / 64 = 4.5 wide, the same footprint.

Families
  P2      every length of the base times 2^k (exact: the reference's loop is scale-invariant under powers of two
          while nothing over- or underflows, so frame and steps must equal k = 0's and distance() must be 2^k times it).
  DEC     the same, times a power of ten: fl(1/grid_width) is inexact, products round differently at every scale
          (all nine scales in perspective too: at 1e9 and 1e12 the image plane is coarsely quantised by cam_pos + look).
  GW      grid widths at and next to the kernel's specialisations (1, a power of two, anything else) at five
          exponents: 2^e, its two neighbours, 3 * 2^(e-2) and 2^e / 3.  Heights and step_dist are scaled by 2^e; the
          camera looks at the centre of the map as that grid width makes it, from 300 grid widths away.
  FAR     telephoto: the base seen from D = 1e4 .. 1e10 with the field of view that keeps the map in frame.
  OFFSET  relief of 12 on top of an absolute height of 1e3, 1e6, 1e9 (float spacing at 1e9: 64), and mirrored
          below zero with min_height = -H.
  RATIO   step_dist / grid_width from 1e-3 to 1e3 and max_height / grid_width 1e-4 and 1e4.
"""
import math

import numpy as np

import scenes

hmrm = scenes.hmrm
DEG = hmrm.degrees_to_rads

FRAME_W, FRAME_H = 64, 48
MAP_W, MAP_H, MAP_SEED = 192, 160, 78
PROJECTIONS = ((1, "persp"), (2, "sph"), (3, "ortho"))
FAMILIES = ("P2", "DEC", "GW", "FAR", "OFFSET", "RATIO")

HANG, VANG = DEG(-48.0), DEG(120.0)
BASE_D = 300.0
P2_K = (-900, -510, -490, -300, -60, -24, -1, 0, 1, 24, 60, 300, 490, 510, 900)
P2_PERSP_MAX_K = 24      # beyond, cam_pos + look loses the unit `look` (gone entirely from 2^53 on)
P2_PERSP_EXEMPT_K = 60   # ... and this one is kept, marked exempt: every direction NaN, every pixel background
DEC_S = (1e-12, 1e-9, 1e-6, 1e-3, 30.0, 1e3, 1e6, 1e9, 1e12)
GW_E = (-40, -10, 0, 10, 40)
FAR_D = (1e4, 1e6, 1e8, 1e10)
FAR_PERSP_MAX_D = 1e8
OFFSET_H = (1e3, 1e6, 1e9)
RATIO_STEP = (1e-3, 1e-2, 30.0, 1e3)
RATIO_HEIGHT = (1e-4, 1e4)

_maps = {}


def maps(w=MAP_W, h=MAP_H):
    if (w, h) not in _maps:
        _maps[(w, h)] = scenes.small_maps(w, h, MAP_SEED)
    return _maps[(w, h)]


def look_dir(hang, vang):
    return np.array([math.sin(vang) * math.cos(hang), math.sin(vang) * math.sin(hang), math.cos(vang)])


def hfov_for(half_width, dist):
    return 2.0 * math.atan(half_width / dist)


def _camera(proj, target, dist, half_width, step_dist, scale=1.0, hang=HANG, vang=VANG, bg=(12, 34, 56)):
    """Looks at `target` from `dist` away; `half_width` is half the footprint of the frame's width at the target.
    Every length is then multiplied by `scale`."""
    look = look_dir(hang, vang)
    if proj == 3:
        look = look.astype(np.float32).astype(np.float64)  # the orthographic rays' direction (a float round trip): from
        # 1e10 away the difference moves the footprint by a hundred cells
    pos = np.asarray(target, dtype=np.float64) - dist * look
    return hmrm.Camera.make(width=FRAME_W, height=FRAME_H, projection=proj, hfov=hfov_for(half_width, dist), hang=hang,
                            vang=vang, pos=tuple(float(v) * scale for v in pos),
                            ortho_width=2.0 * half_width / FRAME_W * scale, step_dist=step_dist * scale, bg=bg)


def _scaled(proj, s):
    """The base scene with every length times s."""
    params = hmrm.SceneParams.make(0.0, 24.0 * s, grid_width=1.0 * s)
    return params, _camera(proj, (96.0, -80.0, 5.0), BASE_D, 0.75 * MAP_W, 0.25, scale=s)


def _tag(v):
    return ("%g" % v).replace("+", "").replace("-", "m").replace(".", "p")


def _p2(out):
    rgb, cmap = maps()
    for proj, pname in PROJECTIONS:
        for k in P2_K:
            exempt = proj == 1 and k == P2_PERSP_EXEMPT_K
            if proj == 1 and k > P2_PERSP_MAX_K and not exempt:
                continue
            params, cam = _scaled(proj, math.ldexp(1.0, k))
            out.append((f"P2_{pname}_k{_tag(k)}", "P2", rgb, cmap, params, cam, exempt))


def _dec(out):
    rgb, cmap = maps()
    for proj, pname in PROJECTIONS:
        for s in DEC_S:
            # (perspective too: at 1e9 and 1e12 cam_pos + look quantises the image plane coarsely, a hazard of its own --
            # 1e12 keeps 523 of the base's 932 colours -- and the frames still meet every condition)
            params, cam = _scaled(proj, s)
            out.append((f"DEC_{pname}_s{_tag(s)}", "DEC", rgb, cmap, params, cam, False))


def gw_members(e):
    p = math.ldexp(1.0, e)
    return (("pow2", p), ("below", float(np.nextafter(p, 0.0))), ("above", float(np.nextafter(p, np.inf))),
            ("x0p75", 3.0 * math.ldexp(1.0, e - 2)), ("third", p / 3.0))


def _gw(out):
    rgb, cmap = maps()
    for proj, pname in PROJECTIONS:
        for e in GW_E:
            s = math.ldexp(1.0, e)
            for gname, gw in gw_members(e):
                r = gw / s  # (1, 1 -+ an ulp, 0.75, 1/3)
                params = hmrm.SceneParams.make(0.0, 24.0 * s, grid_width=gw)
                cam = _camera(proj, (96.0 * r, -80.0 * r, 5.0), BASE_D * r, 0.75 * MAP_W * r, 0.25, scale=s)
                out.append((f"GW_{pname}_e{_tag(e)}_{gname}", "GW", rgb, cmap, params, cam, False))


def _far(out):
    rgb, cmap = maps()
    params = hmrm.SceneParams.make(0.0, 24.0, grid_width=1.0)
    for proj, pname in PROJECTIONS:
        for d in FAR_D:
            if proj == 1 and d > FAR_PERSP_MAX_D:
                continue
            cam = _camera(proj, (96.0, -80.0, 5.0), d, 0.75 * MAP_W, 0.25)
            out.append((f"FAR_{pname}_d{_tag(d)}", "FAR", rgb, cmap, params, cam, False))


def offset_scene(h, mirrored):
    """Heights h + [0, 12] from a height image whose blue channel is 128 and whose red channel keeps the map:
    value = eps * red + 128, heightmap = value / 255 * (max - min) + min, threshold = heightmap + min (the reference
    adds min_height twice).  Plain: min 0, max = h * 255 / 128, so value 128 is height h and eps * 255 spans 12.
    Mirrored: min = -h, max = +h: thresholds 128 / 255 * 2h - 2h = -0.996 h, inside the box [-h, h], relief 12 again.
    -> (rgb, cmap, params, lowest threshold, highest threshold)"""
    rgb, cmap = maps()
    rgb = rgb.copy()
    rgb[:, :, 2] = 128
    if mirrored:
        lo, hi = -h, h
    else:
        lo, hi = 0.0, h * 255.0 / 128.0
    eps = 12.0 / (hi - lo)
    params = hmrm.SceneParams.make(lo, hi, lum=(eps, 0.0, 1.0), grid_width=1.0)
    base = 128.0 / 255.0 * (hi - lo) + 2.0 * lo
    return rgb, cmap, params, base, base + 12.0


def _offset(out):
    for mirrored in (False, True):
        for h in OFFSET_H:
            rgb, cmap, params, base, top = offset_scene(h, mirrored)
            for proj, pname in PROJECTIONS:
                cam = hmrm.Camera.make(width=FRAME_W, height=FRAME_H, projection=proj, hfov=DEG(150.0 if proj == 2 else 80.0),
                                       hang=HANG, vang=DEG(117.0), pos=(-30.0, 40.0, top + 70.0), ortho_width=3.0,
                                       step_dist=0.25, bg=(12, 34, 56))
                out.append((f"OFFSET_{pname}_{'neg' if mirrored else 'pos'}{_tag(h)}", "OFFSET", rgb, cmap, params, cam, False))


def _ratio(out):
    for proj, pname in PROJECTIONS:
        for ratio in RATIO_STEP:
            if ratio < 1.0:
                # many steps per cell: a 48x40 map keeps a ray below 30 000 steps
                mw, mh = 48, 40
                rgb, cmap = maps(mw, mh)
                params = hmrm.SceneParams.make(0.0, 6.0, grid_width=1.0)
                cam = _camera(proj, (mw / 2.0, -mh / 2.0, 1.25), 75.0, 0.75 * mw, ratio)
            else:
                # a step is many cells: a ray samples the terrain once or a few times.  Seen from low and level, the
                # rays enter through the box's sides, where the first sample already is below the border cells' tops
                rgb, cmap = maps()
                params = hmrm.SceneParams.make(0.0, 24.0, grid_width=1.0)
                # (30 cells a step: the map's 250-cell diagonal allows at most 8 samples; aimed just below the box's top, a
                # fifth of the rays skims the terrain for 4 to 8 of them before it hits or leaves.  1000 cells: one sample.)
                cam = _camera(proj, (96.0, -80.0, 22.0 if ratio == 30.0 else 12.0), BASE_D, 48.0, ratio, vang=DEG(93.0))
            out.append((f"RATIO_{pname}_step{_tag(ratio)}", "RATIO", rgb, cmap, params, cam, False))
        rgb, cmap = maps()
        # a slab 1e-4 grid widths thick: every entering ray is below it after the entry nudge and hits at once
        params = hmrm.SceneParams.make(0.0, 1e-4, grid_width=1.0)
        cam = _camera(proj, (96.0, -80.0, 0.0), BASE_D, 0.6 * MAP_W, 0.25)
        out.append((f"RATIO_{pname}_height1em04", "RATIO", rgb, cmap, params, cam, False))
        # a tower 1e4 grid widths tall, seen from beside it at 6/10 of its height: every ray enters through its sides
        params = hmrm.SceneParams.make(0.0, 1e4, grid_width=1.0)
        cam = _camera(proj, (96.0, -80.0, 6000.0), BASE_D, 0.75 * MAP_W, 0.25)
        out.append((f"RATIO_{pname}_height1e04", "RATIO", rgb, cmap, params, cam, False))


_cases = None


def cases():
    """-> list of (name, family, rgb, cmap, SceneParams, Camera, exempt); the arrays are shared: do not write to them."""
    global _cases
    if _cases is None:
        out = []
        for fill in (_p2, _dec, _gw, _far, _offset, _ratio):
            fill(out)
        assert len({c[0] for c in out}) == len(out)
        _cases = out
    return _cases


def family(fam, proj=None):
    return [c for c in cases() if c[1] == fam and (proj is None or c[5].projection == proj)]


def ends_and_middle(members):
    """The two extreme members and the middle member of a sweep (in generation order)."""
    idx = sorted({0, len(members) // 2, len(members) - 1})
    return [members[i] for i in idx]
