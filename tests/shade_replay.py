"""hmrm_render_shaded (include/hmrm.h) in numpy, on top of tests/lit_replay.py: the primary records and, unless
HMRM_SHADE_NO_SHADOWS, the shadow rays are lit_replay's; every hit pixel then gets a weight w -- the ambient level when it is
shadowed, 255 without HMRM_SHADE_DIFFUSE, else ambient + ((255 - ambient) * q + 127) // 255 with q the diffuse level of the
hit -- and keeps (c * w + 127) // 255 of R, G and B.  numpy's float64 ufuncs are plain IEEE operations (no contraction) and
np.sqrt is correctly rounded, so `levels` is the header's arithmetic operation for operation."""
import numpy as np

import lit_replay as lr
import ray_replay
import segment_replay as sr
from ray_replay import _bil, box

HIT = lr.HIT
DIFFUSE, NO_SHADOWS = 1, 2


def table(heights, params, sampling):
    """T: heightmap_buf + min_height, through float for HMRM_NEAREST_F32 (flat, row-major)."""
    mh, mw = heights.shape
    c0, _c1 = box(params, mw, mh)
    thr = heights.reshape(-1) + c0[2]
    if sampling == 2:
        thr = thr.astype(np.float32).astype(np.float64)
    return thr


def gradients(primary, heights, params, sampling):
    """(gx, gy) of every record (0 where the ray did not hit)."""
    mh, mw = heights.shape
    c0, _c1 = box(params, mw, mh)
    gw = params.grid_width
    thr = table(heights, params, sampling)
    hit = primary["status"] == HIT
    with np.errstate(all="ignore"):
        if sampling == 1:
            qx = np.where(hit, (primary["point"][:, 0] - c0[0]) / gw, 0.0)
            qy = np.where(hit, -(primary["point"][:, 1] - c0[1]) / gw, 0.0)
            (c00, c10, c01, c11), tx, ty = _bil(qx, qy, mw, mh)
            a, b = thr[c10] - thr[c00], thr[c11] - thr[c01]
            gx = (a + ty * (b - a)) / gw
            c, d = thr[c01] - thr[c00], thr[c11] - thr[c10]
            gy = (c + tx * (d - c)) / gw
        else:
            cx = np.where(hit, primary["cell_x"].astype(np.int64), 0)
            cy = np.where(hit, primary["cell_y"].astype(np.int64), 0)
            xm, xp = np.maximum(cx - 1, 0), np.minimum(cx + 1, mw - 1)
            ym, yp = np.maximum(cy - 1, 0), np.minimum(cy + 1, mh - 1)
            gx = np.where(xp > xm, (thr[xp + cy * mw] - thr[xm + cy * mw]) / ((xp - xm).astype(np.float64) * gw), 0.0)
            gy = np.where(yp > ym, (thr[cx + yp * mw] - thr[cx + ym * mw]) / ((yp - ym).astype(np.float64) * gw), 0.0)
    return np.where(hit, gx, 0.0), np.where(hit, gy, 0.0)


def levels_of(gx, gy, sun_dir):
    """q of the gradients under the sun direction as given."""
    s = np.asarray(sun_dir, dtype=np.float64)
    with np.errstate(all="ignore"):
        nx, ny = -gx, gy
        dot = (nx * s[0] + ny * s[1]) + s[2]
        length = np.sqrt(((nx * nx + ny * ny) + 1.0) * ((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]))
        k = dot / length
        k = np.where(k > 0.0, np.where(k < 1.0, k, 1.0), 0.0)
        return (k * 255.0 + 0.5).astype(np.uint32)


def levels(primary, heights, params, sampling, sun_dir):
    """q in 0..255 of every record (junk where the ray did not hit)."""
    gx, gy = gradients(primary, heights, params, sampling)
    return levels_of(gx, gy, sun_dir)


def weights(primary, heights, params, sampling, sun_dir, ambient, diffuse, shadowed):
    """w of every record that hit (255 elsewhere: such pixels are untouched)."""
    n = primary.shape[0]
    hit = primary["status"] == HIT
    amb = int(ambient)
    w = np.full(n, 255, dtype=np.int64)
    if diffuse:
        q = levels(primary, heights, params, sampling, sun_dir).astype(np.int64)
        w = amb + ((255 - amb) * q + 127) // 255
    w = np.where(shadowed, amb, w)
    return np.where(hit, w, 255)


def apply(rgba, w):
    out = rgba.copy()
    out[:, 0:3] = ((rgba[:, 0:3].astype(np.int64) * w[:, None] + 127) // 255).astype(np.uint8)
    return out


def replay(rays, heights, cmap, params, step_dist, sun_dir, sun_step_dist, bg=(0, 0, 0), sampling=0, step_cap=1 << 26,
           max_steps=0, ambient=128, interior=False, diffuse=True, shadows=True, primary=None, lit=None):
    """lit: lit_replay.replay's dict of the same arguments when the caller has it (used when `shadows`); primary: the primary
    records alone.  -> dict: rgba, primary, shadowed, w, q, capped."""
    if shadows:
        if lit is None:
            lit = lr.replay(rays, heights, cmap, params, step_dist, sun_dir, sun_step_dist, bg=bg, sampling=sampling,
                            step_cap=step_cap, max_steps=max_steps, ambient=ambient, interior=interior, primary=primary)
        primary, shadowed, capped = lit["primary"], lit["shadowed"], lit["capped"]
    else:
        if primary is None and lit is not None:
            primary = lit["primary"]
        if primary is None:
            if interior:
                primary = sr.replay(rays, heights, cmap, params, step_dist, bg=bg, sampling=sampling, step_cap=step_cap, interior=True)
            else:
                primary = ray_replay.replay(rays, heights, cmap, params, step_dist, bg=bg, sampling=sampling, step_cap=step_cap)
        shadowed = np.zeros(primary.shape[0], dtype=bool)
        capped = int((primary["status"] == lr.CAPPED).sum())
    w = weights(primary, heights, params, sampling, sun_dir, ambient, diffuse, shadowed)
    q = levels(primary, heights, params, sampling, sun_dir)
    return dict(rgba=apply(primary["rgba"], w), primary=primary, shadowed=shadowed, w=w, q=q, capped=capped)
