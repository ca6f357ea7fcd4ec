"""hmrm_cell_map (include/hmrm.h) in numpy: the ray of every cell built exactly as the header writes it, its status from
tests/segment_replay.py (interior rule on, the struct's step limit), the diffuse level from tests/shade_replay.py's table,
gradients and levels_of -- fed one record per cell that says HIT in the cell itself at the ray's origin, and, in point mode,
the per-cell direction as arrays.  numpy's float64 ufuncs are plain IEEE operations, no contraction."""
import numpy as np

import segment_replay as sr
import shade_replay as shr
from ray_replay import RAY_HIT_DTYPE

MISS, HIT, CAPPED, END = sr.MISS, sr.HIT, sr.CAPPED, sr.END
TOWARDS_POINT, WEIGHT, DIFFUSE, NO_SHADOWS = 1, 2, 4, 8  # HMRM_MAP_*


def cell_rays(heights, params, sampling, target, lift=0.0, point=False):
    """(W * H, 6) rays, row-major over the map's cells, and the cell coordinates (cx, cy)."""
    mh, mw = heights.shape
    gw = float(params.grid_width)
    T = shr.table(heights, params, sampling)
    cy, cx = (a.reshape(-1) for a in np.mgrid[0:mh, 0:mw])
    tx, ty, tz = (np.float64(v) for v in target)
    with np.errstate(all="ignore"):
        pos_x = (cx.astype(np.float64) + 0.5) * gw
        pos_y = -((cy.astype(np.float64) + 0.5) * gw)
        pos_z = T + np.float64(lift)
        if point:
            d = (tx - pos_x, ty - pos_y, tz - pos_z)
        else:
            d = (np.full(cx.size, tx), np.full(cx.size, ty), np.full(cx.size, tz))
    return np.ascontiguousarray(np.stack([pos_x, pos_y, pos_z, d[0], d[1], d[2]], axis=1)), cx, cy


def statuses(heights, cmap, params, sampling, target, step_dist, lift=0.0, max_steps=0, point=False, step_cap=1 << 26):
    """(H, W) uint8: the status of every cell's ray."""
    rays, _cx, _cy = cell_rays(heights, params, sampling, target, lift, point)
    rec = sr.replay(rays, heights, cmap, params, step_dist, sampling=sampling, step_cap=step_cap, interior=True, max_steps=max_steps)
    return rec["status"].astype(np.uint8).reshape(heights.shape)


def levels(heights, params, sampling, target, lift=0.0, point=False):
    """(H, W): q of every cell under its own direction."""
    rays, cx, cy = cell_rays(heights, params, sampling, target, lift, point)
    rec = np.zeros(rays.shape[0], dtype=RAY_HIT_DTYPE)
    rec["status"] = HIT
    rec["cell_x"], rec["cell_y"] = cx, cy
    rec["point"] = rays[:, 0:3]
    gx, gy = shr.gradients(rec, heights, params, sampling)
    return shr.levels_of(gx, gy, (rays[:, 3], rays[:, 4], rays[:, 5])).reshape(heights.shape)


def weights(shape, status, q, flags, ambient):
    """(H, W) uint8: w from the statuses (not looked at with NO_SHADOWS) and the levels (not looked at without DIFFUSE)."""
    amb = int(ambient)
    w = np.full(shape, 255, dtype=np.int64)
    if flags & DIFFUSE:
        w = amb + ((255 - amb) * q.astype(np.int64) + 127) // 255
    if not flags & NO_SHADOWS:
        w = np.where(status == HIT, amb, w)
    return w.astype(np.uint8)


def replay(heights, cmap, params, target, step_dist, lift=0.0, max_steps=0, flags=0, sampling=0, ambient=128, step_cap=1 << 26,
           status=None):
    """-> (H, W) uint8, the bytes of the whole map's hmrm_cell_map.  status: statuses() of the same arguments, if the caller has it."""
    point = bool(flags & TOWARDS_POINT)
    if status is None and not flags & NO_SHADOWS:
        status = statuses(heights, cmap, params, sampling, target, step_dist, lift, max_steps, point, step_cap)
    if not flags & WEIGHT:
        return status
    q = levels(heights, params, sampling, target, lift, point) if flags & DIFFUSE else None
    return weights(heights.shape, status, q, flags, ambient)
