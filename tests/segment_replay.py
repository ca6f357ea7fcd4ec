"""tests/ray_replay.replay plus the two segment rules of hmrm_trace_segments / hmrm_render_interior (include/hmrm.h), in numpy.

INTERIOR RULE: a ray whose origin lies strictly inside the box (all six comparisons true, NaN fails them) runs the body of
hmap.cpp:989-1057 as if distance() had returned +0.0; every other ray is untouched; entry_d stays distance()'s own value.
STEP LIMIT: ray i has L_i = the smaller of the non-zero values among max_steps and per_ray[i] (0 = none) and a budget
min(step_cap, L_i); per trip: the range test (hmap.cpp:1006), then the budget, then the load.  Running out of budget inside
the grid is END (3) when L_i != 0 and L_i < step_cap, else CAPPED (2).

With the rules off (interior=False, max_steps=0, per_ray=None) the records are ray_replay.replay's, byte for byte
(tests/test_segments_cpu.py), and the interior rule is pinned there to the unchanged C oracle."""
import numpy as np

import ray_replay
from ray_replay import RAY_HIT_DTYPE, MISS, HIT, CAPPED, _bil, _mix, box, distance, miss_shade  # noqa: F401

END = 3


def strictly_inside(o, c0, c1):
    with np.errstate(all="ignore"):
        return ((c0[0] < o[:, 0]) & (o[:, 0] < c1[0]) & (c1[1] < o[:, 1]) & (o[:, 1] < c0[1]) &
                (c0[2] < o[:, 2]) & (o[:, 2] < c1[2]))


def limits(n, max_steps=0, per_ray=None):
    """L_i: the smaller of the non-zero values among max_steps and per_ray[i]; 0 = none."""
    own = np.zeros(n, dtype=np.int64) if per_ray is None else np.asarray(per_ray, dtype=np.int64).reshape(n)
    u = np.full(n, int(max_steps), dtype=np.int64)
    return np.where(u == 0, own, np.where(own == 0, u, np.minimum(u, own)))


def replay(rays, heights, cmap, params, step_dist, bg=(0, 0, 0), sampling=0, step_cap=1 << 26, interior=False, max_steps=0,
           per_ray=None):
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    n = rays.shape[0]
    o, d = rays[:, 0:3], rays[:, 3:6]
    mh, mw = heights.shape
    gw = params.grid_width
    c0, c1 = box(params, mw, mh)
    out = np.zeros(n, dtype=RAY_HIT_DTYPE)
    out["cell_x"] = -1
    out["cell_y"] = -1
    lim = limits(n, max_steps, per_ray)
    ends = (lim != 0) & (lim < step_cap)
    budget = np.where(ends, lim, step_cap)
    with np.errstate(all="ignore"):
        dist = distance(o, d, c0, c1)
        enters = ~((dist == np.inf) | (dist < 0.0))  # intersection(), AABB.cpp:33-44
        dd = np.where(enters, dist, 0.0)
        if interior:
            inside = strictly_inside(o, c0, c1)
            enters = enters | inside
            dd = np.where(inside, 0.0, dd)  # as if distance() had returned +0.0
        nudge = gw * 0.01
        x = (o[:, 0] + dd * d[:, 0]) + nudge * d[:, 0]
        y = (o[:, 1] + dd * d[:, 1]) + nudge * d[:, 1]
        z = (o[:, 2] + dd * d[:, 2]) + nudge * d[:, 2]
        sx, sy, sz = step_dist * d[:, 0], step_dist * d[:, 1], step_dist * d[:, 2]
        thr = heights.reshape(-1) + c0[2]  # heightmap_z + hmap_c0.z, hmap.cpp:1016
        if sampling == 2:
            thr = thr.astype(np.float32).astype(np.float64)
        flat_c = cmap.reshape(-1, 4)
        bgpx = np.array([bg[0], bg[1], bg[2], 255], dtype=np.uint8)
        steps = np.zeros(n, dtype=np.int64)
        status = np.zeros(n, dtype=np.uint32)
        rgba = np.zeros((n, 4), dtype=np.uint8)
        active = enters.copy()
        while active.any():
            qx = (x - c0[0]) / gw
            qy = -(y - c0[1]) / gw
            active &= (qx > -1.0) & (qx < mw) & (qy > -1.0) & (qy < mh)  # the range test first
            spent = active & (steps >= budget)  # then the budget
            status[spent] = np.where(ends[spent], END, CAPPED)
            active &= ~spent
            idx = np.nonzero(active)[0]
            if idx.size == 0:
                break
            gx = qx[idx].astype(np.int64)
            gy = qy[idx].astype(np.int64)
            cell = gx + gy * mw
            steps[idx] += 1  # then the load
            if sampling == 1:
                (c00, c10, c01, c11), tx, ty = _bil(qx[idx], qy[idx], mw, mh)
                t = _mix(tx, ty, thr[c00], thr[c10], thr[c01], thr[c11])
            else:
                t = thr[cell]
            now = z[idx] < t
            if now.any():
                h = idx[now]
                texel = flat_c[cell[now]]
                col = texel.copy()
                if sampling == 1:
                    for k in range(3):
                        f = _mix(tx[now], ty[now], flat_c[c00[now], k].astype(np.float64), flat_c[c10[now], k].astype(np.float64),
                                 flat_c[c01[now], k].astype(np.float64), flat_c[c11[now], k].astype(np.float64))
                        col[:, k] = np.floor(np.clip(f + 0.5, 0.0, 255.0)).astype(np.uint8)
                col = np.where(texel[:, 3:4] == 0, bgpx[None, :], col)  # hmap.cpp:1020
                col[:, 3] = 255
                rgba[h] = col
                status[h] = HIT
                out["point"][h, 0] = x[h]
                out["point"][h, 1] = y[h]
                out["point"][h, 2] = z[h]
                out["cell_x"][h] = gx[now]
                out["cell_y"][h] = gy[now]
                active[h] = False
            x = np.where(active, x + sx, x)
            y = np.where(active, y + sy, y)
            z = np.where(active, z + sz, z)
        miss = status != HIT
        rgba[miss] = miss_shade(d[:, 2], bg)[miss]
    out["entry_d"] = dist
    out["steps"] = steps.astype(np.uint32)
    out["rgba"] = rgba
    out["status"] = status
    return out


def scalar_ray(ray, heights, cmap, params, step_dist, bg, step_cap, interior, limit):
    """One ray at a time in plain Python floats, nearest sampling: the cross-check of the vectorised replay above.
    -> (status, steps, point, cell, rgba, entry_d)"""
    import math
    px, py, pz, dx, dy, dz = (float(v) for v in ray)
    mh, mw = heights.shape
    gw = float(params.grid_width)
    c0 = (0.0, 0.0, float(params.min_height))
    c1 = (0.0 + mw * gw, 0.0 - mh * gw, float(params.max_height))
    inf = math.inf

    def div(a, b):
        if b != 0.0:
            return a / b
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(inf, a) * math.copysign(1.0, b)

    lo, hi, dist = -inf, inf, None
    for i, (oo, ddv) in enumerate(((px, dx), (py, dy), (pz, dz))):
        dl, dh = div(c0[i] - oo, ddv), div(c1[i] - oo, ddv)
        if dl > dh:
            dl, dh = dh, dl
        if dh < lo or dl > hi:
            dist = inf
            break
        if dl > lo:
            lo = dl
        if dh < hi:
            hi = dh
    if dist is None:
        dist = inf if lo > hi else lo
    enters = not (dist == inf or dist < 0.0)
    d_used = dist
    if interior and c0[0] < px < c1[0] and c1[1] < py < c0[1] and c0[2] < pz < c1[2]:
        enters, d_used = True, 0.0

    def mul(a, b):  # IEEE: 0 * inf = NaN (Python floats do that already)
        return a * b

    status, steps, point, cell = MISS, 0, (0.0, 0.0, 0.0), (-1, -1)
    rgba = None
    if enters:
        nudge = gw * 0.01
        x = (px + mul(d_used, dx)) + mul(nudge, dx)
        y = (py + mul(d_used, dy)) + mul(nudge, dy)
        z = (pz + mul(d_used, dz)) + mul(nudge, dz)
        sx, sy, sz = mul(step_dist, dx), mul(step_dist, dy), mul(step_dist, dz)
        ends = limit != 0 and limit < step_cap
        budget = limit if ends else step_cap
        while True:
            qx, qy = (x - c0[0]) / gw, -(y - c0[1]) / gw
            if not (qx > -1.0 and qx < mw and qy > -1.0 and qy < mh):
                break
            if steps >= budget:
                status = END if ends else CAPPED
                break
            gx, gy = int(qx), int(qy)
            steps += 1
            if z < float(heights[gy, gx]) + c0[2]:
                status, point, cell = HIT, (x, y, z), (gx, gy)
                t = cmap[gy, gx]
                rgba = (bg[0], bg[1], bg[2], 255) if t[3] == 0 else (int(t[0]), int(t[1]), int(t[2]), 255)
                break
            x, y, z = x + sx, y + sy, z + sz
    if rgba is None:
        rgba = tuple(int(v) for v in miss_shade(np.array([dz]), bg)[0])
    return status, steps, point, cell, rgba, dist
