"""The reference's per-ray body (main/hmap.cpp:989-1057) for ARBITRARY rays (pos, dir), in numpy, vectorised over the
rays: distance() with its early returns (src/AABB.cpp:49-77), intersection() (:33-44), the nudge (hmap.cpp:998), the
sequential adds (:1037), cell truncation (:1001-1011), the hit tests of the three sampling modes, the colour rules
(:1018-1031) and the sky (:1041-1057).  Adapted from tests/np_marcher.py (which tests/test_oracle.py pins to the C
oracle); tests/test_trace_rays_cpu.py pins THIS file to the oracle on camera rays of every projection and sampling mode,
which is what lets the GPU tests use it for rays no camera can express.  numpy's float64 ufuncs are plain IEEE
operations (no FMA contraction).  Returns records in the layout of hmrm_ray_hit (include/hmrm.h)."""
import numpy as np

RAY_HIT_DTYPE = np.dtype([("point", np.float64, 3), ("entry_d", np.float64), ("steps", np.uint32),
                          ("cell_x", np.int32), ("cell_y", np.int32), ("rgba", np.uint8, 4),
                          ("status", np.uint32), ("reserved", np.uint32)])
MISS, HIT, CAPPED = 0, 1, 2


def box(params, map_w, map_h):
    """hmap.cpp:968-974"""
    gw = params.grid_width
    c0 = np.array([0.0, 0.0, params.min_height], dtype=np.float64)
    c1 = np.array([c0[0] + map_w * gw, c0[1] - map_h * gw, params.max_height], dtype=np.float64)
    return c0, c1


def distance(o, d, c0, c1):
    """AABB.cpp:49-77 for n rays (o, d: n x 3), its early returns as masks."""
    n = o.shape[0]
    lo = np.full(n, -np.inf)
    hi = np.full(n, np.inf)
    dead = np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(3):
            dl = (c0[i] - o[:, i]) / d[:, i]
            dh = (c1[i] - o[:, i]) / d[:, i]
            swap = dl > dh
            dl, dh = np.where(swap, dh, dl), np.where(swap, dl, dh)
            dead |= (~dead) & ((dh < lo) | (dl > hi))
            lo = np.where((~dead) & (dl > lo), dl, lo)
            hi = np.where((~dead) & (dh < hi), dh, hi)
        return np.where(dead | (lo > hi), np.inf, lo)


def _bil(qx, qy, w, h):
    """oracle/hmrm_oracle.c bil_setup"""
    u, v = qx - 0.5, qy - 0.5
    fu, fv = np.floor(u), np.floor(v)
    tx, ty = u - fu, v - fv
    iu, iv = fu.astype(np.int64), fv.astype(np.int64)
    i0, i1 = np.clip(iu, 0, w - 1), np.clip(iu + 1, 0, w - 1)
    j0, j1 = np.clip(iv, 0, h - 1), np.clip(iv + 1, 0, h - 1)
    return (i0 + j0 * w, i1 + j0 * w, i0 + j1 * w, i1 + j1 * w), tx, ty


def _mix(tx, ty, f00, f10, f01, f11):
    a = f00 + tx * (f10 - f00)
    c = f01 + tx * (f11 - f01)
    return a + ty * (c - a)


def miss_shade(dz, bg):
    """hmap.cpp:1041-1057 -> n x 4 uint8"""
    n = dz.shape[0]
    out = np.empty((n, 4), dtype=np.uint8)
    out[:] = np.array([bg[0], bg[1], bg[2], 255], dtype=np.uint8)
    with np.errstate(all="ignore"):
        sky = dz > 0.0
        z = np.where(sky, dz, 0.0)
        chans = (220.0 * (z * z) + float(bg[0]), 240.0 * (z * z) + float(bg[1]), 255.0 * z + float(bg[2]))
        for k, c in enumerate(chans):
            v = np.floor(np.clip(c, 0.0, 255.0)).astype(np.uint8)
            out[sky, k] = v[sky]
    return out


def replay(rays, heights, cmap, params, step_dist, bg=(0, 0, 0), sampling=0, step_cap=1 << 26):
    """rays: n x 6 float64 (pos, dir); heights: HxW float64 heightmap_buf (oracle.update_heightmap); cmap: HxWx4 uint8.
    -> n records (RAY_HIT_DTYPE)."""
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    n = rays.shape[0]
    o, d = rays[:, 0:3], rays[:, 3:6]
    mh, mw = heights.shape
    gw = params.grid_width
    c0, c1 = box(params, mw, mh)
    out = np.zeros(n, dtype=RAY_HIT_DTYPE)
    out["cell_x"] = -1
    out["cell_y"] = -1
    with np.errstate(all="ignore"):
        dist = distance(o, d, c0, c1)
        enters = ~((dist == np.inf) | (dist < 0.0))  # intersection(), AABB.cpp:33-44
        dd = np.where(enters, dist, 0.0)
        nudge = gw * 0.01
        x = (o[:, 0] + dd * d[:, 0]) + nudge * d[:, 0]
        y = (o[:, 1] + dd * d[:, 1]) + nudge * d[:, 1]
        z = (o[:, 2] + dd * d[:, 2]) + nudge * d[:, 2]
        sx, sy, sz = step_dist * d[:, 0], step_dist * d[:, 1], step_dist * d[:, 2]
        flat_h = heights.reshape(-1)
        thr = flat_h + c0[2]  # heightmap_z + hmap_c0.z, hmap.cpp:1016
        if sampling == 2:
            thr = thr.astype(np.float32).astype(np.float64)
        flat_c = cmap.reshape(-1, 4)
        bgpx = np.array([bg[0], bg[1], bg[2], 255], dtype=np.uint8)
        steps = np.zeros(n, dtype=np.int64)
        status = np.zeros(n, dtype=np.uint32)
        rgba = np.zeros((n, 4), dtype=np.uint8)
        active = enters.copy()
        it = 0
        while active.any():
            qx = (x - c0[0]) / gw
            qy = -(y - c0[1]) / gw
            # (int)q in [0, W)  <=>  -1 < q < W  (truncation toward zero; NaN and out-of-range give INT_MIN: outside)
            active &= (qx > -1.0) & (qx < mw) & (qy > -1.0) & (qy < mh)
            if it >= step_cap:
                status[active] = CAPPED
                break
            idx = np.nonzero(active)[0]
            if idx.size == 0:
                break
            gx = qx[idx].astype(np.int64)
            gy = qy[idx].astype(np.int64)
            cell = gx + gy * mw
            steps[idx] += 1
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
            it += 1
        miss = status != HIT
        rgba[miss] = miss_shade(d[:, 2], bg)[miss]
    out["entry_d"] = dist
    out["steps"] = steps.astype(np.uint32)
    out["rgba"] = rgba
    out["status"] = status
    return out


def hit_points(rays, entry_d, steps, params, step_dist):
    """Where a ray that hits with its `steps`-th load stands then: the entry point, the nudge and steps - 1 sequential
    adds (hmap.cpp:996-998, :1037) -> (points n x 3, gridx, gridy of hmap.cpp:1001-1004).  Rows with steps == 0 are junk."""
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    o, d = rays[:, 0:3], rays[:, 3:6]
    gw = params.grid_width
    steps = np.asarray(steps, dtype=np.int64)
    with np.errstate(all="ignore"):
        dd = np.where(np.isfinite(entry_d), entry_d, 0.0)
        p = (o + dd[:, None] * d) + (gw * 0.01) * d
        s = step_dist * d
        for k in range(1, int(steps.max()) if steps.size else 0):
            p = np.where((steps > k)[:, None], p + s, p)
        qx = np.where(steps > 0, (p[:, 0] - 0.0) / gw, 0.0)
        qy = np.where(steps > 0, -(p[:, 1] - 0.0) / gw, 0.0)
        gx = np.where(np.isfinite(qx) & (np.abs(qx) < 2.0 ** 31), qx, 0.0).astype(np.int64)
        gy = np.where(np.isfinite(qy) & (np.abs(qy) < 2.0 ** 31), qy, 0.0).astype(np.int64)
    return p, gx, gy


def camera_rays(oracle, cfg):
    """The oracle's GetRay for every pixel of cfg's frame, row-major -> n x 6."""
    W, H = cfg.screen_width, cfg.screen_height
    out = np.empty((H * W, 6), dtype=np.float64)
    for py in range(H):
        for px in range(W):
            pos, dirv, _ = oracle.probe_ray(cfg, px, py)
            out[py * W + px, 0:3] = pos
            out[py * W + px, 3:6] = dirv
    return out


def expected_from_oracle(oracle, cfg, heights, cmap, rays, params):
    """The records hmrm_trace_rays owes for the camera rays of cfg's frame: rgba / steps / entry_d / status from
    oracle.render(per_pixel=True), point and cell from hit_points."""
    fb, _total, _capped, steps, entry = oracle.render(cfg, heights, cmap, per_pixel=True)
    n = cfg.screen_width * cfg.screen_height
    s = steps.reshape(-1)
    capped = s < 0
    s = np.where(capped, -1 - s, s)
    out = np.zeros(n, dtype=RAY_HIT_DTYPE)
    out["entry_d"] = entry.reshape(-1)
    out["steps"] = s.astype(np.uint32)
    out["rgba"] = fb.reshape(-1, 4)
    # a ray ends on terrain iff its last load hit: the position of load `steps` is below that cell's threshold
    p, gx, gy = hit_points(rays, out["entry_d"], s, params, cfg.step_dist)
    mh, mw = heights.shape
    inside = (s > 0) & (gx >= 0) & (gx < mw) & (gy >= 0) & (gy < mh)
    hit = np.zeros(n, dtype=bool)
    if cfg.sampling == 1:
        thr = heights.reshape(-1) + params.min_height
        qx, qy = p[:, 0] / params.grid_width, -p[:, 1] / params.grid_width
        (c00, c10, c01, c11), tx, ty = _bil(np.where(inside, qx, 0.0), np.where(inside, qy, 0.0), mw, mh)
        t = _mix(tx, ty, thr[c00], thr[c10], thr[c01], thr[c11])
    else:
        t = heights[np.where(inside, gy, 0), np.where(inside, gx, 0)] + params.min_height
        if cfg.sampling == 2:
            t = t.astype(np.float32).astype(np.float64)
    hit = inside & ~capped & (p[:, 2] < t)
    out["status"] = np.where(hit, HIT, np.where(capped, CAPPED, MISS)).astype(np.uint32)
    out["point"] = np.where(hit[:, None], p, 0.0)
    out["cell_x"] = np.where(hit, gx, -1)
    out["cell_y"] = np.where(hit, gy, -1)
    return out
