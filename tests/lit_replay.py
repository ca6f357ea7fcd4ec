"""hmrm_render_lit (include/hmrm.h) in numpy, composed of the replays that exist: every pixel first gets its primary ray's
pixel -- ray_replay.replay, or segment_replay.replay(interior=True) under HMRM_TRACE_INTERIOR -- then every pixel whose primary
ray HIT casts a shadow ray: segment_replay.replay(interior=True, max_steps=L) from (P.x, P.y, t) along the sun's direction,
P the record's hit point and t the threshold the hitting load compared z with (heights + min_height; its float round trip
for HMRM_NEAREST_F32; _bil / _mix at P for HMRM_BILINEAR).  A pixel whose shadow ray's status is HIT keeps
(c * ambient + 127) // 255 of R, G and B.  Capped primary rays and capped shadow rays are counted together."""
import numpy as np

import ray_replay
import segment_replay as sr
from ray_replay import _bil, _mix, box

MISS, HIT, CAPPED, END = sr.MISS, sr.HIT, sr.CAPPED, sr.END


def hit_thresholds(primary, heights, params, sampling):
    """t of every primary record (junk where the ray did not hit): what z was compared with when hmap.cpp:1016 fired."""
    mh, mw = heights.shape
    c0, _c1 = box(params, mw, mh)
    thr = heights.reshape(-1) + c0[2]
    if sampling == 2:
        thr = thr.astype(np.float32).astype(np.float64)
    hit = primary["status"] == HIT
    if sampling == 1:
        gw = params.grid_width
        with np.errstate(all="ignore"):
            qx = np.where(hit, (primary["point"][:, 0] - c0[0]) / gw, 0.0)
            qy = np.where(hit, -(primary["point"][:, 1] - c0[1]) / gw, 0.0)
            (c00, c10, c01, c11), tx, ty = _bil(qx, qy, mw, mh)
            return _mix(tx, ty, thr[c00], thr[c10], thr[c01], thr[c11])
    cell = np.where(hit, primary["cell_x"].astype(np.int64) + primary["cell_y"].astype(np.int64) * mw, 0)
    return thr[cell]


def shadow_rays(primary, t, sun_dir):
    """The shadow rays of the records that hit -> (indices, n x 6 rays)."""
    idx = np.nonzero(primary["status"] == HIT)[0]
    rays = np.empty((idx.size, 6), dtype=np.float64)
    rays[:, 0] = primary["point"][idx, 0]
    rays[:, 1] = primary["point"][idx, 1]
    rays[:, 2] = t[idx]
    rays[:, 3:6] = np.asarray(sun_dir, dtype=np.float64)
    return idx, rays


def darken(rgba, ambient):
    out = rgba.copy()
    out[:, 0:3] = ((rgba[:, 0:3].astype(np.int64) * int(ambient) + 127) // 255).astype(np.uint8)
    return out


def replay(rays, heights, cmap, params, step_dist, sun_dir, sun_step_dist, bg=(0, 0, 0), sampling=0, step_cap=1 << 26,
           max_steps=0, ambient=128, interior=False, primary=None):
    """primary: the primary rays' records when the caller has them already (they do not depend on the sun).
    -> dict: rgba (n x 4, the lit frame's pixels in ray order), primary (the primary records), t, shadow_index / shadow
    (the shadow rays' ray numbers and records), shadowed (n bools), capped (primary + shadow rays stopped by the step cap)."""
    if primary is not None:
        pass
    elif interior:
        primary = sr.replay(rays, heights, cmap, params, step_dist, bg=bg, sampling=sampling, step_cap=step_cap, interior=True)
    else:
        primary = ray_replay.replay(rays, heights, cmap, params, step_dist, bg=bg, sampling=sampling, step_cap=step_cap)
    t = hit_thresholds(primary, heights, params, sampling)
    idx, srays = shadow_rays(primary, t, sun_dir)
    shadow = sr.replay(srays, heights, cmap, params, sun_step_dist, bg=bg, sampling=sampling, step_cap=step_cap, interior=True,
                       max_steps=max_steps)
    shadowed = np.zeros(primary.shape[0], dtype=bool)
    shadowed[idx] = shadow["status"] == HIT
    rgba = primary["rgba"].copy()
    rgba[shadowed] = darken(rgba[shadowed], ambient)
    capped = int((primary["status"] == CAPPED).sum() + (shadow["status"] == CAPPED).sum())
    return dict(rgba=rgba, primary=primary, t=t, shadow_index=idx, shadow_rays=srays, shadow=shadow, shadowed=shadowed,
                capped=capped)
