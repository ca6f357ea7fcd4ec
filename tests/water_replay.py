"""hmrm_render_water (include/hmrm.h) in numpy, composed of the replays that exist: every pixel first gets its primary ray's
pixel -- ray_replay.replay, or segment_replay.replay(interior=True) under HMRM_TRACE_INTERIOR -- then every pixel whose primary
ray HIT with t <= level (lit_replay.hit_thresholds: the threshold the hitting load compared z with) casts a mirror ray:
segment_replay.replay(interior=True, max_steps=L) from (P.x, P.y, t) along the primary direction with the sign bit of z flipped.
The mirror pixel m -- that record's rgba: the hit cell's colour, or the miss shade of the mirror ray's own dz -- is blended into
the base b, the primary pixel or the water's own colour: (b * (255 - r) + m * r + 127) // 255 per channel.  Capped primary rays
and capped mirror rays are counted together."""
import numpy as np

import lit_replay as lr
import ray_replay
import segment_replay as sr

MISS, HIT, CAPPED, END = sr.MISS, sr.HIT, sr.CAPPED, sr.END


def flip_sign(v):
    """-v with nothing but the sign bit changed, NaN included."""
    return (np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) ^ np.uint64(1 << 63)).view(np.float64)


def mirror_rays(rays, primary, t, level):
    """The mirror rays of the records that hit at or below the level -> (indices, n x 6 rays).  A NaN level: none."""
    with np.errstate(invalid="ignore"):
        wet = (primary["status"] == HIT) & (t <= float(level))
    idx = np.nonzero(wet)[0]
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    out = np.empty((idx.size, 6), dtype=np.float64)
    out[:, 0] = primary["point"][idx, 0]
    out[:, 1] = primary["point"][idx, 1]
    out[:, 2] = t[idx]
    out[:, 3] = rays[idx, 3]
    out[:, 4] = rays[idx, 4]
    out[:, 5] = flip_sign(rays[idx, 5])
    return idx, out


def blend(base, mirror, r):
    """(b * (255 - r) + m * r + 127) // 255 for R, G and B; A stays 255."""
    out = np.array(base, dtype=np.uint8).reshape(-1, 4).copy()
    b = out[:, 0:3].astype(np.int64)
    m = np.asarray(mirror, dtype=np.uint8).reshape(-1, 4)[:, 0:3].astype(np.int64)
    out[:, 0:3] = ((b * (255 - int(r)) + m * int(r) + 127) // 255).astype(np.uint8)
    out[:, 3] = 255
    return out


def replay(rays, heights, cmap, params, step_dist, level, mirror_step_dist, bg=(0, 0, 0), sampling=0, step_cap=1 << 26,
           max_steps=0, reflectivity=128, color=None, interior=False, primary=None):
    """primary: the primary rays' records when the caller has them already (they do not depend on the water).
    -> dict: rgba (n x 4, the water frame's pixels in ray order), primary (the primary records), t, mirror_index / mirror_rays /
    mirror (the mirror rays' ray numbers, rays and records), water (n bools), capped (primary + mirror rays stopped by the cap)."""
    if primary is not None:
        pass
    elif interior:
        primary = sr.replay(rays, heights, cmap, params, step_dist, bg=bg, sampling=sampling, step_cap=step_cap, interior=True)
    else:
        primary = ray_replay.replay(rays, heights, cmap, params, step_dist, bg=bg, sampling=sampling, step_cap=step_cap)
    t = lr.hit_thresholds(primary, heights, params, sampling)
    idx, mrays = mirror_rays(rays, primary, t, level)
    mirror = sr.replay(mrays, heights, cmap, params, mirror_step_dist, bg=bg, sampling=sampling, step_cap=step_cap, interior=True,
                       max_steps=max_steps)
    water = np.zeros(primary.shape[0], dtype=bool)
    water[idx] = True
    rgba = primary["rgba"].copy()
    base = rgba[idx]
    if color is not None:
        base = np.tile(np.array([color[0], color[1], color[2], 255], dtype=np.uint8), (idx.size, 1))
    rgba[idx] = blend(base, mirror["rgba"], reflectivity)
    capped = int((primary["status"] == CAPPED).sum() + (mirror["status"] == CAPPED).sum())
    return dict(rgba=rgba, primary=primary, t=t, mirror_index=idx, mirror_rays=mrays, mirror=mirror, water=water, capped=capped)
