"""hmrm_render_water_lit (include/hmrm.h) in numpy, composed of the replays that exist and no marching code of its own:
water_replay.replay gives the primary and the mirror records; lit_replay.hit_thresholds / shadow_rays and segment_replay.replay
give the shadow rays of the primary hits and -- hit_thresholds applied to the mirror records too -- of the mirror hits;
shade_replay.weights / apply weight either side by its own hit; water_replay.blend mixes them.  Capped rays of all four kinds are
counted together."""
import numpy as np

import lit_replay as lr
import segment_replay as sr
import shade_replay as sh
import water_replay as wr

MISS, HIT, CAPPED, END = sr.MISS, sr.HIT, sr.CAPPED, sr.END


def shadows_of(records, heights, cmap, params, sampling, sun_dir, sun_step_dist, sun_max_steps, bg, step_cap):
    """The shadow rays of the records that hit -> (shadowed: one bool per record, the shadow records, their rays)."""
    t = lr.hit_thresholds(records, heights, params, sampling)
    idx, rays = lr.shadow_rays(records, t, sun_dir)
    shadow = sr.replay(rays, heights, cmap, params, sun_step_dist, bg=bg, sampling=sampling, step_cap=step_cap, interior=True,
                       max_steps=sun_max_steps)
    shadowed = np.zeros(records.shape[0], dtype=bool)
    shadowed[idx] = shadow["status"] == HIT
    return shadowed, shadow, rays


def replay(rays, heights, cmap, params, step_dist, level, mirror_step_dist, sun_dir, sun_step_dist, bg=(0, 0, 0), sampling=0,
           step_cap=1 << 26, max_steps=0, reflectivity=128, color=None, sun_max_steps=0, ambient=128, diffuse=True, shadows=True,
           interior=False, primary=None, wet=None):
    """wet: water_replay.replay's dict of the same water when the caller has it; primary: the primary records alone.
    -> dict: rgba (n x 4), primary, water (n bools), mirror_index, mirror, shadowed (n bools: the primary hit is shadowed),
    mirror_shadowed (one bool per mirror ray), w (n weights), mirror_w (one per mirror ray), shadow / mirror_shadow (the shadow
    records, None without shadow rays), shadow_rays / mirror_shadow_rays, capped (all four kinds of ray together)."""
    if wet is None:
        wet = wr.replay(rays, heights, cmap, params, step_dist, level, mirror_step_dist, bg=bg, sampling=sampling, step_cap=step_cap,
                        max_steps=max_steps, reflectivity=reflectivity, color=color, interior=interior, primary=primary)
    primary, mirror, idx = wet["primary"], wet["mirror"], wet["mirror_index"]
    shadow = mirror_shadow = srays = msrays = None
    shadowed = np.zeros(primary.shape[0], dtype=bool)
    mirror_shadowed = np.zeros(mirror.shape[0], dtype=bool)
    capped = int((primary["status"] == CAPPED).sum() + (mirror["status"] == CAPPED).sum())
    if shadows:
        shadowed, shadow, srays = shadows_of(primary, heights, cmap, params, sampling, sun_dir, sun_step_dist, sun_max_steps, bg, step_cap)
        mirror_shadowed, mirror_shadow, msrays = shadows_of(mirror, heights, cmap, params, sampling, sun_dir, sun_step_dist,
                                                           sun_max_steps, bg, step_cap)
        capped += int((shadow["status"] == CAPPED).sum() + (mirror_shadow["status"] == CAPPED).sum())
    w = sh.weights(primary, heights, params, sampling, sun_dir, ambient, diffuse, shadowed)
    mirror_w = sh.weights(mirror, heights, params, sampling, sun_dir, ambient, diffuse, mirror_shadowed)
    base = primary["rgba"].copy()
    if color is not None:
        base[idx] = np.array([color[0], color[1], color[2], 255], dtype=np.uint8)
    rgba = sh.apply(base, w)  # (w is 255 where the primary ray did not hit: untouched)
    rgba[idx] = wr.blend(rgba[idx], sh.apply(mirror["rgba"], mirror_w), reflectivity)  # (255 for MISS, END and CAPPED mirror rays)
    return dict(rgba=rgba, primary=primary, water=wet["water"], mirror_index=idx, mirror=mirror, shadowed=shadowed,
                mirror_shadowed=mirror_shadowed, w=w, mirror_w=mirror_w, shadow=shadow, mirror_shadow=mirror_shadow,
                shadow_rays=srays, mirror_shadow_rays=msrays, mirror_rays=wet["mirror_rays"], capped=capped)
