"""Water frames (hmrm_render_water: mirror rays marched in the render kernel) on one box (tools only).

Modelled on tools/lit_bench.py: C3's content -- the 3840 x 2160 spherical camera over the 4096^2 map -- flooded at the luminance
that puts about --share of the dry frame's hit pixels on water (the height image clamped from below, np.maximum(rgb, L); the
level is the lake's threshold plus a quarter of a luminance step).  Every launch is timed by HIP events, the candidates of a
comparison alternate in the same process, --warmup launches of each come first, and a median is printed with its range.

  (a) the water frame against hmrm_render of the same camera on the same flooded scene (hmrm_last_kernel_ms: events around the
      kernel launch): what the reflections cost.
  (b) the water frame against the two-pass route: that hmrm_render time plus an hmrm_trace_segments_device batch of exactly the
      frame's mirror rays, prepared beforehand (hmrm_trace_rays of the camera's rays for the hit points, the thresholds from the
      scene's heights; the rays stay in the frame kernel's wave order).  The tool checks that the batch's records give the
      frame's mirror pixels (the frame at reflectivity 255).
  (c) the antialiased water frame at factor 2 (hmrm_render_water_aa) against hmrm_render_aa at factor 2, both at half the
      resolution each way: the super frame is (a)'s frame, so the two also stand beside (a)'s.
  (d) the water frame under the scene's light plane (HMRM_WATER_BAKED; a formula plane, full scale 1000: the cost does not depend
      on the words) against hmrm_render_baked and, once more, against the plain water frame.
  (e) the sun-lit water frame (hmrm_render_water_lit, diffuse levels and shadow rays, a sun 15 degrees above the horizon) beside the
      water frame, beside hmrm_render_shaded with the same flags, and beside the multi-launch route it replaces: hmrm_render_shaded
      plus an hmrm_trace_segments_device batch of the frame's mirror rays plus one of the mirror hits' shadow rays, both prepared
      beforehand -- copies and glue not counted.  The tool checks that the batches' records (with the primary hits' shadow batch, for
      the check alone) reproduce the frame.

    python tools/water_bench.py [--pairs 9] [--warmup 8] [--share 0.27] [--res 3840x2160] [--cases abcde]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hm = importlib.import_module("heightmap-ray-marcher_amd")
import rays_bench  # noqa: E402  (camera_rays, wave_order)
from segments_bench import alternate, med  # noqa: E402

lib = importlib.import_module("heightmap-ray-marcher_amd.lib").lib


def box_filter_2(frame):
    """hmrm_render_aa's 2 x 2 box filter of a frame, (S + 2) >> 2 per channel, alpha 255."""
    h, w = frame.shape[:2]
    s = frame[:, :, :3].astype(np.int64).reshape(h // 2, 2, w // 2, 2, 3).sum(axis=(1, 3))
    out = np.empty((h // 2, w // 2, 4), dtype=np.uint8)
    out[:, :, :3] = (s + 2) >> 2
    out[:, :, 3] = 255
    return out


def diffuse_weights(records, thr2d, params, sun_dir, ambient, shadowed):
    """hmrm_render_shaded's weight of every record that hit, nearest sampling, in include/hmrm.h's operation order (255 elsewhere)."""
    mh, mw = thr2d.shape
    hit = records["status"] == hm.RAY_HIT
    cx, cy = np.where(hit, records["cell_x"], 0).astype(np.int64), np.where(hit, records["cell_y"], 0).astype(np.int64)
    xm, xp, ym, yp = np.maximum(cx - 1, 0), np.minimum(cx + 1, mw - 1), np.maximum(cy - 1, 0), np.minimum(cy + 1, mh - 1)
    gw = params.grid_width
    s = np.asarray(sun_dir, dtype=np.float64)
    with np.errstate(all="ignore"):
        gx = np.where(xp > xm, (thr2d[cy, xp] - thr2d[cy, xm]) / ((xp - xm).astype(np.float64) * gw), 0.0)
        gy = np.where(yp > ym, (thr2d[yp, cx] - thr2d[ym, cx]) / ((yp - ym).astype(np.float64) * gw), 0.0)
        nx, ny = -gx, gy
        k = ((nx * s[0] + ny * s[1]) + s[2]) / np.sqrt(((nx * nx + ny * ny) + 1.0) * ((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]))
        q = (np.where(k > 0.0, np.where(k < 1.0, k, 1.0), 0.0) * 255.0 + 0.5).astype(np.int64)
    w = int(ambient) + ((255 - int(ambient)) * q + 127) // 255
    return np.where(hit, np.where(shadowed, int(ambient), w), 255)


def weighted(rgba, w):
    out = rgba.copy()
    out[:, 0:3] = ((rgba[:, 0:3].astype(np.int64) * w[:, None] + 127) // 255).astype(np.uint8)
    return out


def lit_water_case(args, torch, scene, cam, params, wl, rays, order, heights, level, water, bg, frame_ms, results):
    """(e): the sun-lit water frame beside the water frame, the shaded frame and the multi-launch route."""
    sun_dir, ambient = (0.837, 0.483, 0.259), 96
    sun = hm.Sun.make(sun_dir, cam.step_dist, ambient=ambient)
    thr2d = heights + params.min_height
    thr = thr2d.reshape(-1)
    f_lit_water = lambda: frame_ms(lambda: scene.render_water_lit(cam, water, sun))
    f_water = lambda: frame_ms(lambda: scene.render_water(cam, water))
    f_shaded = lambda: frame_ms(lambda: scene.render_shaded(cam, sun))
    lw1_ms, water_ms = alternate(f_lit_water, f_water, args.warmup, args.pairs)
    lw2_ms, shaded_ms = alternate(f_lit_water, f_shaded, args.warmup, args.pairs)
    # the batches: the frame's mirror rays and the mirror hits' shadow rays, in the frame kernel's wave order
    stream = torch.cuda.Stream()

    def segments(batch_rays):
        """-> (records of the batch, a callable that runs it once more and returns its time by events)"""
        k = batch_rays.shape[0]
        d_rays = torch.from_numpy(np.ascontiguousarray(batch_rays)).cuda()
        d_hits = torch.zeros(max(k, 1) * 56, dtype=torch.uint8, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()

        def run():
            with torch.cuda.stream(stream):
                e0.record(stream)
                scene.trace_segments_device(d_rays.data_ptr(), k, d_hits.data_ptr(), cam.step_dist, bg=bg, interior=True,
                                            stream=stream.cuda_stream)
                e1.record(stream)
            e1.synchronize()
            return float(e0.elapsed_time(e1))

        run()
        scene.take_capped(stream.cuda_stream, allow_capped=True)
        return d_hits.cpu().numpy().view(hm.RAY_HIT_DTYPE)[:k].copy(), run, (d_rays, d_hits)

    def shadow_rays_of(records):
        hit = records["status"] == hm.RAY_HIT
        cell = np.where(hit, records["cell_x"].astype(np.int64) + records["cell_y"].astype(np.int64) * wl.map_size, 0)
        out = np.empty((int(hit.sum()), 6), dtype=np.float64)
        out[:, 0:2] = records["point"][hit, 0:2]
        out[:, 2] = thr[cell[hit]]
        out[:, 3:6] = np.asarray(sun_dir, dtype=np.float64)
        return hit, out

    primary = scene.trace_rays(rays, cam.step_dist, bg=bg)
    hit, srays = shadow_rays_of(primary)
    cell = np.where(hit, primary["cell_x"].astype(np.int64) + primary["cell_y"].astype(np.int64) * wl.map_size, 0)
    wet = hit & (thr[cell] <= level)
    mrays = np.empty((int(wet.sum()), 6), dtype=np.float64)
    mrays[:, 0:2] = primary["point"][wet, 0:2]
    mrays[:, 2] = thr[cell[wet]]
    mrays[:, 3:5] = rays[wet, 3:5]
    mrays[:, 5] = -rays[wet, 5]
    mirror, run_mirror, keep1 = segments(mrays)
    mhit, msrays = shadow_rays_of(mirror)
    mshadow, run_mshadow, keep2 = segments(msrays)
    lw3_ms, mirror_ms = alternate(f_lit_water, run_mirror, args.warmup, args.pairs)
    lw4_ms, mshadow_ms = alternate(f_lit_water, run_mshadow, args.warmup, args.pairs)
    scene.take_capped(stream.cuda_stream, allow_capped=True)
    # the check: the records reproduce the frame (the primary hits' shadow batch is run for this alone)
    shadow, _run, keep3 = segments(srays)
    shadowed = np.zeros(primary.shape[0], dtype=bool)
    shadowed[hit] = shadow["status"] == hm.RAY_HIT
    mshadowed = np.zeros(mirror.shape[0], dtype=bool)
    mshadowed[mhit] = mshadow["status"] == hm.RAY_HIT
    want = weighted(primary["rgba"], diffuse_weights(primary, thr2d, params, sun_dir, ambient, shadowed))
    m = weighted(mirror["rgba"], diffuse_weights(mirror, thr2d, params, sun_dir, ambient, mshadowed))
    r = int(water.reflectivity)
    want[wet, 0:3] = ((want[wet, 0:3].astype(np.int64) * (255 - r) + m[:, 0:3].astype(np.int64) * r + 127) // 255).astype(np.uint8)
    frame = scene.render_water_lit(cam, water, sun).reshape(-1, 4)[order]
    agree = bool((frame == want).all())
    route = statistics.median(shaded_ms) + statistics.median(mirror_ms) + statistics.median(mshadow_ms)
    lit_all = lw1_ms + lw2_ms + lw3_ms + lw4_ms
    r_water = sorted(x / y for x, y in zip(lw1_ms, water_ms))
    r_shaded = sorted(x / y for x, y in zip(lw2_ms, shaded_ms))
    print(f"(e) sun-lit water frame {med(lit_all)}; beside the water frame {med(water_ms)}: ratio {statistics.median(r_water):.3f} "
          f"[{r_water[0]:.3f} .. {r_water[-1]:.3f}]; beside hmrm_render_shaded {med(shaded_ms)}: ratio {statistics.median(r_shaded):.3f} "
          f"[{r_shaded[0]:.3f} .. {r_shaded[-1]:.3f}]; mirror batch of {mrays.shape[0]} rays {med(mirror_ms)}; mirror hits' shadow batch of "
          f"{msrays.shape[0]} rays {med(mshadow_ms)}; hmrm_render_shaded + the two batches {route:.4f} ms; frame / route "
          f"{statistics.median(lit_all) / route:.3f}; shadowed primary hits {int(shadowed.sum())} of {int(hit.sum())}, shadowed mirror hits "
          f"{int(mshadowed.sum())} of {int(mhit.sum())}; the batches' records reproduce the frame: {agree}; kernel {scene.kernel_choice()}", flush=True)
    results.append({"case": "e", "lit_water_ms": lit_all, "water_ms": water_ms, "shaded_ms": shaded_ms, "mirror_batch_ms": mirror_ms,
                    "mirror_shadow_batch_ms": mshadow_ms, "mirror_rays": int(mrays.shape[0]), "mirror_shadow_rays": int(msrays.shape[0]),
                    "agree": agree})
    del keep1, keep2, keep3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--share", type=float, default=0.27)
    ap.add_argument("--res", default="3840x2160")
    ap.add_argument("--cases", default="abcde", help="which comparisons to run; (b) needs (a)'s times")
    args = ap.parse_args()
    import torch
    hm.set_device(0)
    wl = hm.synth.WORKLOADS["C3"]
    rgb, cmap = hm.synth.synth_maps(wl.map_size)
    params, cam = wl.scene_params(), wl.camera()
    cam.width, cam.height = (int(v) for v in args.res.split("x"))
    n = cam.width * cam.height
    bg = (cam.bg_r, cam.bg_g, cam.bg_b)
    order = rays_bench.wave_order(cam.width, cam.height)
    rays = rays_bench.camera_rays(cam, params, wl.map_size, wl.map_size)[order]

    # the lake's luminance: the --share quantile of the brightest channel over the cells the dry frame's rays hit
    dry = hm.Scene(rgb, cmap, params)
    primary = dry.trace_rays(rays, cam.step_dist, bg=bg)
    hit = primary["status"] == hm.RAY_HIT
    top = rgb.max(axis=2)[primary["cell_y"][hit], primary["cell_x"][hit]]
    lum = int(np.quantile(top, args.share))
    dry.close()
    del primary
    scene = hm.Scene(np.maximum(rgb, np.uint8(lum)), cmap, params)
    heights = scene.read_heights()
    lake_t = float(heights.min()) + params.min_height
    level = lake_t + (params.max_height - params.min_height) / 255.0 / 4.0
    water = hm.Water.make(level, cam.step_dist, reflectivity=128)
    mirror_only = hm.Water.make(level, cam.step_dist, reflectivity=255)
    results = []

    def frame_ms(fn):
        fn()
        return float(lib.hmrm_last_kernel_ms())

    if "e" in args.cases:
        lit_water_case(args, torch, scene, cam, params, wl, rays, order, heights, level, water, bg, frame_ms, results)
    if not set("abcd") & set(args.cases):
        scene.close()
        print(json.dumps(results))
        return

    # ---- (a) the water frame against hmrm_render ----
    f_water = lambda: frame_ms(lambda: scene.render_water(cam, water))
    f_plain = lambda: frame_ms(lambda: scene.render(cam))
    water_ms, plain_ms = alternate(f_water, f_plain, args.warmup, args.pairs)
    ratios = sorted(x / y for x, y in zip(water_ms, plain_ms))
    primary = scene.trace_rays(rays, cam.step_dist, bg=bg)
    hit = primary["status"] == hm.RAY_HIT
    thr = (heights + params.min_height).reshape(-1)
    cell = np.where(hit, primary["cell_x"].astype(np.int64) + primary["cell_y"].astype(np.int64) * wl.map_size, 0)
    wet = hit & (thr[cell] <= level)
    m = int(wet.sum())
    print(f"(a) water frame {med(water_ms)}; hmrm_render {med(plain_ms)}; ratio {statistics.median(ratios):.3f} "
          f"[{ratios[0]:.3f} .. {ratios[-1]:.3f}]; lake luminance {lum}, level {level:.6g}: {m} water pixels of {int(hit.sum())} hit "
          f"pixels ({m / max(1, int(hit.sum())):.3f}) of {n}; kernel {scene.kernel_choice()}", flush=True)
    results.append({"case": "a", "water_ms": water_ms, "render_ms": plain_ms, "lake_luminance": lum, "water_pixels": m,
                    "hit_pixels": int(hit.sum())})

    # ---- (b) against hmrm_render + a batch of the frame's mirror rays ----
    mrays = np.empty((m, 6), dtype=np.float64)
    mrays[:, 0:2] = primary["point"][wet, 0:2]
    mrays[:, 2] = thr[cell[wet]]
    mrays[:, 3:5] = rays[wet, 3:5]
    mrays[:, 5] = -rays[wet, 5]
    d_rays = torch.from_numpy(mrays).cuda()
    d_hits = torch.zeros(m * 56, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()

    def batch():
        with torch.cuda.stream(stream):
            e0.record(stream)
            scene.trace_segments_device(d_rays.data_ptr(), m, d_hits.data_ptr(), cam.step_dist, bg=bg, interior=True,
                                        stream=stream.cuda_stream)
            e1.record(stream)
        e1.synchronize()
        return float(e0.elapsed_time(e1))

    water2_ms, batch_ms = alternate(f_water, batch, args.warmup, args.pairs)
    scene.take_capped(stream.cuda_stream, allow_capped=True)
    mirror = d_hits.cpu().numpy().view(hm.RAY_HIT_DTYPE)
    frame = scene.render_water(cam, mirror_only).reshape(-1, 4)[order]
    plain = scene.render(cam).reshape(-1, 4)[order]
    agree = bool((frame[wet] == mirror["rgba"]).all()) and bool((frame[~wet] == plain[~wet]).all())
    sums = sorted(p + b for p, b in zip(plain_ms, batch_ms))
    two_pass = statistics.median(plain_ms) + statistics.median(batch_ms)
    status = mirror["status"]
    print(f"(b) water frame {med(water2_ms)}; mirror-ray batch of {m} rays {med(batch_ms)}; hmrm_render + batch {two_pass:.4f} ms "
          f"[{sums[0]:.4f} .. {sums[-1]:.4f} pairwise]; water / (render + batch) {statistics.median(water2_ms) / two_pass:.3f}; mirror rays "
          f"that hit {int((status == hm.RAY_HIT).sum())}, miss {int((status == hm.RAY_MISS).sum())}, capped "
          f"{int((status == hm.RAY_CAPPED).sum())}; the batch's records give the frame's mirror pixels: {agree}", flush=True)
    results.append({"case": "b", "water_ms": water2_ms, "batch_ms": batch_ms, "mirror_rays": m, "agree": agree})

    # ---- (c) antialiased: the water frame at factor 2 against hmrm_render_aa at factor 2 ----
    half = hm.Camera.from_buffer_copy(cam)
    half.width, half.height = cam.width // 2, cam.height // 2
    f_water_aa = lambda: frame_ms(lambda: scene.render_water_aa(half, water, factor=2))
    f_plain_aa = lambda: frame_ms(lambda: scene.render_aa(half, 2))
    water_aa_ms, plain_aa_ms = alternate(f_water_aa, f_plain_aa, args.warmup, args.pairs)
    ratios = sorted(x / y for x, y in zip(water_aa_ms, plain_aa_ms))
    same = scene.render_water_aa(half, water, factor=2).tobytes() == \
        box_filter_2(scene.render_water(cam, water)).tobytes() if cam.width % 2 == 0 and cam.height % 2 == 0 else None
    print(f"(c) {half.width} x {half.height} at factor 2: water frame {med(water_aa_ms)}; hmrm_render_aa {med(plain_aa_ms)}; ratio "
          f"{statistics.median(ratios):.3f} [{ratios[0]:.3f} .. {ratios[-1]:.3f}]; the frame is the filtered water frame of (a): {same}", flush=True)
    results.append({"case": "c", "water_aa_ms": water_aa_ms, "render_aa_ms": plain_aa_ms, "filtered_agrees": same})

    # ---- (d) under the light plane: the baked water frame against hmrm_render_baked and against the water frame ----
    y, x = np.mgrid[0:wl.map_size, 0:wl.map_size].astype(np.int64)
    scene.set_light(((37 * x + 101 * y + 29 * ((x * y) % 13)) % 1001).astype(np.uint16), 1000)
    del y, x
    f_baked_water = lambda: frame_ms(lambda: scene.render_water_aa(cam, water, baked=True))
    f_baked = lambda: frame_ms(lambda: scene.render_baked(cam))
    bw_ms, baked_ms = alternate(f_baked_water, f_baked, args.warmup, args.pairs)
    bw2_ms, water3_ms = alternate(f_baked_water, f_water, args.warmup, args.pairs)
    r1 = sorted(x / y for x, y in zip(bw_ms, baked_ms))
    r2 = sorted(x / y for x, y in zip(bw2_ms, water3_ms))
    print(f"(d) baked water frame {med(bw_ms)}; hmrm_render_baked {med(baked_ms)}; ratio {statistics.median(r1):.3f} [{r1[0]:.3f} .. "
          f"{r1[-1]:.3f}]; baked water frame {med(bw2_ms)} beside the water frame {med(water3_ms)}; ratio {statistics.median(r2):.3f} "
          f"[{r2[0]:.3f} .. {r2[-1]:.3f}]", flush=True)
    results.append({"case": "d", "baked_water_ms": bw_ms, "baked_ms": baked_ms, "baked_water2_ms": bw2_ms, "water_ms": water3_ms})
    scene.close()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
