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

    python tools/water_bench.py [--pairs 9] [--warmup 8] [--share 0.27] [--res 3840x2160]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--share", type=float, default=0.27)
    ap.add_argument("--res", default="3840x2160")
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
