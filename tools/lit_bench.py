"""Lit frames (hmrm_render_lit: sun shadows marched in the render kernel) on one box (tools only).

Modelled on tools/segments_bench.py: C3's content -- the 3840 x 2160 spherical camera over the 4096^2 map -- with the sun at
--elevation degrees (default 30).  Every launch is timed by HIP events, the candidates of a comparison alternate in the same
process, --warmup launches of each come first, and a median is printed with its range.

  (a) the lit frame against hmrm_render of the same camera (hmrm_last_kernel_ms: events around the kernel launch): what
      shadows cost.
  (b) the lit frame against the two-pass route: that hmrm_render time plus an hmrm_trace_segments_device batch of exactly
      the frame's shadow rays, prepared beforehand (hmrm_trace_rays of the camera's rays for the hit points, the thresholds
      from the scene's heights; the rays stay in the frame kernel's wave order).  The tool checks that the batch's HIT set is
      the set of pixels the lit frame darkens.

    python tools/lit_bench.py [--pairs 9] [--warmup 8] [--elevation 30] [--azimuth 40] [--res 3840x2160]
"""
import argparse
import importlib
import json
import math
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--elevation", type=float, default=30.0)
    ap.add_argument("--azimuth", type=float, default=40.0)
    ap.add_argument("--res", default="3840x2160")
    args = ap.parse_args()
    import torch
    hm.set_device(0)
    wl = hm.synth.WORKLOADS["C3"]
    rgb, cmap = hm.synth.synth_maps(wl.map_size)
    params, cam = wl.scene_params(), wl.camera()
    cam.width, cam.height = (int(v) for v in args.res.split("x"))
    scene = hm.Scene(rgb, cmap, params)
    n = cam.width * cam.height
    el, az = math.radians(args.elevation), math.radians(args.azimuth)
    sun_dir = (math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el))
    sun = hm.Sun.make(sun_dir, cam.step_dist, ambient=0)
    bg = (cam.bg_r, cam.bg_g, cam.bg_b)
    results = []

    def frame_ms(fn):
        fn()
        return float(lib.hmrm_last_kernel_ms())

    # ---- (a) the lit frame against hmrm_render ----
    f_lit = lambda: frame_ms(lambda: scene.render_lit(cam, sun))
    f_plain = lambda: frame_ms(lambda: scene.render(cam))
    lit_ms, plain_ms = alternate(f_lit, f_plain, args.warmup, args.pairs)
    ratios = sorted(x / y for x, y in zip(lit_ms, plain_ms))
    lit = scene.render_lit(cam, sun).reshape(-1, 4)
    plain = scene.render(cam).reshape(-1, 4)
    darkened = (lit != plain).any(axis=1)
    print(f"(a) lit frame {med(lit_ms)}; hmrm_render {med(plain_ms)}; ratio {statistics.median(ratios):.3f} "
          f"[{ratios[0]:.3f} .. {ratios[-1]:.3f}]; sun {sun_dir}, {int(darkened.sum())} of {n} pixels darkened; kernel "
          f"{scene.kernel_choice()}", flush=True)
    results.append({"case": "a", "lit_ms": lit_ms, "render_ms": plain_ms, "darkened": int(darkened.sum())})

    # ---- (b) against hmrm_render + a batch of the frame's shadow rays ----
    order = rays_bench.wave_order(cam.width, cam.height)
    rays = rays_bench.camera_rays(cam, params, wl.map_size, wl.map_size)[order]
    primary = scene.trace_rays(rays, cam.step_dist, bg=bg)
    hit = primary["status"] == hm.RAY_HIT
    thr = (scene.read_heights() + params.min_height).reshape(-1)
    cell = primary["cell_x"][hit].astype(np.int64) + primary["cell_y"][hit].astype(np.int64) * wl.map_size
    srays = np.empty((int(hit.sum()), 6), dtype=np.float64)
    srays[:, 0:2] = primary["point"][hit, 0:2]
    srays[:, 2] = thr[cell]
    srays[:, 3:6] = sun_dir
    m = srays.shape[0]
    d_rays = torch.from_numpy(srays).cuda()
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

    lit2_ms, batch_ms = alternate(f_lit, batch, args.warmup, args.pairs)
    scene.take_capped(stream.cuda_stream, allow_capped=True)
    shadow = d_hits.cpu().numpy().view(hm.RAY_HIT_DTYPE)
    shadowed = np.zeros(n, dtype=bool)
    shadowed[np.nonzero(hit)[0]] = shadow["status"] == hm.RAY_HIT
    by_pixel = np.zeros(n, dtype=bool)
    by_pixel[order] = shadowed
    # (a shadowed pixel whose colour is black already does not change: the darkened set is a subset)
    agree = bool((darkened <= by_pixel).all()) and bool((plain[by_pixel & ~darkened, 0:3] == 0).all())
    two_pass = statistics.median(plain_ms) + statistics.median(batch_ms)
    print(f"(b) lit frame {med(lit2_ms)}; shadow-ray batch of {m} rays {med(batch_ms)}; hmrm_render + batch {two_pass:.4f} ms; "
          f"lit / (render + batch) {statistics.median(lit2_ms) / two_pass:.3f}; shadowed {int(by_pixel.sum())}, the lit frame "
          f"darkens exactly those: {agree}", flush=True)
    results.append({"case": "b", "lit_ms": lit2_ms, "batch_ms": batch_ms, "shadow_rays": m, "shadowed": int(by_pixel.sum()),
                    "agree": agree})
    scene.close()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
