"""Accumulated lit frames (hmrm_render_lit_sum: K directions per pixel in one launch) on one box (tools only).

Modelled on tools/lit_bench.py and tools/cell_sum_bench.py: C3's content and camera -- the 3840 x 2160 spherical camera over the
4096^2 map --, the shadow rays' step the camera's, ambient 64, and K = rings * per_ring sky directions from hmrm_sky_directions
(4 x 4 = 16 and 4 x 16 = 64), with shade_flags 0 and HMRM_SHADE_DIFFUSE.  The two candidates of a comparison alternate in the
same process, --warmup rounds of each come first, and a median is printed with its range.

  hmrm_render_lit_sum_device into device planes, timed by HIP events on a stream of its own, against the route a user has
  without it: K hmrm_render_shaded frames of the same camera, one per direction, each timed by the events around its kernel
  (hmrm_last_kernel_ms) and added up.  Those K launches march the primary rays K times; the gaps between them, their copies and
  the summation that caller would still need are NOT timed.  Both favour that route.
  First the tool checks, on a scene with an all-white opaque colour map, that the light plane is the sum of the R channels of
  those K frames on the hit pixels (a geometry frame's cell plane says which) and 0xFFFF elsewhere.
  The bar: the median of the per-pair ratios sum / K launches is below 1 + the half-width of the run's own range of ratios.
  Also printed: the launch's time per direction over one hmrm_render_lit frame (the median of the K frames with shade_flags 0).

    python tools/lit_sum_bench.py [--pairs 9] [--warmup 8] [--res 3840x2160] [--k 16,64]
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
from segments_bench import alternate, med  # noqa: E402

lib = importlib.import_module("heightmap-ray-marcher_amd.lib").lib
RINGS = {16: (4, 4), 64: (4, 16)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--res", default="3840x2160")
    ap.add_argument("--k", default="16,64")
    args = ap.parse_args()
    import torch
    hm.set_device(0)
    wl = hm.synth.WORKLOADS["C3"]
    rgb, cmap = hm.synth.synth_maps(wl.map_size)
    params, cam = wl.scene_params(), wl.camera()
    cam.width, cam.height = (int(v) for v in args.res.split("x"))
    w, h = cam.width, cam.height
    scene = hm.Scene(rgb, cmap, params)
    white = hm.Scene(rgb, np.full_like(cmap, 255), params)
    sun = hm.Sun.make((0.0, 0.0, -1.0), cam.step_dist, ambient=64)  # (the direction is not looked at)
    hit = white.render_geometry(cam, rgba=False, range=False, slope=False)["cell"] >= 0
    d_rgba = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    d_light = torch.zeros((h, w), dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    results = []

    for K in (int(v) for v in args.k.split(",")):
        sky = hm.sky_directions(*RINGS.get(K, (1, K)))
        assert len(sky) == K
        d_dirs = torch.from_numpy(sky).cuda()
        torch.cuda.synchronize()
        for name, diffuse in (("shade_flags 0", False), ("HMRM_SHADE_DIFFUSE", True)):
            # ---- the check, over the white colour map ----
            total = np.zeros((h, w), dtype=np.int64)
            for d in sky:
                total += white.render_shaded(cam, hm.Sun.make(tuple(d), cam.step_dist, ambient=64), diffuse=diffuse, shadows=True)[:, :, 0]
            light = white.render_lit_sum(cam, sun, sky, diffuse=diffuse, light=True, rgba=False)
            agree = bool(np.array_equal(light[hit].astype(np.int64), total[hit])) and bool((light[~hit] == 0xFFFF).all())

            # ---- the timing, over C3's own colour map ----
            def summed():
                with torch.cuda.stream(stream):
                    e0.record(stream)
                    scene.render_lit_sum_device(cam, sun, d_dirs.data_ptr(), K, rgba=(d_rgba.data_ptr(), 4 * w), light=(d_light.data_ptr(), 2 * w),
                                                diffuse=diffuse, stream=stream.cuda_stream)
                    e1.record(stream)
                e1.synchronize()
                return float(e0.elapsed_time(e1))

            each = []

            def one_by_one():
                ms = []
                for d in sky:
                    scene.render_shaded(cam, hm.Sun.make(tuple(d), cam.step_dist, ambient=64), diffuse=diffuse, shadows=True)
                    ms.append(float(lib.hmrm_last_kernel_ms()))
                each.append(statistics.median(ms))
                return sum(ms)

            sum_ms, frames_ms = alternate(summed, one_by_one, args.warmup, args.pairs)
            ratios = sorted(x / y for x, y in zip(sum_ms, frames_ms))
            median, half = statistics.median(ratios), 0.5 * (ratios[-1] - ratios[0])
            one_frame = statistics.median(each[-args.pairs:])
            print(f"K = {K}, {name}: hmrm_render_lit_sum_device {med(sum_ms)}; {K} hmrm_render_shaded kernels {med(frames_ms)}; per-pair ratio "
                  f"median {median:.4f} [{ratios[0]:.4f} .. {ratios[-1]:.4f}], bar 1 + {half:.4f}: {'met' if median < 1.0 + half else 'NOT met'}; "
                  f"per direction {statistics.median(sum_ms) / K:.4f} ms against one frame's {one_frame:.4f} ms: "
                  f"{statistics.median(sum_ms) / K / one_frame:.4f}; kernel {scene.kernel_choice()}; {int(hit.sum())} of {w * h} pixels hit, sums "
                  f"{int(total[hit].min())} .. {int(total[hit].max())}; the light plane is the sum of the {K} frames: {agree}", flush=True)
            results.append({"K": K, "mode": name, "sum_ms": sum_ms, "frames_ms": frames_ms, "ratio_median": median,
                            "ratio_range": [ratios[0], ratios[-1]], "one_frame_ms": one_frame, "agree": agree})
    scene.take_capped(stream.cuda_stream, allow_capped=True)
    scene.close()
    white.close()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
