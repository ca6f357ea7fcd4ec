"""Accumulated cell maps (hmrm_cell_map_sum: K targets in one launch, one uint16 per map cell) on one box (tools only).

Modelled on tools/cell_map_bench.py: C3's content -- the 4096^2 map of bench.py --, its step, lift and ambient level, and
K = rings * per_ring sky directions from hmrm_sky_directions (default 4 x 16 = 64).  Every candidate is timed by HIP events on a
stream of its own, the two candidates of a comparison alternate in the same process, --warmup launches of each come first, and a
median is printed with its range.

  (A) hmrm_cell_map_sum_device over the whole map -- status mode, then HMRM_MAP_WEIGHT | HMRM_MAP_DIFFUSE -- against the route a
      user has without it: K hmrm_cell_map_device launches into K separate byte maps, one pair of events around the K launches.
      The summation that caller would still need is NOT timed, which favours that route.  The tool checks that the word map is
      the integer sum of the K byte maps.
      The bar: the median of the per-pair ratios sum / K launches is at most 1 + the half-width of the run's own range of pair
      ratios, i.e. equal within what the box resolves.

    python tools/cell_sum_bench.py [--pairs 9] [--warmup 8] [--rings 4] [--per-ring 16] [--map 4096] [--lift 0]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rings", type=int, default=4)
    ap.add_argument("--per-ring", type=int, default=16)
    ap.add_argument("--map", type=int, default=0, help="map side (default: C3's)")
    ap.add_argument("--lift", type=float, default=0.0)
    args = ap.parse_args()
    import torch
    hm.set_device(0)
    wl = hm.synth.WORKLOADS["C3"]
    size = args.map or wl.map_size
    rgb, cmap = hm.synth.synth_maps(size)
    params, cam = wl.scene_params(), wl.camera()
    scene = hm.Scene(rgb, cmap, params)
    n = size * size
    sky = hm.sky_directions(args.rings, args.per_ring)
    K = len(sky)
    step = cam.step_dist
    results = []

    d_targets = torch.from_numpy(sky).cuda()
    d_maps = torch.zeros((K, n), dtype=torch.uint8, device="cuda")  # the K separate maps of the route without the sum
    d_sum = torch.zeros(n, dtype=torch.int16, device="cuda")
    stream = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()

    def timed(fn):
        def run():
            with torch.cuda.stream(stream):
                e0.record(stream)
                fn()
                e1.record(stream)
            e1.synchronize()
            return float(e0.elapsed_time(e1))
        return run

    def summed(**kw):
        return timed(lambda: scene.cell_map_sum_device(d_sum.data_ptr(), 2 * size, d_targets.data_ptr(), K, step, lift=args.lift, ambient=64,
                                                       stream=stream.cuda_stream, **kw))

    def one_by_one(**kw):
        def launches():
            for k in range(K):
                scene.cell_map_device(d_maps[k].data_ptr(), size, tuple(sky[k]), step, lift=args.lift, ambient=64,
                                      stream=stream.cuda_stream, **kw)
        return timed(launches)

    for name, kw in (("status", {}), ("weight+diffuse", dict(weight=True, diffuse=True))):
        sum_ms, each_ms = alternate(summed(**kw), one_by_one(**kw), args.warmup, args.pairs)
        ratios = sorted(x / y for x, y in zip(sum_ms, each_ms))
        median, half = statistics.median(ratios), 0.5 * (ratios[-1] - ratios[0])
        want = torch.zeros(n, dtype=torch.int32, device="cuda")
        for k in range(K):  # (chunked: no K x n int32 temporary)
            want += d_maps[k].to(torch.int32) if kw else (d_maps[k] != hm.RAY_HIT).to(torch.int32)
        got = d_sum.to(torch.int32) & 0xffff
        agree = bool(torch.equal(got, want))
        print(f"(A) {name}, K = {K}: hmrm_cell_map_sum_device {med(sum_ms)}; {K} hmrm_cell_map_device launches {med(each_ms)}; per-pair "
              f"ratio median {median:.4f} [{ratios[0]:.4f} .. {ratios[-1]:.4f}], bar 1 + {half:.4f}: {'met' if median <= 1.0 + half else 'NOT met'}; "
              f"kernel {scene.kernel_choice()}; sums {int(want.min())} .. {int(want.max())}, mean {float(want.float().mean()):.2f}; "
              f"the word map is the sum of the {K} byte maps: {agree}", flush=True)
        results.append({"case": "A", "mode": name, "K": K, "sum_ms": sum_ms, "each_ms": each_ms, "ratio_median": median,
                        "ratio_range": [ratios[0], ratios[-1]], "agree": agree})
        del want, got
    scene.take_capped(stream.cuda_stream, allow_capped=True)
    scene.close()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
