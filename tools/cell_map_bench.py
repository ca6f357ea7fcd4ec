"""Cell maps (hmrm_cell_map: one byte per map cell, the rays made in the kernel) on one box (tools only).

Modelled on tools/lit_bench.py: C3's content -- the 4096^2 map of bench.py -- with the sun at --elevation degrees (default 30,
DESIGN.md 5.11's).  Every launch is timed by HIP events on a stream of its own, the candidates of a comparison alternate in
the same process, --warmup launches of each come first, and a median is printed with its range.

  (A) hmrm_cell_map_device over the whole map -- the status map, then HMRM_MAP_WEIGHT | HMRM_MAP_DIFFUSE -- against the route a
      user has without it: hmrm_trace_segments_device over the same W * H rays, built beforehand on the device (48 bytes per
      ray in, 56 bytes per record out; building them is not timed).  The tool checks that the status map is the batch's
      status column.
  (B) for scale: hmrm_bench_kernel_ms of C3's frame, and HMRM_MAP_WEIGHT | HMRM_MAP_DIFFUSE | HMRM_MAP_NO_SHADOWS alone -- no
      ray is marched: the cost of the prologue and the epilogue.

    python tools/cell_map_bench.py [--pairs 9] [--warmup 8] [--elevation 30] [--azimuth 40] [--map 4096] [--lift 0]
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
from segments_bench import alternate, med  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--elevation", type=float, default=30.0)
    ap.add_argument("--azimuth", type=float, default=40.0)
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
    el, az = math.radians(args.elevation), math.radians(args.azimuth)
    sun_dir = (math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el))
    step = cam.step_dist
    results = []

    # the W * H rays of the definition, row-major over the cells, on the device
    gw = float(params.grid_width)
    thr = scene.read_heights() + params.min_height
    rays = np.empty((n, 6), dtype=np.float64)
    cy, cx = np.mgrid[0:size, 0:size]
    rays[:, 0] = ((cx.reshape(-1).astype(np.float64) + 0.5) * gw)
    rays[:, 1] = -((cy.reshape(-1).astype(np.float64) + 0.5) * gw)
    rays[:, 2] = thr.reshape(-1) + args.lift
    rays[:, 3:6] = sun_dir
    del cx, cy
    d_rays = torch.from_numpy(rays).cuda()
    del rays
    d_hits = torch.zeros(n * 56, dtype=torch.uint8, device="cuda")
    d_map = torch.zeros(n, dtype=torch.uint8, device="cuda")
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

    batch = timed(lambda: scene.trace_segments_device(d_rays.data_ptr(), n, d_hits.data_ptr(), step, interior=True, stream=stream.cuda_stream))

    def cells(**kw):
        return timed(lambda: scene.cell_map_device(d_map.data_ptr(), size, sun_dir, step, lift=args.lift, ambient=64, stream=stream.cuda_stream, **kw))

    # ---- (A) against the batch route ----
    for name, kw in (("status", {}), ("weight+diffuse", dict(weight=True, diffuse=True))):
        map_ms, batch_ms = alternate(cells(**kw), batch, args.warmup, args.pairs)
        ratios = sorted(x / y for x, y in zip(map_ms, batch_ms))
        line = (f"(A) cell map, {name}: {med(map_ms)}; hmrm_trace_segments_device of the same {n} rays {med(batch_ms)}; ratio "
                f"{statistics.median(ratios):.3f} [{ratios[0]:.3f} .. {ratios[-1]:.3f}]; kernel {scene.kernel_choice()}")
        if not kw:
            cells()()
            status = d_map.cpu().numpy()
            want = d_hits.cpu().numpy().view(hm.RAY_HIT_DTYPE)["status"].astype(np.uint8)
            agree = bool(np.array_equal(status, want))
            line += f"; HIT {int((status == hm.RAY_HIT).sum())}, MISS {int((status == hm.RAY_MISS).sum())}; the map is the batch's status column: {agree}"
            results.append({"case": "A", "mode": name, "map_ms": map_ms, "batch_ms": batch_ms, "agree": agree})
        else:
            results.append({"case": "A", "mode": name, "map_ms": map_ms, "batch_ms": batch_ms})
        print(line, flush=True)
    scene.take_capped(stream.cuda_stream, allow_capped=True)

    # ---- (B) for scale ----
    bare = cells(weight=True, diffuse=True, shadows=False)
    frame = lambda: float(scene.bench_kernel_ms(cam, 1))
    bare_ms, frame_ms = alternate(bare, frame, args.warmup, args.pairs)
    print(f"(B) HMRM_MAP_NO_SHADOWS alone (prologue and epilogue, no march) {med(bare_ms)}; hmrm_bench_kernel_ms of C3's "
          f"{cam.width} x {cam.height} frame {med(frame_ms)}", flush=True)
    results.append({"case": "B", "no_shadows_ms": bare_ms, "frame_ms": frame_ms})
    scene.close()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
