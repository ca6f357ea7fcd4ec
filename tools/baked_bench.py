"""Baked-light frames (hmrm_render_baked: a per-cell light plane read by the frame kernels) on one box (tools only).

Modelled on tools/lit_sum_bench.py: C3's content and camera -- the 3840 x 2160 spherical camera over the 4096^2 map --, the
shadow rays' step the camera's, ambient 64, and the K = 64 sky directions of hmrm_sky_directions(4, 16).  The light plane is baked
once with hmrm_scene_bake_light (status mode: the count of open directions per cell, full scale 64); then four frames of the same
camera take turns in one process, the order rotated from round to round, --warmup rounds first, medians printed with their range:

  hmrm_render_baked                          the baked frame, kernel time by the events around its launch (hmrm_last_kernel_ms)
  hmrm_render                                the plain frame, timed the same way (its launch order is calibrated, as in production;
                                             the others' is the plain rotation)
  hmrm_render_shaded(DIFFUSE | NO_SHADOWS)   the hill-shaded frame without shadow rays, timed the same way
  hmrm_render_lit_sum_device                 the per-pixel route over the same 64 directions, timed by events on a stream of its own

and the one-off cost of the bake (wall time of the synchronous call, median of --bakes).  Also printed: per-round ratios baked /
plain and baked / shaded, and a check that under a plane whose every word is the full scale the baked frame is hmrm_render's.

    python tools/baked_bench.py [--rounds 15] [--warmup 8] [--res 3840x2160] [--bakes 5]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hm = importlib.import_module("heightmap-ray-marcher_amd")
from segments_bench import med  # noqa: E402

lib = importlib.import_module("heightmap-ray-marcher_amd.lib").lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--res", default="3840x2160")
    ap.add_argument("--bakes", type=int, default=5)
    args = ap.parse_args()
    import torch
    hm.set_device(0)
    wl = hm.synth.WORKLOADS["C3"]
    rgb, cmap = hm.synth.synth_maps(wl.map_size)
    params, cam = wl.scene_params(), wl.camera()
    cam.width, cam.height = (int(v) for v in args.res.split("x"))
    w, h = cam.width, cam.height
    scene = hm.Scene(rgb, cmap, params)
    sky = hm.sky_directions(4, 16)
    sun = hm.Sun.make((0.5, 0.5, 0.7071067811865476), cam.step_dist, ambient=64)

    # ---- the identity check, then the bake ----
    scene.set_light(np.full((scene.map_h, scene.map_w), 64, dtype=np.uint16), 64)
    identity = scene.render_baked(cam).tobytes() == scene.render(cam).tobytes()
    bake_ms = []
    for _ in range(args.bakes):
        t0 = time.perf_counter()
        scene.bake_light(sky, cam.step_dist, sampling=cam.sampling, ambient=64, allow_capped=True)
        bake_ms.append(1e3 * (time.perf_counter() - t0))
    plane, full_scale = scene.light()

    d_rgba = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    d_dirs = torch.from_numpy(sky).cuda()
    stream = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()

    def baked():
        scene.render_baked(cam)
        return float(lib.hmrm_last_kernel_ms())

    def plain():
        scene.render(cam)
        return float(lib.hmrm_last_kernel_ms())

    def shaded():
        scene.render_shaded(cam, sun, diffuse=True, shadows=False)
        return float(lib.hmrm_last_kernel_ms())

    def summed():
        with torch.cuda.stream(stream):
            e0.record(stream)
            scene.render_lit_sum_device(cam, sun, d_dirs.data_ptr(), len(sky), rgba=(d_rgba.data_ptr(), 4 * w), stream=stream.cuda_stream)
            e1.record(stream)
        e1.synchronize()
        return float(e0.elapsed_time(e1))

    runs = (("hmrm_render_baked", baked), ("hmrm_render", plain), ("hmrm_render_shaded(DIFFUSE | NO_SHADOWS)", shaded),
            ("hmrm_render_lit_sum_device, 64 directions", summed))
    ms = {name: [] for name, _ in runs}
    for k in range(args.warmup + args.rounds):
        for j in range(len(runs)):
            name, fn = runs[(j + k) % len(runs)]  # (the order rotates from round to round)
            v = fn()
            if k >= args.warmup:
                ms[name].append(v)
    for name, _ in runs:
        print(f"{name}: {med(ms[name])}", flush=True)
    for other in ("hmrm_render", "hmrm_render_shaded(DIFFUSE | NO_SHADOWS)"):
        ratios = sorted(a / b for a, b in zip(ms["hmrm_render_baked"], ms[other]))
        print(f"per-round ratio hmrm_render_baked / {other}: median {statistics.median(ratios):.4f} [{ratios[0]:.4f} .. {ratios[-1]:.4f}]")
    print(f"hmrm_scene_bake_light, 64 directions over {scene.map_w} x {scene.map_h} cells, wall: {med(bake_ms)}; full scale {full_scale}, "
          f"light {int(plane.min())} .. {int(plane.max())}; kernel {scene.kernel_choice()}; L = D everywhere is hmrm_render: {identity}")
    scene.take_capped(stream.cuda_stream, allow_capped=True)
    scene.close()
    print(json.dumps({"ms": ms, "bake_ms": bake_ms, "identity": identity}))


if __name__ == "__main__":
    main()
