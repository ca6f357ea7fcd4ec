"""Segment batches and interior frames (hmrm_trace_segments_device, hmrm_render_interior) on one box (tools only).

Modelled on tools/rays_bench.py, whose rays it uses: the C3 camera's (3840 x 2160 spherical over the 4096^2 map) in the
frame kernel's wave order ("coherent") and permuted at random.  Every launch is timed by HIP events on its stream, the
candidates of a comparison alternate in the same process, --warmup launches of each come first, and a median is printed
with its range.

  (b) rules off: hmrm_trace_segments_device with flags = 0 and no limit against hmrm_trace_rays_device, same batch.
  (c) the interior rule and a limit: the same camera moved INSIDE the box (x, y mirrored into the map, z = 0.9 max_height),
      every ray interior, max_steps = --limit; rays/s.
  (d) an interior frame: hmrm_render_interior of that camera against hmrm_render of the same camera lifted just above
      max_height (hmrm_last_kernel_ms: events around the kernel launch), ms per frame and their ratio.

    python tools/segments_bench.py [--pairs 9] [--warmup 8] [--limit 64] [--res 3840x2160]
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

lib = importlib.import_module("heightmap-ray-marcher_amd.lib").lib


def med(v):
    return f"{statistics.median(v):.4f} ms [{min(v):.4f} .. {max(v):.4f}]"


def alternate(fa, fb, warmup, pairs):
    for _ in range(warmup):
        fa()
        fb()
    a, b = [], []
    for k in range(pairs):  # alternate which of the two goes first
        if k % 2 == 0:
            a.append(fa())
            b.append(fb())
        else:
            b.append(fb())
            a.append(fa())
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--limit", type=int, default=64)
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
    order = rays_bench.wave_order(cam.width, cam.height)
    perm = np.random.RandomState(1).permutation(n)
    stream = torch.cuda.Stream()
    d_hits = torch.zeros(n * 56, dtype=torch.uint8, device="cuda")
    d_hits2 = torch.zeros(n * 56, dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    bg = (cam.bg_r, cam.bg_g, cam.bg_b)
    results = []

    def timed(fn):
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        e1.synchronize()
        return float(e0.elapsed_time(e1))

    # ---- (b) rules off against hmrm_trace_rays ----
    rays = rays_bench.camera_rays(cam, params, wl.map_size, wl.map_size)[order]
    for kind, r in (("coherent", rays), ("permuted", rays[perm])):
        d_rays = torch.from_numpy(np.ascontiguousarray(r)).cuda()
        torch.cuda.synchronize()
        seg = lambda: timed(lambda: scene.trace_segments_device(d_rays.data_ptr(), n, d_hits.data_ptr(), cam.step_dist, bg=bg,
                                                                stream=stream.cuda_stream))
        ray = lambda: timed(lambda: scene.trace_rays_device(d_rays.data_ptr(), n, d_hits2.data_ptr(), cam.step_dist, bg=bg,
                                                            stream=stream.cuda_stream))
        a, b = alternate(seg, ray, args.warmup, args.pairs)
        same = bool(torch.equal(d_hits, d_hits2))
        ratios = sorted(x / y for x, y in zip(a, b))
        print(f"(b) rules off, {kind}: trace_segments {med(a)}, trace_rays {med(b)}, ratio {statistics.median(ratios):.3f} "
              f"[{ratios[0]:.3f} .. {ratios[-1]:.3f}], records equal: {same}", flush=True)
        results.append({"case": f"b {kind}", "segments_ms": a, "rays_ms": b, "records_equal": same})
        del d_rays
    # ---- (c) interior rays with a limit ----
    s = float(wl.map_size) * wl.grid_width
    inside = hm.Camera.from_buffer_copy(cam)
    inside.pos[0], inside.pos[1], inside.pos[2] = s / 8.0, -s / 8.0, 0.9 * params.max_height
    above = hm.Camera.from_buffer_copy(inside)
    above.pos[2] = params.max_height * 1.001
    irays = rays_bench.camera_rays(inside, params, wl.map_size, wl.map_size)[order]
    for kind, r in (("coherent", irays), ("permuted", irays[perm])):
        d_rays = torch.from_numpy(np.ascontiguousarray(r)).cuda()
        torch.cuda.synchronize()
        for what, lim in (("no limit", 0), (f"max_steps {args.limit}", args.limit)):
            f = lambda: timed(lambda: scene.trace_segments_device(d_rays.data_ptr(), n, d_hits.data_ptr(), cam.step_dist, bg=bg,
                                                                  interior=True, max_steps=lim, stream=stream.cuda_stream))
            for _ in range(args.warmup):
                f()
            a = [f() for _ in range(args.pairs)]
            capped = scene.take_capped(stream.cuda_stream, allow_capped=True)
            hits = d_hits.cpu().numpy().view(hm.RAY_HIT_DTYPE)
            st = np.bincount(hits["status"], minlength=4).tolist()
            print(f"(c) interior rays, {kind}, {what}: {med(a)}, {n / (statistics.median(a) * 1e-3):.3e} rays/s, "
                  f"steps {int(hits['steps'].sum(dtype=np.uint64))}, miss/hit/capped/end {st}, capped counted {capped}", flush=True)
            results.append({"case": f"c {kind} {what}", "ms": a, "status": st})
        del d_rays
    # ---- (d) an interior frame ----
    def frame_ms(fn, c):
        fn(c)
        return float(lib.hmrm_last_kernel_ms())

    fi = lambda: frame_ms(lambda c: scene.render_interior(c, allow_capped=True), inside)
    fo = lambda: frame_ms(scene.render, above)
    a, b = alternate(fi, fo, args.warmup, args.pairs)
    ratios = sorted(x / y for x, y in zip(a, b))
    fb = scene.render_interior(inside, allow_capped=True).reshape(-1, 4)
    sky = scene.render(inside).reshape(-1, 4)
    print(f"(d) interior frame {med(a)}; the camera lifted above max_height, hmrm_render {med(b)}; ratio "
          f"{statistics.median(ratios):.3f} [{ratios[0]:.3f} .. {ratios[-1]:.3f}]; pixels that differ from hmrm_render of the "
          f"inside camera: {int((fb != sky).any(axis=1).sum())} of {n}; kernel {scene.kernel_choice()}", flush=True)
    results.append({"case": "d", "interior_ms": a, "above_ms": b})
    scene.close()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
