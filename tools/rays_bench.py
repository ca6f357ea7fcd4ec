"""Ray batches (hmrm_trace_rays_device) against the frame launch of the same rays, on one box (tools only).

The rays of a camera (default: C3, 3840 x 2160 spherical over the 4096^2 map) are computed on the host from the library's
own per-frame record (hmrm_debug_frame: the products the kernel forms) and laid out in the frame kernel's WAVE ORDER --
batch rays 64 k .. 64 k + 63 are the 8 x 8 pixels of the frame's k-th wave -- so that the "coherent" batch gives every wave
the rays the frame launch gives it; the "incoherent" batch is the same rays permuted at random.  Each batch launch is
bracketed by HIP events on its stream and alternated with one plain launch of the frame (hmrm_bench_kernel_ms, one
iteration): --warmup launches of each first (they settle the frame's launch-order calibration and the scene's kernel probe),
then --pairs timed pairs.  A batch reads 48 B and writes 56 B per ray where the frame writes 4 B, computes distance() for
every ray (the frame proves most misses from sign bits) and keeps exact step counts.  Prints medians, rays/s and the
batch / frame ratio with its spread, the records' agreement with the frame (rgba against hmrm_render), and a JSON list.

    python tools/rays_bench.py [--pairs 9] [--warmup 8] [--workload C3] [--res 3840x2160]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hm = importlib.import_module("heightmap-ray-marcher_amd")


def camera_rays(cam, params, map_w, map_h):
    """GetRay for every pixel, row-major (H*W x 6), with the kernel's operations (csrc/device_common.hpp make_ray)."""
    rec = hm.debug_frame(cam, params, map_w, map_h)
    W, H = cam.width, cam.height
    out = np.empty((H, W, 6), dtype=np.float64)
    if cam.projection == hm.SPHERICAL:
        sva, cva = rec["row_sin_va"][:, None], rec["row_cos_va"][:, None]
        cha, sha = rec["col_cos_ha"][None, :], rec["col_sin_ha"][None, :]
        out[:, :, 0:3] = rec["cam"]
        out[:, :, 3] = sva * cha
        out[:, :, 4] = sva * sha
        out[:, :, 5] = cva + 0.0 * cha
        return out.reshape(-1, 6)
    w = (np.arange(W, dtype=np.float64) / np.float64(W - 1))[None, :]
    h = (np.arange(H, dtype=np.float64) / np.float64(H - 1))[:, None]
    o = [(rec["upper_left"][i] + w * rec["plane_right"][i]) + h * rec["plane_down"][i] for i in range(3)]
    if cam.projection == hm.PERSPECTIVE:
        v = [o[i] - rec["cam"][i] for i in range(3)]
        inv = 1.0 / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        out[:, :, 0:3] = rec["cam"]
        for i in range(3):
            out[:, :, 3 + i] = v[i] * inv
    else:
        for i in range(3):
            out[:, :, i] = o[i]
        out[:, :, 3:6] = rec["look"]
    return out.reshape(-1, 6)


def wave_order(W, H):
    """Pixel index (y * W + x) of batch ray i when the batch repeats the frame launch's waves: 8 x 8 pixels per wave, two
    waves (16 rows) per tile, tiles row by row."""
    assert W % 8 == 0 and H % 16 == 0, "whole tiles only"
    i = np.arange(W * H, dtype=np.int64)
    wave, lane = i // 64, i % 64
    tile, half = wave // 2, wave % 2
    tx, ty = tile % (W // 8), tile // (W // 8)
    x = tx * 8 + lane % 8
    y = ty * 16 + half * 8 + lane // 8
    return y * W + x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--workload", default="C3")
    ap.add_argument("--res", default="3840x2160")
    args = ap.parse_args()
    import torch
    hm.set_device(0)
    wl = hm.synth.WORKLOADS[args.workload]
    rgb, cmap = hm.synth.synth_maps(wl.map_size)
    params, cam = wl.scene_params(), wl.camera()
    cam.width, cam.height = (int(v) for v in args.res.split("x"))
    scene = hm.Scene(rgb, cmap, params)
    n = cam.width * cam.height
    order = wave_order(cam.width, cam.height)
    rays = camera_rays(cam, params, wl.map_size, wl.map_size)[order]
    perm = np.random.RandomState(1).permutation(n)
    frame = scene.render(cam).reshape(-1, 4)
    stream = torch.cuda.Stream()
    d_hits = torch.zeros(n * 56, dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    bg = (cam.bg_r, cam.bg_g, cam.bg_b)
    # what moving a batch's bytes costs by itself: a device copy of n * 52 bytes reads and writes as many bytes (104 per
    # ray) as the batch kernel reads rays (48) and writes records (56)
    src = torch.zeros(n * 52, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    io = []
    for _ in range(args.warmup + args.pairs):
        with torch.cuda.stream(stream):
            e0.record(stream)
            dst.copy_(src)
            e1.record(stream)
        e1.synchronize()
        io.append(float(e0.elapsed_time(e1)))
    io_ms = statistics.median(io[args.warmup:])
    del src, dst
    print(f"device copy of {n * 52} bytes (the batch's 104 bytes per ray of traffic): {io_ms:.4f} ms", flush=True)
    results = []
    for kind, r, pix in (("coherent (wave order)", rays, order), ("incoherent (permuted)", rays[perm], order[perm])):
        d_rays = torch.from_numpy(np.ascontiguousarray(r)).cuda()
        torch.cuda.synchronize()

        def batch_ms():
            with torch.cuda.stream(stream):
                e0.record(stream)
                scene.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), cam.step_dist, bg=bg, sampling=cam.sampling,
                                        stream=stream.cuda_stream)
                e1.record(stream)
            e1.synchronize()
            return float(e0.elapsed_time(e1))

        def frame_ms():
            return scene.bench_kernel_ms(cam, 1)

        for _ in range(args.warmup):
            batch_ms()
            frame_ms()
        a, b = [], []
        for k in range(args.pairs):  # alternate which of the two goes first
            if k % 2 == 0:
                a.append(batch_ms())
                b.append(frame_ms())
            else:
                b.append(frame_ms())
                a.append(batch_ms())
        assert scene.take_capped(stream.cuda_stream) == 0
        hits = d_hits.cpu().numpy().view(hm.RAY_HIT_DTYPE)
        same = bool(np.array_equal(hits["rgba"], frame[pix]))
        ratios = sorted(x / y for x, y in zip(a, b))
        ma, mb = statistics.median(a), statistics.median(b)
        res = {"case": f"{args.workload} {args.res} {kind}", "rays": n, "kernel_choice": scene.kernel_choice(), "batch_ms": round(ma, 4),
               "batch_ms_min": round(min(a), 4), "batch_ms_max": round(max(a), 4), "frame_ms": round(mb, 4),
               "frame_ms_min": round(min(b), 4), "frame_ms_max": round(max(b), 4), "batch_rays_per_s": n / (ma * 1e-3),
               "ratio_median": round(statistics.median(ratios), 4), "ratio_min": round(ratios[0], 4), "ratio_max": round(ratios[-1], 4),
               "steps": int(hits["steps"].sum(dtype=np.uint64)), "hits": int((hits["status"] == hm.RAY_HIT).sum()),
               "rgba_equals_frame": same, "copy_104_bytes_per_ray_ms": round(io_ms, 4), "pairs": args.pairs}
        results.append(res)
        print(f"{res['case']:>40}: batch {ma:.4f} ms [{min(a):.4f} .. {max(a):.4f}], frame {mb:.4f} ms [{min(b):.4f} .. {max(b):.4f}], "
              f"{res['batch_rays_per_s']:.3e} rays/s, batch/frame {res['ratio_median']:.3f} [{res['ratio_min']:.3f} .. {res['ratio_max']:.3f}], "
              f"rgba == frame: {same}, kernel {res['kernel_choice']}", flush=True)
        del d_rays
    scene.close()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
