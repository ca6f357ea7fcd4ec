"""Antialiased launches (hmrm_render_aa) against plain launches of their super frames, on one box (tools only).

Each case renders a W x H frame with factor n and, alternately, the plain nW x nH frame of the same camera: both are one
launch bracketed by HIP events on the scene's stream (hmrm_last_kernel_ms after hmrm_render_aa; hmrm_bench_kernel_ms
with one iteration for the plain frame, which stays on the device -- a 4K frame at n = 8 is 2.1 GB).  Both kinds share
the super camera's launch-order calibration; --warmup launches of each settle it before the --pairs timed A/B pairs.
Prints one line per case (medians, samples/s, the antialiased / plain ratio and its spread over the pairs) and a JSON
list at the end.

    python tools/aa_bench.py [--pairs 9] [--warmup 8] [--cases C2:960x540:2,C3:1920x1080:2,...]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hm = importlib.import_module("heightmap-ray-marcher_amd")

DEFAULT_CASES = "C2:960x540:2,C3:1920x1080:2,C3:3840x2160:2,C3:3840x2160:4,C3:3840x2160:8"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--cases", default=DEFAULT_CASES)
    args = ap.parse_args()
    hm.set_device(0)
    scenes = {}
    results = []
    for spec in args.cases.split(","):
        name, res, n = spec.split(":")
        w, h = (int(v) for v in res.split("x"))
        n = int(n)
        wl = hm.synth.WORKLOADS[name]
        if name not in scenes:
            for s in scenes.values():
                s.close()
            rgb, cmap = hm.synth.synth_maps(wl.map_size)
            scenes = {name: hm.Scene(rgb, cmap, wl.scene_params())}
        scene = scenes[name]
        cam = wl.camera()
        cam.width, cam.height = w, h
        sup = hm.Camera.from_buffer_copy(cam)
        sup.width, sup.height = w * n, h * n
        lib = importlib.import_module("heightmap-ray-marcher_amd.lib").lib

        def aa_ms():
            scene.render_aa(cam, n)
            return float(lib.hmrm_last_kernel_ms())

        def plain_ms():
            return scene.bench_kernel_ms(sup, 1)

        for _ in range(args.warmup):
            aa_ms()
            plain_ms()
        a, b = [], []
        for k in range(args.pairs):  # alternate which of the two goes first
            if k % 2 == 0:
                a.append(aa_ms())
                b.append(plain_ms())
            else:
                b.append(plain_ms())
                a.append(aa_ms())
        ratios = sorted(x / y for x, y in zip(a, b))
        samples = n * n * w * h
        ma, mb = statistics.median(a), statistics.median(b)
        r = {"case": f"{name} {w}x{h} n={n}", "super": f"{w * n}x{h * n}", "samples": samples, "aa_ms": round(ma, 4),
             "plain_ms": round(mb, 4), "aa_samples_per_s": samples / (ma * 1e-3), "plain_samples_per_s": samples / (mb * 1e-3),
             "ratio_median": round(statistics.median(ratios), 4), "ratio_min": round(ratios[0], 4),
             "ratio_max": round(ratios[-1], 4), "pairs": args.pairs}
        results.append(r)
        print(f"{r['case']:>24} (super {r['super']}): aa {ma:.4f} ms, plain {mb:.4f} ms, "
              f"{r['aa_samples_per_s']:.3e} samples/s, aa/plain {r['ratio_median']:.3f} "
              f"[{r['ratio_min']:.3f} .. {r['ratio_max']:.3f}]", flush=True)
    for s in scenes.values():
        s.close()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
