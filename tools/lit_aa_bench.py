"""Antialiased lit frames (hmrm_render_shaded_aa) against hmrm_render_shaded of their super frames, on one box (tools only).

Modelled on tools/aa_bench.py and tools/lit_bench.py: C3's content -- the spherical camera over the 4096^2 map -- with the sun
at --elevation degrees (default 30), azimuth --azimuth (default 40), shadow step_dist = the camera's.  Each case renders a
W x H frame with factor n and, alternately, the shaded nW x nH frame of the same camera -- the comparison launch is the
non-antialiased kernel, the antialiased one marches the same samples and filters them in the launch.  Both are one launch
bracketed by HIP events on the scene's stream (hmrm_last_kernel_ms); --warmup launches of each come first, then --pairs timed
A/B pairs that alternate which of the two goes first.  With shadows and without (HMRM_SHADE_NO_SHADOWS).  Prints one line
per case (median ms of both with their ranges, the median and range of the per-pair ratio) and a JSON list at the end.

--record N: also the rate of a recorded orbit, N frames at C5's size (3840 x 2160 perspective over the 4096^2 map) through
hmrm_record_orbit_shaded into a temporary directory: plain and shaded with shadows, each without and with HMRM_AA(2);
frames/s, PNG encoding included.

    python tools/lit_aa_bench.py [--pairs 9] [--warmup 8] [--cases 1920x1080:2,3840x2160:2,3840x2160:4] [--record 32]
"""
import argparse
import importlib
import json
import math
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hm = importlib.import_module("heightmap-ray-marcher_amd")
from segments_bench import alternate, med  # noqa: E402

lib = importlib.import_module("heightmap-ray-marcher_amd.lib").lib

DEFAULT_CASES = "1920x1080:2,3840x2160:2,3840x2160:4"


def sun_direction(elevation, azimuth):
    el, az = math.radians(elevation), math.radians(azimuth)
    return (math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el))


def record_rates(sun_dir, frames, results):
    wl = hm.synth.WORKLOADS["C5"]
    rgb, cmap = hm.synth.synth_maps(wl.map_size)
    params, base = wl.scene_params(), wl.camera()
    scene = hm.Scene(rgb, cmap, params)
    sun = hm.Sun.make(sun_dir, base.step_dist, ambient=96)
    s = wl.map_size * params.grid_width
    orbit = (s / 2.0, -s / 2.0, 0.9 * s, hm.degrees_to_rads(-45.0))
    for name, the_sun in (("plain", None), ("shaded + shadows", sun)):
        for aa in (1, 2):
            out = tempfile.mkdtemp(prefix="lit_aa_bench_")
            try:
                hm.record_orbit_shaded([scene], base, *orbit, 4, out, 1, the_sun, aa=aa)  # (warm-up: the ring, the encoders)
                t0 = time.perf_counter()
                hm.record_orbit_shaded([scene], base, *orbit, frames, out, 2, the_sun, aa=aa)
                dt = time.perf_counter() - t0
            finally:
                shutil.rmtree(out, ignore_errors=True)
            print(f"record orbit, {frames} frames {base.width}x{base.height}, {name}, antialias {aa}: {frames / dt:.2f} frames/s "
                  f"({dt:.2f} s)", flush=True)
            results.append({"case": f"record {name} aa={aa}", "frames": frames, "seconds": dt, "frames_per_s": frames / dt})
    scene.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--elevation", type=float, default=30.0)
    ap.add_argument("--azimuth", type=float, default=40.0)
    ap.add_argument("--cases", default=DEFAULT_CASES)
    ap.add_argument("--record", type=int, default=0)
    args = ap.parse_args()
    hm.set_device(0)
    wl = hm.synth.WORKLOADS["C3"]
    rgb, cmap = hm.synth.synth_maps(wl.map_size)
    scene = hm.Scene(rgb, cmap, wl.scene_params())
    sun_dir = sun_direction(args.elevation, args.azimuth)
    results = []
    for spec in args.cases.split(","):
        res, n = spec.split(":")
        w, h = (int(v) for v in res.split("x"))
        n = int(n)
        cam = wl.camera()
        cam.width, cam.height = w, h
        sup = hm.Camera.from_buffer_copy(cam)
        sup.width, sup.height = w * n, h * n
        sun = hm.Sun.make(sun_dir, cam.step_dist, ambient=96)
        for shadows in (True, False):
            def aa_ms():
                scene.render_shaded(cam, sun, shadows=shadows, aa=n)
                return float(lib.hmrm_last_kernel_ms())

            def super_ms():
                scene.render_shaded(sup, sun, shadows=shadows)
                return float(lib.hmrm_last_kernel_ms())

            a, b = alternate(aa_ms, super_ms, args.warmup, args.pairs)
            ratios = sorted(x / y for x, y in zip(a, b))
            r = {"case": f"C3 {w}x{h} n={n} shadows={'on' if shadows else 'off'}", "super": f"{w * n}x{h * n}", "aa_ms": a, "super_ms": b,
                 "ratio_median": statistics.median(ratios), "ratio_min": ratios[0], "ratio_max": ratios[-1], "kernel": scene.kernel_choice()}
            results.append(r)
            print(f"{r['case']:>36} (super {r['super']}): antialiased {med(a)}; shaded super frame {med(b)}; ratio "
                  f"{r['ratio_median']:.3f} [{ratios[0]:.3f} .. {ratios[-1]:.3f}]; kernel {r['kernel']}", flush=True)
    scene.close()
    if args.record > 0:
        record_rates(sun_dir, args.record, results)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
