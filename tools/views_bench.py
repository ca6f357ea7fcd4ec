"""View batches (hmrm_render_views_device: N cameras of one scene in one launch) against the routes they replace, on one box
(tools only).

Modelled on tools/water_bench.py.  C3's map (4096^2, its step) seen by N = 16, 64 and 256 cameras of 64 x 64, 128 x 128 and 256 x
256 pixels on C3's orbit (hmrm_orbit_camera: every camera has its own hang, so a spherical batch has N pairs of column tables
and one pair of row tables), spherical and perspective, all frames into one torch tensor of shape (N, H, W).  For each case
three routes are timed, alternated in the same process, --warmup rounds of each first, then --reps rounds; a median is printed
with its range:

  (a) one hmrm_render_views_device batch on a torch stream;
  (b) the best route without batches: N hmrm_render_device_begin tickets (HMRM_NO_PROBE), three in flight -- ticket i is begun,
      ticket i - 3 waited for;
  (c) N back-to-back hmrm_render_rows_device calls (whole frames) on one stream.

What is timed is WALL time from before the route's first call until its last frame is done (a stream synchronize, the last
tickets' waits): the host's share of N launches is what a batch saves, so events around the kernels would miss the point.  The
calls go straight to the C ABI through ctypes with cameras made beforehand (about 2 us of Python per call stay in (b) and (c)).
Repeated cameras find their cached records in (b) and (c) while N fits the 64 records a stream keeps; (a) builds its N records
in every call, and its host time per call -- the call's own duration, before the wait -- is printed beside it.  One frame of every
case is compared between (a) and (c), bytewise.

    python tools/views_bench.py [--reps 9] [--warmup 3] [--counts 16,64,256] [--sizes 64,128,256] [--json out.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hm = importlib.import_module("heightmap-ray-marcher_amd")
lib = importlib.import_module("heightmap-ray-marcher_amd.lib").lib


def med(v, scale=1.0):
    return f"{statistics.median(v) * scale:.2f} [{min(v) * scale:.2f} .. {max(v) * scale:.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--counts", default="16,64,256")
    ap.add_argument("--sizes", default="64,128,256")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import torch
    hm.set_device(0)
    wl = hm.synth.WORKLOADS["C3"]
    rgb, cmap = hm.synth.synth_maps(wl.map_size)
    scene = hm.Scene(rgb, cmap, wl.scene_params())
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    results = []
    print(f"per-view times in microseconds, wall clock, median [range] of {args.reps} rounds; map {wl.map_size}^2, step {wl.step_dist}")
    for proj, pname in ((hm.SPHERICAL, "spherical"), (hm.PERSPECTIVE, "perspective")):
        for side in (int(v) for v in args.sizes.split(",")):
            for n in (int(v) for v in args.counts.split(",")):
                cams = []
                for k in range(n):
                    c = wl.camera(k, max(n, 2))
                    c.width, c.height, c.projection = side, side, proj
                    if proj == hm.PERSPECTIVE:
                        c.hfov = hm.degrees_to_rads(90.0)
                    cams.append(c)
                arr, _ = hm.camera_array(cams)
                refs = [C.byref(arr[k]) for k in range(n)]
                out = torch.zeros((n, side, side), dtype=torch.int32, device="cuda")
                ptrs = [C.c_void_p(out.data_ptr() + k * side * side * 4) for k in range(n)]
                base, stride, vstride = C.c_void_p(out.data_ptr()), side * 4, side * side * 4
                host_a = []

                def route_a():
                    t0 = time.perf_counter()
                    rc = lib.hmrm_render_views_device(scene._h, arr, n, 0, base, stride, vstride, sp)
                    t1 = time.perf_counter()
                    stream.synchronize()
                    t2 = time.perf_counter()
                    assert rc == 0, hm.last_error()
                    host_a.append(t1 - t0)
                    return t2 - t0

                def route_b():
                    tickets = []
                    t = C.c_int32()
                    t0 = time.perf_counter()
                    for k in range(n):
                        rc = lib.hmrm_render_device_begin_flags(scene._h, refs[k], ptrs[k], stride, hm.NO_PROBE, C.byref(t))
                        assert rc == 0, hm.last_error()
                        tickets.append(t.value)
                        if k >= 3:
                            lib.hmrm_render_device_wait(scene._h, tickets[k - 3])
                    for k in range(max(n - 3, 0), n):
                        lib.hmrm_render_device_wait(scene._h, tickets[k])
                    return time.perf_counter() - t0

                def route_c():
                    t0 = time.perf_counter()
                    for k in range(n):
                        rc = lib.hmrm_render_rows_device(scene._h, refs[k], ptrs[k], stride, 0, side, 0, 0, 1, sp)
                        assert rc == 0, hm.last_error()
                    stream.synchronize()
                    return time.perf_counter() - t0

                routes = (route_a, route_b, route_c)
                for _ in range(args.warmup):
                    for r in routes:
                        r()
                host_a.clear()
                times = ([], [], [])
                for rep in range(args.reps):  # (rotate which route goes first)
                    for j in range(3):
                        i = (rep + j) % 3
                        times[i].append(routes[i]())
                # one comparison, bytewise: the batch against the N single frames
                route_c()
                singles = out.cpu().numpy().copy()
                out.zero_()
                route_a()
                same = bool((out.cpu().numpy() == singles).all())
                scene.take_capped(stream.cuda_stream, allow_capped=True)
                per = [[t / n for t in ts] for ts in times]
                a, b, c = (statistics.median(p) for p in per)
                print(f"{pname:11s} {side:3d} x {side:<3d} N {n:3d}: (a) batch {med(per[0], 1e6)}  (b) tickets {med(per[1], 1e6)}  (c) rows calls "
                      f"{med(per[2], 1e6)}  a/b {a / b:.2f}  a/c {a / c:.2f}  (a) host per call {med(host_a, 1e6)} us = "
                      f"{statistics.median(host_a) / n * 1e6:.2f} us per view; same frames: {same}", flush=True)
                results.append({"projection": pname, "side": side, "n": n, "batch_s": times[0], "tickets_s": times[1], "rows_s": times[2],
                                "batch_host_s": list(host_a), "same": same})
                del out
    scene.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f)


if __name__ == "__main__":
    main()
