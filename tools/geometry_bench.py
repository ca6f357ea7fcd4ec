"""Geometry frames (hmrm_render_geometry_device: colour, hit cell, range and slope planes from one launch) on one box (tools only).

Modelled on tools/cell_sum_bench.py: C3's content and camera -- the 4096^2 map and the 3840 x 2160 spherical camera of bench.py.
Every candidate is timed by HIP events on one stream, the two candidates of a comparison alternate in the same process,
--warmup launches of each come first, and a median is printed with its range.

  (A) the geometry frame with the rgba plane alone, with each other plane added to it, and with all four, each against
      hmrm_render_rows_device (the whole frame) of the PARENT commit's library (--parent-lib: its libhmrm.so, loaded beside this
      build's; without it this build's own, whose plain kernels are the parent's instruction for instruction).  A plain frame of a
      repeated camera runs in its calibrated launch order, a geometry frame in the plain rotation, like an interior frame: the
      difference includes that.
  (B) the same geometry frames against the parent's hmrm_render_interior of the same camera, which is launched the way a
      geometry frame is: its kernel time as hmrm_last_kernel_ms reports it (HIP events around the launch), alternated with
      the geometry frame's.
  (C) all four planes against the route a user had without them (recipe 1): hmrm_trace_rays_device over the
      frame's 8.3 M camera rays, 48 B of ray in and 56 B of record out per pixel; building the rays and deriving the planes from
      the records is NOT timed, which favours that route.  The tool checks that the cell plane is the records'.

    python tools/geometry_bench.py [--pairs 9] [--warmup 24] [--parent-lib path/to/parent/libhmrm.so]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hm = importlib.import_module("heightmap-ray-marcher_amd")
from segments_bench import alternate, med  # noqa: E402


class ParentLib:
    """The few entry points of another build's libhmrm.so that the comparisons need (the ABI is additive: same structs)."""

    def __init__(self, path, rgb, cmap, params):
        self.lib = C.CDLL(path)
        vp = C.c_void_p
        self.lib.hmrm_scene_create.argtypes = [vp, vp, C.c_int32, C.c_int32, C.POINTER(hm.SceneParams), C.POINTER(vp)]
        self.lib.hmrm_render_rows_device.argtypes = [vp, C.POINTER(hm.Camera), vp, C.c_size_t] + [C.c_int32] * 5 + [vp]
        self.lib.hmrm_render_interior.argtypes = [vp, C.POINTER(hm.Camera), vp, C.c_size_t]
        self.lib.hmrm_last_kernel_ms.restype = C.c_double
        self.lib.hmrm_scene_destroy.argtypes = [vp]
        self.lib.hmrm_scene_destroy.restype = None
        self.h = vp()
        rc = self.lib.hmrm_scene_create(rgb.ctypes.data, cmap.ctypes.data, rgb.shape[1], rgb.shape[0], C.byref(params), C.byref(self.h))
        assert rc == 0, rc

    def rows_device(self, cam, d_ptr, stride, stream):
        assert self.lib.hmrm_render_rows_device(self.h, C.byref(cam), d_ptr, stride, 0, cam.height, 0, 0, 1, stream) == 0

    def interior_kernel_ms(self, cam, host_frame):
        assert self.lib.hmrm_render_interior(self.h, C.byref(cam), host_frame.ctypes.data, cam.width * 4) in (0, hm.HMRM_E_NOTERM)
        return float(self.lib.hmrm_last_kernel_ms())

    def close(self):
        self.lib.hmrm_scene_destroy(self.h)


def camera_rays(cam, params, size):
    """GetRay of every pixel of a spherical camera from the frame record's own tables (Spherical.cpp:23-25) -> (H * W, 6)."""
    assert cam.projection == hm.SPHERICAL
    rec = hm.debug_frame(cam, params, size, size)
    W, H = cam.width, cam.height
    cha, sha, sva, cva = rec["col_cos_ha"], rec["col_sin_ha"], rec["row_sin_va"], rec["row_cos_va"]
    rays = np.empty((H, W, 6), dtype=np.float64)
    rays[:, :, 0:3] = np.asarray(rec["cam"])
    rays[:, :, 3] = sva[:, None] * cha[None, :]
    rays[:, :, 4] = sva[:, None] * sha[None, :]
    rays[:, :, 5] = cva[:, None]
    return rays.reshape(-1, 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--parent-lib", default="")
    args = ap.parse_args()
    import torch
    hm.set_device(0)
    wl = hm.synth.WORKLOADS["C3"]
    rgb, cmap = hm.synth.synth_maps(wl.map_size)
    params, cam = wl.scene_params(), wl.camera()
    scene = hm.Scene(rgb, cmap, params)
    parent = ParentLib(args.parent_lib, rgb, cmap, params) if args.parent_lib else None
    W, H = cam.width, cam.height
    d = dict(rgba=torch.zeros((H, W), dtype=torch.int32, device="cuda"), cell=torch.zeros((H, W), dtype=torch.int32, device="cuda"),
             range=torch.zeros((H, W), dtype=torch.float32, device="cuda"), slope=torch.zeros((H, W, 2), dtype=torch.float32, device="cuda"))
    d_plain = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    host_frame = np.zeros((H, W, 4), dtype=np.uint8)
    stream = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    results = []

    def timed(fn):
        def run():
            with torch.cuda.stream(stream):
                e0.record(stream)
                fn()
                e1.record(stream)
            e1.synchronize()
            return float(e0.elapsed_time(e1))
        return run

    def geometry(names):
        kw = {k: (d[k].data_ptr(), W * (8 if k == "slope" else 4)) for k in names}
        return timed(lambda: scene.render_geometry_device(cam, stream=stream.cuda_stream, **kw))

    if parent:
        plain = timed(lambda: parent.rows_device(cam, d_plain.data_ptr(), W * 4, stream.cuda_stream))
        interior = lambda: parent.interior_kernel_ms(cam, host_frame)
    else:
        plain = timed(lambda: scene.render_rows_device(cam, d_plain.data_ptr(), W * 4, 0, H, stream=stream.cuda_stream))
        interior = lambda: (scene.render_interior(cam, allow_capped=True), float(hm.lib.hmrm_last_kernel_ms()))[1]
    whose = "the parent's" if parent else "this build's"
    sets = (("rgba",), ("rgba", "cell"), ("rgba", "range"), ("rgba", "slope"), ("rgba", "cell", "range", "slope"))
    for names in sets:
        g_ms, p_ms = alternate(geometry(names), plain, args.warmup, args.pairs)
        print(f"(A) geometry frame {'+'.join(names)} {med(g_ms)}; {whose} hmrm_render_rows_device {med(p_ms)}; kernel {scene.kernel_choice()}", flush=True)
        results.append({"case": "A", "planes": names, "geometry_ms": g_ms, "plain_ms": p_ms})
    assert torch.equal(d["rgba"], d_plain), "the rgba plane is not the plain frame"
    for names in sets:
        g_ms, i_ms = alternate(geometry(names), interior, args.warmup, args.pairs)
        print(f"(B) geometry frame {'+'.join(names)} {med(g_ms)}; {whose} hmrm_render_interior (kernel) {med(i_ms)}", flush=True)
        results.append({"case": "B", "planes": names, "geometry_ms": g_ms, "interior_ms": i_ms})

    rays = camera_rays(cam, params, wl.map_size)
    n = rays.shape[0]
    d_rays = torch.from_numpy(rays).cuda()
    d_hits = torch.zeros((n, 56), dtype=torch.uint8, device="cuda")
    del rays
    torch.cuda.synchronize()
    by_hand = timed(lambda: scene.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), cam.step_dist, bg=(cam.bg_r, cam.bg_g, cam.bg_b),
                                                    sampling=cam.sampling, stream=stream.cuda_stream))
    g_ms, r_ms = alternate(geometry(sets[-1]), by_hand, args.warmup, args.pairs)
    hits = d_hits.cpu().numpy().view(hm.RAY_HIT_DTYPE).reshape(-1)
    cell = np.where(hits["status"] == hm.RAY_HIT, hits["cell_y"].astype(np.int64) * wl.map_size + hits["cell_x"], -1)
    agree = bool(np.array_equal(cell, d["cell"].cpu().numpy().reshape(-1)))
    print(f"(C) geometry frame, all four planes {med(g_ms)} ({20 * n / 1e6:.0f} MB out); hmrm_trace_rays_device over {n} camera rays {med(r_ms)} "
          f"({48 * n / 1e6:.0f} MB in, {56 * n / 1e6:.0f} MB out); the cell plane is the records': {agree}", flush=True)
    results.append({"case": "C", "geometry_ms": g_ms, "trace_rays_ms": r_ms, "agree": agree})
    scene.take_capped(stream.cuda_stream, allow_capped=True)
    if parent:
        parent.close()
    scene.close()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
