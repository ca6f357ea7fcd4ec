"""Haze frames (hmrm_render_haze, hmrm_render_haze_device: distance fog blended by the render kernel) on one box (tools only).

Modelled on tools/geometry_bench.py: C3's content and camera -- the 4096^2 map and the 3840 x 2160 spherical camera of bench.py.
Every candidate is timed by HIP events on one stream, the two candidates of a comparison alternate in the same process, --warmup
launches of each come first, and a median is printed with its range.  The haze is picked from the frame itself: start and far the
10th and 90th percentile of the hit ranges (one geometry frame, not timed), 256 entries of the EXP law at density 3, the sky hazed.

  (A) the haze frame against hmrm_render_interior of the PARENT commit's library (--parent-lib: its libhmrm.so, loaded beside this
      build's; without it this build's own, whose interior kernels are the parent's instruction for instruction) for the same
      camera.  Both are launched the same way -- one launch in the plain rotation, the scene's current kernel -- and both are read
      as hmrm_last_kernel_ms reports them: HIP events around the launch inside the host entry.  The haze frame's device entry,
      timed by this tool's own events, is printed beside them.
  (B) the haze frame (device entry) against the two-pass route it replaces: hmrm_render_geometry_device with
      the rgba and range planes, then the composite in torch on the same stream -- eager elementwise operations, several launches,
      what a caller has without writing a kernel.  That route fogs by the float-rounded range: the tool counts the pixels that
      differ from the haze frame.
  (C) the haze frame at factor 2 against the parent's hmrm_render_aa at factor 2, both as hmrm_last_kernel_ms reports them.

    python tools/haze_bench.py [--pairs 9] [--warmup 24] [--parent-lib path/to/parent/libhmrm.so]
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

COLOR = (200, 210, 220)
ENTRIES = 256


class ParentLib:
    """The few entry points of another build's libhmrm.so that the comparisons need (the ABI is additive: same structs)."""

    def __init__(self, path, rgb, cmap, params):
        self.lib = C.CDLL(path)
        vp = C.c_void_p
        self.lib.hmrm_scene_create.argtypes = [vp, vp, C.c_int32, C.c_int32, C.POINTER(hm.SceneParams), C.POINTER(vp)]
        self.lib.hmrm_render_interior.argtypes = [vp, C.POINTER(hm.Camera), vp, C.c_size_t]
        self.lib.hmrm_render_aa.argtypes = [vp, C.POINTER(hm.Camera), C.c_int32, vp, C.c_size_t, vp]
        self.lib.hmrm_last_kernel_ms.restype = C.c_double
        self.lib.hmrm_scene_destroy.argtypes = [vp]
        self.lib.hmrm_scene_destroy.restype = None
        self.h = vp()
        rc = self.lib.hmrm_scene_create(rgb.ctypes.data, cmap.ctypes.data, rgb.shape[1], rgb.shape[0], C.byref(params), C.byref(self.h))
        assert rc == 0, rc

    def interior_kernel_ms(self, cam, host_frame):
        assert self.lib.hmrm_render_interior(self.h, C.byref(cam), host_frame.ctypes.data, cam.width * 4) in (0, hm.HMRM_E_NOTERM)
        return float(self.lib.hmrm_last_kernel_ms())

    def aa_kernel_ms(self, cam, factor, host_frame):
        assert self.lib.hmrm_render_aa(self.h, C.byref(cam), factor, host_frame.ctypes.data, cam.width * 4, None) in (0, hm.HMRM_E_NOTERM)
        return float(self.lib.hmrm_last_kernel_ms())

    def close(self):
        self.lib.hmrm_scene_destroy(self.h)


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
    d_haze = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    d_rgba = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    d_range = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    d_out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
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

    # the haze of this frame, from its own ranges
    scene.render_geometry_device(cam, range=(d_range.data_ptr(), W * 4), stream=stream.cuda_stream)
    scene.take_capped(stream.cuda_stream, allow_capped=True)
    rng = d_range.cpu().numpy().reshape(-1).astype(np.float64)
    hit = np.isfinite(rng)
    start, far = float(np.percentile(rng[hit], 10)), float(np.percentile(rng[hit], 90))
    haze = hm.Haze.make(start, far, ENTRIES, COLOR, sky=True)
    table = hm.haze_table(hm.HAZE_EXP, 3.0, ENTRIES)
    d_table = torch.from_numpy(table).cuda()
    t_table = d_table.to(torch.int32)
    t_color = torch.tensor(COLOR, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    print(f"C3: {int(hit.sum())} of {hit.size} pixels hit; haze from {start:.4f} to {far:.4f}, {ENTRIES} entries, kernel {scene.kernel_choice()}", flush=True)

    def haze_host_kernel_ms(factor=1):
        scene.render_haze(cam, haze, table, factor=factor, allow_capped=True)
        return float(hm.lib.lib.hmrm_last_kernel_ms())

    haze_device = timed(lambda: scene.render_haze_device(cam, haze, d_table.data_ptr(), d_haze.data_ptr(), W * 4, stream=stream.cuda_stream))

    def composite():
        """The two-pass route: the geometry frame's two planes, then the fog in eager torch."""
        scene.render_geometry_device(cam, rgba=(d_rgba.data_ptr(), W * 4), range=(d_range.data_ptr(), W * 4), stream=stream.cuda_stream)
        u = torch.nan_to_num((d_range.to(torch.float64) - start) * float(haze.scale), nan=0.0, posinf=float(ENTRIES - 1))
        f = t_table[u.clamp_(0.0, float(ENTRIES - 1)).to(torch.int64)].unsqueeze(-1)
        c = d_rgba.view(torch.uint8).reshape(H, W, 4)[:, :, :3].to(torch.int32)
        d_out[:, :, :3] = torch.div(c * (255 - f) + t_color * f + 127, 255, rounding_mode="floor").to(torch.uint8)
        d_out[:, :, 3] = 255

    if parent:
        interior = lambda: parent.interior_kernel_ms(cam, host_frame)
        aa2 = lambda: parent.aa_kernel_ms(cam, 2, host_frame)
    else:
        interior = lambda: (scene.render_interior(cam, allow_capped=True), float(hm.lib.lib.hmrm_last_kernel_ms()))[1]
        aa2 = lambda: (scene.render_aa(cam, 2, allow_capped=True), float(hm.lib.lib.hmrm_last_kernel_ms()))[1]
    whose = "the parent's" if parent else "this build's"

    h_ms, i_ms = alternate(haze_host_kernel_ms, interior, args.warmup, args.pairs)
    print(f"(A) haze frame (kernel) {med(h_ms)}; {whose} hmrm_render_interior (kernel) {med(i_ms)}", flush=True)
    results.append({"case": "A", "haze_ms": h_ms, "interior_ms": i_ms})
    d_ms, i2_ms = alternate(haze_device, interior, args.warmup, args.pairs)
    print(f"(A) haze frame, device entry (events of this tool) {med(d_ms)}; {whose} hmrm_render_interior (kernel) {med(i2_ms)}", flush=True)
    results.append({"case": "A-device", "haze_ms": d_ms, "interior_ms": i2_ms})

    d_ms, t_ms = alternate(haze_device, timed(composite), args.warmup, args.pairs)
    stream.synchronize()
    differ = int((d_out.view(torch.int32).reshape(H, W) != d_haze).sum().item())
    print(f"(B) haze frame, device entry {med(d_ms)} ({4 * W * H / 1e6:.0f} MB out); geometry frame rgba + range, then the composite in eager torch "
          f"{med(t_ms)}; pixels of the two routes that differ (float-rounded range): {differ} of {W * H}", flush=True)
    results.append({"case": "B", "haze_ms": d_ms, "two_pass_ms": t_ms, "differ": differ})

    h2_ms, a2_ms = alternate(lambda: haze_host_kernel_ms(2), aa2, max(4, args.warmup // 4), args.pairs)
    print(f"(C) haze frame at factor 2 (kernel) {med(h2_ms)}; {whose} hmrm_render_aa at factor 2 (kernel) {med(a2_ms)}", flush=True)
    results.append({"case": "C", "haze_ms": h2_ms, "aa_ms": a2_ms})
    scene.take_capped(stream.cuda_stream, allow_capped=True)
    if parent:
        parent.close()
    scene.close()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
