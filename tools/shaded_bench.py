"""Hill-shaded frames (hmrm_render_shaded: diffuse sun shading in the render kernel) on one box (tools only).

Modelled on tools/lit_bench.py: C3's content -- the 3840 x 2160 spherical camera over the 4096^2 map -- with the sun at
--elevation degrees (default 30), ambient 96.  Every launch is timed by HIP events (hmrm_last_kernel_ms: events around the
kernel launch), the candidates of a comparison alternate in the same process, --warmup launches of each come first, and a
median is printed with its range.

  (a) HMRM_SHADE_DIFFUSE | HMRM_SHADE_NO_SHADOWS against hmrm_render of the same camera: what hill shading alone costs.
  (b) HMRM_SHADE_DIFFUSE against hmrm_render_lit: what it costs on top of the shadow rays.

    python tools/shaded_bench.py [--pairs 9] [--warmup 8] [--elevation 30] [--azimuth 40] [--res 3840x2160]
"""
import argparse
import importlib
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hm = importlib.import_module("heightmap-ray-marcher_amd")
from segments_bench import alternate, med  # noqa: E402

lib = importlib.import_module("heightmap-ray-marcher_amd.lib").lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--elevation", type=float, default=30.0)
    ap.add_argument("--azimuth", type=float, default=40.0)
    ap.add_argument("--res", default="3840x2160")
    args = ap.parse_args()
    hm.set_device(0)
    wl = hm.synth.WORKLOADS["C3"]
    rgb, cmap = hm.synth.synth_maps(wl.map_size)
    params, cam = wl.scene_params(), wl.camera()
    cam.width, cam.height = (int(v) for v in args.res.split("x"))
    scene = hm.Scene(rgb, cmap, params)
    n = cam.width * cam.height
    el, az = math.radians(args.elevation), math.radians(args.azimuth)
    sun_dir = (math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el))
    sun = hm.Sun.make(sun_dir, cam.step_dist, ambient=96)
    results = []

    def frame_ms(fn):
        fn()
        return float(lib.hmrm_last_kernel_ms())

    def ratio_line(xs, ys):
        r = sorted(x / y for x, y in zip(xs, ys))
        return f"{statistics.median(r):.3f} [{r[0]:.3f} .. {r[-1]:.3f}]"

    f_plain = lambda: frame_ms(lambda: scene.render(cam))
    f_lit = lambda: frame_ms(lambda: scene.render_lit(cam, sun))
    f_bare = lambda: frame_ms(lambda: scene.render_shaded(cam, sun, shadows=False))
    f_full = lambda: frame_ms(lambda: scene.render_shaded(cam, sun))

    # ---- (a) hill shading without shadow rays against hmrm_render ----
    bare_ms, plain_ms = alternate(f_bare, f_plain, args.warmup, args.pairs)
    plain = scene.render(cam).reshape(-1, 4)
    bare = scene.render_shaded(cam, sun, shadows=False).reshape(-1, 4)
    changed = int((bare != plain).any(axis=1).sum())
    print(f"(a) shaded frame without shadows {med(bare_ms)}; hmrm_render {med(plain_ms)}; ratio {ratio_line(bare_ms, plain_ms)}; "
          f"sun {sun_dir}, {changed} of {n} pixels changed; kernel {scene.kernel_choice()}", flush=True)
    results.append({"case": "a", "shaded_ms": bare_ms, "render_ms": plain_ms, "changed": changed})

    # ---- (b) hill shading with shadow rays against hmrm_render_lit ----
    full_ms, lit_ms = alternate(f_full, f_lit, args.warmup, args.pairs)
    lit = scene.render_lit(cam, sun).reshape(-1, 4)
    full = scene.render_shaded(cam, sun).reshape(-1, 4)
    darkened = (lit != plain).any(axis=1)
    same_shadows = bool((full[darkened] == lit[darkened]).all())
    print(f"(b) shaded frame with shadows {med(full_ms)}; hmrm_render_lit {med(lit_ms)}; ratio {ratio_line(full_ms, lit_ms)}; "
          f"{int(darkened.sum())} pixels darkened by shadows, the same bytes in both frames: {same_shadows}", flush=True)
    results.append({"case": "b", "shaded_ms": full_ms, "lit_ms": lit_ms, "darkened": int(darkened.sum()), "same_shadows": same_shadows})
    scene.close()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
