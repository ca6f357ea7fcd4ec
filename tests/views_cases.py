"""What tests/test_views_cpu.py and tests/test_views_gpu.py share: the cameras of the view batches over tests/segment_cases.py's
map and grid widths, the batches made of them, and a cache of expected frames -- the C oracle's for plain views,
tests/segment_replay.py's for views under the interior rule -- computed once per (camera, size), read-only.

The seven cameras differ in everything a batch lets differ (position, both angles, hfov, ortho_width, step_dist, background):
  0  segment_cases' outside camera
  1  a camera strictly inside the box (plain: every pixel a miss, as in the reference; interior: it marches)
  2  a camera above the box that looks up: only sky, no ray enters
  3  another outside camera: narrower hfov, a longer step, a wider orthographic plane
  4  camera 0's hang and hfov with another vang      (spherical: shares 0's column tables, not its row tables)
  5  camera 0's vang and hfov with another hang      (spherical: shares 0's row tables, not its column tables)
  6  camera 3's angles and hfov from another place   (spherical: shares both of 3's)
Cameras 1 and 2 share no table with anyone.  No ray of any of them comes near BASE_CAP steps (expected() asserts it), so the
frames are those of any larger cap; the one case with capped rays is the GPU module's own.  (The views are taller than wide, so
a spherical camera's rows span hfov * height / width: camera 1's spherical hfov is narrow, or its top rows would look straight up
from inside the box and run to the cap.)"""
import numpy as np

import segment_cases as sc
import segment_replay as sr
from segment_cases import MAP_H, MAP_W

BASE_CAP = 4096
SIZES = ((8, 16), (9, 17), (1, 1), (24, 33))  # one tile; four tiles, mostly dead lanes; one pixel; three tile rows, the last partial
SIZE_IDS = ["8x16", "9x17", "1x1", "24x33"]
COUNTS = (1, 2, 3, 7)
N_CAMS = 7

# (position in grid widths, hang, vang in degrees, hfov for perspective and orthographic / spherical, ortho_width and step_dist in
# grid widths, background)
_CAMS = (
    ((-6.0, 8.0, 14.0), sc.HANG_DEG, sc.VANG_DEG, (80, 150), 1.3, 0.2, sc.BG),
    ((20.0, -20.0, 7.5), -20, 100, (70, 40), 3.0, 0.25, (200, 10, 90)),
    ((30.0, -24.0, 20.0), 35, 30, (60, 100), 1.5, 0.2, (1, 2, 3)),
    ((70.0, 6.0, 12.0), -140, 115, (60, 120), 2.0, 0.3, (90, 80, 70)),
    ((-6.0, 8.0, 14.0), sc.HANG_DEG, 105, (80, 150), 1.3, 0.2, (0, 255, 0)),
    ((-4.0, 2.0, 11.0), -35, sc.VANG_DEG, (80, 150), 1.1, 0.15, (255, 0, 255)),
    ((66.0, 3.0, 10.0), -140, 115, (60, 120), 0.9, 0.2, (7, 7, 7)),
)


def camera(hmrm, gw, proj, k, sampling=0, width=24, height=33):
    pos, hang, vang, hfov, ortho, step, bg = _CAMS[k]
    deg = hmrm.degrees_to_rads
    return hmrm.Camera.make(width=width, height=height, projection=proj, hfov=deg(hfov[1 if proj == 2 else 0]), hang=deg(hang),
                            vang=deg(vang), pos=tuple(p * gw for p in pos), ortho_width=ortho * gw, step_dist=step * gw, bg=bg,
                            sampling=sampling)


def batch_indices(n, first=0):
    """Which cameras a batch of n holds: n consecutive ones starting at `first`, cyclically."""
    return [(first + i) % N_CAMS for i in range(n)]


def group_tables(cams):
    """The Python statement of the table deduplication: (col_index, row_index) per view -- tables numbered in the order of
    their first view, keyed by the bits of (hang, hfov) and (vang, hfov); width and height are the batch's -- or -1 everywhere for
    a batch that is not spherical."""
    cams = list(cams)
    if cams[0].projection != 2:
        return [-1] * len(cams), [-1] * len(cams)
    bits = lambda v: np.float64(v).tobytes()
    cols, rows, ci, ri = {}, {}, [], []
    for c in cams:
        ci.append(cols.setdefault((bits(c.hang), bits(c.hfov)), len(cols)))
        ri.append(rows.setdefault((bits(c.vang), bits(c.hfov)), len(rows)))
    return ci, ri


class Expected:
    """Expected frames per (gw, proj, sampling, camera, width, height, interior): HxWx4 uint8, and whether any ray hit."""

    def __init__(self, hmrm, oracle):
        self.hmrm, self.oracle = hmrm, oracle
        self.rgb, self.cmap = sc.maps()
        self.params = {gw: sc.scene_params(hmrm, gw) for gw in sc.GRID_WIDTHS}
        self.heights = {gw: oracle.update_heightmap(self.rgb, p) for gw, p in self.params.items()}
        self._frames = {}

    def frame(self, gw, proj, sampling, k, width, height, interior, step_cap=BASE_CAP):
        """(frame, ray-steps or hits, capped rays) of camera k."""
        key = (gw, proj, sampling, k, width, height, interior, step_cap)
        if key not in self._frames:
            cam = camera(self.hmrm, gw, proj, k, sampling, width, height)
            cfg = self.oracle.make_cfg(cam, self.params[gw], MAP_W, MAP_H, step_cap)
            if not interior:
                fb, total, capped, _, _ = self.oracle.render(cfg, self.heights[gw], self.cmap)
                work = total
            else:
                import ray_replay
                rays = ray_replay.camera_rays(self.oracle, cfg)
                r = sr.replay(rays, self.heights[gw], self.cmap, self.params[gw], cam.step_dist, bg=(cam.bg_r, cam.bg_g, cam.bg_b),
                              sampling=sampling, step_cap=step_cap, interior=True)
                fb = np.ascontiguousarray(r["rgba"]).reshape(height, width, 4).copy()
                capped, work = int((r["status"] == sr.CAPPED).sum()), int((r["status"] == sr.HIT).sum())
            fb.setflags(write=False)
            self._frames[key] = (fb, work, capped)
        return self._frames[key]

    def batch(self, gw, proj, sampling, indices, width, height, interior, step_cap=BASE_CAP, capped_ok=False):
        """(n, H, W, 4) expected frames of the cameras `indices`; asserts that no ray was capped unless capped_ok."""
        frames = [self.frame(gw, proj, sampling, k, width, height, interior, step_cap) for k in indices]
        assert capped_ok or all(f[2] == 0 for f in frames), [(k, f[2]) for k, f in zip(indices, frames)]
        return np.stack([f[0] for f in frames])

    def cameras(self, gw, proj, sampling, indices, width, height):
        return [camera(self.hmrm, gw, proj, k, sampling, width, height) for k in indices]
