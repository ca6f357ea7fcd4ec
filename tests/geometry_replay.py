"""hmrm_render_geometry (include/hmrm.h) in numpy: the four planes of a geometry frame from the primary records of its camera
rays (tests/ray_replay.py, tests/segment_replay.py) and the rays themselves.  `rgba` and `cell` are the record's; `range` is
the header's sqrt((ex * ex + ey * ey) + ez * ez) from the ray's origin to the record's point -- numpy's float64 ufuncs are plain
IEEE operations (no contraction), np.sqrt is correctly rounded, astype(np.float32) rounds to nearest even -- and `slope` is
tests/shade_replay.py's gradient pair, the doubles of hmrm_render_shaded's level, rounded to float."""
import numpy as np

import shade_replay as shr

HIT = shr.HIT
INF_BITS = 0x7F800000


def planes(primary, rays, heights, params, sampling):
    """-> dict of flat arrays, one entry per record: rgba (n, 4) uint8, cell (n,) int32, range (n,) float32, slope (n, 2)
    float32."""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
    _mh, mw = heights.shape
    hit = primary["status"] == HIT
    cell = np.where(hit, primary["cell_y"].astype(np.int64) * mw + primary["cell_x"].astype(np.int64), -1).astype(np.int32)
    with np.errstate(all="ignore"):
        ex = primary["point"][:, 0] - rays[:, 0]
        ey = primary["point"][:, 1] - rays[:, 1]
        ez = primary["point"][:, 2] - rays[:, 2]
        r = np.sqrt((ex * ex + ey * ey) + ez * ez)
        rng = np.where(hit, r.astype(np.float32), np.float32(np.inf)).astype(np.float32)
        gx, gy = shr.gradients(primary, heights, params, sampling)
        slope = np.stack([gx.astype(np.float32), gy.astype(np.float32)], axis=1)
    slope[~hit] = 0.0
    return dict(rgba=np.ascontiguousarray(primary["rgba"]), cell=cell, range=rng, slope=np.ascontiguousarray(slope))


def counts(want, primary):
    """(hits, misses, capped, distinct range values among the hits, distinct hit cells) of replayed planes."""
    hit = primary["status"] == HIT
    capped = int((primary["status"] == 2).sum())
    return (int(hit.sum()), int((~hit).sum()) - capped, capped, int(np.unique(want["range"][hit].view(np.uint32)).size),
            int(np.unique(want["cell"][hit]).size))


def read_pfm(path):
    """A PFM reader in numpy: (h, w) or (h, w, 3) float32, rows top to bottom."""
    with open(path, "rb") as f:
        data = f.read()
    magic, dims, scale, body = data.split(b"\n", 3)
    comp = {b"Pf": 1, b"PF": 3}[magic]
    w, h = (int(v) for v in dims.split())
    dtype = "<f4" if float(scale) < 0 else ">f4"
    assert len(body) == w * h * comp * 4
    a = np.frombuffer(body, dtype=dtype).astype(np.float32).reshape(h, w, comp)[::-1]
    return a[:, :, 0] if comp == 1 else a
