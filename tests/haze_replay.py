"""hmrm_render_haze (include/hmrm.h) in numpy: a haze frame from the primary records of its camera rays (tests/ray_replay.py,
tests/segment_replay.py) and the rays themselves -- tests/geometry_replay.py's inputs.  The range is the header's
sqrt((ex * ex + ey * ey) + ez * ez) from the ray's origin to the record's point, kept as a double (numpy's float64 ufuncs are
plain IEEE operations, no contraction; np.sqrt is correctly rounded); the index is one subtract, one multiply, two comparisons
and a truncation; the blend is the water frame's, in integers.  An antialiased frame is the super camera's frame, hazed per
sample, through tests/aa_box.py."""
import numpy as np

import aa_box

HIT, CAPPED = 1, 2


def ranges(primary, rays):
    """r of every record as a double (meaningless where the ray did not hit)."""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 6)
    with np.errstate(all="ignore"):
        ex = primary["point"][:, 0] - rays[:, 0]
        ey = primary["point"][:, 1] - rays[:, 1]
        ez = primary["point"][:, 2] - rays[:, 2]
        return np.sqrt((ex * ex + ey * ey) + ez * ez)


def indices(r, start, scale, n):
    """The table index of every range: n - 1 for u >= n - 1, else (int)u for u > 0, else 0 (NaN: 0)."""
    with np.errstate(all="ignore"):
        u = (np.asarray(r, dtype=np.float64) - np.float64(start)) * np.float64(scale)
    top = u >= np.float64(n - 1)
    mid = ~top & (u > 0.0)
    i = np.zeros(u.shape, dtype=np.int64)
    i[top] = n - 1
    i[mid] = np.trunc(u[mid]).astype(np.int64)
    return i


def blend(rgba, color, f):
    """(c * (255 - f) + h * f + 127) // 255 per channel; A stays.  rgba (n, 4) uint8, color three bytes, f (n,) amounts."""
    out = np.array(rgba, dtype=np.uint8, copy=True)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 1)
    h = np.array([int(v) for v in color], dtype=np.int64).reshape(1, 3)
    out[:, :3] = (out[:, :3].astype(np.int64) * (255 - f) + h * f + 127) // 255
    return out


def frame(primary, rays, start, scale, table, color, sky=False):
    """-> dict: rgba (n, 4) uint8 the hazed pixels, hit (n,) bool, r (n,) float64, index (n,) int64 (of the hits; -1 else)."""
    table = np.asarray(table, dtype=np.uint8).reshape(-1)
    n = int(table.size)
    hit = primary["status"] == HIT
    r = ranges(primary, rays)
    idx = np.where(hit, indices(r, start, scale, n), -1)
    amount = np.where(hit, table[np.maximum(idx, 0)], table[n - 1] if sky else 0)
    return dict(rgba=blend(primary["rgba"], color, amount), hit=hit, r=r, index=idx,
                capped=int((primary["status"] == CAPPED).sum()))


def filtered(want, width, height, factor):
    """The antialiased frame of a replayed super frame ((factor * height) x (factor * width) samples)."""
    return aa_box.box_filter(np.ascontiguousarray(want["rgba"]).reshape(height * factor, width * factor, 4), factor)
