"""What tests/test_cell_map_sum_cpu.py and tests/test_cell_map_sum_gpu.py share: the target lists of the accumulated cell maps
(hmrm_cell_map_sum; include/hmrm.h) and the expected map -- the int64 sum, over the targets, of tests/cell_map_cases.py's
replayed hmrm_cell_map bytes in WEIGHT mode, or of `status != HIT` in status mode.  Nothing here marches a ray."""
import numpy as np

import cell_map_cases as cc
import cell_map_replay as cmr
from cell_map_cases import SUNS

UP = (0.0, 0.0, 1.0)
CAP_TARGETS = (SUNS[0], UP, UP)  # one sun, straight up twice: at a small step cap the interior rays straight up are CAPPED
ODD_TARGETS = (SUNS[0], (np.nan, 0.5, 0.35), SUNS[1], (0.6, np.inf, 0.35), (0.0, 0.0, 0.0), SUNS[2])
SMALL_CAP = 300


def points(gw):
    """Point mode: the two observers of the cell-map module, one above the box and one inside it."""
    return (cc.point_above(gw), cc.point_inside(gw))


def summed(replays, gw, sampling, targets, step_dist, flags, lift=0.0, max_steps=0, ambient=cc.AMBIENT, step_cap=cc.BASE_CAP,
           which="A"):
    """The (H, W) uint16 map hmrm_cell_map_sum must write for `targets`."""
    total = None
    for t in targets:
        b = replays.bytes(gw, sampling, t, step_dist, flags, lift, max_steps, ambient, step_cap, which)
        v = b.astype(np.int64) if flags & cmr.WEIGHT else (b != cmr.HIT).astype(np.int64)
        total = v if total is None else total + v
    assert 0 <= total.min() and total.max() <= 255 * len(targets) <= 65280
    return total.astype(np.uint16)


def capped_rays(replays, gw, sampling, targets, step_dist, lift, max_steps, step_cap, which="A", point=False):
    """How many rays of the launch the step cap stops: one per target and cell."""
    return sum(int((replays.status(gw, sampling, t, step_dist, lift, max_steps, point, step_cap, which) == cmr.CAPPED).sum())
               for t in targets)
