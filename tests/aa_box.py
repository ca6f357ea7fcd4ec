"""The antialiased frame's definition (include/hmrm.h hmrm_render_aa) in numpy: the super frame's n x n blocks summed
per channel and rounded half up, (S + n*n/2) >> (2 log2 n), alpha 255."""
import numpy as np


def box_filter(frame: np.ndarray, n: int) -> np.ndarray:
    """(n*H, n*W, 4) uint8 super frame -> (H, W, 4) uint8."""
    nh, nw = frame.shape[:2]
    assert n in (1, 2, 4, 8) and nh % n == 0 and nw % n == 0
    s = frame[:, :, :3].astype(np.int64).reshape(nh // n, n, nw // n, n, 3).sum(axis=(1, 3))
    shift = 2 * (n.bit_length() - 1)
    out = np.empty((nh // n, nw // n, 4), dtype=np.uint8)
    out[:, :, :3] = (s + (n * n) // 2) >> shift
    out[:, :, 3] = 255
    return out


def super_camera(hmrm, cam, n: int):
    """The camera of the n x n larger frame whose samples the antialiased frame filters."""
    sc = hmrm.Camera.from_buffer_copy(cam)
    sc.width, sc.height = cam.width * n, cam.height * n
    return sc
