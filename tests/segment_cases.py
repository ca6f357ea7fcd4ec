"""What the ray-query, segment and sun-lit test modules share: the 64 x 48 map (not square, not a multiple of 16, alpha-0
texels, zero-height cells), its grid widths and cameras (the inside camera's orthographic plane is 3 cells wide, so that one
frame mixes interior origins with exterior rays that enter; tests/test_trace_rays_gpu.py has its own, 0.02 cells wide), and
the rays no camera makes."""
import numpy as np

import ray_replay
import scenes

MAP_W, MAP_H = 64, 48
GRID_WIDTHS = (1.0, 0.5, 0.05)  # grid modes 0, 1, 2 of the kernels
GW_IDS = ["gw1", "gw0.5", "gw0.05"]
BG = (12, 34, 56)


def maps():
    rgb, cmap = scenes.small_maps(MAP_W, MAP_H, 31)
    rgb[5:9, 40:47] = 0  # zero-height cells
    return rgb, cmap


HANG_DEG, VANG_DEG = -50, 112
MAX_HEIGHT_GW, STEP_DIST_GW = 8.0, 0.2  # in grid widths


def hfov_deg(proj):
    return 150 if proj == 2 else 80


def camera_pos(gw, inside):
    return (20.0 * gw, -20.0 * gw, 7.5 * gw) if inside else (-6.0 * gw, 8.0 * gw, 14.0 * gw)


def scene_params(hmrm, gw):
    return hmrm.SceneParams.make(0.0, MAX_HEIGHT_GW * gw, grid_width=gw)


def camera(hmrm, gw, proj, inside, sampling=0, width=40, height=30):
    deg = hmrm.degrees_to_rads
    return hmrm.Camera.make(width=width, height=height, projection=proj, hfov=deg(hfov_deg(proj)), hang=deg(HANG_DEG),
                            vang=deg(VANG_DEG), pos=camera_pos(gw, inside), ortho_width=(3.0 if inside else 1.3) * gw,
                            step_dist=STEP_DIST_GW * gw, bg=BG, sampling=sampling)


_rays = {}


def camera_rays(hmrm, oracle, gw, proj, inside, width=40, height=30):
    """The oracle's GetRay for every pixel (read-only, computed once)."""
    key = (gw, proj, inside, width, height)
    if key not in _rays:
        cam = camera(hmrm, gw, proj, inside, width=width, height=height)
        r = ray_replay.camera_rays(oracle, oracle.make_cfg(cam, scene_params(hmrm, gw), MAP_W, MAP_H))
        r.setflags(write=False)
        _rays[key] = r
    return _rays[key]


def ulp_in(v, towards):
    return float(np.nextafter(np.float64(v), np.float64(towards)))


def odd_rays(gw, exterior):
    """About 600 rays no camera makes, most of them interior: origins one ulp inside each of the six faces, on it and one
    ulp outside; underground origins; axis-parallel and zero directions; NaN and inf components; directions scaled
    1e-3 .. 1e3; rising rays that hit a taller neighbour -- permuted into waves with `exterior` rays (n x 6)."""
    W, H, top = MAP_W * gw, MAP_H * gw, 8.0 * gw
    rng = np.random.RandomState(23)
    out = []
    mid = (0.5 * W, -0.5 * H, 0.6 * top)
    faces = [(0, 0.0, W), (0, W, 0.0), (1, 0.0, -H), (1, -H, 0.0), (2, 0.0, top), (2, top, 0.0)]
    for axis, face, other in faces:
        for where in (ulp_in(face, other), face, ulp_in(face, 2.0 * face - other if face != 0.0 else -other)):
            for k in range(6):
                o = [mid[0] + (k - 3) * 2.3 * gw, mid[1] + (k - 2) * 1.7 * gw, mid[2]]
                o[axis] = where
                d = rng.uniform(-1.0, 1.0, 3)
                d[axis] = abs(d[axis]) * (1.0 if other > face else -1.0)  # into the box
                d[2] = d[2] if axis == 2 else -abs(d[2]) * 0.3
                out.append(o + list(d))
    # underground: below the local terrain, inside the box
    for k in range(40):
        out.append([(3.0 + 1.4 * k) * gw, -(2.0 + 1.1 * k) * gw, 0.01 * gw * (1 + k % 5), rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.5, 1.0)])
    # axis-parallel from inside (never straight up without a way out: those run to the cap and have a test of their own)
    for k in range(20):
        x, y = (4.25 + 2.9 * k) * gw, -(3.5 + 2.1 * k) * gw
        out.append([x, y, 7.9 * gw, 0.0, 0.0, -1.0])
        out.append([x, y, 6.5 * gw, 1.0, 0.0, 0.0])
        out.append([x, y, 7.0 * gw, -1.0, 0.0, 0.0])
        out.append([x, y, 7.5 * gw, 0.0, 1.0, 0.0])
        out.append([x, y, 7.7 * gw, 0.0, -1.0, 0.0])
    # zero directions and straight up, inside: to the step cap (the tests set a small one)
    for k in range(6):
        out.append([(10.25 + 3 * k) * gw, -(10.25 + 2 * k) * gw, 7.8 * gw, 0.0, 0.0, 0.0])
        out.append([(11.25 + 3 * k) * gw, -(9.25 + 2 * k) * gw, 7.8 * gw, 0.0, 0.0, 1.0])
    # NaN / inf in every component, interior origins
    for k in range(3):
        base = np.array([(12.0 + 9 * k) * gw, -(14.0 + 5 * k) * gw, 7.2 * gw, 0.4, -0.3, -0.2])
        for comp in range(6):
            for v in (np.nan, np.inf, -np.inf):
                q = base.copy()
                q[comp] = v
                out.append(list(q))
    # directions scaled 1e-3 .. 1e3
    for k in range(120):
        o = [rng.uniform(0.05, 0.95) * W, -rng.uniform(0.05, 0.95) * H, rng.uniform(0.3, 0.99) * top]
        d = rng.uniform(-1.0, 1.0, 3)
        d[2] = -abs(d[2]) * 0.4 if k % 3 else d[2] * 0.2
        d[k % 2] += np.copysign(0.3, d[k % 2])
        out.append(o + list(d * 10.0 ** rng.uniform(-3, 3)))
    # rising rays from low down: they hit a taller neighbour or leave through the top... of the grid's side
    for k in range(120):
        o = [rng.uniform(0.1, 0.9) * W, -rng.uniform(0.1, 0.9) * H, rng.uniform(0.02, 0.5) * top]
        a = rng.uniform(0, 2 * np.pi)
        out.append(o + [np.cos(a), np.sin(a), rng.uniform(0.02, 0.4)])
    own = np.asarray(out, dtype=np.float64)
    rays = np.concatenate([own, np.asarray(exterior, dtype=np.float64).reshape(-1, 6)])
    return np.ascontiguousarray(rays[np.random.RandomState(5).permutation(rays.shape[0])])
