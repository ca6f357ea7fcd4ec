"""What the GPU test modules share: environment knobs, the kernel variants and their samplings, the `gpu` and `world` fixtures,
the scenes of a replay object, bytewise comparisons that name the first difference, and the `hmap` CLI's config preamble and
run.  A plain module (tests/ is on sys.path): `import gpu_support as gs`, and `from gpu_support import gpu` for the fixture."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import segment_cases as sc

KERNEL_VARIANTS = ("leap", "group", "simple", "rec")  # (leap: the production kernel)
SAMPLINGS = (0, 1, 2)
PROJ_IDS = ["persp", "sph", "ortho"]
PROJ_NAMES = {1: "perspective", 2: "spherical", 3: "orthographic"}


@contextlib.contextmanager
def env(**kw):
    """Temporarily set environment knobs (the Python wrappers make a live scene re-read them: hmrm_debug_reload_env); a value of
    None unsets the variable.  Everything is as it was on exit."""
    old = {k: os.environ.get(k) for k in kw}

    def put(values):
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    put(kw)
    try:
        yield
    finally:
        put(old)


def kernel_variant(name):
    """HMRM_KERNEL=name; None: the scene's own choice."""
    return env(HMRM_KERNEL=name)


def samplings_of(variant, nearest_only=("rec",)):
    """The sampling modes a kernel variant is run with: the record kernel applies to nearest sampling only, and where a
    family's literal loop does too the module says so with nearest_only=("rec", "simple")."""
    return (0,) if variant in nearest_only else SAMPLINGS


@pytest.fixture(scope="module")
def gpu(hmrm):
    assert hmrm.device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    hmrm.set_device(0)
    return hmrm


def world_fixture(cls):
    """The module-scoped `world` fixture of a World class: cls(gpu, oracle), closed behind the module's last test."""
    @pytest.fixture(scope="module")
    def world(gpu, oracle):
        w = cls(gpu, oracle)
        yield w
        w.close()
    return world


class Maps:
    """What a Replays class starts from, for a World without one: tests/segment_cases.py's map, and per grid width its scene
    parameters and the oracle's heights."""

    def __init__(self, hmrm, oracle):
        self.hmrm, self.oracle = hmrm, oracle
        self.rgb, self.cmap = sc.maps()
        self.params = {gw: sc.scene_params(hmrm, gw) for gw in sc.GRID_WIDTHS}
        self.heights = {gw: oracle.update_heightmap(self.rgb, p) for gw, p in self.params.items()}


class Scenes:
    """Mix-in in front of a Replays class (rgb, cmap, params per grid width): one gpu.Scene per grid width, and close()."""

    def __init__(self, gpu, oracle):
        super().__init__(gpu, oracle)
        self.gpu = gpu
        self.scenes = {gw: gpu.Scene(self.rgb, self.cmap, p) for gw, p in self.params.items()}

    def close(self):
        for s in self.scenes.values():
            s.close()


# ---- bytewise comparisons ----
def same_frame(got, want_rgba, what):
    want = np.asarray(want_rgba).reshape(got.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere((got != want).any(axis=2))
        y, x = bad[0]
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.shape[0] * got.shape[1]} pixels differ; first ({x}, {y}): got {got[y, x]}, want {want[y, x]}")


def same_records(got, want, what):
    if got.tobytes() == want.tobytes():
        return
    for name in want.dtype.names:
        a, b = got[name], want[name]
        bad = np.nonzero((a.reshape(a.shape[0], -1).view(np.uint8) != b.reshape(b.shape[0], -1).view(np.uint8)).any(axis=1))[0]
        if bad.size:
            i = int(bad[0])
            raise AssertionError(f"{what}: field {name!r} differs for {bad.size} of {want.shape[0]} rays; first {i}: got {got[i]}, want {want[i]}")
    raise AssertionError(f"{what}: records differ in padding")


def same_cells(got, want, what, dtype):
    """A cell map of `dtype` against the replay's values (which may come in a wider type)."""
    if got.shape != want.shape or got.dtype != dtype:
        raise AssertionError((what, got.shape, want.shape, got.dtype))
    if np.ascontiguousarray(got).tobytes() != np.ascontiguousarray(want).astype(dtype).tobytes():
        bad = np.argwhere(got != want)
        y, x = bad[0]
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.size} cells differ; first ({x}, {y}): got {got[y, x]}, want {want[y, x]}")


# ---- the hmap CLI ----
def cli_preamble(gw, heightmap, colormap, output=None, inside=False, proj=1, width=40, height=30):
    """segment_cases.camera(gw, proj, inside) and segment_cases.scene_params(gw) as config text, `output` last if given."""
    pos = sc.camera_pos(gw, inside)
    return (f"resolution {width} {height}\nhfov {sc.hfov_deg(proj)}\nhang {sc.HANG_DEG}\nvang {sc.VANG_DEG}\n"
            f"pos {pos[0]:.17g} {pos[1]:.17g} {pos[2]:.17g}\n"
            f"min_height 0.0\nmax_height {sc.MAX_HEIGHT_GW * gw:.17g}\ngrid_width {gw:.17g}\nstep_dist {sc.STEP_DIST_GW * gw:.17g}\n"
            f"bg_color {sc.BG[0]} {sc.BG[1]} {sc.BG[2]}\ncycle 1\n"
            f"projection {PROJ_NAMES[proj]}\nheightmap {heightmap}\ncolormap {colormap}\n" + (f"output {output}\n" if output else ""))


def cli_config(gpu, world, tmp_path, gw, inside=False, extra="", output=True, **camera):
    """Write the world's maps as h.ppm and c.png and the config c.txt (the preamble + extra) under tmp_path.  Returns the
    config's path, the preamble and the output path frame.png -- which the preamble names unless output=False, for tests
    that send their runs to different places.  **camera: proj, width, height of cli_preamble."""
    hp, cp, outp = str(tmp_path / "h.ppm"), str(tmp_path / "c.png"), str(tmp_path / "frame.png")
    gpu.write_ppm(hp, world.rgb)
    gpu.write_png(cp, world.cmap)
    text = cli_preamble(gw, hp, cp, outp if output else None, inside, **camera)
    cfgp = tmp_path / "c.txt"
    cfgp.write_text(text + extra)
    return cfgp, text, outp


def hmap_exe(gpu):
    return os.path.join(os.path.dirname(gpu.LIB_PATH), "hmap")


def run_hmap(gpu, cfg_path):
    """Run the CLI on a config file; it must exit with 0 (stderr is the message otherwise).  Returns the completed process."""
    r = subprocess.run([hmap_exe(gpu), str(cfg_path)], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise AssertionError(r.stderr)
    return r
