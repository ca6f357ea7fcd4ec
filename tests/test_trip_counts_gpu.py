"""Same traversal: the instrumented march kernel's per-frame counters -- steps, rays, hits, groups, leap attempts, leaps
and leaped steps -- reproduce exactly what the recorded build counted (tests/golden/trip_counts.json).  Pixels and step
counts alone do not pin the traversal: a change that makes a ray attempt, jump or march differently can still land on
the same pixels.  These counters move with every such change, so a rewrite of the loop that is meant to issue fewer
instructions per trip, and nothing else, must leave all of them as they were.

Re-record (only for a change that is meant to change the traversal): python tests/test_trip_counts_gpu.py --record"""
import contextlib
import json
import os
import sys

import pytest

from gpu_support import gpu

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trip_counts.json")
FIELDS = ("steps", "rays", "hits", "groups", "leap_attempts", "leaps", "leaped_steps")

# name -> (workload, HMRM_KERNEL or None)
CASES = {
    "C2": ("C2", None),
    "C3": ("C3", None),
    "C3h": ("C3h", None),
    "C4": ("C4", None),
    "C5": ("C5", None),
    "C3/white": (("C3", "white"), None),
    "C3/spikes": (("C3", "spikes"), None),
    "C3/needles": (("C3", "needles"), None),
    "C3/canyon": (("C3", "canyon"), None),
    "C3/needles/rec": (("C3", "needles"), "rec"),
    "C3/white/rec": (("C3", "white"), "rec"),
    "C2/group": ("C2", "group"),
    "C3/gw0.05": (("C3", 0.05), None),
    "REFDEF": ("REFDEF", None),
}


@contextlib.contextmanager
def kernel_env(name):
    old = os.environ.get("HMRM_KERNEL")
    if name is None:
        os.environ.pop("HMRM_KERNEL", None)
    else:
        os.environ["HMRM_KERNEL"] = name
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("HMRM_KERNEL", None)
        else:
            os.environ["HMRM_KERNEL"] = old


def workload(hmrm, spec):
    if isinstance(spec, str):
        return hmrm.synth.WORKLOADS[spec]
    base, arg = spec
    return hmrm.synth.grid_workload(base, arg) if isinstance(arg, float) else hmrm.synth.content_workload(base, arg)


def count(hmrm, name):
    """The instrumented kernel's counters of one full frame of case `name`."""
    spec, kernel = CASES[name]
    wl = workload(hmrm, spec)
    rgb, cmap = wl.maps()
    with kernel_env(kernel):  # (set before the scene exists: the scene reads its knobs when created)
        scene = hmrm.Scene(rgb, cmap, wl.scene_params())
        try:
            _, st, _, _ = scene.render_stats(wl.camera())
        finally:
            scene.close()
    return {k: int(getattr(st, k)) for k in FIELDS}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_every_case(golden):
    assert set(golden["cases"]) == set(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_counters_match_recorded_traversal(gpu, golden, name):
    got = count(gpu, name)
    assert got["rays"] > 0 and got["steps"] > 0
    assert got == golden["cases"][name], f"{name}: the traversal changed"


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import importlib
    hmrm = importlib.import_module("heightmap-ray-marcher_amd")
    hmrm.set_device(0)
    cases = {}
    for name in CASES:
        cases[name] = count(hmrm, name)
        print(name, cases[name], flush=True)
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        json.dump({"what": "k_render_fast instrumented counters per full frame (hmrm_render_stats)", "cases": cases}, f,
                  indent=1, sort_keys=True)
        f.write("\n")
