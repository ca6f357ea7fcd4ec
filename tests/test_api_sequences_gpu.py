"""A time-boxed slice of the sequence fuzzer (tests/deep_fuzz_api.py) inside the GPU suite: whole call sequences over live
scenes -- every entry point of the ABI that returns pixels, tickets in flight across height updates, antialiased frames
through the cache records of their super cameras, strips on caller streams, step caps -- every byte against the oracle."""
import os
import re
import subprocess
import sys

import pytest

from gpu_support import gpu
from test_api_sequences_cpu import F, SLICE_SEED

pytestmark = pytest.mark.gpu

SLICE_S = 40   # this slice's own time box (not part of the shares of test_parity_gpu._FUZZ_SHARES)


def _run(args, timeout):
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k not in ("HMRM_KERNEL", "HMRM_STEP_CAP", "HMRM_TILE_SEGMENTS", "HMRM_TILE_ORDER", "HMRM_TRY_GROUP")}
    return subprocess.run([sys.executable, os.path.join(here, "deep_fuzz_api.py")] + [str(a) for a in args], capture_output=True, text=True,
                          timeout=timeout, env=env)


def test_api_sequence_slice(gpu):
    """SLICE_S seconds of the op stream of SLICE_SEED: no mismatch, and at least F ops -- the first F ops of this seed hold every
    op kind, kernel variant, projection, sampling mode and factor, an update with tickets in flight, arena regrowths, evictions,
    a camera repeated 12 times and a run of 8 fresh ones on sizes the calibration takes (test_api_sequences_cpu.py), so
    coverage holds whenever this passes.  F is a condition, not a speed measurement: measured on an MI355X box the 40 s slice
    runs 156 841 ops (3 900 per second, 79 922 oracle frames computed), far beyond 2 F = 600.  The summary lines are printed (pytest -rP
    shows them)."""
    r = _run([SLICE_SEED, 1000000, SLICE_S], timeout=SLICE_S + 260)
    tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0 and "mismatches 0" in r.stdout, tail
    m = re.search(r"^api: ops (\d+), mismatches 0, per-kind \{\}", r.stdout, flags=re.M)
    assert m and int(m.group(1)) >= F, tail
    assert "api: missing []" in r.stdout, tail
    print("\n".join(line for line in r.stdout.splitlines() if line.startswith("api:")))
