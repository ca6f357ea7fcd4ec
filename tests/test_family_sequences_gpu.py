"""The family fuzzer (tests/deep_fuzz_families.py) inside the GPU suite: the first F ops of the suite's seed over live scenes --
ray and segment batches, picks, interior, sun-lit, geometry, accumulated and baked frames, cell maps and their sums, the light plane
swapped under tickets in flight, host and device forms on caller streams, every kernel setting and the step caps -- every byte
against the numpy replays.  F ops, not a time box: the first F ops hold the whole coverage list (test_family_sequences_cpu.py)."""
import os
import re
import subprocess
import sys

import pytest

from gpu_support import gpu
from test_family_sequences_cpu import F, SUITE_SEED

pytestmark = pytest.mark.gpu


def test_family_sequence_slice(gpu):
    """One fresh process, one GPU context, exactly F ops: return code 0, no mismatch, nothing missing from the coverage list --
    the run-time half included (every device form with a non-zero capped count taken on two caller streams).  Measured on an
    MI355X box: DESIGN.md 5.6.3.  The summary lines are printed (pytest -rP shows them)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k not in ("HMRM_KERNEL", "HMRM_STEP_CAP", "HMRM_TILE_SEGMENTS", "HMRM_TILE_ORDER", "HMRM_TRY_GROUP")}
    r = subprocess.run([sys.executable, os.path.join(here, "deep_fuzz_families.py"), str(SUITE_SEED), str(F)], capture_output=True, text=True,
                       timeout=300, env=env)
    tail = (r.stdout + r.stderr)[-4000:]
    print("\n".join(line for line in r.stdout.splitlines() if line.startswith("fam:")))
    assert r.returncode == 0 and "mismatches 0" in r.stdout, tail
    m = re.search(r"^fam: ops (\d+), mismatches 0, per-kind \{\}", r.stdout, flags=re.M)
    assert m and int(m.group(1)) == F, tail
    assert "fam: missing []" in r.stdout, tail
