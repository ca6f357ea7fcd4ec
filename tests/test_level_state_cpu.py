"""The per-level state the march kernels fetch (csrc/frame.hpp level_state_table, leap_common.hpp level_state) and the level
policy's moves, through the host hook hmrm_debug_level_state: every level including the whole map, both values of `young`,
every min_level, against the formulas of frame.hpp written out again here.  The header checks the same with a static_assert
for whatever HMRM_LEVEL_STEP / HMRM_DENSE_FROM it is compiled with; the last test compiles it with the other settings."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_HPP = os.path.join(ROOT, "heightmap-ray-marcher_amd", "csrc", "frame.hpp")

# the build's constants (frame.hpp defaults)
LEVEL_STEP, DENSE_FROM, ADAPT_AFTER = 1, 1, 8


def win_strides(l):
    return 2 if l < DENSE_FROM else 4


def win_cells(l):
    return 4 << (LEVEL_STEP * l)


def stride_shift(l):
    return LEVEL_STEP * l + (1 if l < DENSE_FROM else 0)


def test_symbol_is_exported_and_declared(hmrm):
    assert "hmrm_debug_level_state" in hmrm.EXPORTED_SYMBOLS
    with open(os.path.join(ROOT, "include", "hmrm.h")) as f:
        assert "hmrm_debug_level_state(" in f.read()


def test_every_level_young_and_min_level(hmrm):
    _, levels = hmrm.level_state(0, True, 0)
    assert levels == 7
    seen = 0
    for min_level in range(levels):
        for young in (False, True):
            lstep = 2 if young else 1
            for level in range(levels + 1):
                got, n = hmrm.level_state(level, young, min_level)
                assert n == levels
                top = level == levels
                if top:  # the one window of the top plane: window 0 for every cell, as wide as any map
                    assert got["stride_shift"] == 28 and got["cells"] == 1 << 30
                else:
                    assert got["stride_shift"] == stride_shift(level)
                    assert got["back"] == win_strides(level) - 1
                    assert got["cells"] == win_cells(level) == win_strides(level) << stride_shift(level)
                assert got["byte"] == got["stride_shift"] | (got["back"] << 5) and got["byte"] < 256
                assert got["lstep"] == lstep
                assert got["coarser"] == min(level + lstep, levels - 1)                      # clamped at the coarsest level
                assert got["finer"] == (levels - 1 if top else max(level - lstep, min_level))  # clamped at the frame's finest
                assert got["at_finest"] == (1 if level == min_level else 0)
                assert 0 <= got["finer"] <= levels - 1 and 0 <= got["coarser"] <= levels - 1
                seen += 1
    assert seen == levels * 2 * (levels + 1)


@pytest.mark.parametrize("args", [(-1, 0, 0), (8, 0, 0), (0, 0, -1), (0, 0, 7)])
def test_bad_arguments(hmrm, args):
    with pytest.raises(hmrm.HmrmError):
        hmrm.level_state(*args)


@pytest.mark.parametrize("level_step,dense_from", [(1, 0), (1, 1), (1, 99), (2, 0), (2, 1), (2, 99)])
def test_header_sweep_holds_for_the_other_settings(level_step, dense_from):
    """frame.hpp's static_assert sweep of the level state bytes, compiled for the host with the other settings.  (Settings the
    record kernel does not support stop at ITS assertion, which is as before; none may stop at the level state's.)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-w", f"-DHMRM_LEVEL_STEP={level_step}", f"-DHMRM_DENSE_FROM={dense_from}",
                        "-x", "c++", FRAME_HPP], capture_output=True, text=True)
    errors = [l for l in r.stderr.splitlines() if "error" in l]
    foreign = "the record level's windows"
    assert all(foreign in l for l in errors), r.stderr  # (nothing else may stop the compile, the level state's sweep least of all)
    assert "level state" not in r.stderr, r.stderr
    supported_by_records = level_step == 1 and dense_from <= 2
    assert (r.returncode == 0) == supported_by_records, r.stderr
    assert bool(errors) == (not supported_by_records)
