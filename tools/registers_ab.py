#!/usr/bin/env python3
"""VGPRs / SGPRs / resident waves per SIMD of every kernel of two builds' `make asm` outputs, side by side (no GPU needed).

usage: registers_ab.py <parent csrc/_build> <change csrc/_build>
Waves per SIMD from the vector registers alone: 512 per lane and SIMD, allocated in granules of 8.  A kernel is flagged when
the change costs it a resident wave, and when it uses scratch or spills."""
import glob
import os
import re
import sys


def regs(d):
    out = {}
    for f in sorted(glob.glob(os.path.join(d, "*.s"))):
        if f.endswith("_lines.s"):
            continue
        s = open(f).read()
        for blk in s.split("  - .agpr_count:")[1:]:
            g = lambda key: re.search(r"\." + key + r":\s+(\S+)", blk)
            if not g("name"):
                continue
            out[(os.path.basename(f)[:-2], g("name").group(1))] = (int(g("vgpr_count").group(1)), int(g("sgpr_count").group(1)),
                int(g("private_segment_fixed_size").group(1)), int(g("group_segment_fixed_size").group(1)), int(g("vgpr_spill_count").group(1)))
    return out


def waves(v):  # unified 512-entry file, granule 8
    g = (v + 7) // 8 * 8
    return min(8, 512 // g)


a = regs(sys.argv[1]); b = regs(sys.argv[2])
print(f"{'unit':22s} {'kernel (mangled template arguments)':60s} {'parent v/s/w':>14s} {'change v/s/w':>14s}  note")
bad = 0
for k in sorted(set(a) | set(b)):
    pa, pb = a.get(k), b.get(k)
    short = re.sub(r"^_ZN4hmrm", "", k[1])
    short = re.sub(r"EEv.*$", "", short)[:60]
    fa = f"{pa[0]}/{pa[1]}/{waves(pa[0])}" if pa else "-"
    fb = f"{pb[0]}/{pb[1]}/{waves(pb[0])}" if pb else "-"
    note = ""
    if pb and (pb[2] or pb[3] or pb[4]):
        note += f" scratch={pb[2]} lds={pb[3]} spills={pb[4]}"
    if pa and pb and waves(pb[0]) < waves(pa[0]):
        note += " LOSES A WAVE"
        bad += 1
    if pa and pb and pb[0] != pa[0]:
        note += f" ({pb[0] - pa[0]:+d} VGPR)"
    print(f"{k[0]:22s} {short:60s} {fa:>14s} {fb:>14s} {note}")
print("instantiations that lose a wave per SIMD:", bad)
