#!/usr/bin/env python3
"""The register table of the view-batch kernels, and how they fetch their frame record (profiles/r15_views_registers.txt; no GPU
needed).

usage: views_registers.py BUILD_DIR

BUILD_DIR holds the .s files of `make -C heightmap-ray-marcher_amd/csrc asm`: every instantiation of render_views.hip beside its
counterpart of render_interior.hip as vector registers / scalar registers / resident waves per SIMD (tools/haze_registers.py's
rule), with scratch where a kernel has any.  Then, for every instantiation, the memory instructions of the kernel by kind: the
view kernel reads its DevFrame from a device array, the interior kernel from its arguments, so the view kernel may have MORE
scalar loads than its counterpart but must have NO MORE vector loads -- a per-lane fetch of a record field would show as one."""
import collections
import os
import re
import sys

from haze_registers import FOUR, by_args, fmt, kernels, waves


def bodies(path):
    """{mangled name: its instructions} of one .s file."""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_ZN4hmrm\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        lines = [l.split(";")[0].strip() for l in m.group(2).split("\n")]
        out[m.group(1)] = [l for l in lines if l and not l.endswith(":") and not l.startswith(".")]
    return out


def loads(ins):
    """(scalar loads, vector loads, vector stores, instructions) of a kernel."""
    c = collections.Counter(i.split()[0] for i in ins)
    scalar = sum(v for k, v in c.items() if k.startswith("s_load") or k.startswith("s_buffer_load"))
    vload = sum(v for k, v in c.items() if re.match(r"(global|flat|buffer|scratch)_load", k))
    vstore = sum(v for k, v in c.items() if re.match(r"(global|flat|buffer|scratch)_store", k))
    return scalar, vload, vstore, len(ins)


def main(argv):
    if len(argv) != 1:
        sys.exit(__doc__)
    d = argv[0]
    views = by_args(kernels(os.path.join(d, "render_views.s")), "k_render_views", FOUR)
    interior = by_args(kernels(os.path.join(d, "render_interior.s")), "k_render_interior", FOUR)
    assert len(views) == len(interior) == 63, (len(views), len(interior))
    vb = by_args(bodies(os.path.join(d, "render_views.s")), "k_render_views", FOUR)
    ib = by_args(bodies(os.path.join(d, "render_interior.s")), "k_render_interior", FOUR)
    assert len(vb) == len(ib) == 63, (len(vb), len(ib))
    print("PROJ GWM LEAP SAMP   interior v/s/w      views v/s/w   interior sload/vload/vstore/instr      views sload/vload/vstore/instr   note")
    fewer = more_vloads = 0
    for k in sorted(views):
        note = ""
        if views[k][2] or views[k][3]:
            note += f" views: scratch={views[k][2]} spills={views[k][3]}"
        if interior[k][2] or interior[k][3]:
            note += f" interior: scratch={interior[k][2]} spills={interior[k][3]}"
        if waves(views[k][0]) < waves(interior[k][0]):
            note += " FEWER WAVES than interior"
            fewer += 1
        li, lv = loads(ib[k]), loads(vb[k])
        if lv[1] > li[1]:
            note += " MORE VECTOR LOADS than interior"
            more_vloads += 1
        print(f"{k[0]:4d} {k[1]:3d} {k[2]:4d} {k[3]:4d} {fmt(interior[k]):>16s} {fmt(views[k]):>16s} {'/'.join(map(str, li)):>36s} {'/'.join(map(str, lv)):>36s}  {note}")
    print(f"instantiations with fewer resident waves than their counterpart: {fewer} of 63")
    print(f"instantiations with more vector loads than their counterpart (a per-lane fetch of the record): {more_vloads} of 63")
    lit = kernels(os.path.join(d, "render.s"))
    print("\nThe literal loop (nearest sampling), beside the interior one:")
    for name in sorted(lit):
        if "k_render_views_literal" in name or "k_render_interior_literal" in name:
            print(f"  {re.sub(r'^_ZN4hmrm', '', name).split('EEv')[0]:40s} {fmt(lit[name]):>12s}" + (f"  scratch={lit[name][2]}" if lit[name][2] else ""))


if __name__ == "__main__":
    main(sys.argv[1:])
