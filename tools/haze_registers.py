#!/usr/bin/env python3
"""The register table of the haze frames (profiles/r14_haze_registers.txt; no GPU needed).

usage: haze_registers.py BUILD_DIR [NAME=AB_DIR ...]

BUILD_DIR holds the .s files of `make -C heightmap-ray-marcher_amd/csrc asm`: every instantiation of render_haze.hip beside its
counterpart of render_interior.hip and every one of render_haze_aa.hip beside the antialiased plain kernel of render_fast_aa.hip,
as vector registers / scalar registers / resident waves per SIMD (tools/registers_ab.py's rule: 512 registers per lane, granules of
8), with scratch where a kernel has any.  Each AB_DIR holds render_haze.s and render_haze_aa.s of an A/B build (EXTRA_HIPFLAGS with
one of HMRM_HAZE_CHAIN=1, HMRM_HAZE_CARRY=1, HMRM_HAZE_DEFER=0) and is summarised against BUILD_DIR's."""
import os
import re
import sys


def waves(v):
    return min(8, 512 // ((v + 7) // 8 * 8))


def kernels(path):
    """{mangled name: (vgprs, sgprs, scratch bytes, spilled vgprs)} of one .s file."""
    out = {}
    for blk in open(path).read().split("  - .agpr_count:")[1:]:
        g = lambda key: re.search(r"\." + key + r":\s+(\S+)", blk)
        if g("name"):
            out[g("name").group(1)] = (int(g("vgpr_count").group(1)), int(g("sgpr_count").group(1)), int(g("private_segment_fixed_size").group(1)),
                                       int(g("vgpr_spill_count").group(1)))
    return out


def by_args(ks, stem, pattern):
    """{(PROJ, GWM, LEAP, SAMP): registers} of the kernels named `stem` whose template arguments match `pattern`."""
    out = {}
    for name, r in ks.items():
        m = re.match(r"_ZN4hmrm\d+" + stem + "I" + pattern + "EEEv", name)
        if m:
            out[tuple(int(v) for v in m.groups())] = r
    return out


FOUR = r"Li(\d)ELi(\d)ELi(\d)ELi(\d)"
FAST_AA = r"Li(\d)ELb0ELi(\d)ELi(\d)ELi(\d)ELb1"  # (k_render_fast<PROJ, STATS = false, GWM, LEAP, SAMP, AA = true>)


def fmt(r):
    return f"{r[0]}/{r[1]}/{waves(r[0])}"


def main(argv):
    if not argv:
        sys.exit(__doc__)
    d = argv[0]
    haze = by_args(kernels(os.path.join(d, "render_haze.s")), "k_render_haze", FOUR)
    haze_aa = by_args(kernels(os.path.join(d, "render_haze_aa.s")), "k_render_haze_aa", FOUR)
    interior = by_args(kernels(os.path.join(d, "render_interior.s")), "k_render_interior", FOUR)
    fast_aa = by_args(kernels(os.path.join(d, "render_fast_aa.s")), "k_render_fast", FAST_AA)
    assert len(haze) == len(haze_aa) == len(interior) == len(fast_aa) == 63, (len(haze), len(haze_aa), len(interior), len(fast_aa))
    print("PROJ GWM LEAP SAMP   interior v/s/w       haze v/s/w    fast_aa v/s/w    haze_aa v/s/w   note")
    fewer = fewer_aa = 0
    for k in sorted(haze):
        note = ""
        for what, r in (("haze", haze[k]), ("haze_aa", haze_aa[k])):
            if r[2] or r[3]:
                note += f" {what}: scratch={r[2]} spills={r[3]}"
        if waves(haze[k][0]) < waves(interior[k][0]):
            note += " FEWER WAVES than interior"
            fewer += 1
        if waves(haze_aa[k][0]) < waves(fast_aa[k][0]):
            note += " FEWER WAVES than fast_aa"
            fewer_aa += 1
        print(f"{k[0]:4d} {k[1]:3d} {k[2]:4d} {k[3]:4d} {fmt(interior[k]):>16s} {fmt(haze[k]):>16s} {fmt(fast_aa[k]):>16s} {fmt(haze_aa[k]):>16s}  {note}")
    print(f"instantiations with fewer resident waves than their counterpart: haze {fewer} of 63, haze_aa {fewer_aa} of 63")
    lit = kernels(os.path.join(d, "render.s"))
    print("\nThe literal loop (nearest sampling), beside the interior one:")
    for name in sorted(lit):
        if "k_render_haze_literal" in name or "k_render_interior_literal" in name:
            print(f"  {re.sub(r'^_ZN4hmrm', '', name).split('EEv')[0]:40s} {fmt(lit[name]):>12s}" + (f"  scratch={lit[name][2]}" if lit[name][2] else ""))
    for arg in argv[1:]:
        label, ab = arg.split("=", 1)
        print(f"\nA/B build {label}:")
        for unit, stem, base in (("render_haze", "k_render_haze", haze), ("render_haze_aa", "k_render_haze_aa", haze_aa)):
            other = by_args(kernels(os.path.join(ab, unit + ".s")), stem, FOUR)
            delta = {k: other[k][0] - base[k][0] for k in base}
            changed = {k: v for k, v in delta.items() if v}
            lose = [k for k in base if waves(other[k][0]) < waves(base[k][0])]
            gain = [k for k in base if waves(other[k][0]) > waves(base[k][0])]
            scratch = [(k, base[k][2], other[k][2]) for k in base if other[k][2] != base[k][2]]
            span = f"{min(changed.values()):+d} .. {max(changed.values()):+d} vector registers" if changed else "no change"
            print(f"  {unit}: {len(changed)} of 63 instantiations change ({span}); {len(lose)} lose a resident wave, {len(gain)} gain one")
            kinds = {}
            for k in lose + gain:  # (by kernel kind and sampling: the projections and grid modes of a kind move together)
                kinds.setdefault((k[2], k[3]), []).append(k)
            for (leap, samp), ks in sorted(kinds.items()):
                k = ks[0]
                print(f"    LEAP {leap} SAMP {samp}: {len(ks)} of 9, e.g. PROJ {k[0]} GWM {k[1]}: {fmt(base[k])} -> {fmt(other[k])}")
            for k, was, now in scratch:
                print(f"    scratch PROJ {k[0]} GWM {k[1]} LEAP {k[2]} SAMP {k[3]}: {was} -> {now} bytes")

if __name__ == "__main__":
    main(sys.argv[1:])
