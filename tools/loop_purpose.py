#!/usr/bin/env python3
"""What the production march loop spends its instructions on, by purpose (no GPU needed).

Every instruction of the march loop of one k_render_fast instantiation (default: the C3 headline's, spherical, leaps,
nearest cell) is attributed to a purpose -- start cell, window geometry, refresh, estimate, landing, policy, group, ...
-- by the source line of march.hpp it was compiled from.  The lines come from a second compile of render_fast.hip with
-gline-tables-only and otherwise the flags of `make asm`; the tool first checks that this compile emits exactly the
instruction stream of the plain one (line tables must not change the code they describe), else it stops.  Inlined
helpers (cvt_i32_sat, axis_refresh, ...) are attributed to the line of render_wave_tile they were inlined into.

VALU instructions are priced with tools/isa_cost.py's measured table; SALU instructions are counted.  Per wave-trip of
the loop each basic block is weighted by how often it runs (profiles/r04_raw/attempt_diag.txt, r05_experiments section
2): attempt blocks 0.96, the three refresh blocks 0.68 per attempt in total (a third each), group blocks 0.58, blocks of
loop control 1, the literal loop near the step cap 0.  A block's kind is the kind of the purposes of most of its VALU
instructions.

usage: loop_purpose.py [--csrc DIR] [--asm FILE --lines FILE] [instantiation substring]
  --csrc DIR      the csrc directory to compile (default: this tree's); both compiles go to DIR/_build
  --asm, --lines  reuse existing plain / line-table assembly instead of compiling"""
import argparse
import collections
import os
import re
import shlex
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import isa_cost  # noqa: E402

DEFAULT_CSRC = os.path.join(os.path.dirname(HERE), "heightmap-ray-marcher_amd", "csrc")
C3 = "ILi2ELb0ELi0ELi1ELi0ELb0E"

MARCH_SRC = "march.hpp"  # the file that holds render_wave_tile

# A line of it gets the purpose of the last marker at or above it (markers in source order).
MARKERS = [
    ("bool done = entry_nan;", "loop control"),
    ("const bool attempt = REC", "attempt decision"),
    ("auto refresh_stale = [&]() {", "stale checks"),
    ("if (stale_x) axis_refresh", "refresh"),
    ("if (!kEarlyLoad) refresh_stale();", "start cell"),
    ("const bool top = lev == kTopLevel;", "window geometry"),
    ("const unsigned widx =", "pyramid load"),
    ("if (kEarlyLoad) refresh_stale();", "refresh"),
    ("const bool exact = kStepsLeft", "stale checks"),
    ("const int wx0 = ix << hs", "window geometry"),
    ("double room_lat = 0.0;", "lateral room"),
    ("const double m = (double)mf;", "height test, cand"),
    ("room = room_lat;", "estimate n"),
    ("const double nn = (double)", "landing, verification"),
    ("x = ok ? xn : x;", "commit"),
    ("diag.on_attempt_done", "level policy"),
    ("diag.on_trip(f, LEAP, skip_group);", "loop control"),
    ("double X[U], Y[U], Z[U], T[U];", "group: positions, cells"),
    ("diag.load_begin(f, 18);", "group: loads"),
    ("if (budget >= U) {", "group: tests, advance"),
    ("// (almost never) close to the step cap", "cap path"),
    ("x = X[U - 1] + sx;", "group: tests, advance"),
    ("if (COUNT) my_steps =", "epilogue"),
]
KIND = {"loop control": "control", "attempt decision": "control", "refresh": "refresh", "cap path": "cap",
        "epilogue": "control"}
KIND.update({p: "group" for _, p in MARKERS if p.startswith("group")})
REFRESH_BLOCKS = 3


def kind_of(purpose):
    return KIND.get(purpose, "attempt")


WEIGHT = {"attempt": 0.96, "refresh": 0.96 * 0.68 / REFRESH_BLOCKS, "group": 0.58, "control": 1.0, "cap": 0.0}


def compile_cmd(csrc):
    """The command `make asm` runs for render_fast.s, as words."""
    out = subprocess.run(["make", "-s", "-n", "-C", csrc, "asm"], capture_output=True, text=True, check=True).stdout
    line = next(l for l in out.splitlines() if "render_fast.hip" in l and "render_fast_aa" not in l)
    return shlex.split(line)


def build(csrc, lines):
    cmd = compile_cmd(csrc)
    if lines:
        o = cmd.index("-o")
        cmd[o + 1] = cmd[o + 1].replace("render_fast.s", "render_fast_lines.s")
        cmd.insert(o, "-gline-tables-only")
    os.makedirs(os.path.join(csrc, "_build"), exist_ok=True)
    subprocess.run(cmd, cwd=csrc, check=True, stderr=subprocess.DEVNULL)
    return os.path.join(csrc, cmd[cmd.index("-o") + 1])


def function_text(path, want):
    s = open(path).read()
    parts = re.split(r'\t\.type\t(_ZN4hmrm13k_render_fastI[^,]+),@function\n', s)
    for i in range(1, len(parts), 2):
        if want in parts[i]:
            return parts[i + 1].split('s_endpgm')[0]
    sys.exit(f"no instantiation matching {want} in {os.path.basename(path)}")


HEADERS = set()  # loop header labels seen by instructions()


def instructions(text):
    """[(block label, in loop, instruction, .loc comment or None)] in stream order."""
    out, label, loop, loc = [], "entry", False, None
    for raw in text.split("\n"):
        t = raw.strip()
        m = re.match(r'^(\.LBB\d+_\d+):', t)
        if m:
            label, loop = m.group(1), ("in Loop" in t or "Loop Header" in t)
            if "Loop Header" in t and "Depth=1" in t:
                HEADERS.add(label)
            continue
        if t.startswith(".loc"):
            loc = t.split(";", 1)[1].strip() if ";" in t else None
            continue
        if not t or t.startswith((";", ".")):
            continue
        out.append((label, loop, t.split(";")[0].strip(), loc))
    return out


def source_line(loc, lo, hi):
    """The innermost march.hpp line of an inline chain ('a.hpp:12:3 @[ march.hpp:283:5 @[ ... ] ]')
    that lies inside render_wave_tile's body [lo, hi]."""
    if not loc:
        return None
    for f, ln in re.findall(r'([\w./-]+):(\d+):\d+', loc):
        if os.path.basename(f) == MARCH_SRC and lo <= int(ln) <= hi:
            return int(ln)
    return None


def marker_lines(src_path):
    src = open(src_path).read().split("\n")
    body_lo = next(i for i, l in enumerate(src, 1) if "render_wave_tile(const DevFrame" in l)
    body_hi = next(i for i, l in enumerate(src, 1) if i > body_lo and l.startswith("}"))
    marks, start = [], body_lo
    for text, purpose in MARKERS:
        ln = next((i for i, l in enumerate(src, 1) if i >= start and text in l), None)
        if ln is None:
            sys.exit(f"marker not found in {MARCH_SRC}: {text!r}")
        marks.append((ln, purpose))
        start = ln
    return marks, body_lo, body_hi


def purpose_of_line(ln, marks):
    p = "loop control"
    for m, purpose in marks:
        if ln >= m:
            p = purpose
    return p


def vop3_cmp_sel(ins):
    op = ins.split()[0]
    return op.startswith(("v_cmp", "v_cmpx")) or op.startswith("v_cndmask_b32_e64")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("want", nargs="?", default=C3)
    ap.add_argument("--csrc", default=DEFAULT_CSRC)
    ap.add_argument("--asm")
    ap.add_argument("--lines")
    a = ap.parse_args()
    asm = a.asm or build(a.csrc, lines=False)
    lines = a.lines or build(a.csrc, lines=True)

    plain = instructions(function_text(asm, a.want))
    tagged = instructions(function_text(lines, a.want))
    if [(b, i) for b, _, i, _ in plain] != [(b, i) for b, _, i, _ in tagged]:
        k = next((j for j, (x, y) in enumerate(zip(plain, tagged)) if x[:3] != y[:3]), min(len(plain), len(tagged)))
        sys.exit(f"the -gline-tables-only build differs from `make asm` at instruction {k}: "
                 f"{plain[k][2] if k < len(plain) else '(end)'!r} vs {tagged[k][2] if k < len(tagged) else '(end)'!r}")

    marks, lo, hi = marker_lines(os.path.join(a.csrc, MARCH_SRC))
    # purposes per instruction: own line, else the previous attributed instruction of the block
    rows, last = [], {}
    for blk, loop, ins, loc in tagged:
        if not loop:
            continue
        ln = source_line(loc, lo, hi)
        p = purpose_of_line(ln, marks) if ln is not None else last.get(blk)
        rows.append([blk, ins, p])
        if p is not None:
            last[blk] = p
    by_block = collections.OrderedDict()
    for r in rows:
        by_block.setdefault(r[0], []).append(r)
    for blk, rs in by_block.items():  # leading unattributed instructions: the block's first purpose
        first = next((r[2] for r in rs if r[2] is not None), "loop control")
        for r in rs:
            if r[2] is None:
                r[2] = first

    def price(ins):
        return isa_cost.COST[isa_cost.classify(ins)]

    print(f"march loop of k_render_fast{a.want}: {len(rows)} instructions in {len(by_block)} blocks; the -gline-tables-only "
          f"build emits the same {len(plain)} instructions as `make asm`")
    print()
    print(f"{'block':12s} {'kind':8s} {'weight':>6s} {'VALU':>5s} {'cycles':>7s} {'VOP3 cmp/sel':>12s} {'SALU':>5s}  purposes")
    per_trip_v = per_trip_s = 0.0
    purpose = collections.OrderedDict((p, [0, 0.0, 0, 0, 0.0, 0.0]) for _, p in MARKERS)  # VALU, cycles, cmp/sel, SALU, per trip
    # a block's kind: that of most of its VALU instructions' purposes.  Blocks with nothing but loop control (exec-mask
    # joins, moves, no VALU) run as often as the block they lead into -- the next block in layout order that has a kind
    # of its own -- except the latch (the block before the loop header), which runs on every trip.
    labels = list(by_block)
    kinds = {}
    for blk, rs in by_block.items():
        c = collections.Counter(kind_of(r[2]) for r in rs if r[1].startswith("v_") and kind_of(r[2]) != "control")
        kinds[blk] = c.most_common(1)[0][0] if c else None
    order = re.findall(r'^(\.LBB\d+_\d+):', open(lines).read(), re.M)
    for i, blk in enumerate(labels):
        if kinds[blk] is None:
            nxt = order[order.index(blk) + 1] if blk in order and order.index(blk) + 1 < len(order) else None
            if nxt in HEADERS:
                kinds[blk] = "control"
            else:
                kinds[blk] = next((kinds[b] for b in labels[i + 1:] if kinds[b] is not None), "control")
    for blk, rs in by_block.items():
        kind = kinds[blk]
        w = WEIGHT[kind]
        v = [r for r in rs if r[1].startswith("v_")]
        s = [r for r in rs if r[1].startswith("s_")]
        cyc = sum(price(r[1]) for r in v)
        per_trip_v += w * cyc
        per_trip_s += w * len(s)
        for r in v:
            e = purpose[r[2]]
            e[0] += 1
            e[1] += price(r[1])
            e[2] += vop3_cmp_sel(r[1])
            e[4] += w * price(r[1])
        for r in s:
            purpose[r[2]][3] += 1
            purpose[r[2]][5] += w
        names = ", ".join(dict.fromkeys(r[2] for r in rs))
        print(f"{blk:12s} {kind:8s} {w:6.3f} {len(v):5d} {cyc:7.1f} {sum(vop3_cmp_sel(r[1]) for r in v):12d} {len(s):5d}  {names}")
    print()
    print(f"{'purpose':24s} {'VALU':>5s} {'cycles':>7s} {'VOP3 cmp/sel':>12s} {'SALU':>5s} {'cycles/trip':>11s} {'SALU/trip':>9s}")
    for p, (n, c, cs, ns, ct, st) in purpose.items():
        if n or ns:
            print(f"{p:24s} {n:5d} {c:7.1f} {cs:12d} {ns:5d} {ct:11.1f} {st:9.1f}")
    print()
    print(f"priced VALU cycles per wave-trip: {per_trip_v:.1f}")
    print(f"SALU instructions per wave-trip:  {per_trip_s:.1f}")
    print(f"(weights per wave-trip: {', '.join(f'{k} {v:.3f}' for k, v in WEIGHT.items())}; prices: {isa_cost.COST})")


if __name__ == "__main__":
    main()
