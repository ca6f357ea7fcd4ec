#!/usr/bin/env python3
"""Do two builds of the kernels have the same instructions?  (no GPU needed)

usage: asm_same.py PARENT_BUILD_DIR TREE_BUILD_DIR

Compares the .s files `make -C heightmap-ray-marcher_amd/csrc asm` wrote into the two _build directories, kernel by
kernel.  A kernel's text runs from its `.type <name>,@function` line to the end of its function (the label behind its
last s_endpgm); its resources are the `.amdhsa_*` lines of its descriptor.  Comments, `.loc` lines and `__hip_cuid_*`
lines are dropped and the `.LBB*` labels are renumbered in order of appearance.  Every kernel is then one of

  identical  the same lines in the same order
  reordered  the same descriptor (registers, scratch, LDS, accumulator offset, ...) and the same lines as a multiset:
             only their order differs
  changed    anything else, a kernel that only the parent has included
  added      a kernel that only the tree has: a new unit's, or a new kernel of an existing unit

Instruction text is compared as opaque lines.  Prints the counts per unit with the names of the kernels that are not
identical; the exit status is 1 if any kernel changed.  Added kernels are named and counted and leave the status alone: a feature
that brings kernels of its own keeps the existing ones, which is what the status says."""
import collections
import os
import re
import sys

CLASSES = ("identical", "reordered", "changed")


def clean(line):
    return line.split(";", 1)[0].strip()


def renumbered(lines):
    """The lines with their .LBB labels numbered in order of appearance."""
    names = {}
    return [re.sub(r'\.LBB\d+_\d+', lambda m: names.setdefault(m.group(0), f".LBB_{len(names)}"), l) for l in lines]


def kernels(text):
    """{kernel name: (its lines, its descriptor's lines)} of one .s file."""
    text = "\n".join(l for l in text.split("\n") if "__hip_cuid_" not in l)
    desc = {}
    for m in re.finditer(r'^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel', text, re.M | re.S):
        desc[m.group(1)] = [c for c in map(clean, m.group(2).split("\n")) if c]
    out = {}
    parts = re.split(r'^\s*\.type\s+([^\s,]+),@function[^\n]*\n', text, flags=re.M)
    for name, body in zip(parts[1::2], parts[2::2]):
        if name not in desc:  # (a function that is no kernel)
            continue
        end = re.search(r'^\.Lfunc_end\d+:', body, re.M)
        body = body[:end.start()] if end else body[:body.rfind("s_endpgm") + len("s_endpgm")]
        lines = [c for c in map(clean, body.split("\n")) if c and not c.startswith(".loc")]
        out[name] = (renumbered(lines), desc[name])
    return out


def classify(a, b):
    """a, b: (lines, descriptor) of one kernel on either side, or None where the side does not have it."""
    if a is None and b is not None:
        return "added"
    if a is None or b is None:
        return "changed"
    if a == b:
        return "identical"
    if a[1] == b[1] and collections.Counter(a[0]) == collections.Counter(b[0]):
        return "reordered"
    return "changed"


def compare_texts(parent, tree):
    """{kernel name: class} for the texts of one unit's two .s files."""
    ka, kb = kernels(parent), kernels(tree)
    return {n: classify(ka.get(n), kb.get(n)) for n in sorted(set(ka) | set(kb))}


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    listing = [sorted(f for f in os.listdir(d) if f.endswith(".s")) for d in argv]
    changed = 0
    for unit in sorted(set(listing[0]) | set(listing[1])):
        texts = [open(os.path.join(d, unit)).read() if unit in files else "" for d, files in zip(argv, listing)]
        result = compare_texts(*texts)
        count = collections.Counter(result.values())
        changed += count["changed"]
        print(f"{unit}: " + ", ".join(f"{count[c]} {c}" for c in CLASSES) + (f", {count['added']} added" if count["added"] else ""))
        for name, c in result.items():
            if c != "identical":
                print(f"    {c}: {name}")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
