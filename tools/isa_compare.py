#!/usr/bin/env python3
"""Are the kernels of two builds the same instruction text?  usage: tools/isa_compare.py DIR_A DIR_B

DIR_A and DIR_B each hold one `hipcc -S --cuda-device-only` listing (*.s) per translation unit, made with the Makefile's flags for
that unit.  A kernel is a symbol with a `.amdhsa_kernel` descriptor; its text runs from its label to `.Lfunc_end`, with local labels
renumbered in order of appearance and the .loc / .file / .cfi / .p2align lines and comments dropped.  Prints both inventories (kernels
per unit) and, for every kernel, `same`, `DIFFERS`, `only in A` or `only in B`; the exit status is 1 if any kernel present in both
differs.  Whole texts are compared for equality, nothing else.  A kernel is matched by its symbol wherever it lies: moving it to another
unit is no difference."""
import glob
import os
import re
import subprocess
import sys


def kernels(path):
    lines = open(path).read().split("\n")
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        text, labels = [], {}
        for l in lines[start + 1:]:
            t = l.split(";")[0].strip()
            if t.startswith(".Lfunc_end"):
                break
            if not t or t.split()[0] in (".loc", ".file", ".p2align") or t.startswith(".cfi"):
                continue
            text.append(t)
        for t in text:                                  # local labels, in order of definition
            m = re.match(r"^(\.L\w+):$", t)
            if m:
                labels.setdefault(m.group(1), ".L%d" % len(labels))
        out[name] = "\n".join(re.sub(r"\.L\w+", lambda m: labels.get(m.group(0), m.group(0)), t) for t in text)
    return out


def inventory(d):
    inv = {}
    for f in sorted(glob.glob(os.path.join(d, "*.s"))):
        for name, text in kernels(f).items():
            assert name not in inv, "kernel %s emitted by two units of %s" % (name, d)
            inv[name] = (os.path.basename(f)[:-2], text)
    return inv


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(.*", "", d[5:] if d.startswith("void ") else d) for n, d in zip(names, out)}


A, B = inventory(sys.argv[1]), inventory(sys.argv[2])
pretty = demangle(sorted(set(A) | set(B)))
for tag, d, inv in (("A", sys.argv[1], A), ("B", sys.argv[2], B)):
    units = {}
    for n, (u, _) in inv.items():
        units[u] = units.get(u, 0) + 1
    print("inventory %s (%s): %d kernels  %s" % (tag, d, len(inv), "  ".join("%s %d" % kv for kv in sorted(units.items()))))
bad = 0
for n in sorted(set(A) | set(B), key=lambda n: pretty[n]):
    if n in A and n in B:
        same = A[n][1] == B[n][1]
        bad += not same
        where = A[n][0] if A[n][0] == B[n][0] else "%s -> %s" % (A[n][0], B[n][0])
        print("%-8s %-60s %s" % ("same" if same else "DIFFERS", pretty[n], where))
    else:
        print("%-8s %-60s %s" % ("only in A" if n in A else "only in B", pretty[n], (A.get(n) or B.get(n))[0]))
both = len(set(A) & set(B))
print("%d kernels in both, %d differ; %d only in A, %d only in B" % (both, bad, len(set(A) - set(B)), len(set(B) - set(A))))
sys.exit(1 if bad else 0)
