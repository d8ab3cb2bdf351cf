#!/usr/bin/env python3
"""Static instruction counts of one kernel of csrc/rt_kernels.hip by the source function they were inlined from.

    hipcc <the Makefile's flags for build/rt_kernels.o> -gline-tables-only -S --cuda-device-only -o k.s csrc/rt_kernels.hip
    tools/valu_by_block.py k.s '_ZN2rt8k_renderILb1ELi0ELi4EEEvNS_10RenderArgsE' [csrc/rt_kernels.hip]

The listing's `.loc` lines name the source line of every instruction (the innermost inlined function); a line belongs to the
function or lambda whose definition starts last before it (RT_DEV functions, kernels, the lambdas of k_render).  Counts of the
code object, not measurements: multiply by how often a wave executes a block (tools/stats.py, wave-pass build)."""
import collections
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
asm, kernel = sys.argv[1], sys.argv[2]
src = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "dd2360-raytracing_amd", "csrc", "rt_kernels.hip")

starts = []          # (line, name)
pat = re.compile(r"^(?:RT_DEV|__device__ __forceinline__|static)\s.*?\b(\w+)\s*\(|^__global__.*?\bvoid\s+(\w+)\s*\(|^\s+auto\s+(\w+)\s*=\s*\[&\]")
for n, line in enumerate(open(src), 1):
    m = pat.match(line)
    if m:
        starts.append((n, next(g for g in m.groups() if g)))
# the main loop of k_render is a block of its own: everything after `while (true) {` up to the kernel's end
for n, line in enumerate(open(src), 1):
    if line.startswith("    while (true) {") and any(s[1] == "end_pixel" and s[0] < n for s in starts):
        starts.append((n, "k_render:main_loop")); break
starts.sort()


def owner(line):
    name = "?"
    for n, f in starts:
        if n > line: break
        name = f
    return name


fileno = None
inside = False
cur = ("?", 0)
valu = collections.Counter(); salu = collections.Counter(); vmem = collections.Counter(); lds = collections.Counter(); other = collections.Counter()
files = {}
for line in open(asm):
    t = line.strip()
    if t.startswith(".file"):
        m = re.match(r'\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', t)
        if m: files[int(m.group(1))] = (m.group(3) or m.group(2))
        continue
    if t.startswith(kernel + ":"): inside = True; continue
    if not inside: continue
    if t.startswith(".Lfunc_end"): break
    if t.startswith(".loc"):
        p = t.split()
        cur = (files.get(int(p[1]), ""), int(p[2]))
        continue
    if not t or t.startswith((".", ";", "//")) or t.endswith(":"): continue
    op = t.split()[0]
    who = owner(cur[1]) if cur[0].endswith("rt_kernels.hip") else "(header: %s)" % os.path.basename(cur[0])
    if op.startswith("v_"): valu[who] += 1
    elif op.startswith("s_"): salu[who] += 1
    elif op.startswith(("global_", "flat_", "buffer_", "scratch_")): vmem[who] += 1
    elif op.startswith("ds_"): lds[who] += 1
    else: other[who] += 1
print("%-28s %7s %7s %6s %6s" % ("inlined from", "VALU", "SALU", "VMEM", "LDS"))
for who in sorted(set(valu) | set(salu) | set(vmem) | set(lds), key=lambda w: -valu[w]):
    print("%-28s %7d %7d %6d %6d" % (who, valu[who], salu[who], vmem[who], lds[who]))
print("%-28s %7d %7d %6d %6d" % ("total", sum(valu.values()), sum(salu.values()), sum(vmem.values()), sum(lds.values())))
