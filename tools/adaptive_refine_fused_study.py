#!/usr/bin/env python3
"""The refinement in one render launch (rt_render_adaptive_refine_fused: the seed pass and ONE k_render<*,4,*>) against the rounds
(rt_render_adaptive_refine), and both against the difference they stand for, begin(to) - begin(from), on ONE GPU.

Method: a frame is begun once at `from` (rt_render_adaptive_begin) and its fb, counts, RNG states and state are kept; before every
timed refinement they are copied back into the working buffers and the device is idle, so every repeat refines the same begun state.
Device events on the stream around each call (the seed, every round and every check are inside); one warm-up call of each kind, then
the calls alternate within one process, rep by rep; REPS repeats, the median and the range [min .. max] are printed.  The two
refinements are compared bit for bit (fb, counts, RNG states, state) once per configuration.  begin(from) and begin(to) are timed in
the same alternation, from rt_render_init's states.

  python tools/adaptive_refine_fused_study.py [OUT.txt] [--skip-c5] [--package DIR]
        --package DIR: the directory that holds rt_amd.py and librt_amd.so (default: this tree's).  A library without the fused
        refinement (an earlier build) gets the rounds' column alone: the check that the yardstick did not move.
  python tools/adaptive_refine_fused_study.py --trace      begin(0.2) on C3 8/128/8, then three times copy-back + fused refine(0.2 -> 0.1)
                                                           and nothing else: the run to put under a kernel trace
  python tools/adaptive_refine_fused_study.py --kernel-report DIR OUT.txt     the kernels of that run's trace, written to OUT.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REPS = 7
FLOOR = 0.02


def kernel_report(d, path):
    import kernel_trace as kt
    ev = kt.read_trace(d)
    names = [kt.short_name(n) for n, _ in ev]
    lines = ["kernels of the traced run, by name: launches, total and mean device time"]
    total = {}
    for n, us in zip(names, (us for _, us in ev)):
        c, t = total.get(n, (0, 0.0))
        total[n] = (c + 1, t + us)
    for n, (c, t) in sorted(total.items(), key=lambda x: -x[1][1]):
        lines.append("%6d x %-64s total %10.1f us  mean %10.1f us" % (c, n[:64], t, t / c))
    last = max(i for i, n in enumerate(names) if "k_adapt_refine_seed" in n)
    first = max(i for i, n in enumerate(names[:last]) if "k_adapt_zero" in n)
    lines += ["", "the last refinement, in start order:"]
    lines += ["  %-64s %10.1f us" % (names[i][:64], ev[i][1]) for i in range(first, len(ev)) if i <= last + 2]
    count = lambda key: sum(1 for n in names if key in n)
    mode = lambda m: sum(1 for n, _ in ev if any(kt.is_instance(n, "k_render", t, m, g) for t, g in ((True, 1), (True, 2), (True, 4), (True, 5), (False, 1))))
    lines += ["", "k_adapt_refine_seed launches: %d; k_adapt_refine_check launches: %d; k_render<*,2,*> launches: %d; k_render<*,4,*> launches: %d"
              % (count("k_adapt_refine_seed"), count("k_adapt_refine_check"), mode(2), mode(4))]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    argv = sys.argv[1:]
    if "--kernel-report" in argv:
        i = argv.index("--kernel-report")
        return kernel_report(argv[i + 1], argv[i + 2])
    package = os.path.join(ROOT, "dd2360-raytracing_amd")
    if "--package" in argv:
        i = argv.index("--package")
        package = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    sys.path.insert(0, package)
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    path = next((a for a in argv if not a.startswith("--")), None)
    have_fused = hasattr(rt, "render_adaptive_refine_fused")
    out = []

    def say(line=""):
        print(line, flush=True)
        out.append(line)

    def timed(fn, init):
        init()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def compare(calls):
        """calls: {name: (fn, init)}; returns {name: (median, min, max)} of REPS alternating repeats after one warm-up of each"""
        for fn, init in calls.values():
            timed(fn, init)
        t = {k: [] for k in calls}
        for _ in range(REPS):
            for k, (fn, init) in calls.items():
                t[k].append(timed(fn, init))
        return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}

    def row(name, r):
        return "%-40s median %8.2f ms   range [%8.2f .. %8.2f]" % (name, r[0], r[1], r[2])

    class Buffers:
        def __init__(self, nx, ny, part):
            self.nx, self.ny, self.part = nx, ny, part
            n = rt.part_pixels(nx, ny, part)
            self.st = rt.alloc_rand_state(nx, ny, part)
            self.fb = rt.alloc_fb(nx, ny, part)
            self.spp = torch.zeros(n, dtype=torch.int32, device="cuda")
            self.state = rt.alloc_adaptive_state(nx, ny, part)
            self.kept = None

        def all(self):
            return (self.fb, self.spp, self.st, self.state)

        def init(self):
            rt.render_init(self.nx, self.ny, self.st, self.part)

        def keep(self):
            torch.cuda.synchronize()
            self.kept = [t.clone() for t in self.all()]

        def restore(self):
            for t, k in zip(self.all(), self.kept):
                t.copy_(k)

        def bits(self):
            torch.cuda.synchronize()
            return [t.clone().view(torch.uint8) for t in self.all()]

    def study(B, W, O, lo, hi, step, a, b):
        """one configuration: the frame begun at rel_error a, refined to b"""
        nx, ny = B.nx, B.ny
        Pa, Pb = rt.Adaptive(lo, hi, step, a, FLOOR), rt.Adaptive(lo, hi, step, b, FLOOR)
        B.init()
        rt.render_adaptive_begin(B.fb, nx, ny, Pa, W, B.st, B.state, O, B.spp, B.part)
        B.keep()
        before = B.kept[1].clone()
        calls = {"rt_render_adaptive_refine": (lambda: rt.render_adaptive_refine(B.fb, nx, ny, Pa, Pb, W, B.st, B.state, O, B.spp, B.part), B.restore)}
        if have_fused:
            calls["rt_render_adaptive_refine_fused"] = (lambda: rt.render_adaptive_refine_fused(B.fb, nx, ny, Pa, Pb, W, B.st, B.state, O, B.spp, B.part), B.restore)
        calls["rt_render_adaptive_begin(%.2f)" % a] = (lambda: rt.render_adaptive_begin(B.fb, nx, ny, Pa, W, B.st, B.state, O, B.spp, B.part), B.init)
        calls["rt_render_adaptive_begin(%.2f)" % b] = (lambda: rt.render_adaptive_begin(B.fb, nx, ny, Pb, W, B.st, B.state, O, B.spp, B.part), B.init)
        r = compare(calls)
        got = []
        for fn, init in list(calls.values())[:2 if have_fused else 1]:
            init()
            fn()
            got.append(B.bits())
        inside = got[0][1].view(torch.int32) > 0
        after = got[0][1].view(torch.int32)
        listed = int((after > before).sum())
        same = "equal" if have_fused and all(torch.equal(x, y) for x, y in zip(*got)) else ("DIFFER" if have_fused else "not compared")
        say()
        say("### %d/%d/%d, refine(%.2f -> %.2f): bits %s; mean spp %.2f -> %.2f, %d of %d pixels resumed"
            % (lo, hi, step, a, b, same, float(before[inside].float().mean()), float(after[inside].float().mean()), listed, int(inside.sum())))
        for k in r:
            say(row(k, r[k]))
        rounds = r["rt_render_adaptive_refine"]
        diff = r["rt_render_adaptive_begin(%.2f)" % b][0] - r["rt_render_adaptive_begin(%.2f)" % a][0]
        say("begin(%.2f) - begin(%.2f) = %.2f ms; rounds / difference = %.2f" % (b, a, diff, rounds[0] / diff))
        if have_fused:
            fused = r["rt_render_adaptive_refine_fused"]
            spread = max(fused[2] - fused[1], rounds[2] - rounds[1])
            gain = rounds[0] - fused[0]
            say("fused / difference = %.2f" % (fused[0] / diff))
            say("fused is %s than the rounds by %.2f ms (rounds / fused = %.2fx); spread of the repeats %.2f ms -> %s" % (
                "faster" if gain > 0 else "SLOWER", abs(gain), rounds[0] / fused[0], spread, "beyond the spread" if abs(gain) > spread else "WITHIN the spread"))

    if "--trace" in argv:
        nx, ny = 1200, 800
        W = rt.World(10000, nx, ny).upload()
        O = rt.Octree(W, 32).upload()
        B = Buffers(nx, ny, rt.WHOLE)
        Pa, Pb = rt.Adaptive(8, 128, 8, 0.2, FLOOR), rt.Adaptive(8, 128, 8, 0.1, FLOOR)
        B.init()
        rt.render_adaptive_begin(B.fb, nx, ny, Pa, W, B.st, B.state, O, B.spp)
        B.keep()
        for _ in range(3):
            B.restore()
            rt.render_adaptive_refine_fused(B.fb, nx, ny, Pa, Pb, W, B.st, B.state, O, B.spp)
            torch.cuda.synchronize()
        print("traced: begin(0.2) and 3 fused refinements 0.2 -> 0.1 of C3 8/128/8, kernel %s, mean spp %.2f" % (rt.render_kernel_name(W, O, 4), float(B.spp.float().mean())))
        return

    say("# tools/adaptive_refine_fused_study.py on %s, library of %s: device events around each call, %d alternating repeats after a warm-up,"
        % (torch.cuda.get_device_name(0), os.path.relpath(package, ROOT), REPS))
    say("# median and range; every refinement starts from a copy of one begun state; floor %.2f" % FLOOR)

    nx, ny = 1200, 800
    W = rt.World(10000, nx, ny).upload()
    O = rt.Octree(W, 32).upload()
    B = Buffers(nx, ny, rt.WHOLE)
    say()
    say("## C3: %dx%d, N = 10000, octree SPL 32, kernels %s / %s" % (nx, ny, rt.render_kernel_name(W, O, 0), rt.render_kernel_name(W, O, 4) if have_fused else "-"))
    for a, b in ((0.2, 0.1), (0.1, 0.05)):
        study(B, W, O, 8, 128, 8, a, b)
    O.close()
    W.close()

    if "--skip-c5" not in argv:
        nx, ny = 3840, 2160
        W = rt.World(100000, nx, ny).upload()
        O = rt.Octree(W, 320).upload()
        B = Buffers(nx, ny, rt.Partition(0, 8))
        say()
        say("## C5's scene, part 0 of 8 (runs): %dx%d, N = 100000, octree SPL 320, kernels %s / %s"
            % (nx, ny, rt.render_kernel_name(W, O, 0), rt.render_kernel_name(W, O, 4) if have_fused else "-"))
        study(B, W, O, 16, 256, 16, 0.2, 0.1)
        O.close()
        W.close()
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
