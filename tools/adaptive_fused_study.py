#!/usr/bin/env python3
"""The fused adaptive frame (rt_render_adaptive_fused: one scheduling pass, one render launch, the stop rule inside the kernel) against
the rounds (rt_render_adaptive_begin / rt_render_adaptive_part) and against rt_render, on ONE GPU.

Method: device events on the stream around each call (so the scheduling pass, every round and every check are inside); every shape gets
a warm-up call of each kind first (the context's kept schedule is then in place for all of them alike); the compared calls alternate
within one process, rep by rep; REPS repeats, the median and the range [min .. max] are printed.  Before every call the RNG states are
initialised again and the device is idle.  The two adaptive calls are also compared bit for bit (fb, counts) once per configuration.

  python tools/adaptive_fused_study.py [OUT.txt] [--skip-c5]
  python tools/adaptive_fused_study.py --trace      one warm-up and two fused C3 frames (16/64/16, rel_error 0.1) and nothing else: the run
                                                    to put under a kernel trace
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))

REPS = 7
FLOOR = 0.02


def main():
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    argv = sys.argv[1:]
    path = next((a for a in argv if not a.startswith("--")), None)
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

    def compare(calls, init):
        """calls: {name: fn}; returns {name: (median, min, max)} of REPS alternating repeats after one warm-up of each"""
        for fn in calls.values():
            timed(fn, init)
        t = {k: [] for k in calls}
        for _ in range(REPS):
            for k, fn in calls.items():
                t[k].append(timed(fn, init))
        return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}

    def row(name, r):
        return "%-34s median %8.2f ms   range [%8.2f .. %8.2f]" % (name, r[0], r[1], r[2])

    def verdict(fused, rounds):
        spread = max(fused[2] - fused[1], rounds[2] - rounds[1])
        gain = rounds[0] - fused[0]
        return "fused is %s than the rounds by %.2f ms (%.2fx); spread of the repeats %.2f ms -> %s" % (
            "faster" if gain > 0 else "SLOWER", abs(gain), rounds[0] / fused[0], spread, "beyond the spread" if abs(gain) > spread else "WITHIN the spread")

    class Buffers:
        def __init__(self, nx, ny, part):
            self.nx, self.ny, self.part = nx, ny, part
            n = rt.part_pixels(nx, ny, part)
            self.st = rt.alloc_rand_state(nx, ny, part)
            self.fb = rt.alloc_fb(nx, ny, part)
            self.spp = torch.zeros(n, dtype=torch.int32, device="cuda")
            self.state = rt.alloc_adaptive_state(nx, ny, part)

        def init(self):
            rt.render_init(self.nx, self.ny, self.st, self.part)

        def bits(self):
            torch.cuda.synchronize()
            return self.fb.view(torch.int32).clone(), self.spp.clone()

    if "--trace" in argv:
        nx, ny = 1200, 800
        W = rt.World(10000, nx, ny).upload()
        O = rt.Octree(W, 32).upload()
        B = Buffers(nx, ny, rt.WHOLE)
        P = rt.Adaptive(16, 64, 16, 0.1, FLOOR)
        for _ in range(3):
            B.init()
            rt.render_adaptive_fused(B.fb, nx, ny, P, W, B.st, B.state, O, B.spp)
            torch.cuda.synchronize()
        print("traced: 3 fused C3 frames 16/64/16 rel_error 0.1, kernel %s, mean spp %.2f" % (rt.render_kernel_name(W, O, 3), float(B.spp.float().mean())))
        return

    say("# tools/adaptive_fused_study.py on %s: device events around each call, %d alternating repeats after a warm-up, median and range; floor %.2f"
        % (torch.cuda.get_device_name(0), REPS, FLOOR))

    # ---- C3
    nx, ny = 1200, 800
    W = rt.World(10000, nx, ny).upload()
    O = rt.Octree(W, 32).upload()
    B = Buffers(nx, ny, rt.WHOLE)
    say()
    say("## C3: %dx%d, N = 10000, octree SPL 32, kernels %s / %s" % (nx, ny, rt.render_kernel_name(W, O, 0), rt.render_kernel_name(W, O, 3)))

    def adaptive_calls(P):
        return {"rt_render_adaptive_fused": lambda: rt.render_adaptive_fused(B.fb, B.nx, B.ny, P, W, B.st, B.state, O, B.spp, B.part),
                "rt_render_adaptive_begin": lambda: rt.render_adaptive_begin(B.fb, B.nx, B.ny, P, W, B.st, B.state, O, B.spp, B.part)}

    def same_bits(P):
        got = []
        for fn in adaptive_calls(P).values():
            B.init()
            fn()
            got.append(B.bits())
        return all(torch.equal(a, b) for a, b in zip(*got)), float(got[0][1].float().mean())

    P = rt.Adaptive(16, 64, 16, 0.0, FLOOR)
    calls = adaptive_calls(P)
    calls["rt_render(64)"] = lambda: rt.render(B.fb, nx, ny, 64, W, B.st, O)
    r = compare(calls, B.init)
    same, mean = same_bits(P)
    say()
    say("### 16/64/16, rel_error 0 (every pixel to 64): bits %s, mean spp %.2f" % ("equal" if same else "DIFFER", mean))
    for k in calls:
        say(row(k, r[k]))
    say("fused / rt_render(64) = %.3f (target <= 1.25); rounds / rt_render(64) = %.3f" % (r["rt_render_adaptive_fused"][0] / r["rt_render(64)"][0],
                                                                                        r["rt_render_adaptive_begin"][0] / r["rt_render(64)"][0]))
    say(verdict(r["rt_render_adaptive_fused"], r["rt_render_adaptive_begin"]))
    for rel in (0.2, 0.1, 0.05):
        P = rt.Adaptive(8, 128, 8, rel, FLOOR)
        r = compare(adaptive_calls(P), B.init)
        same, mean = same_bits(P)
        say()
        say("### 8/128/8, rel_error %.2f: bits %s, mean spp %.2f" % (rel, "equal" if same else "DIFFER", mean))
        for k in r:
            say(row(k, r[k]))
        say(verdict(r["rt_render_adaptive_fused"], r["rt_render_adaptive_begin"]))
    O.close()
    W.close()

    # ---- an eighth of C5
    if "--skip-c5" not in argv:
        nx, ny = 3840, 2160
        W = rt.World(100000, nx, ny).upload()
        O = rt.Octree(W, 320).upload()
        B = Buffers(nx, ny, rt.Partition(0, 8))
        say()
        say("## C5's scene, part 0 of 8 (runs): %dx%d, N = 100000, octree SPL 320, kernels %s / %s; 16/256/16"
            % (nx, ny, rt.render_kernel_name(W, O, 0), rt.render_kernel_name(W, O, 3)))
        for rel in (0.0, 0.10):
            P = rt.Adaptive(16, 256, 16, rel, FLOOR)
            calls = {"rt_render_adaptive_fused": lambda: rt.render_adaptive_fused(B.fb, nx, ny, P, W, B.st, None, O, B.spp, B.part),
                     "rt_render_adaptive_part": lambda: rt.render_adaptive_part(B.fb, nx, ny, P, W, B.st, O, B.spp, B.part)}
            r = compare(calls, B.init)
            got = []
            for fn in calls.values():
                B.init()
                fn()
                got.append(B.bits())
            same = all(torch.equal(a, b) for a, b in zip(*got))
            s = got[0][1]
            say()
            say("### rel_error %.2f: bits %s, mean spp %.2f" % (rel, "equal" if same else "DIFFER", float(s[s > 0].float().mean())))
            for k in r:
                say(row(k, r[k]))
            say(verdict(r["rt_render_adaptive_fused"], r["rt_render_adaptive_part"]))
        O.close()
        W.close()
    if path:
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
