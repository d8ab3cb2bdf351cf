#!/usr/bin/env python3
"""Adaptive sampling on parts of a frame, measured on ONE GPU: the whole adaptive frame (rt_render_adaptive) against every part of
N = 2 / 4 / 8 runs parts (rt_render_adaptive_part: the tiles rank p of an N-GPU rt_multi_render_adaptive renders), for a rel_error
that leaves a mixed frame and for rel_error = 0 (every pixel to max_spp).  The slowest part x N / whole frame is the efficiency the
split allows before any exchange; each part's rounds (the rounds that still had active pixels: its largest count) and times are listed.
Times: host clock around the call and a device synchronise (launch), and the context's events from round 0 to the last check
(device); the minimum of REPS runs after a warm-up.  No multi-GPU number: one GPU renders the parts one after the other.

  python tools/adaptive_parts_study.py [OUT.txt] [--c3-only]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))

REPS = 3
FLOOR = 0.02
# (name, nx, ny, spheres, SPL, min_spp, batch, max_spp, the mixed-frame rel_error)
CASES = [
    ("C3", 1200, 800, 10000, 32, 8, 8, 128, 0.10),
    ("C5", 3840, 2160, 100000, 320, 16, 16, 256, 0.10),
]
NPARTS = (2, 4, 8)


def main():
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    cases = CASES[:1] if "--c3-only" in sys.argv[1:] else CASES
    out = []

    def say(line):
        print(line, flush=True)
        out.append(line)

    say("# tools/adaptive_parts_study.py on %s, %d runs per figure (minimum after a warm-up), floor %.2f" % (torch.cuda.get_device_name(0), REPS, FLOOR))
    ctx = rt.RenderCtx()
    for name, nx, ny, n, spl, lo, step, hi, rel_mixed in cases:
        W = rt.World(n, nx, ny).upload()
        O = rt.Octree(W, spl).upload()
        say("")
        say("## %s: %dx%d, N = %d, octree SPL %d, kernel %s, adaptive %d/%d/%d" % (name, nx, ny, n, spl, rt.render_kernel_name(W, O), lo, step, hi))
        for rel in (rel_mixed, 0.0):
            P = rt.Adaptive(lo, hi, step, rel, FLOOR)

            def run(part):
                npx = rt.part_pixels(nx, ny, part)
                st = rt.alloc_rand_state(nx, ny, part)
                fb = rt.alloc_fb(nx, ny, part)
                spp = torch.zeros(npx, dtype=torch.int32, device="cuda")
                best_host, best_dev = 1e30, 1e30
                for rep in range(REPS + 1):
                    rt.render_init(nx, ny, st, part)
                    torch.cuda.synchronize()
                    ctx.times()
                    t0 = time.perf_counter()
                    ctx.render_adaptive_part(fb, nx, ny, P, W, st, O, spp, part)
                    torch.cuda.synchronize()
                    t = (time.perf_counter() - t0) * 1e3
                    dev = float(ctx.times()[-1])
                    if rep:
                        best_host, best_dev = min(best_host, t), min(best_dev, dev)
                s = spp.cpu().numpy()
                s = s[s > 0]                                     # (padding elements stay 0)
                rounds = (int(s.max()) - lo) // step + 1
                return best_host, best_dev, float(s.mean()), rounds

            wh, wd, wmean, wrounds = run(rt.WHOLE)
            say("")
            say("### rel_error %.2f: whole frame %.2f ms launch, %.2f ms device, mean spp %.2f, %d of %d rounds with work"
                % (rel, wh, wd, wmean, wrounds, (hi - lo) // step + 1))
            say("%-14s %10s %10s %9s %7s" % ("part", "launch ms", "device ms", "mean spp", "rounds"))
            for nparts in NPARTS:
                worst = 0.0
                for p in range(nparts):
                    h, d, mean, rounds = run(rt.Partition(p, nparts))
                    worst = max(worst, h)
                    say("%-14s %10.2f %10.2f %9.2f %7d" % ("%d of %d" % (p, nparts), h, d, mean, rounds))
                say("N = %d: slowest part %.2f ms against whole / %d = %.2f ms -> split efficiency %.3f (launch times)"
                    % (nparts, worst, nparts, wh / nparts, wh / (nparts * worst)))
        O.close()
        W.close()
    ctx.close()
    if path:
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
