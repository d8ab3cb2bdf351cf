#!/usr/bin/env python3
"""Refining an adaptive frame, measured on ONE GPU: begin(0.2) -> refine(0.2 -> 0.1) -> refine(0.1 -> 0.05) (rt_render_adaptive_begin /
rt_render_adaptive_refine) against begin(0.1) and begin(0.05) from scratch, and rt_render_adaptive at the same three targets (what
begin pays for keeping the state).  Every step of the chain is checked against the begin of its target, bit for bit, once.
Times: host clock around the call and a device synchronise (launch), and the context's events from the first to the last launch of
the call (device); the minimum of REPS runs after a warm-up.  "empty" counts the rounds whose list held no pixel.

  python tools/adaptive_refine_study.py [OUT.txt] [--c3-only]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))

REPS = 3
FLOOR = 0.02
TARGETS = (0.2, 0.1, 0.05)
# (name, nx, ny, spheres, SPL, min_spp, batch, max_spp)
CASES = [
    ("C3", 1200, 800, 10000, 32, 8, 8, 128),
    ("C5", 3840, 2160, 100000, 320, 16, 16, 256),
]


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

    say("# tools/adaptive_refine_study.py on %s, %d runs per figure (minimum after a warm-up), floor %.2f"
        % (torch.cuda.get_device_name(0), REPS, FLOOR))
    ctx = rt.RenderCtx()
    for name, nx, ny, n, spl, lo, step, hi in cases:
        W = rt.World(n, nx, ny).upload()
        O = rt.Octree(W, spl).upload()
        npx = nx * ny
        rounds = (hi - lo) // step
        P = {rel: rt.Adaptive(lo, hi, step, rel, FLOOR) for rel in TARGETS}
        st = rt.alloc_rand_state(nx, ny)
        fb = rt.alloc_fb(nx, ny)
        spp = torch.zeros(npx, dtype=torch.int32, device="cuda")
        state = rt.alloc_adaptive_state(nx, ny)

        def timed(call):
            torch.cuda.synchronize()
            ctx.times()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, float(ctx.times()[-1])

        def snap():
            torch.cuda.synchronize()
            return (fb.cpu().numpy().view(np.uint32).copy(), spp.cpu().numpy().copy(), st.cpu().numpy().copy(), state.cpu().numpy().copy())

        def best(a, b):
            return (min(a[0], b[0]), min(a[1], b[1])) if a else b

        # the chain, and the begin of every target (the reference frames of the check), REPS + 1 times each
        chain = [None] * len(TARGETS)
        fresh = {rel: None for rel in TARGETS}
        plain = {rel: None for rel in TARGETS}
        counts, frames = [], {}
        for rep in range(REPS + 1):
            rt.render_init(nx, ny, st)
            for i, rel in enumerate(TARGETS):
                if i == 0:
                    t = timed(lambda: ctx.render_adaptive_begin(fb, nx, ny, P[rel], W, st, state, O, spp))
                else:
                    t = timed(lambda: ctx.render_adaptive_refine(fb, nx, ny, P[TARGETS[i - 1]], P[rel], W, st, state, O, spp))
                if rep:
                    chain[i] = best(chain[i], t)
                else:
                    frames[("chain", rel)] = snap()
                    counts.append(frames[("chain", rel)][1])
            for rel in TARGETS:
                rt.render_init(nx, ny, st)
                t = timed(lambda: ctx.render_adaptive_begin(fb, nx, ny, P[rel], W, st, state, O, spp))
                if rep:
                    fresh[rel] = best(fresh[rel], t)
                else:
                    frames[("begin", rel)] = snap()
                rt.render_init(nx, ny, st)
                t = timed(lambda: ctx.render_adaptive(fb, nx, ny, P[rel], W, st, O, spp))
                if rep:
                    plain[rel] = best(plain[rel], t)
                else:
                    a, b = snap()[:3], frames[("begin", rel)][:3]
                    assert all(np.array_equal(x, y) for x, y in zip(a, b)), "begin differs from rt_render_adaptive at %.2f" % rel
        for rel in TARGETS:
            a, b = frames[("chain", rel)], frames[("begin", rel)]
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), "the chain differs from begin at %.2f" % rel

        say("")
        say("## %s: %dx%d, N = %d, octree SPL %d, kernel %s, adaptive %d/%d/%d; every chain step equals begin of its target, bit for bit"
            % (name, nx, ny, n, spl, rt.render_kernel_name(W, O), lo, step, hi))
        say("%-24s %10s %10s %9s %7s" % ("call", "launch ms", "device ms", "mean spp", "empty"))
        for i, rel in enumerate(TARGETS):
            s = counts[i]
            if i == 0:
                label, empty = "begin(%.2f)" % rel, rounds + 1 - ((int(s.max()) - lo) // step + 1)
            else:
                label = "refine(%.2f -> %.2f)" % (TARGETS[i - 1], rel)
                empty = rounds - int(((s - counts[i - 1]) // step).max())
            say("%-24s %10.2f %10.2f %9.2f %7d" % (label, chain[i][0], chain[i][1], float(s.mean()), empty))
        for rel in TARGETS:
            s = counts[TARGETS.index(rel)]
            e = rounds + 1 - ((int(s.max()) - lo) // step + 1)
            say("%-24s %10.2f %10.2f %9.2f %7d" % ("begin(%.2f)" % rel, fresh[rel][0], fresh[rel][1], float(s.mean()), e))
            say("%-24s %10.2f %10.2f %9.2f %7d" % ("rt_render_adaptive(%.2f)" % rel, plain[rel][0], plain[rel][1], float(s.mean()), e))
        for rel in TARGETS:
            say("begin(%.2f) / rt_render_adaptive(%.2f): %.3f (launch), %.3f (device)"
                % (rel, rel, fresh[rel][0] / plain[rel][0], fresh[rel][1] / plain[rel][1]))
        for i in range(1, len(TARGETS)):
            a, b = TARGETS[i - 1], TARGETS[i]
            say("refine(%.2f -> %.2f) / (begin(%.2f) - begin(%.2f)): %.3f (launch), %.3f (device)"
                % (a, b, b, a, chain[i][0] / (fresh[b][0] - fresh[a][0]), chain[i][1] / (fresh[b][1] - fresh[a][1])))
        say("chain begin(%.2f) + refines / begin(%.2f): %.3f (launch)" % (TARGETS[0], TARGETS[-1], sum(c[0] for c in chain) / fresh[TARGETS[-1]][0]))
        O.close()
        W.close()
    ctx.close()
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
