#!/usr/bin/env python3
"""Adaptive sampling of a binary16 world (rt_render_adaptive_h16: the stop rule inside k_render_h<*,3>) against
rt_render on the same world, on ONE GPU.  Configuration C4: 1200x800, 10 000 spheres, octree SPL 32, binary16.

Method: every call goes through one render context on torch's current stream.  Per repeat the RNG states are initialised again and the
device is idle; "kernel" is the device time rt_render_ctx_times reports for the call (the render kernel), "wall" the host's time
from a synchronisation before the call to one after it (the scheduling pass, reused after the warm-up, and the launch overheads
are inside).  Every configuration gets one warm-up call of each kind, then the compared
calls alternate rep by rep; REPS repeats, the median and the range [min .. max] are printed.

  python tools/adaptive_h16_study.py [OUT.txt]
"""
import os
import sys
import time

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

    nx, ny = 1200, 800
    W = rt.World(10000, nx, ny, precision=rt.FP16).upload()
    O = rt.Octree(W, 32).upload()
    ctx = rt.RenderCtx()
    n = nx * ny
    st = rt.alloc_rand_state(nx, ny)
    fb = rt.alloc_fb(nx, ny, precision=rt.FP16)
    spp = torch.zeros(n, dtype=torch.int32, device="cuda")
    state = rt.alloc_adaptive_state(nx, ny)

    def init():
        rt.render_init(nx, ny, st)

    def timed(fn, before=init):
        """(kernel ms, wall ms) of one call"""
        before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return ctx.times()[-1], wall

    def compare(calls):
        """calls: {name: fn or (fn, before)}; {name: ((median, min, max) kernel, (median, min, max) wall)}"""
        calls = {k: v if isinstance(v, tuple) else (v, init) for k, v in calls.items()}
        for fn, before in calls.values():
            timed(fn, before)
        t = {k: [] for k in calls}
        for _ in range(REPS):
            for k, (fn, before) in calls.items():
                t[k].append(timed(fn, before))
        stat = lambda v: (float(np.median(v)), float(min(v)), float(max(v)))
        return {k: (stat([a for a, _ in v]), stat([b for _, b in v])) for k, v in t.items()}

    def row(name, r, extra=""):
        return "%-44s kernel %8.2f ms [%8.2f .. %8.2f]   wall %8.2f ms [%8.2f .. %8.2f]%s" % ((name,) + r[0] + r[1] + (extra,))

    def render(ns):
        return lambda: ctx.render(fb, nx, ny, ns, W, st, O)

    def h16(P, with_state=True):
        return lambda: ctx.render_adaptive_h16(fb, nx, ny, P, W, st, state if with_state else None, O, spp)

    def mean_spp(fn, before=init):
        before()
        fn()
        torch.cuda.synchronize()
        return float(spp.float().mean())

    say("# tools/adaptive_h16_study.py on %s: C4 (%dx%d, N = 10000, octree SPL 32, binary16), kernels %s / %s" %
        (torch.cuda.get_device_name(0), nx, ny, rt.render_kernel_name(W, O, 0), rt.render_kernel_name(W, O, 3)))
    say("# kernel: rt_render_ctx_times; wall: sync to sync; %d alternating repeats after a warm-up of each call: median [min .. max]; floor %.2f" % (REPS, FLOOR))

    # ---- the price of the mode
    P = rt.Adaptive(16, 64, 16, 0.0, FLOOR)
    r = compare({"rt_render(64)": render(64), "rt_render_adaptive_h16 16/64/16 rel 0": h16(P), "... without a state": h16(P, False)})
    say()
    say("## the price of the mode: 16/64/16 at rel_error 0 (every pixel to 64) against rt_render(64); mean spp %.2f" % mean_spp(h16(P)))
    for k in r:
        say(row(k, r[k]))
    base = r["rt_render(64)"][0]
    ratio = r["rt_render_adaptive_h16 16/64/16 rel 0"][0][0] / base[0]
    spread = (base[2] - base[1]) / base[0]
    say("MODE 3 / rt_render(64), kernel medians: %.4f; min-to-max spread of the %d rt_render(64) repeats: %.4f of their median -> %s" %
        (ratio, REPS, spread, "the ratio exceeds 1 by MORE than the spread" if ratio - 1.0 > spread else "within the spread"))

    # ---- the gain
    say()
    say("## the gain: 8/128/8 against rt_render(128)")
    r128 = compare({"rt_render(128)": render(128)})["rt_render(128)"]
    say(row("rt_render(128)", r128, "   mean spp 128.00"))
    for rel in (0.2, 0.1, 0.05):
        P = rt.Adaptive(8, 128, 8, rel, FLOOR)
        rr = compare({"h16": h16(P)})["h16"]
        m = mean_spp(h16(P))
        say(row("rt_render_adaptive_h16 8/128/8 rel %.2f" % rel, rr, "   mean spp %6.2f   kernel / rt_render(128) %.3f   kernel us per 1000 samples taken %.3f"
                % (m, rr[0][0] / r128[0][0], rr[0][0] * 1e3 / (m * n / 1e3))))

    ctx.close()
    O.close()
    W.close()
    if path:
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
