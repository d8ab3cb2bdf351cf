#!/usr/bin/env python3
"""Adaptive sample budgets, measured on ONE GPU (rt_adaptive_budget_select / rt_render_adaptive_spend, DESIGN.md §5.9 "Budgets").

  python tools/adaptive_budget_study.py [OUT.txt]      does a budget pay, and how predictable is it (C3):
      RMSE against rt_render(1024) at an equal mean of 32 spp — uniform 32 against begin at 8 or 16 spp plus a spend — raw and after
      rt_denoise_adaptive with its defaults, with the wall time of each; then the time of a spend of 8, 16 and 32 extra mean spp,
      minimum and maximum of REPS runs after a warm-up (host clock around the call and a device synchronise; the context's events).
  python tools/adaptive_budget_study.py --select [OUT.txt]
      the selection alone at the C3 and C5 frame sizes: host clock over CALLS back-to-back calls and one synchronise, minimum of REPS
      after a warm-up, and a checksum of the chosen set.  RT_AMD_LIB selects another build of the library (a parent commit's, a
      tools/mkvariant.sh variant): equal checksums say both choose the same sets, the times are the A/B.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/adaptive_budget_study.py --kernels
  python tools/adaptive_budget_study.py --kernel-report DIR OUT.txt
      device times of one round: the selection kernels, seed and finalise, the round's render kernel, and k_adapt_refine_seed plus one
      k_adapt_refine_check of a refinement on the same frame (the closest existing per-round bookkeeping); median of REPS calls.
"""
import os
import sys
import time
import zlib

import numpy as np

from kernel_trace import read_trace, short_name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))

REPS = 3
CALLS = 20
FLOOR = 0.02
MAX_SPP = 1024
# (name, nx, ny, spheres, SPL, begin spp)
FRAMES = [("C3", 1200, 800, 10000, 32, 8), ("C5", 3840, 2160, 100000, 320, 16)]


def writer(path):
    out = []

    def say(line=""):
        print(line, flush=True)
        out.append(line)

    def close():
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "a") as f:
                f.write("\n".join(out) + "\n")
    return say, close


def main(path):
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    say, close = writer(path)
    name, nx, ny, n, spl, _ = FRAMES[0]
    npx = nx * ny
    W = rt.World(n, nx, ny).upload()
    O = rt.Octree(W, spl).upload()
    ctx = rt.RenderCtx()
    st = rt.alloc_rand_state(nx, ny)
    fb = rt.alloc_fb(nx, ny)
    den = rt.alloc_fb(nx, ny)
    state = rt.alloc_adaptive_state(nx, ny)
    spp = torch.zeros(npx, dtype=torch.int32, device="cuda")
    hits = rt.alloc_guides(nx, ny)
    work = rt.alloc_denoise_work(nx, ny)
    say("# tools/adaptive_budget_study.py on %s: %s %dx%d, N = %d, octree SPL %d, floor %.2f, %d runs per figure after a warm-up"
        % (torch.cuda.get_device_name(0), name, nx, ny, n, spl, FLOOR, REPS))

    def host(t):
        torch.cuda.synchronize()
        return t.cpu().numpy().reshape(-1, 3).astype(np.float64)

    rt.render_init(nx, ny, st)
    rt.render(fb, nx, ny, 1024, W, st, O)
    ref = host(fb)
    rt.render_guides(W, O, nx, ny, hits)

    def rmse(img):
        m = np.isfinite(ref).all(1) & np.isfinite(img).all(1)
        return float(np.sqrt(np.mean((img[m] - ref[m]) ** 2)))

    def wall(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def frame(lo, extra, batch, rounds):
        """begin at lo spp for every pixel, then a spend of `extra` mean spp; returns (wall ms of begin + spend, of the spend, its device ms)"""
        rt.render_init(nx, ny, st)
        P = rt.Adaptive(lo, lo, 1, 0.0, FLOOR)
        t = wall(lambda: ctx.render_adaptive_begin(fb, nx, ny, P, W, st, state, O, spp))
        if not extra:
            return t, 0.0, 0.0
        B = rt.Budget(extra * npx, rounds, batch, MAX_SPP, FLOOR)
        ctx.times()
        s = wall(lambda: ctx.render_adaptive_spend(fb, nx, ny, B, W, st, state, O, spp))
        return t + s, s, float(ctx.times()[-1])

    def denoised():
        return wall(lambda: rt.denoise_adaptive(den, fb, nx, ny, hits, state, rt.denoise_var_params(), work))

    # ---- 1. does a budget pay: equal total samples, a mean of 32 spp
    say()
    say("## RMSE against rt_render(1024) at a mean of 32 spp, gamma-corrected frame; wall ms = render calls (+ rt_denoise_adaptive, defaults)")
    say("%-34s %9s %9s %8s %10s %10s %10s" % ("frame", "mean spp", "max spp", "wall ms", "RMSE raw", "denoised", "+denoise ms"))
    rows = [("uniform 32 (begin 32/32)", 32, 0, 1, 1)]
    for lo in (8, 16):
        for batch, rounds in ((8, 1), (8, 4), (4, 12), (8, 12)):
            rows.append(("begin %d + spend %d x batch %d" % (lo, rounds, batch), lo, 32 - lo, batch, rounds))
    for label, lo, extra, batch, rounds in rows:
        best = None
        for rep in range(REPS + 1):
            t = frame(lo, extra, batch, rounds)[0]
            td = denoised()
            if rep:
                best = (min(best[0], t), min(best[1], td)) if best else (t, td)
        k = spp.cpu().numpy()
        say("%-34s %9.2f %9d %8.2f %10.6f %10.6f %10.2f" % (label, float(k.mean()), int(k.max()), best[0], rmse(host(fb)), rmse(host(den)), best[1]))

    # ---- 2. predictability: the time of a spend against its budget
    say()
    say("## time of a spend after begin 8/8: batch 8, 4 rounds; minimum and maximum of %d runs" % REPS)
    say("%-16s %10s %10s %10s %10s %12s" % ("extra mean spp", "wall min", "wall max", "device min", "device max", "ms per spp"))
    for extra in (8, 16, 32):
        ts = [frame(8, extra, 8, 4) for _ in range(REPS + 1)][1:]
        w = [t[1] for t in ts]
        d = [t[2] for t in ts]
        say("%-16d %10.2f %10.2f %10.2f %10.2f %12.3f" % (extra, min(w), max(w), min(d), max(d), min(w) / extra))
    rt.render_init(nx, ny, st)
    say("uniform rt_render(32): %.2f ms wall" % min(wall(lambda: rt.render(fb, nx, ny, 32, W, st, O)) for _ in range(REPS + 1)))
    ctx.close()
    close()


def frames_with_state(rt, torch):
    for name, nx, ny, n, spl, lo in FRAMES:
        W = rt.World(n, nx, ny).upload()
        O = rt.Octree(W, spl).upload()
        st = rt.alloc_rand_state(nx, ny)
        fb = rt.alloc_fb(nx, ny)
        state = rt.alloc_adaptive_state(nx, ny)
        spp = torch.zeros(nx * ny, dtype=torch.int32, device="cuda")
        rt.render_init(nx, ny, st)
        rt.render_adaptive_begin(fb, nx, ny, rt.Adaptive(lo, lo, 1, 0.0, FLOOR), W, st, state, O, spp)
        torch.cuda.synchronize()
        yield name, nx, ny, lo, W, O, st, fb, state, spp
        O.close()
        W.close()


def select(path):
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    say, close = writer(path)
    say("# tools/adaptive_budget_study.py --select with %s: %d calls back to back, minimum of %d runs after a warm-up"
        % (os.path.basename(rt.LIB_PATH), CALLS, REPS))
    say("%-6s %10s %10s %12s %12s %12s" % ("frame", "picks", "chosen", "us per call", "us alone", "crc32 of set"))
    ctx = rt.RenderCtx()
    for name, nx, ny, lo, W, O, st, fb, state, spp in frames_with_state(rt, torch):
        npx = nx * ny
        for K in (npx // 4, npx // 64):
            lst = torch.zeros(K, dtype=torch.int32, device="cuda")
            cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
            B = rt.Budget(0, 1, 8, MAX_SPP, FLOOR)
            many, one = [], []
            for rep in range(REPS + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    ctx.adaptive_budget_select(state, nx, ny, B, K, lst, cnt)
                torch.cuda.synchronize()
                many.append((time.perf_counter() - t0) * 1e6 / CALLS)
                t0 = time.perf_counter()
                ctx.adaptive_budget_select(state, nx, ny, B, K, lst, cnt)
                torch.cuda.synchronize()
                one.append((time.perf_counter() - t0) * 1e6)
            c = int(cnt.cpu().numpy().view(np.uint32)[0])
            ids = np.sort(lst.cpu().numpy().view(np.uint32)[:c])
            say("%-6s %10d %10d %12.1f %12.1f %12s" % (name, K, c, min(many[1:]), min(one[1:]), "%08x" % zlib.crc32(ids.tobytes())))
    ctx.close()
    close()


def kernels():
    """per frame, REPS + 1 times: a spend of one round (a quarter of the frame, batch 8), then begin(0.2) and refine(0.2 -> 0.1)"""
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    ctx = rt.RenderCtx()
    for name, nx, ny, lo, W, O, st, fb, state, spp in frames_with_state(rt, torch):
        a, b = rt.Adaptive(lo, lo + 8, 8, 0.2, FLOOR), rt.Adaptive(lo, lo + 8, 8, 0.1, FLOOR)
        for _ in range(REPS + 1):
            ctx.render_adaptive_spend(fb, nx, ny, rt.Budget(8 * (nx * ny // 4), 1, 8, MAX_SPP, FLOOR), W, st, state, O, spp)
            torch.cuda.synchronize()
        for _ in range(REPS + 1):
            rt.render_init(nx, ny, st)
            ctx.render_adaptive_begin(fb, nx, ny, a, W, st, state, O, spp)
            ctx.render_adaptive_refine(fb, nx, ny, a, b, W, st, state, O, spp)
            torch.cuda.synchronize()
        print("%s: %d x spend, %d x (begin + refine)" % (name, REPS + 1, REPS + 1), flush=True)
    ctx.close()


def kernel_report(d, path):
    ev = [(short_name(name), dur) for name, dur in read_trace(d)]
    say, close = writer(path)
    say()
    say("## one round under rocprofv3 --kernel-trace --stats (tools/adaptive_budget_study.py --kernels): a quarter of the frame, batch 8;")
    say("## device time of the kernels, us, median of %d calls after a warm-up" % REPS)
    # split the trace into the frames: every frame's part starts with its first k_budget_keys
    spends, cur, refine = [], None, []
    i = 0
    while i < len(ev):
        nm, dur = ev[i]
        if nm.startswith("k_budget_keys"):
            cur = {"select": 0.0, "seed": 0.0, "final": 0.0, "render": 0.0, "per": {}}
            spends.append(cur)
        if cur is not None and nm.startswith("k_budget_"):
            key = "seed" if "seed" in nm else "final" if "final" in nm else "select"
            cur[key] += dur
            if key == "select":
                cur["per"][nm] = cur["per"].get(nm, 0.0) + dur
            if "final" in nm:
                cur = None
        elif cur is not None and nm.startswith("k_render"):
            cur["render"] += dur
        elif cur is not None and ("rocprim" in nm or "radix" in nm.lower() or "sort" in nm.lower()):
            cur["select"] += dur
            cur["per"]["rocprim sort"] = cur["per"].get("rocprim sort", 0.0) + dur
        if nm.startswith("k_adapt_refine_seed"):
            chk = next((e[1] for e in ev[i + 1:i + 8] if e[0].startswith("k_adapt_refine_check")), float("nan"))
            refine.append((dur, chk))
        i += 1
    per = REPS + 1
    med = lambda v: float(np.median(v))
    say("%-6s %10s %8s %8s %12s %22s %22s" % ("frame", "selection", "seed", "final", "k_render", "k_adapt_refine_seed", "k_adapt_refine_check"))
    for k, fr in enumerate(FRAMES):
        sp = spends[k * per:(k + 1) * per][1:]
        rf = refine[k * per:(k + 1) * per][1:]
        say("%-6s %10.1f %8.1f %8.1f %12.1f %22.1f %22.1f" % (fr[0], med([s["select"] for s in sp]), med([s["seed"] for s in sp]),
            med([s["final"] for s in sp]), med([s["render"] for s in sp]), med([r[0] for r in rf]), med([r[1] for r in rf])))
        for nm in sp[0]["per"]:
            say("         %-28s %8.1f" % (nm, med([s["per"].get(nm, 0.0) for s in sp])))
    close()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--kernels" in sys.argv[1:]:
        kernels()
    elif "--kernel-report" in sys.argv[1:]:
        kernel_report(args[0], args[1])
    elif "--select" in sys.argv[1:]:
        select(args[0] if args else None)
    else:
        main(args[0] if args else None)
