#!/usr/bin/env python3
"""Filter-aware budgets, measured on ONE GPU (rt_adaptive_budget_select_filtered / rt_render_adaptive_spend_filtered, DESIGN.md §5.9
"Filter-aware priority").

  python tools/filtered_budget_study.py [OUT.txt]      does ranking by the filtered error pay (C3):
      RMSE against rt_render(1024) after rt_denoise_adaptive (defaults) at a mean of 16, 32 and 64 spp — U uniform, R begin at a quarter
      of the mean plus rt_render_adaptive_spend (4 rounds), F the same with the filtered spend — raw RMSE and wall time beside it
      (minimum of REPS runs after a warm-up, host clock around the calls and a device synchronise); then the histogram of the
      per-pixel sample counts of R and F at a mean of 32, with 4 rounds of batch 8 and with 12 rounds of batch 8.
  python tools/filtered_budget_study.py --select [OUT.txt]
      the filtered selection alone at the C3 and C5 frame sizes: host clock over CALLS back-to-back calls and one synchronise,
      minimum of REPS after a warm-up, checksums of the key map and of the chosen set.  RT_AMD_LIB selects another build of the
      library (a parent commit's, a tools/mkvariant.sh variant): equal checksums say both rank alike, the times are the A/B.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/filtered_budget_study.py --kernels
  python tools/filtered_budget_study.py --kernel-report DIR OUT.txt
      device times of the key kernel (k_budget_keys_filtered), of the rest of the selection, of k_budget_keys and of one raw and one
      filtered round's render kernel; median of REPS calls after a warm-up.  Once per library as well.
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
    filt = rt.denoise_var_params()
    say("# tools/filtered_budget_study.py on %s: %s %dx%d, N = %d, octree SPL %d, floor %.2f, %d runs per time after a warm-up"
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

    def frame(lo, extra, batch, rounds, filtered):
        """begin at lo spp for every pixel, then a spend of `extra` mean spp; wall ms of both"""
        rt.render_init(nx, ny, st)
        t = wall(lambda: ctx.render_adaptive_begin(fb, nx, ny, rt.Adaptive(lo, lo, 1, 0.0, FLOOR), W, st, state, O, spp))
        if extra:
            B = rt.Budget(extra * npx, rounds, batch, MAX_SPP, FLOOR)
            if filtered:
                t += wall(lambda: ctx.render_adaptive_spend_filtered(fb, nx, ny, B, filt, hits, W, st, state, O, spp))
            else:
                t += wall(lambda: ctx.render_adaptive_spend(fb, nx, ny, B, W, st, state, O, spp))
        return t

    def measure(lo, extra, batch, rounds, filtered):
        best = min([frame(lo, extra, batch, rounds, filtered) for _ in range(REPS + 1)][1:])
        rt.denoise_adaptive(den, fb, nx, ny, hits, state, filt, work)
        k = spp.cpu().numpy()
        return best, rmse(host(fb)), rmse(host(den)), k

    say()
    say("## RMSE against rt_render(1024), gamma-corrected frame, raw and after rt_denoise_adaptive (defaults); wall ms = the render calls")
    say("%-8s %-40s %9s %8s %8s %10s %10s" % ("mean", "frame", "mean spp", "max spp", "wall ms", "RMSE raw", "denoised"))
    hist = {}
    for mean in (16, 32, 64):
        lo, batch = mean // 4, mean // 4
        rows = [("U uniform %d" % mean, mean, 0, 1, 1, False),
                ("R begin %d + spend 4 x batch %d" % (lo, batch), lo, mean - lo, batch, 4, False),
                ("F begin %d + spend_filtered 4 x batch %d" % (lo, batch), lo, mean - lo, batch, 4, True)]
        if mean == 32:
            rows += [("R begin 8 + spend 12 x batch 8", 8, 24, 8, 12, False), ("F begin 8 + spend_filtered 12 x batch 8", 8, 24, 8, 12, True)]
        for label, lo_, extra, b, r, f in rows:
            t, e_raw, e_den, k = measure(lo_, extra, b, r, f)
            say("%-8d %-40s %9.3f %8d %8.2f %10.6f %10.6f" % (mean, label, float(k.mean()), int(k.max()), t, e_raw, e_den))
            if mean == 32 and extra:
                hist[label] = k
    say()
    say("## share of the pixels (per cent) at every sample count, mean of 32 spp")
    counts = sorted(set(int(v) for k in hist.values() for v in np.unique(k)))
    say("%-40s " % "frame" + " ".join("%6d" % c for c in counts))
    for label, k in hist.items():
        say("%-40s " % label + " ".join("%6.2f" % (100.0 * float((k == c).mean())) for c in counts))
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
        hits = rt.alloc_guides(nx, ny)
        rt.render_init(nx, ny, st)
        rt.render_adaptive_begin(fb, nx, ny, rt.Adaptive(lo, lo, 1, 0.0, FLOOR), W, st, state, O, spp)
        rt.render_guides(W, O, nx, ny, hits)
        torch.cuda.synchronize()
        yield name, nx, ny, lo, W, O, st, fb, state, spp, hits
        O.close()
        W.close()


def select(path):
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    say, close = writer(path)
    say("# tools/filtered_budget_study.py --select with %s: %d calls back to back, minimum of %d runs after a warm-up"
        % (os.path.basename(rt.LIB_PATH), CALLS, REPS))
    say("%-6s %10s %10s %12s %12s %14s %14s" % ("frame", "picks", "chosen", "us per call", "raw select", "crc32 of keys", "crc32 of set"))
    ctx = rt.RenderCtx()
    filt = rt.denoise_var_params()
    for name, nx, ny, lo, W, O, st, fb, state, spp, hits in frames_with_state(rt, torch):
        npx = nx * ny
        keys = torch.zeros(npx, dtype=torch.float32, device="cuda")
        for K in (npx // 4, npx // 64):
            lst = torch.zeros(K, dtype=torch.int32, device="cuda")
            cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
            B = rt.Budget(0, 1, 8, MAX_SPP, FLOOR)
            many, raw = [], []
            for rep in range(REPS + 1):
                for which, call in ((raw, lambda: ctx.adaptive_budget_select(state, nx, ny, B, K, lst, cnt)),
                                    (many, lambda: ctx.adaptive_budget_select_filtered(state, hits, nx, ny, B, filt, K, lst, cnt))):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(CALLS):
                        call()
                    torch.cuda.synchronize()
                    which.append((time.perf_counter() - t0) * 1e6 / CALLS)
            ctx.adaptive_budget_select_filtered(state, hits, nx, ny, B, filt, K, lst, cnt, keys)
            torch.cuda.synchronize()
            c = int(cnt.cpu().numpy().view(np.uint32)[0])
            ids = np.sort(lst.cpu().numpy().view(np.uint32)[:c])
            say("%-6s %10d %10d %12.1f %12.1f %14s %14s" % (name, K, c, min(many[1:]), min(raw[1:]), "%08x" % zlib.crc32(keys.cpu().numpy().tobytes()),
                                                       "%08x" % zlib.crc32(ids.tobytes())))
    ctx.close()
    close()


def kernels():
    """per frame, REPS + 1 times each: a filtered selection, then a raw and a filtered spend of one round (a quarter of the frame, batch 8)"""
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    ctx = rt.RenderCtx()
    filt = rt.denoise_var_params()
    for name, nx, ny, lo, W, O, st, fb, state, spp, hits in frames_with_state(rt, torch):
        K = nx * ny // 4
        lst = torch.zeros(K, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        B0, B1 = rt.Budget(0, 1, 8, MAX_SPP, FLOOR), rt.Budget(8 * K, 1, 8, MAX_SPP, FLOOR)
        for _ in range(REPS + 1):
            ctx.adaptive_budget_select_filtered(state, hits, nx, ny, B0, filt, K, lst, cnt)
            torch.cuda.synchronize()
        for _ in range(REPS + 1):
            ctx.render_adaptive_spend(fb, nx, ny, B1, W, st, state, O, spp)
            torch.cuda.synchronize()
        for _ in range(REPS + 1):
            ctx.render_adaptive_spend_filtered(fb, nx, ny, B1, filt, hits, W, st, state, O, spp)
            torch.cuda.synchronize()
        print("%s: %d x select_filtered, spend, spend_filtered" % (name, REPS + 1), flush=True)
    ctx.close()


KEY_KERNELS = ("k_budget_keys_filtered",)


def kernel_report(d, path):
    ev = [(short_name(name), dur) for name, dur in read_trace(d)]
    say, close = writer(path)
    say()
    say("## %s under rocprofv3 --kernel-trace --stats (tools/filtered_budget_study.py --kernels): K a quarter of the frame, batch 8;" % os.path.basename(d.rstrip("/")))
    say("## device time of the kernels, us, median of %d calls after a warm-up" % REPS)
    # a call's kernels start with its key kernel(s); the next key kernel after a k_budget_compact starts the next call
    groups, cur = [], None
    for nm, dur in ev:
        base = nm.split("<")[0]
        if base in ("k_budget_keys", "k_budget_keys_filtered") and (cur is None or cur["done"]):
            cur = {"keys": {}, "rest": 0.0, "render": 0.0, "done": False}
            groups.append(cur)
        if cur is None:
            continue
        if base in KEY_KERNELS or base == "k_budget_keys":
            cur["keys"][base] = cur["keys"].get(base, 0.0) + dur
        elif base in ("k_budget_hist", "k_budget_ties", "k_budget_scan", "k_budget_compact"):
            cur["rest"] += dur
            cur["done"] = base == "k_budget_compact"
        elif base.startswith("k_render"):
            cur["render"] += dur
    fixed = groups
    med = lambda v: float(np.median(v)) if len(v) else float("nan")
    per = REPS + 1
    say("%-6s %-16s %-28s %10s" % ("frame", "call", "kernel", "us"))
    i = 0
    for fr in FRAMES:
        for call in ("select_filtered", "spend (raw)", "spend_filtered"):
            gs = fixed[i:i + per][1:]
            i += per
            names = list(gs[0]["keys"]) if gs else []
            for nm in names:
                say("%-6s %-16s %-28s %10.1f" % (fr[0], call, nm, med([g["keys"].get(nm, 0.0) for g in gs])))
            say("%-6s %-16s %-28s %10.1f" % (fr[0], call, "all key kernels", med([sum(g["keys"].values()) for g in gs])))
            say("%-6s %-16s %-28s %10.1f" % (fr[0], call, "hist x3, ties, scan, compact", med([g["rest"] for g in gs])))
            if call != "select_filtered":
                say("%-6s %-16s %-28s %10.1f" % (fr[0], call, "k_render (the round)", med([g["render"] for g in gs])))
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
