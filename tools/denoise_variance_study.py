"""Quality and cost of rt_denoise_adaptive (the variance-guided filter on the adaptive state) on one GPU.

  python tools/denoise_variance_study.py [OUT.txt]              the default sweep and the quality table on C3, written to OUT.txt
  python tools/denoise_variance_study.py --kernels              rt_denoise and rt_denoise_adaptive, LEVELS levels each, REPS + 1 times,
                                                                on C3 and on C5's world at 3840x2160: the run to put under
                                                                rocprofv3 --kernel-trace --stats (RT_AMD_LIB selects a variant library)
  python tools/denoise_variance_study.py --kernel-report DIR OUT LABEL   per-level times of both filters from that run's kernel trace,
                                                                appended to OUT under LABEL

C3 is 1200x800, N = 10 000, octree SPL 32.  The reference image is rt_render(1024).  RMSE is that of the gamma-corrected frame over the
pixels that are finite in the reference, the raw and both filtered frames.  A uniform frame of n spp is rt_render_adaptive_begin with
min_spp = max_spp = n (rel_error 0): bit for bit rt_render(n), plus the state.  The adaptive frame is that of DESIGN.md §5.9:
8 / 8 / 128, rel_error 0.10, floor 0.02.
"""
import os
import sys

import numpy as np

from kernel_trace import read_trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))

NX, NY, N, SPL = 1200, 800, 10000, 32
REPS = 7
LEVELS = 5
SWEEP_SPP = (16, 64, 128)
SWEEP_SV = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0)
SWEEP_LEVELS = (1, 2, 3, 5)
TABLE_SPP = (16, 32, 64, 128, 256)
ADAPTIVE = (8, 128, 8, 0.10, 0.02)


def main():
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    out = []

    def say(line=""):
        print(line, flush=True)
        out.append(line)

    W = rt.World(N, NX, NY)
    O = rt.Octree(W, SPL)
    st = rt.alloc_rand_state(NX, NY)
    fb = rt.alloc_fb(NX, NY)
    den = rt.alloc_fb(NX, NY)
    state = rt.alloc_adaptive_state(NX, NY)
    spp = torch.zeros(NX * NY, dtype=torch.int32, device="cuda")
    hits = rt.alloc_guides(NX, NY)
    work = rt.alloc_denoise_work(NX, NY)

    def host(t):
        torch.cuda.synchronize()
        return t.cpu().numpy().reshape(-1, 3).astype(np.float64)

    def begin(P):
        rt.render_init(NX, NY, st)
        rt.render_adaptive_begin(fb, NX, NY, rt.Adaptive(*P), W, st, state, O, spp)
        return host(fb)

    say("# tools/denoise_variance_study.py: C3 scene %dx%d, N = %d, octree SPL %d, %s" % (NX, NY, N, SPL, torch.cuda.get_device_name(0)))
    rt.render_init(NX, NY, st)
    rt.render(fb, NX, NY, 1024, W, st, O)
    ref = host(fb)
    rt.render_guides(W, O, NX, NY, hits)
    d = rt.DENOISE_VAR_DEFAULTS

    def rmse(img, *others):
        m = np.isfinite(ref).all(1) & np.isfinite(img).all(1)
        for o in others:
            m &= np.isfinite(o).all(1)
        return float(np.sqrt(np.mean((img[m] - ref[m]) ** 2)))

    def filtered(**kw):
        rt.denoise_adaptive(den, fb, NX, NY, hits, state, rt.denoise_var_params(**kw), work)
        return host(den)

    # ---- 1. the default sweep: sigma_variance x prefilter x levels at three sample counts
    say()
    say("## default sweep: normal_pow_log2 %d, sigma_position %g; RMSE against rt_render(1024)" % (d["normal_pow_log2"], d["sigma_position"]))
    table = {}
    for n in SWEEP_SPP:
        raw = begin((n, n, 4, 0.0, 0.0))
        say("# %d spp: raw %.6f" % (n, rmse(raw)))
        say("%-6s %-8s %-10s %-16s %10s" % ("spp", "levels", "prefilter", "sigma_variance", "RMSE"))
        for lv in SWEEP_LEVELS:
            for pre in (0, 1):
                for sv in SWEEP_SV:
                    if sv == 0.0 and pre == 1:
                        continue                              # the blur feeds the variance term only
                    e = rmse(filtered(levels=lv, prefilter=pre, sigma_variance=sv), raw)
                    table[(n, lv, pre, sv)] = e
                    say("%-6d %-8d %-10d %-16g %10.6f" % (n, lv, pre, sv, e))
    say()
    say("## one setting for all three sample counts: the worst loss against each count's own optimum, per setting (the ten best)")
    own = {n: min(e for (m, _, _, _), e in table.items() if m == n) for n in SWEEP_SPP}
    settings = sorted({k[1:] for k in table})
    loss = {s: max(table[(n,) + s] / own[n] - 1.0 for n in SWEEP_SPP) for s in settings if all((n,) + s in table for n in SWEEP_SPP)}
    for s in sorted(loss, key=loss.get)[:10]:
        say("levels %d prefilter %d sigma_variance %-5g  worst loss %5.1f %%   " % (s + (100 * loss[s],)) +
            "  ".join("%d spp %.6f (+%.1f %%)" % (n, table[(n,) + s], 100 * (table[(n,) + s] / own[n] - 1.0)) for n in SWEEP_SPP))
    for n in SWEEP_SPP:
        k = min((k for k in table if k[0] == n), key=table.get)
        say("# %d spp optimum: levels %d prefilter %d sigma_variance %g: %.6f" % (k + (own[n],)))

    # ---- 2. raw / rt_denoise defaults / rt_denoise_adaptive defaults
    say()
    say("## raw against rt_denoise (defaults) and rt_denoise_adaptive (defaults: %d levels, prefilter %d, sigma_variance %g)"
        % (d["levels"], d["prefilter"], d["sigma_variance"]))
    say("%-22s %10s %12s %20s %10s" % ("frame", "RMSE raw", "rt_denoise", "rt_denoise_adaptive", "mean spp"))
    for label, P in [("uniform %d spp" % n, (n, n, 4, 0.0, 0.0)) for n in TABLE_SPP] + [("adaptive 8/8/128 0.10", ADAPTIVE)]:
        raw = begin(P)
        rt.denoise(den, fb, NX, NY, hits, rt.denoise_params(), work)
        old = host(den)
        new = filtered()
        say("%-22s %10.6f %12.6f %20.6f %10.2f" % (label, rmse(raw, old, new), rmse(old, raw, new), rmse(new, raw, old), float(spp.float().mean())))
    O.close()
    W.close()
    if path:
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


def kernels():
    """rt_denoise then rt_denoise_adaptive (default weights, LEVELS levels) REPS + 1 times on C3 and on C5's world at 3840x2160"""
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    for n, spl, nx, ny in ((N, SPL, NX, NY), (100000, 320, 3840, 2160)):
        W = rt.World(n, nx, ny)
        O = rt.Octree(W, spl)
        st = rt.alloc_rand_state(nx, ny)
        fb = rt.alloc_fb(nx, ny)
        den = rt.alloc_fb(nx, ny)
        state = rt.alloc_adaptive_state(nx, ny)
        hits = rt.alloc_guides(nx, ny)
        work = rt.alloc_denoise_work(nx, ny)
        rt.render_init(nx, ny, st)
        rt.render_adaptive_begin(fb, nx, ny, rt.Adaptive(4, 8, 4, 0.1, 0.02), W, st, state, O)
        rt.render_guides(W, O, nx, ny, hits)
        torch.cuda.synchronize()
        for _ in range(REPS + 1):
            rt.denoise(den, fb, nx, ny, hits, rt.denoise_params(levels=LEVELS), work)
            rt.denoise_adaptive(den, fb, nx, ny, hits, state, rt.denoise_var_params(levels=LEVELS), work)
            torch.cuda.synchronize()
        print("%dx%d N=%d: %d x (denoise + denoise_adaptive)" % (nx, ny, n, REPS + 1), flush=True)
        O.close()
        W.close()


def kernel_report(d, path, label):
    """per-level times of both filters from the kernel trace of a --kernels run: a prepare kernel opens a call, the level kernels
    that follow are its levels in order; the first call of each filter on each frame is the warm-up"""
    calls, cur = [], None
    for name, dur in read_trace(d):
        name = name.split("(")[0]
        if "k_denoise" not in name:
            continue
        if "prepare" in name:
            cur = ["var" if "k_denoise_var" in name else "old", dur]
            calls.append(cur)
        elif cur is not None:
            cur.append(dur)
    per = len(calls) // 2
    lines = ["", "## %s: kernel times under rocprofv3 --kernel-trace --stats (tools/denoise_variance_study.py --kernels), median of %d calls, us"
             % (label, REPS)]
    for k, frame in enumerate(("C3 1200x800", "C5 world 3840x2160")):
        group = calls[k * per:(k + 1) * per]
        old = np.array([c[1:] for c in group if c[0] == "old"][1:])
        var = np.array([c[1:] for c in group if c[0] == "var"][1:])
        lines.append("# %s" % frame)
        lines.append("%-10s %16s %22s %8s" % ("kernel", "k_denoise_level", "k_denoise_var_level", "ratio"))
        mo, mv = np.median(old, axis=0), np.median(var, axis=0)
        for q in range(old.shape[1]):
            what = "prepare" if q == 0 else "step %d" % (1 << (q - 1))
            lines.append("%-10s %16.1f %22.1f %8.2f" % (what, mo[q], mv[q], mv[q] / mo[q]))
        lines.append("%-10s %16.1f %22.1f %8.2f" % ("call", mo.sum(), mv.sum(), mv.sum() / mo.sum()))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(path, "a") as fo:
        fo.write(text)


if __name__ == "__main__":
    if "--kernels" in sys.argv[1:]:
        kernels()
    elif "--kernel-report" in sys.argv[1:]:
        i = sys.argv.index("--kernel-report")
        kernel_report(sys.argv[i + 1], sys.argv[i + 2], sys.argv[i + 3])
    else:
        main()
