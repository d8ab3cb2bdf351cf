"""Quality and cost of rt_render_guides + rt_denoise on one GPU.

  python tools/denoise_study.py [OUT.txt]                 the default sweep and the quality table on C3, written to OUT.txt
  python tools/denoise_study.py --sweep-only              the sweep alone
  python tools/denoise_study.py --kernels                 guides + a 5-level filter (default weights), REPS times, on C3 and on C5's
                                                          world at 3840x2160:
                                                          the run to put under rocprofv3 --kernel-trace --stats
  python tools/denoise_study.py --kernel-report DIR OUT   per-kernel and per-level times from that run's kernel trace, appended to OUT

C3 is 1200x800, N = 10 000, octree SPL 32.  The reference image is rt_render(1024).  RMSE is that of the gamma-corrected frame, over
the pixels that are finite in the reference, the raw and the denoised frame (the reference's dielectric can take the root of a
negative number, material.h:95); SSIM is tools/image_metrics.py's (the reference notebook's, on 8-bit greyscale).  Times: host clock
around a device synchronise, median of REPS runs after a warm-up.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kernel_trace import read_trace, short_name      # noqa: E402

NX, NY, N, SPL = 1200, 800, 10000, 32
REPS = 7
LEVELS = 5
SWEEP_POW = (-1, 2, 4, 6, 8)
SWEEP_POS = (0.0, 0.002, 0.005, 0.01, 0.02, 0.05)
SWEEP_COL = (0.0, 0.1, 0.2, 0.3, 0.4, 0.6, 1.0)


def median_ms(fn, torch):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    import torch
    import rt_amd as rt
    from image_metrics import compare_frames
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
    hits = rt.alloc_guides(NX, NY)
    work = rt.alloc_denoise_work(NX, NY)

    def render(ns):
        rt.render_init(NX, NY, st)
        rt.render(fb, NX, NY, ns, W, st, O)

    def host(t):
        torch.cuda.synchronize()
        return t.cpu().numpy().reshape(-1, 3).astype(np.float64)

    say("# tools/denoise_study.py: C3 scene %dx%d, N = %d, octree SPL %d, %s" % (NX, NY, N, SPL, torch.cuda.get_device_name(0)))
    render(1024)
    ref = host(fb)
    rt.render_guides(W, O, NX, NY, hits)

    def rmse(img, other):
        m = np.isfinite(ref).all(1) & np.isfinite(img).all(1) & np.isfinite(other).all(1)
        return float(np.sqrt(np.mean((img[m] - ref[m]) ** 2)))

    # ---- 1. the default sweep: C3 at 16 spp, LEVELS levels
    render(16)
    raw = host(fb)
    say()
    say("## default sweep: C3 at 16 spp, %d levels, GAMMA input; RMSE against rt_render(1024) (raw 16 spp: %.6f)" % (LEVELS, rmse(raw, raw)))
    say("%-16s %-16s %-12s %10s" % ("normal_pow_log2", "sigma_position", "sigma_color", "RMSE"))
    best = None
    for npow in SWEEP_POW:
        for sp in SWEEP_POS:
            for sc in SWEEP_COL:
                p = rt.DenoiseParams(rt.DENOISE_INPUT_GAMMA, 1, LEVELS, npow, sp, sc)
                rt.denoise(den, fb, NX, NY, hits, p, work)
                e = rmse(host(den), raw)
                say("%-16d %-16.3g %-12.3g %10.6f" % (npow, sp, sc, e))
                if best is None or e < best[0]:
                    best = (e, npow, sp, sc)
    say("# lowest: normal_pow_log2 %d, sigma_position %g, sigma_color %g: RMSE %.6f" % (best[1:] + (best[0],)))
    e, npow, sp, sc = best
    say()
    say("## levels with those weights (C3, 16 spp)")
    for lv in range(1, rt.DENOISE_MAX_LEVELS + 1):
        rt.denoise(den, fb, NX, NY, hits, rt.DenoiseParams(rt.DENOISE_INPUT_GAMMA, 1, lv, npow, sp, sc), work)
        say("levels %d   RMSE %.6f" % (lv, rmse(host(den), raw)))

    if "--sweep-only" in sys.argv[1:]:
        return
    # ---- 2. quality per time with the library's defaults
    d = rt.DENOISE_DEFAULTS
    P = rt.denoise_params()
    say()
    say("## raw against denoised (defaults: %d levels, normal_pow_log2 %d, sigma_position %g, sigma_color %g); time = median of %d, ms"
        % (d["levels"], d["normal_pow_log2"], d["sigma_position"], d["sigma_color"], REPS))
    say("%-6s %10s %10s %10s %10s | %10s %10s %8s %8s" % ("spp", "render", "guides", "denoise", "total", "RMSE raw", "RMSE den", "SSIM raw", "SSIM den"))
    t_guides = median_ms(lambda: rt.render_guides(W, O, NX, NY, hits), torch)
    for ns in (4, 8, 16, 32, 64, 128):
        t_render = median_ms(lambda: render(ns), torch)
        raw = host(fb)
        t_den = median_ms(lambda: rt.denoise(den, fb, NX, NY, hits, P, work), torch)
        dn = host(den)
        s_raw = compare_frames(raw.reshape(NY, NX, 3), ref.reshape(NY, NX, 3))["ssim"]
        s_den = compare_frames(dn.reshape(NY, NX, 3), ref.reshape(NY, NX, 3))["ssim"]
        say("%-6d %10.2f %10.3f %10.3f %10.2f | %10.6f %10.6f %8.4f %8.4f" % (ns, t_render, t_guides, t_den, t_render + t_guides + t_den,
                                                                          rmse(raw, dn), rmse(dn, raw), s_raw, s_den))
    O.close()
    W.close()
    if path:
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


def kernels():
    """guides + denoise (default weights, 5 levels) REPS + 1 times on C3 and on C5's world at 3840x2160, one stream, nothing else on the GPU"""
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    for n, spl, nx, ny in ((N, SPL, NX, NY), (100000, 320, 3840, 2160)):
        W = rt.World(n, nx, ny)
        O = rt.Octree(W, spl)
        st = rt.alloc_rand_state(nx, ny)
        fb = rt.alloc_fb(nx, ny)
        den = rt.alloc_fb(nx, ny)
        hits = rt.alloc_guides(nx, ny)
        work = rt.alloc_denoise_work(nx, ny)
        rt.render_init(nx, ny, st)
        rt.render(fb, nx, ny, 4, W, st, O)
        torch.cuda.synchronize()
        for _ in range(REPS + 1):
            rt.render_guides(W, O, nx, ny, hits)
            rt.denoise(den, fb, nx, ny, hits, rt.denoise_params(levels=5), work)
            torch.cuda.synchronize()
        print("%dx%d N=%d: %d x (guides + denoise)" % (nx, ny, n, REPS + 1), flush=True)
        O.close()
        W.close()


def kernel_report(d, path):
    """per-kernel times from the kernel trace of a --kernels run: launches are grouped into calls (k_guides, prepare, then a level
    kernel per level) in trace order; the first call of each frame is the warm-up"""
    calls, cur = [], None
    for name, dur in read_trace(d):
        if name.startswith("void rt::k_guides") or name.startswith("rt::k_guides") or "k_guides" in name.split("(")[0]:
            cur = [("guides " + short_name(name), dur)]
            calls.append(cur)
        elif cur is not None and ("k_denoise" in name.split("(")[0]):
            cur.append(("prepare" if "prepare" in name else "level %d" % (len(cur) - 2), dur))
    frames = [("C3 1200x800", 960000), ("C5 world 3840x2160", 3840 * 2160)]
    per = len(calls) // 2
    lines = ["", "## kernel times under rocprofv3 --kernel-trace --stats (tools/denoise_study.py --kernels), median of %d calls, us" % (per - 1)]
    for k, (label, npx) in enumerate(frames):
        group = calls[k * per + 1:(k + 1) * per]
        lines.append("# %s: %d pixels; a level moves ~%.0f MB of unique data (16 B colour + 32 B guide in, 16 B out per pixel)"
                     % (label, npx, npx * 64 / 1e6))
        names = [nm for nm, _ in group[0]]
        total = 0.0
        for q, nm in enumerate(names):
            med = float(np.median([g[q][1] for g in group]))
            total += med if q > 0 else 0.0
            gbs = ""
            if nm.startswith("level"):
                gbs = "   %6.0f GB/s of unique traffic" % (npx * 64 / (med * 1e-6) / 1e9)
            lines.append("%-34s %10.1f%s" % (nm, med, gbs))
        lines.append("%-34s %10.1f" % ("prepare + levels", total))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(path, "a") as fo:
        fo.write(text)


if __name__ == "__main__":
    if "--kernels" in sys.argv[1:]:
        kernels()
    elif "--kernel-report" in sys.argv[1:]:
        i = sys.argv.index("--kernel-report")
        kernel_report(sys.argv[i + 1], sys.argv[i + 2])
    else:
        main()
