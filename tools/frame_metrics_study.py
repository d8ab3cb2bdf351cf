"""rt_frame_compare / rt_frame_levels against the host route they replace, on one GPU.

  python tools/frame_metrics_study.py [OUT.txt]                 metrics and wall times of both routes on C3 and on C5's 3840x2160 frame,
                                                                written to OUT.txt
  python tools/frame_metrics_study.py --kernels                 REPS + 1 x (frame_compare, frame_levels RGBA8) on both frame sizes: the run
                                                                to put under rocprofv3 --kernel-trace --stats
  python tools/frame_metrics_study.py --kernel-report DIR OUT   kernel times from that run's trace, appended to OUT

C3 is 1200x800, N = 10 000, octree SPL 32: rt_render(1024) against 16 spp, raw and denoised (rt_denoise defaults).  The 4K pair is C5's
world (N = 100 000, SPL 320) at 3840x2160, 64 spp against 8 spp.  The host route is what every study tool does today: copy both float
frames to the host, tools/image_metrics.compare_frames (numpy / scipy) and the studies' RMSE over the pixels finite in both frames.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kernel_trace import read_trace      # noqa: E402

REPS = 7
FRAMES = (("C3 1200x800", 10000, 32, 1200, 800, 1024, 16), ("C5 world 3840x2160", 100000, 320, 3840, 2160, 64, 8))


def render_pair(rt, torch, n, spl, nx, ny, ns_ref, ns, denoised):
    """the reference frame, the raw frame and (denoised) the rt_denoise'd raw frame, all on the device"""
    W = rt.World(n, nx, ny)
    O = rt.Octree(W, spl)
    st = rt.alloc_rand_state(nx, ny)
    frames = []
    for s in (ns_ref, ns):
        fb = rt.alloc_fb(nx, ny)
        rt.render_init(nx, ny, st)
        rt.render(fb, nx, ny, s, W, st, O)
        frames.append(fb)
    if denoised:
        hits = rt.alloc_guides(nx, ny)
        rt.render_guides(W, O, nx, ny, hits)
        den = rt.alloc_fb(nx, ny)
        rt.denoise(den, frames[1], nx, ny, hits, rt.denoise_params(), rt.alloc_denoise_work(nx, ny))
        frames.append(den)
    torch.cuda.synchronize()
    O.close()
    W.close()
    return frames


def median_ms(fn, reps=REPS):
    fn()                                                       # warm-up
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    import torch
    import rt_amd as rt
    import image_metrics as im
    torch.cuda.set_device(0)
    path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    out = []

    def say(line=""):
        print(line, flush=True)
        out.append(line)

    say("# tools/frame_metrics_study.py: %s; wall times are medians of %d after a warm-up" % (torch.cuda.get_device_name(0), REPS))
    for label, n, spl, nx, ny, ns_ref, ns, in FRAMES:
        frames = render_pair(rt, torch, n, spl, nx, ny, ns_ref, ns, denoised=(nx == 1200))
        ref = frames[0]
        work = rt.alloc_compare_work(nx, ny)
        dm = torch.zeros(8, dtype=torch.int64, device="cuda")
        say()
        say("## %s, rt_render(%d) against %d spp: device record next to the host route" % (label, ns_ref, ns))
        say("%-10s %-8s %12s %12s %12s %14s %14s" % ("frame", "route", "SSIM", "PSNR dB", "RMSE", "grey differ", "finite pixels"))
        for name, fb in zip(("raw", "denoised"), frames[1:]):
            m = rt.frame_compare(fb, ref, nx, ny, work)
            say("%-10s %-8s %12.6f %12.3f %12.6f %14d %14d" % (name, "device", m.ssim, m.psnr, m.rmse, m.gray_differ, m.finite_pixels))
            a, b = fb.cpu().numpy().reshape(ny, nx, 3), ref.cpu().numpy().reshape(ny, nx, 3)
            h = im.compare_frames(a, b)
            fin = np.isfinite(a).all(2) & np.isfinite(b).all(2)
            rm = float(np.sqrt(np.mean((a[fin].astype(np.float64) - b[fin].astype(np.float64)) ** 2)))
            say("%-10s %-8s %12.6f %12s %12.6f %14s %14d" % (name, "host", h["ssim"], h["psnr_db"], rm, "", int(fin.sum())))
        fb = frames[1]

        def device_route():
            rt.frame_compare(fb, ref, nx, ny, work, d_metrics=dm)
            return rt.frame_metrics(dm)                        # the 64-byte copy synchronises

        def copies():
            return fb.cpu(), ref.cpu()

        def host_route():
            a, b = (t.numpy().reshape(ny, nx, 3) for t in copies())
            im.compare_frames(a, b)
            fin = np.isfinite(a).all(2) & np.isfinite(b).all(2)
            return float(np.sqrt(np.mean((a[fin].astype(np.float64) - b[fin].astype(np.float64)) ** 2)))

        lv = torch.empty(rt.frame_levels_bytes(nx, ny, rt.LEVELS_RGBA8), dtype=torch.uint8, device="cuda")
        p = rt.LevelsParams(rt.DENOISE_INPUT_GAMMA, 1, rt.LEVELS_RGBA8, 1)

        def device_levels():
            rt.frame_levels(lv, fb, nx, ny, p)
            torch.cuda.synchronize()

        def device_levels_copied():
            rt.frame_levels(lv, fb, nx, ny, p)
            return lv.cpu()

        def host_levels():
            return im.ppm_levels(fb.cpu().numpy().reshape(ny, nx, 3)).astype(np.uint8)

        t_dev, t_copy, t_host = median_ms(device_route), median_ms(copies), median_ms(host_route, 3)
        say("# wall, ms: device route (rt_frame_compare + 64-byte copy) %.3f | the two frame copies alone %.3f | host route (copies + "
            "compare_frames + RMSE) %.1f" % (t_dev, t_copy, t_host))
        say("# device route faster than the two copies alone: %s (%.1fx)" % ("yes" if t_dev < t_copy else "NO", t_copy / t_dev))
        say("# wall, ms: rt_frame_levels RGBA8 %.3f, with its %d-byte copy %.3f | host: frame copy + numpy quantisation %.1f"
            % (median_ms(device_levels), lv.numel(), median_ms(device_levels_copied), median_ms(host_levels, 3)))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


def kernels():
    """REPS + 1 x (frame_compare with a map, frame_compare without, frame_levels RGBA8) on synthetic frames of both sizes (the kernels'
    work does not depend on the content)"""
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    for label, _, _, nx, ny, _, _ in FRAMES:
        g = torch.Generator(device="cuda").manual_seed(1)
        a = torch.rand(nx * ny * 3, generator=g, device="cuda")
        b = (a + 0.05 * torch.rand(nx * ny * 3, generator=g, device="cuda")).contiguous()
        work = rt.alloc_compare_work(nx, ny)
        dm = torch.zeros(8, dtype=torch.int64, device="cuda")
        smap = torch.empty((nx - 6) * (ny - 6), dtype=torch.float64, device="cuda")
        lv = torch.empty(rt.frame_levels_bytes(nx, ny, rt.LEVELS_RGBA8), dtype=torch.uint8, device="cuda")
        p = rt.LevelsParams(rt.DENOISE_INPUT_GAMMA, 1, rt.LEVELS_RGBA8, 1)
        torch.cuda.synchronize()
        for _ in range(REPS + 1):
            rt.frame_compare(a, b, nx, ny, work, d_ssim_map=smap, d_metrics=dm)
            rt.frame_compare(a, b, nx, ny, work, d_metrics=dm)
            rt.frame_levels(lv, a, nx, ny, p)
            torch.cuda.synchronize()
        print("%s: %d x (compare + map, compare, levels)" % (label, REPS + 1), flush=True)


def kernel_report(d, path):
    """median kernel times from the trace of a --kernels run: per frame size, the calls come in the order kernels() issues them and the
    first repetition is the warm-up"""
    dur = [(us, name) for name, us in read_trace(d) if "k_frame" in name]
    per = 5 * (REPS + 1)                                       # compare, final, compare, final, levels
    lines = ["", "## kernel times under rocprofv3 --kernel-trace --stats (tools/frame_metrics_study.py --kernels), median of %d calls, us" % REPS,
             "%-22s %24s %24s %24s %16s" % ("frame", "k_frame_compare + map", "k_frame_compare", "k_frame_compare_final", "k_frame_levels")]
    for k, frame in enumerate(FRAMES):
        g = np.array([t for t, _ in dur[k * per:(k + 1) * per]]).reshape(REPS + 1, 5)[1:]
        names = [nm for _, nm in dur[k * per:k * per + 5]]
        assert "final" in names[1] and "final" in names[3] and "levels" in names[4], names
        m = np.median(g, axis=0)
        lines.append("%-22s %24.1f %24.1f %24.1f %16.1f" % (frame[0], m[0], m[2], (m[1] + m[3]) / 2, m[4]))
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
