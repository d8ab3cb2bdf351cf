"""Quality and time of rt_render_adaptive on the C3 scene (1200x800, 10 000 spheres, octree SPL 32) on one GPU.

  python tools/adaptive_study.py [OUT.txt]
  python tools/adaptive_study.py --overhead-only      (part 1 alone: the run to put under rocprofv3 --kernel-trace --stats)

1. Round overhead: rel_error = 0 with min 16 / batch 16 / max 64 (every pixel takes all 64 samples, in four rounds) against
   rt_render(64), alternating in one process after a warm-up; host clock around a device synchronise, median of REPS runs.
2. Quality per time: the reference image is rt_render(1024); uniform 32 and 64 spp and adaptive renders over a sweep of rel_error
   (min 8 / batch 8 / max 128, floor FLOOR) report mean spp, median time and the RMSE of the gamma-corrected frame against it,
   over the pixels whose reference colour is finite (the reference's dielectric can take the root of a negative number,
   material.h:95: such a pixel is NaN at every sample count).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))

NX, NY, N, SPL = 1200, 800, 10000, 32
REPS = 7
FLOOR = 0.02
SWEEP = (0.30, 0.20, 0.15, 0.12, 0.10, 0.08, 0.06, 0.05)


def main():
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    overhead_only = "--overhead-only" in sys.argv[1:]
    path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    out = []

    def say(line):
        print(line, flush=True)
        out.append(line)

    W = rt.World(N, NX, NY)
    O = rt.Octree(W, SPL)
    st = rt.alloc_rand_state(NX, NY)
    fb = rt.alloc_fb(NX, NY)
    spp = torch.zeros(NX * NY, dtype=torch.int32, device="cuda")

    def run_uniform(ns):
        rt.render_init(NX, NY, st)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rt.render(fb, NX, NY, ns, W, st, O)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def run_adaptive(params):
        rt.render_init(NX, NY, st)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rt.render_adaptive(fb, NX, NY, params, W, st, O, spp)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def frame():
        return fb.cpu().numpy().reshape(-1, 3).astype(np.float64)

    say("# tools/adaptive_study.py: C3 scene %dx%d, N = %d, octree SPL %d, %s" % (NX, NY, N, SPL, torch.cuda.get_device_name(0)))
    say("# kernels: rt_render %s" % rt.render_kernel_name(W, O))
    # ---- 1. round overhead
    zero = rt.Adaptive(16, 64, 16, 0.0, 0.0)
    for _ in range(3):
        run_uniform(64)
        run_adaptive(zero)
    tu, ta = [], []
    for _ in range(REPS):
        tu.append(run_uniform(64))
        ta.append(run_adaptive(zero))
    mu, ma = float(np.median(tu)), float(np.median(ta))
    say("")
    say("## round overhead (rel_error = 0, 16/16/64 = 4 rounds, every pixel 64 spp), median of %d, ms" % REPS)
    say("rt_render(64)            %8.2f   (runs: %s)" % (mu * 1e3, " ".join("%.2f" % (t * 1e3) for t in tu)))
    say("rt_render_adaptive       %8.2f   (runs: %s)" % (ma * 1e3, " ".join("%.2f" % (t * 1e3) for t in ta)))
    say("ratio                    %8.3f" % (ma / mu))
    if overhead_only:
        return

    # ---- 2. quality per time
    run_uniform(1024)
    ref = frame()
    ok = np.isfinite(ref).all(axis=1)

    def rmse(img):
        m = ok & np.isfinite(img).all(axis=1)
        return float(np.sqrt(np.mean((img[m] - ref[m]) ** 2)))

    say("")
    say("## quality per time: RMSE of the gamma-corrected frame against rt_render(1024) over its %d finite pixels (of %d); time = median of %d, ms"
        % (int(ok.sum()), ok.size, REPS))
    say("%-44s %9s %9s %10s" % ("render", "mean spp", "ms", "RMSE"))
    for ns in (16, 32, 64, 128):
        ts = [run_uniform(ns) for _ in range(REPS)]
        say("%-44s %9.2f %9.2f %10.6f" % ("rt_render(%d)" % ns, ns, float(np.median(ts)) * 1e3, rmse(frame())))
    for rel in SWEEP:
        P = rt.Adaptive(8, 128, 8, rel, FLOOR)
        run_adaptive(P)
        ts = [run_adaptive(P) for _ in range(REPS)]
        mean = float(spp.double().mean().item())
        say("%-44s %9.2f %9.2f %10.6f" % ("adaptive 8/8/128 rel_error %.2f floor %.2f" % (rel, FLOOR), mean, float(np.median(ts)) * 1e3, rmse(frame())))
    O.close()
    W.close()
    if path:
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
