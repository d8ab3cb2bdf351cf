"""History-aware budgets (rt_render_adaptive_spend_temporal) against the raw budget and uniform sampling at equal samples, on one GPU.

  python tools/temporal_budget_study.py [OUT.txt]                 the equal-samples table on C3, written to OUT.txt; the d_keys map of the
                                                                  last orbit frame goes next to it as OUT_keys.npy (kept out of git)
  python tools/temporal_budget_study.py --kernels                 rt_temporal_accumulate + rt_adaptive_budget_select_temporal REPS + 1 times
                                                                  on C3 and on C5's world at 3840x2160: the run to put under
                                                                  rocprofv3 --kernel-trace --stats
  python tools/temporal_budget_study.py --kernel-report DIR OUT   the kernel times of that run's trace, appended to OUT

The set-up is that of tools/temporal_study.py: C3 (1200x800, N = 10 000, octree SPL 32), FRAMES frames on a static camera and on the
orbit of STEP degrees a frame, RNG states carried on from frame to frame, the reference rt_render(1024) at the last camera, RMSE of the
gamma-corrected last frame — as rendered ("frame") and after rt_denoise_history at its defaults on the history ("hist+filt") — over
the pixels finite in the reference and in all three results, once over all of them and once over those whose first hit is lambertian.
Every frame spends the same mean of SPP samples a pixel, three ways:
  uniform   rt_render_adaptive_begin at SPP everywhere
  raw       begin at LOW everywhere, then (SPP - LOW) x pixels samples by rt_render_adaptive_spend (this frame's own error)
  history   the same by rt_render_adaptive_spend_temporal (the error left after the merge with the last frame's history)
and each way keeps its own chain of histories: rt_temporal_accumulate (defaults) after the spend.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kernel_trace import durations, read_trace                                             # noqa: E402
from temporal_study import FRAMES, N, NX, NY, REPS, SPL, SPP, STEP, Path, orbit_camera      # noqa: E402

LOW = 8
ROUNDS, BATCH, MAX_SPP, FLOOR = 4, 4, 1024, 0.02
WAYS = ("uniform", "raw", "history")
# bytes k_budget_keys_temporal has to move per pixel: the state (24), this frame's guide (32), of the last frame one guide (32) and one
# history (20) — and the key word written (4; 8 with the float map)
BYTES_PER_PIXEL = 24 + 32 + 32 + 20 + 4


class Chain:
    """one way of spending a frame's samples, over the frames of a camera path: its RNG states, its histories"""

    def __init__(self, rt, torch, way, nx, ny):
        self.rt, self.torch, self.way, self.nx, self.ny = rt, torch, way, nx, ny
        self.st = rt.alloc_rand_state(nx, ny)
        rt.render_init(nx, ny, self.st)
        self.hist = [rt.alloc_temporal_history(nx, ny), rt.alloc_temporal_history(nx, ny)]
        self.prev = None                       # (guides, camera) of the last frame
        self.frames = 0
        self.tp = rt.temporal_params()

    def inputs(self, hits):
        if self.prev is None:
            return self.rt.temporal_inputs(hits)
        return self.rt.temporal_inputs(hits, self.hist[(self.frames + 1) & 1], self.prev[0], self.prev[1])

    def frame(self, W, O, keys_out=None):
        """one frame at the camera of W: returns (fb, state, hits, this frame's history)"""
        rt, nx, ny = self.rt, self.nx, self.ny
        n = nx * ny
        fb, state, hits, spp = rt.alloc_fb(nx, ny), rt.alloc_adaptive_state(nx, ny), rt.alloc_guides(nx, ny), self.torch.zeros(n, dtype=self.torch.int32, device="cuda")
        first = SPP if self.way == "uniform" else LOW
        rt.render_adaptive_begin(fb, nx, ny, rt.Adaptive(first, first, BATCH, 0.0, 0.0), W, self.st, state, O, spp)
        rt.render_guides(W, O, nx, ny, hits)
        budget = rt.Budget((SPP - LOW) * n, ROUNDS, BATCH, MAX_SPP, FLOOR)
        tin = self.inputs(hits)
        if keys_out is not None:
            ctx = rt.RenderCtx()
            lst, cnt = self.torch.zeros(n, dtype=self.torch.int32, device="cuda"), self.torch.zeros(1, dtype=self.torch.int32, device="cuda")
            ctx.adaptive_budget_select_temporal(state, W, nx, ny, budget, tin, self.tp, n // 8, lst, cnt, keys_out)
            self.torch.cuda.synchronize()
            ctx.close()
        if self.way == "raw":
            rt.render_adaptive_spend(fb, nx, ny, budget, W, self.st, state, O, spp)
        elif self.way == "history":
            rt.render_adaptive_spend_temporal(fb, nx, ny, budget, tin, self.tp, W, self.st, state, O, spp)
        out, last = self.hist[self.frames & 1], self.hist[(self.frames + 1) & 1]
        rt.temporal_accumulate(out, last if self.prev else None, hits, self.prev[0] if self.prev else None, self.prev[1] if self.prev else None,
                               state, W, nx, ny, self.tp)
        self.torch.cuda.synchronize()
        self.prev = (hits, W.camera.copy())
        self.frames += 1
        return fb, state, hits, out, spp


def main():
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    out = []

    def say(line=""):
        print(line, flush=True)
        out.append(line)

    def host(t):
        torch.cuda.synchronize()
        return t.cpu().numpy().reshape(-1, 3).astype(np.float64)

    n = NX * NY
    work = rt.alloc_denoise_work(NX, NY)
    d = rt.TEMPORAL_DEFAULTS
    say("# tools/temporal_budget_study.py: C3 scene %dx%d, N = %d, octree SPL %d, %d frames at a mean of %d spp, %s" % (NX, NY, N, SPL, FRAMES, SPP, torch.cuda.get_device_name(0)))
    say("# uniform: %d spp everywhere.  raw / history: begin at %d spp, then %d x pixels samples in %d rounds of batch %d (max_spp %d, floor %g) by"
        % (SPP, LOW, SPP - LOW, ROUNDS, BATCH, MAX_SPP, FLOOR))
    say("# rt_render_adaptive_spend / rt_render_adaptive_spend_temporal.  rt_temporal_accumulate at its defaults (max_history %d, reuse_specular %d,"
        % (d["max_history"], d["reuse_specular"]))
    say("# position_tolerance %g, normal_min_dot %g) after every frame; rt_denoise_history at its defaults on the last." % (d["position_tolerance"], d["normal_min_dot"]))
    base = rt.World(N, NX, NY)
    kind = base.spheres["material"].astype(np.int32)
    for label, step in (("static camera", 0.0), ("orbit, %g degrees a frame" % STEP, STEP)):
        degs = [f * step for f in range(FRAMES)]
        worlds = {deg: rt.World(N, NX, NY, spheres=base.spheres, camera=orbit_camera(rt, deg, NX, NY)) for deg in set(degs)}
        trees = {deg: rt.Octree(W, SPL) for deg, W in worlds.items()}
        res = {}
        for way in WAYS:
            chain = Chain(rt, torch, way, NX, NY)
            for f, deg in enumerate(degs):
                keys = None
                if way == "history" and step and f == FRAMES - 1 and path:
                    keys = torch.zeros(n, dtype=torch.float32, device="cuda")
                fb, state, hits, hist, spp = chain.frame(worlds[deg], trees[deg], keys)
                if keys is not None:
                    kp = os.path.splitext(os.path.abspath(path))[0] + "_keys.npy"
                    os.makedirs(os.path.dirname(kp), exist_ok=True)
                    np.save(kp, keys.cpu().numpy().reshape(NY, NX))
            den = rt.alloc_fb(NX, NY)
            rt.denoise_history(den, fb, NX, NY, hits, hist, rt.denoise_var_params(), work)
            hh = hist.cpu().numpy()
            k = spp.cpu().numpy()
            res[way] = dict(img=host(den), raw=host(fb), neff=hh[4 * n:].copy(), k=k, hits=hits.cpu().numpy().view(rt.hit_record_dtype))
        last_W, last_O = worlds[degs[-1]], trees[degs[-1]]
        fb, st = rt.alloc_fb(NX, NY), rt.alloc_rand_state(NX, NY)
        rt.render_init(NX, NY, st)
        rt.render(fb, NX, NY, 1024, last_W, st, last_O)
        ref = host(fb)
        sphere = res["uniform"]["hits"]["sphere"]
        lamb = (sphere >= 0) & (kind[np.clip(sphere, 0, None)] == rt.MAT_LAMBERTIAN)
        fin = np.isfinite(ref).all(1)
        for way in WAYS:
            fin &= np.isfinite(res[way]["img"]).all(1) & np.isfinite(res[way]["raw"]).all(1)

        def e(img, m):
            return float(np.sqrt(np.mean((img[m] - ref[m]) ** 2)))

        say()
        say("## %s: RMSE of the last frame against rt_render(1024) at its camera (%d pixels, %d lambertian)" % (label, fin.sum(), (fin & lamb).sum()))
        say("%-10s %22s %22s %10s %8s %14s %14s" % ("", "all: frame hist+filt", "lambertian: frame hist+filt", "mean spp", "max spp", "spp lambertian", "spp specular"))
        for way in WAYS:
            r = res[way]
            spec = (sphere >= 0) & ~lamb
            say("%-10s %11.5f %10.5f %11.5f %10.5f %10.3f %8d %14.2f %14.2f"
                % (way, e(r["raw"], fin), e(r["img"], fin), e(r["raw"], fin & lamb), e(r["img"], fin & lamb), r["k"].mean(), r["k"].max(),
                   r["k"][lamb].mean(), r["k"][spec].mean()))
        for T in trees.values():
            T.close()
        for W in worlds.values():
            W.close()
    base.close()
    if path:
        say()
        say("# the history key of every pixel of the last orbit frame (before its spend): %s, float32 [%d, %d]" % (os.path.basename(os.path.splitext(path)[0] + "_keys.npy"), NY, NX))
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


def kernels():
    """two frames STEP degrees apart, then rt_temporal_accumulate and rt_adaptive_budget_select_temporal (defaults, a tenth of the pixels)
    REPS + 1 times, on C3 and on C5's world at 3840x2160"""
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    ctx = rt.RenderCtx()
    tp = rt.temporal_params()
    for n, spl, nx, ny in ((N, SPL, NX, NY), (100000, 320, 3840, 2160)):
        P = Path(rt, torch, n, spl, nx, ny, [0.0, STEP], 4)
        a, b = P.frames
        px = nx * ny
        h0, h1 = rt.alloc_temporal_history(nx, ny), rt.alloc_temporal_history(nx, ny)
        lst, cnt = torch.zeros(px, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        rt.temporal_accumulate(h0, None, a["hits"], None, None, a["state"], a["W"], nx, ny, tp)
        torch.cuda.synchronize()
        tin = rt.temporal_inputs(b["hits"], h0, a["hits"], a["cam"])
        budget = rt.Budget(0, 1, 4, 1024, FLOOR)
        for _ in range(REPS + 1):
            rt.temporal_accumulate(h1, h0, b["hits"], a["hits"], a["cam"], b["state"], b["W"], nx, ny, tp)
            ctx.adaptive_budget_select_temporal(b["state"], b["W"], nx, ny, budget, tin, tp, px // 10, lst, cnt)
            torch.cuda.synchronize()
        took = float((h1[4 * px:] > 4).float().mean())
        print("%dx%d N=%d: %d x (temporal_accumulate + budget_select_temporal), %.1f %% of the pixels took history, %d picked"
              % (nx, ny, n, REPS + 1, 100 * took, int(cnt.cpu().numpy()[0])), flush=True)
        P.close()
    ctx.close()


def kernel_report(d, path):
    """times of k_budget_keys_temporal beside k_temporal_accumulate (the calls with a history) from the kernel trace of a --kernels run:
    median, minimum and maximum of REPS calls; the first call of each kernel on each frame size is the warm-up"""
    ev = read_trace(d)
    acc, key = durations(ev, "k_temporal_accumulate"), durations(ev, "k_budget_keys_temporal")
    lines = ["", "## kernel times under rocprofv3 --kernel-trace --stats (tools/temporal_budget_study.py --kernels), %d calls each, us" % REPS,
             "# k_budget_keys_temporal has to move %d bytes a pixel (state 24, guides 32 + 32, history 20 read, key 4 written); k_temporal_accumulate 128" % BYTES_PER_PIXEL,
             "%-22s %38s %10s %38s" % ("frame", "k_budget_keys_temporal med (min .. max)", "GB/s", "k_temporal_accumulate med (min .. max)")]
    for k, (frame, px) in enumerate((("C3 1200x800", NX * NY), ("C5 world 3840x2160", 3840 * 2160))):
        a = acc[k * (REPS + 2) + 2:(k + 1) * (REPS + 2)]          # per frame size: the first frame's call, the warm-up, REPS timed calls
        b = key[k * (REPS + 1) + 1:(k + 1) * (REPS + 1)]          # the warm-up, REPS timed calls
        lines.append("%-22s %16.1f (%6.1f .. %6.1f) %14.0f %16.1f (%6.1f .. %6.1f)"
                     % (frame, np.median(b), min(b), max(b), BYTES_PER_PIXEL * px / (np.median(b) * 1e-6) / 1e9, np.median(a), min(a), max(a)))
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
