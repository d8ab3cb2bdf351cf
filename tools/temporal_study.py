"""Quality and cost of temporal accumulation (rt_temporal_accumulate, rt_denoise_history) on one GPU.

  python tools/temporal_study.py [OUT.txt]                        the quality tables and the parameter sweeps on C3, written to OUT.txt
  python tools/temporal_study.py --rectify [OUT.txt]              history rectification (rt_temporal_accumulate_rectified): the sweep of
                                                                  gamma, radius and min_count on five camera scenarios and the two moving
                                                                  scenes of tools/animate_study.py, and the setting that loses least
  python tools/temporal_study.py --rectify-kernels                k_temporal_accumulate_moving and k_temporal_accumulate_rectified side
                                                                  by side, REPS + 1 times each on C3 and at 3840x2160: for rocprofv3
  python tools/temporal_study.py --rectify-kernel-report DIR OUT  the kernel times of that run's trace, appended to OUT
  python tools/temporal_study.py --rectify-pmc-report DIR OUT     the counters of --rectify-kernels runs under rocprofv3 --pmc (every
                                                                  *counter_collection.csv below DIR), per kernel and frame size, appended to OUT
  python tools/temporal_study.py --kernels                        rt_temporal_accumulate + rt_denoise_history REPS + 1 times on C3 and on
                                                                  C5's world at 3840x2160: the run to put under rocprofv3 --kernel-trace --stats
  python tools/temporal_study.py --kernel-report DIR OUT          the kernel times of that run's trace, appended to OUT

C3 is 1200x800, N = 10 000, octree SPL 32.  The camera path orbits create_world's camera (lookfrom (13, 2, 3)) about the y axis: FRAMES
frames, STEP degrees apart.  Every frame takes SPP samples a pixel — rt_render_adaptive_begin with min_spp = max_spp = SPP, rel_error 0 —
with the RNG states carried on from frame to frame, never re-initialised.  The reference image is rt_render(1024) at the last camera.
RMSE is that of the gamma-corrected frame (the unfiltered history: sqrt of its mean) over the pixels that are finite in the reference
and in all four frames compared, once over all of them and once over those whose first hit is lambertian.
"""
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))                  # temporal_model.reproject: how far the image moves; world_cases

from kernel_trace import durations, is_instance, read_trace      # noqa: E402
from world_cases import orbit_camera                             # noqa: E402  (the tests' camera path, the same orbit)

NX, NY, N, SPL = 1200, 800, 10000, 32
FRAMES, STEP, SPP = 8, 0.2, 16
REPS = 7
SWEEP_HISTORY = (8, 16, 32, 64, 128, 1 << 30)
SWEEP_TOLERANCE = (0.001, 0.003, 0.01, 0.03, 0.1, 0.3, 1.0)
JOINT_HISTORY, JOINT_TOLERANCE = (8, 16, 24, 32, 48, 64), (0.01, 0.03, 0.1)      # the grid the defaults are chosen on
# bytes k_temporal_accumulate has to move per pixel: the state (24), this frame's guide (32) and history (20 written), and of the last
# frame one guide (32) and one history (20) — the four gathers of neighbouring pixels overlap, each byte of the last frame is needed once
BYTES_PER_PIXEL = 24 + 32 + 20 + 32 + 20


class Path:
    """FRAMES frames of SPP samples on a camera path (degrees per frame), each with its state, frame and guides on the device"""

    def __init__(self, rt, torch, n, spl, nx, ny, degs, spp):
        base = rt.World(n, nx, ny)
        self.kind = base.spheres["material"].astype(np.int32)
        st = rt.alloc_rand_state(nx, ny)
        rt.render_init(nx, ny, st)
        self.worlds, self.trees, self.frames = {}, {}, []
        for deg in degs:
            if deg not in self.worlds:
                self.worlds[deg] = rt.World(n, nx, ny, spheres=base.spheres, camera=orbit_camera(rt, deg, nx, ny))
                self.trees[deg] = rt.Octree(self.worlds[deg], spl)
            W, O = self.worlds[deg], self.trees[deg]
            fb, state, hits = rt.alloc_fb(nx, ny), rt.alloc_adaptive_state(nx, ny), rt.alloc_guides(nx, ny)
            rt.render_adaptive_begin(fb, nx, ny, rt.Adaptive(spp, spp, 4, 0.0, 0.0), W, st, state, O)
            rt.render_guides(W, O, nx, ny, hits)
            self.frames.append(dict(W=W, O=O, cam=W.camera.copy(), fb=fb, state=state, hits=hits))
        torch.cuda.synchronize()
        base.close()

    def history(self, rt, nx, ny, p, rectify=None):
        """the history of the last frame: the chain over all frames with the parameters p (rectify: a TemporalRectify for the rectified call)"""
        bufs = [rt.alloc_temporal_history(nx, ny), rt.alloc_temporal_history(nx, ny)]
        for f, fr in enumerate(self.frames):
            prev = self.frames[f - 1] if f else None
            args = (bufs[f & 1], bufs[(f + 1) & 1] if f else None, fr["hits"], prev["hits"] if f else None, prev["cam"] if f else None,
                    fr["state"], fr["W"], nx, ny, p)
            if rectify is None:
                rt.temporal_accumulate(*args)
            else:
                rt.temporal_accumulate_rectified(*args, rectify)
        return bufs[(len(self.frames) - 1) & 1]

    def close(self):
        for O in self.trees.values():
            O.close()
        for W in self.worlds.values():
            W.close()


def main():
    import torch
    import rt_amd as rt
    import temporal_model
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
    work, den = rt.alloc_denoise_work(NX, NY), rt.alloc_fb(NX, NY)
    d = rt.TEMPORAL_DEFAULTS
    say("# tools/temporal_study.py: C3 scene %dx%d, N = %d, octree SPL %d, %d frames of %d spp, %s" % (NX, NY, N, SPL, FRAMES, SPP, torch.cuda.get_device_name(0)))
    say("# defaults: max_history %d, reuse_specular %d, position_tolerance %g, normal_min_dot %g; rt_denoise_adaptive / rt_denoise_history at their defaults"
        % (d["max_history"], d["reuse_specular"], d["position_tolerance"], d["normal_min_dot"]))
    joint = {}
    for label, step in (("static camera", 0.0), ("orbit, %g degrees a frame" % STEP, STEP)):
        P = Path(rt, torch, N, SPL, NX, NY, [f * step for f in range(FRAMES)], SPP)
        last = P.frames[-1]
        fb, st = rt.alloc_fb(NX, NY), rt.alloc_rand_state(NX, NY)
        rt.render_init(NX, NY, st)
        rt.render(fb, NX, NY, 1024, last["W"], st, last["O"])
        ref = host(fb)
        raw = host(last["fb"])
        rt.denoise_adaptive(den, last["fb"], NX, NY, last["hits"], last["state"], rt.denoise_var_params(), work)
        one = host(den)
        sphere = last["hits"].cpu().numpy().view(rt.hit_record_dtype)["sphere"]
        lamb = (sphere >= 0) & (P.kind[np.clip(sphere, 0, None)] == rt.MAT_LAMBERTIAN)
        if step:
            cur = last["hits"].cpu().numpy().view(rt.hit_record_dtype)
            _, fx, fy = temporal_model.reproject(np.asarray(cur["p"], np.float32), P.frames[-2]["cam"][0], NX, NY)
            j, i = np.divmod(np.arange(n), NX)
            say("# the image moves by a median of %.2f pixels from one frame to the next (first hits of the last frame)"
                % float(np.median(np.hypot(fx - i, fy - j)[sphere >= 0])))

        def row(name, p):
            h = P.history(rt, NX, NY, p)
            rt.denoise_history(den, last["fb"], NX, NY, last["hits"], h, rt.denoise_var_params(), work)
            filt = host(den)
            hh = h.cpu().numpy()
            acc = np.sqrt(hh[:4 * n].reshape(n, 4)[:, :3].astype(np.float64))
            neff = hh[4 * n:]
            acc = np.where((neff > 0)[:, None], acc, raw)                       # an empty pixel shows the frame's own value
            took = neff > SPP
            fin = np.isfinite(ref).all(1) & np.isfinite(raw).all(1) & np.isfinite(one).all(1) & np.isfinite(acc).all(1) & np.isfinite(filt).all(1)

            def e(img, m):
                return float(np.sqrt(np.mean((img[m] - ref[m]) ** 2)))
            cells = []
            for m in (fin, fin & lamb):
                cells += [e(raw, m), e(one, m), e(acc, m), e(filt, m)]
            say("%-34s " % name + " ".join("%9.5f" % c for c in cells) + " %8.1f %% %8.1f %% %8.1f" % (100.0 * took.mean(), 100.0 * took[lamb].mean(), float(neff[took].mean()) if took.any() else 0.0))
            return cells[3]                                                      # rt_denoise_history over all pixels

        say()
        say("## %s: RMSE of the last frame against rt_render(1024) at its camera" % label)
        say("%-34s %s %s %10s %10s %8s" % ("", "all pixels: raw  adaptive   history  hist+filt", " lambertian: raw  adaptive   history  hist+filt", "took", "took lamb", "neff"))
        row("defaults", rt.temporal_params())
        for mh in SWEEP_HISTORY:
            row("max_history %d" % mh, rt.temporal_params(max_history=mh))
        for tol in SWEEP_TOLERANCE:
            row("position_tolerance %g" % tol, rt.temporal_params(position_tolerance=tol))
        for tol in (d["position_tolerance"], 0.1):
            row("reuse_specular 1, tolerance %g" % tol, rt.temporal_params(reuse_specular=1, position_tolerance=tol))
        for nd in (-1.0, 0.5, 0.99):
            row("normal_min_dot %g" % nd, rt.temporal_params(normal_min_dot=nd))
        for mh in JOINT_HISTORY:
            for tol in JOINT_TOLERANCE:
                joint[(label, mh, tol)] = row("max_history %d, tolerance %g" % (mh, tol), rt.temporal_params(max_history=mh, position_tolerance=tol))
        P.close()
    say()
    say("## one setting for both cameras: rt_denoise_history over all pixels, the worst loss against each camera's own optimum on the grid")
    labels = sorted({k[0] for k in joint})
    own = {c: min(e for k, e in joint.items() if k[0] == c) for c in labels}
    loss = {(mh, tol): max(joint[(c, mh, tol)] / own[c] - 1.0 for c in labels) for mh in JOINT_HISTORY for tol in JOINT_TOLERANCE}
    for mh, tol in sorted(loss, key=loss.get)[:8]:
        say("max_history %-3d position_tolerance %-5g worst loss %5.1f %%   " % (mh, tol, 100 * loss[(mh, tol)]) +
            "  ".join("%s %.5f (+%.1f %%)" % (c.split(",")[0], joint[(c, mh, tol)], 100 * (joint[(c, mh, tol)] / own[c] - 1.0)) for c in labels))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


def kernels():
    """two frames STEP degrees apart, then rt_temporal_accumulate and rt_denoise_history (defaults) REPS + 1 times, on C3 and on C5's
    world at 3840x2160"""
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    for n, spl, nx, ny in ((N, SPL, NX, NY), (100000, 320, 3840, 2160)):
        P = Path(rt, torch, n, spl, nx, ny, [0.0, STEP], 4)
        a, b = P.frames
        h0, h1 = rt.alloc_temporal_history(nx, ny), rt.alloc_temporal_history(nx, ny)
        work, den = rt.alloc_denoise_work(nx, ny), rt.alloc_fb(nx, ny)
        rt.temporal_accumulate(h0, None, a["hits"], None, None, a["state"], a["W"], nx, ny, rt.temporal_params())
        torch.cuda.synchronize()
        for _ in range(REPS + 1):
            rt.temporal_accumulate(h1, h0, b["hits"], a["hits"], a["cam"], b["state"], b["W"], nx, ny, rt.temporal_params())
            rt.denoise_history(den, b["fb"], nx, ny, b["hits"], h1, rt.denoise_var_params(), work)
            torch.cuda.synchronize()
        took = float((h1[4 * nx * ny:] > 4).float().mean())
        print("%dx%d N=%d: %d x (temporal_accumulate + denoise_history), %.1f %% of the pixels took history" % (nx, ny, n, REPS + 1, 100 * took), flush=True)
        P.close()


def kernel_report(d, path):
    """median times of k_temporal_accumulate (the calls with a history) and of k_denoise_var_level<true,1> from the kernel trace of a
    --kernels run; the first call on each frame size is the warm-up"""
    ev = read_trace(d)
    acc, lev = durations(ev, "k_temporal_accumulate"), durations(ev, "k_denoise_var_level", True, 1)
    per = REPS + 2                                     # per frame size: the first frame's call, the warm-up and REPS timed calls
    lines = ["", "## kernel times under rocprofv3 --kernel-trace --stats (tools/temporal_study.py --kernels), median of %d calls, us" % REPS,
             "# k_temporal_accumulate has to move %d bytes a pixel (state 24, guides 32 + 32, history 20 read + 20 written)" % BYTES_PER_PIXEL,
             "%-22s %24s %12s %30s" % ("frame", "k_temporal_accumulate", "GB/s", "k_denoise_var_level<true,1>")]
    for k, (frame, px) in enumerate((("C3 1200x800", NX * NY), ("C5 world 3840x2160", 3840 * 2160))):
        a = np.median(acc[k * per + 2:(k + 1) * per])
        first = acc[k * per]
        l = np.median(lev[k * (REPS + 1) + 1:(k + 1) * (REPS + 1)])
        lines.append("%-22s %24.1f %12.0f %30.1f" % (frame, a, BYTES_PER_PIXEL * px / (a * 1e-6) / 1e9, l))
        lines.append("%-22s %24.1f %12s" % ("  (first frame, no history)", first, "-"))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(path, "a") as fo:
        fo.write(text)


RECTIFY_GAMMA, RECTIFY_RADIUS, RECTIFY_MIN_COUNT = (0.5, 1.0, 1.5, 2.0, 3.0), (1, 2), (2, 4)
RECTIFY_SCENARIOS = (("static camera", 0.0, 0), ("static camera, reuse_specular 1", 0.0, 1), ("orbit %g deg" % STEP, STEP, 0),
                     ("orbit %g deg, reuse_specular 1" % STEP, STEP, 1), ("orbit 1 deg", 1.0, 0))


def rectify_main():
    """the sweep of rt_temporal_accumulate_rectified.  The figure of merit of every scenario is the RMSE of the unfiltered history (sqrt
    of its mean, gamma frame) against the reference of the last frame over every pixel that is finite and not empty — the one figure
    that exists for camera paths and moving scenes alike.  (0, 0, 0) is the unrectified call."""
    import torch
    import rt_amd as rt
    import animate_study
    torch.cuda.set_device(0)
    path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    out = []

    def say(line=""):
        print(line, flush=True)
        out.append(line)

    settings = [(0, 0, 0.0)] + [(r, mc, g) for r in RECTIFY_RADIUS for mc in RECTIFY_MIN_COUNT for g in RECTIFY_GAMMA]
    n = NX * NY
    d = rt.TEMPORAL_RECTIFY_DEFAULTS
    say("# tools/temporal_study.py --rectify: C3 scene %dx%d, N = %d, octree SPL %d, %d frames of %d spp, %s" % (NX, NY, N, SPL, FRAMES, SPP, torch.cuda.get_device_name(0)))
    say("# defaults: radius %d, min_count %d, gamma %g; the temporal parameters at their defaults but for reuse_specular where stated"
        % (d["radius"], d["min_count"], d["gamma"]))
    say("# RMSE of sqrt(history) against rt_render(1024) at the last camera; all = every finite non-empty pixel, lamb = lambertian first hits")
    table, paths = {}, {}
    for label, step, spec in RECTIFY_SCENARIOS:
        if step not in paths:
            for P in paths.values():
                P.close()
            paths.clear()
            P = paths[step] = Path(rt, torch, N, SPL, NX, NY, [f * step for f in range(FRAMES)], SPP)
            last = P.frames[-1]
            fb, st = rt.alloc_fb(NX, NY), rt.alloc_rand_state(NX, NY)
            rt.render_init(NX, NY, st)
            rt.render(fb, NX, NY, 1024, last["W"], st, last["O"])
            torch.cuda.synchronize()
            ref = fb.cpu().numpy().reshape(-1, 3).astype(np.float64)
            sphere = last["hits"].cpu().numpy().view(rt.hit_record_dtype)["sphere"]
            lamb = (sphere >= 0) & (P.kind[np.clip(sphere, 0, None)] == rt.MAT_LAMBERTIAN)
        P = paths[step]
        p = rt.temporal_params(reuse_specular=spec)
        say()
        say("## %s" % label)
        say("%-34s %9s %9s %9s %9s %9s" % ("radius, min_count, gamma", "all", "lamb", "took", "neff", "neff<plain"))
        plain = None
        for r, mc, g in settings:
            h = P.history(rt, NX, NY, p, None if g == 0 else rt.temporal_rectify(radius=r, min_count=mc, gamma=g))
            torch.cuda.synchronize()
            hh = h.cpu().numpy()
            acc = np.sqrt(hh[:4 * n].reshape(n, 4)[:, :3].astype(np.float64))
            neff = hh[4 * n:]
            if plain is None:
                plain = neff.copy()
            ok = (neff > 0) & np.isfinite(ref).all(1) & np.isfinite(acc).all(1)
            e = lambda m: float(np.sqrt(np.mean((acc[m] - ref[m]) ** 2)))
            took = plain > SPP
            table[(label, (r, mc, g))] = e(ok)
            say("%-34s %9.5f %9.5f %8.1f%% %9.1f %8.1f%%" % ("unrectified" if g == 0 else "%d, %d, %g" % (r, mc, g), e(ok), e(ok & lamb), 100.0 * took.mean(),
                                                            float(neff[took].mean()), 100.0 * float((neff[took] < plain[took]).mean())))
        # the long history: max_history is the only brake of the unrectified call
        for name, rect in (("max_history 2^30, unrectified", None), ("max_history 2^30, defaults", rt.temporal_rectify())):
            hh = P.history(rt, NX, NY, rt.temporal_params(reuse_specular=spec, max_history=1 << 30), rect).cpu().numpy()
            acc = np.sqrt(hh[:4 * n].reshape(n, 4)[:, :3].astype(np.float64))
            ok = (hh[4 * n:] > 0) & np.isfinite(ref).all(1) & np.isfinite(acc).all(1)
            say("%-34s %9.5f %9.5f %9s %9.1f" % (name, e(ok), e(ok & lamb), "", float(hh[4 * n:][took].mean())))
    for P in paths.values():
        P.close()
    say()
    say("## moving scenes (tools/animate_study.py: %dx%d, %d frames of %d spp, static camera, +%g in x per frame), moving rule"
        % (animate_study.NX, animate_study.NY, animate_study.FRAMES, animate_study.SPP, animate_study.STEP))
    say("%-28s %9s %9s %12s %12s %10s %10s" % ("moved", "pixels on", "compared", "moving rule", "static rule", "neff mov.", "neff st."))
    for every in (1, 7):
        label = "moving: every small sphere" if every == 1 else "moving: every 7th small sphere"
        for key, val in animate_study.quality(rt, torch, say, every, settings).items():
            table[(label, key)] = val
    labels = []
    for (label, _) in table:
        if label not in labels:
            labels.append(label)
    say()
    say("## every non-empty pixel, RMSE by scenario (columns in the order below) and setting")
    for k, label in enumerate(labels):
        say("#   %d: %s" % (k, label))
    for key in settings:
        say("%-16s " % ("unrectified" if key[2] == 0 else "%d, %d, %g" % key) + " ".join("%9.5f" % table[(label, key)] for label in labels))
    say()
    say("## one setting for all: the worst loss against each scenario's own optimum on this grid (the unrectified call is a setting too)")
    own = {label: min(table[(label, key)] for key in settings) for label in labels}
    loss = {key: max(table[(label, key)] / own[label] - 1.0 for label in labels) for key in settings}
    for key in sorted(loss, key=loss.get):
        worst = max(labels, key=lambda label: table[(label, key)] / own[label])
        say("%-16s worst loss %5.1f %%  (%s)" % ("unrectified" if key[2] == 0 else "%d, %d, %g" % key, 100 * loss[key], worst))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


def rectify_kernels():
    """two frames STEP degrees apart, then rt_temporal_accumulate_moving (nothing moved: the yardstick) and
    rt_temporal_accumulate_rectified under the moving rule at radius 1 and 2, REPS + 1 times each in turn, on C3 and at 3840x2160"""
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    for n, spl, nx, ny in ((N, SPL, NX, NY), (100000, 320, 3840, 2160)):
        P = Path(rt, torch, n, spl, nx, ny, [0.0, STEP], 4)
        a, b = P.frames
        h0, h1 = rt.alloc_temporal_history(nx, ny), rt.alloc_temporal_history(nx, ny)
        p = rt.temporal_params()
        geom = b["W"].get_geometry()
        rt.temporal_accumulate(h0, None, a["hits"], None, None, a["state"], a["W"], nx, ny, p)
        torch.cuda.synchronize()
        for _ in range(REPS + 1):
            rt.temporal_accumulate_moving(h1, h0, b["hits"], a["hits"], a["cam"], geom, b["state"], b["W"], nx, ny, p)
            for radius in (1, 2):
                rt.temporal_accumulate_rectified(h1, h0, b["hits"], a["hits"], a["cam"], b["state"], b["W"], nx, ny, p, rt.temporal_rectify(radius=radius),
                                                 d_geom_prev=geom)
            torch.cuda.synchronize()
        print("%dx%d N=%d: %d x (moving, rectified r1, rectified r2)" % (nx, ny, n, REPS + 1), flush=True)
        P.close()


def rectify_kernel_report(d, path):
    """median times of the three kernels of a --rectify-kernels run; the first call of each on each frame size is the warm-up"""
    t = {"moving": [], "r1": [], "r2": []}
    for name, dur in read_trace(d):
        if "k_temporal_accumulate_rectified" in name:
            t["r2" if is_instance(name, "k_temporal_accumulate_rectified", True, 2) else "r1"].append(dur)
        elif "k_temporal_accumulate_moving" in name:
            t["moving"].append(dur)
    lines = ["", "## kernel times under rocprofv3 --kernel-trace --stats (tools/temporal_study.py --rectify-kernels), median of %d calls, us" % REPS,
             "# one run: the three kernels alternate; k_temporal_accumulate_moving is the yardstick (nothing moved, same inputs, same history)",
             "%-22s %30s %28s %8s %28s %8s" % ("frame", "k_temporal_accumulate_moving", "rectified<true, 1>", "ratio", "rectified<true, 2>", "ratio")]
    for k, frame in enumerate(("C3 1200x800", "C5 world 3840x2160")):
        med = {key: float(np.median(v[k * (REPS + 1) + 1:(k + 1) * (REPS + 1)])) for key, v in t.items()}
        lines.append("%-22s %30.1f %28.1f %8.2f %28.1f %8.2f" % (frame, med["moving"], med["r1"], med["r1"] / med["moving"], med["r2"], med["r2"] / med["moving"]))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(path, "a") as fo:
        fo.write(text)


def rectify_pmc_report(d, path):
    """per counter the mean over the timed dispatches (the first of each kernel on each frame size is the warm-up) of the three kernels"""
    acc = {}
    for f in sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)):
        seen = {}
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            if "k_temporal_accumulate_rectified" in name:
                key = "r2" if is_instance(name, "k_temporal_accumulate_rectified", True, 2) else "r1"
            elif "k_temporal_accumulate_moving" in name:
                key = "moving"
            else:
                continue
            ids = seen.setdefault((key, r["Counter_Name"]), [])
            if r["Dispatch_Id"] not in ids:
                ids.append(r["Dispatch_Id"])
            k = ids.index(r["Dispatch_Id"])
            if k % (REPS + 1) == 0:
                continue
            slot = acc.setdefault((r["Counter_Name"], k // (REPS + 1), key), [0.0, set()])
            slot[0] += float(r["Counter_Value"])
            slot[1].add(r["Dispatch_Id"])
    lines = ["", "## counters under rocprofv3 --pmc (runs of their own; tools/temporal_study.py --rectify-kernels), mean of %d dispatches" % REPS,
             "%-32s %-20s %16s %16s %8s %16s %8s" % ("counter", "frame", "moving", "rectified r1", "ratio", "rectified r2", "ratio")]
    for counter in sorted({k[0] for k in acc}):
        for size, frame in enumerate(("C3 1200x800", "C5 world 3840x2160")):
            v = {key: acc[(counter, size, key)][0] / max(1, len(acc[(counter, size, key)][1])) for key in ("moving", "r1", "r2") if (counter, size, key) in acc}
            if len(v) == 3:
                m = v["moving"] or float("nan")
                lines.append("%-32s %-20s %16.0f %16.0f %8.2f %16.0f %8.2f" % (counter, frame, v["moving"], v["r1"], v["r1"] / m, v["r2"], v["r2"] / m))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(path, "a") as fo:
        fo.write(text)


if __name__ == "__main__":
    if "--rectify-pmc-report" in sys.argv[1:]:
        i = sys.argv.index("--rectify-pmc-report")
        rectify_pmc_report(sys.argv[i + 1], sys.argv[i + 2])
    elif "--rectify" in sys.argv[1:]:
        rectify_main()
    elif "--rectify-kernels" in sys.argv[1:]:
        rectify_kernels()
    elif "--rectify-kernel-report" in sys.argv[1:]:
        i = sys.argv.index("--rectify-kernel-report")
        rectify_kernel_report(sys.argv[i + 1], sys.argv[i + 2])
    elif "--kernels" in sys.argv[1:]:
        kernels()
    elif "--kernel-report" in sys.argv[1:]:
        i = sys.argv.index("--kernel-report")
        kernel_report(sys.argv[i + 1], sys.argv[i + 2])
    else:
        main()
