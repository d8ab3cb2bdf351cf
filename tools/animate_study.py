"""One resident world over an animation (rt_world_set_geometry, rt_world_set_camera, rt_temporal_accumulate_moving) on one GPU.

  python tools/animate_study.py [OUT.txt]          both tables, written to OUT.txt

1. Quality: the scenario of tests/test_gpu_temporal_moving.py::test_moving_history_beats_the_static_rule at C3 size — 1200x800,
   N = 10 000, octree SPL 32, FRAMES frames of SPP samples a pixel under a static camera (rt_render_adaptive_begin with min_spp = max_spp,
   rel_error 0, RNG states carried on), the moved spheres +STEP in x per frame, library defaults.  RMSE of sqrt of the last history under
   the moving rule and under rt_temporal_accumulate's static rule against rt_render(REF_SPP) of the last frame's world, over the
   lambertian pixels on moved spheres whose last frame took history under the moving rule.  Two motions: every 7th small sphere, and
   every small sphere (the field as a whole: what the test uses at 203x77, where a sphere is two pixels wide).  Under each row the same
   pixels with rt_temporal_accumulate_rectified at its defaults (both rules), then the lambertian pixels on spheres that did NOT move
   (the lighting lag) and every non-empty pixel, unrectified and rectified.
2. Set-up time of one frame, both ways, at N = 10 000 (SPL 32) and N = 100 000 (SPL 320): this library's setters plus the device build
   (rt_world_get_geometry, rt_world_set_geometry, rt_world_set_camera, rt_build_octree_gpu, rt_free_octree of the old tree) against a
   world per frame (rt_world_create + rt_world_upload + rt_build_octree_gpu, and the two frees).  A host clock around work that ends in a
   device synchronise; REPS + 1 frames each way, alternating, the first is the warm-up; median and range.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))

NX, NY, N, SPL = 1200, 800, 10000, 32
FRAMES, SPP, STEP, REF_SPP = 4, 8, 0.5, 512
REPS = 9
SETUP = ((10000, 32), (100000, 320))


def small_spheres(spheres):
    return np.flatnonzero((spheres["material"] != -1) & (spheres["radius"] < 0.5) & (np.arange(len(spheres)) > 0))


def frames_of(rt, torch, every):
    """the scenario's frames on one resident world: per frame its state, guides, geometry and the geometry before the move"""
    W = rt.World(N, NX, NY)
    kind = W.spheres["material"].astype(np.int32)
    moved = small_spheres(W.spheres)[::every]
    d_moved = torch.from_numpy(moved).cuda()
    st = rt.alloc_rand_state(NX, NY)
    rt.render_init(NX, NY, st)
    frames, tree = [], None
    for f in range(FRAMES):
        d_geom_prev = W.get_geometry()
        if f:
            nxt = d_geom_prev.clone()
            nxt[d_moved, 0] += STEP
            W.set_geometry(nxt)
        if tree is not None:
            tree.close()
        tree = rt.Octree(W, SPL, gpu=True)
        fb, state, hits = rt.alloc_fb(NX, NY), rt.alloc_adaptive_state(NX, NY), rt.alloc_guides(NX, NY)
        rt.render_adaptive_begin(fb, NX, NY, rt.Adaptive(SPP, SPP, 4, 0.0, 0.0), W, st, state, tree)
        rt.render_guides(W, tree, NX, NY, hits)
        frames.append(dict(state=state, hits=hits, d_geom_prev=d_geom_prev, d_geom=W.get_geometry()))
    return W, tree, kind, moved, frames


def chain(rt, torch, W, frames, p, moving, rectify=None):
    """the last frame's history (host) under the static or the moving rule; rectify: a TemporalRectify, or None for the plain calls"""
    h = [rt.alloc_temporal_history(NX, NY), rt.alloc_temporal_history(NX, NY)]
    cam = W.get_camera()
    for f, fr in enumerate(frames):
        W.set_geometry(fr["d_geom"])                     # the moving rule reads this frame's geometry from the world
        out, last, prev = h[f & 1], h[(f + 1) & 1] if f else None, frames[f - 1]["hits"] if f else None
        if rectify is not None:
            rt.temporal_accumulate_rectified(out, last, fr["hits"], prev, cam, fr["state"], W, NX, NY, p, rectify,
                                             d_geom_prev=fr["d_geom_prev"] if moving and f else None)
        elif moving:
            rt.temporal_accumulate_moving(out, last, fr["hits"], prev, cam, fr["d_geom_prev"], fr["state"], W, NX, NY, p)
        else:
            rt.temporal_accumulate(out, last, fr["hits"], prev, cam, fr["state"], W, NX, NY, p)
    torch.cuda.synchronize()
    return h[(len(frames) - 1) & 1].cpu().numpy()


def quality(rt, torch, say, every, settings=()):
    """the table row of one motion, the same pixels under the rectified calls at the library's defaults, and the lighting lag: the
    lambertian pixels on spheres that did NOT move.  Returns {setting: RMSE over every non-empty pixel} of the moving rule for the
    (radius, min_count, gamma) settings asked for; gamma 0 is the unrectified call"""
    W, tree, kind, moved, frames = frames_of(rt, torch, every)
    p = rt.temporal_params()
    ref, rs = rt.alloc_fb(NX, NY), rt.alloc_rand_state(NX, NY)
    rt.render_init(NX, NY, rs)
    rt.render(ref, NX, NY, REF_SPP, W, rs, tree)
    torch.cuda.synchronize()
    n = NX * NY
    ref = ref.cpu().numpy().reshape(-1, 3).astype(np.float64)
    m, s = chain(rt, torch, W, frames, p, True), chain(rt, torch, W, frames, p, False)
    mr, sr = chain(rt, torch, W, frames, p, True, rt.temporal_rectify()), chain(rt, torch, W, frames, p, False, rt.temporal_rectify())
    sphere = frames[-1]["hits"].cpu().numpy().view(rt.hit_record_dtype)["sphere"]
    lamb = (sphere >= 0) & (kind[np.clip(sphere, 0, None)] == rt.MAT_LAMBERTIAN)
    on_moved = np.isin(sphere, moved) & lamb
    img = lambda h: np.sqrt(h[:4 * n].reshape(n, 4)[:, :3].astype(np.float64))
    am, as_ = img(m), img(s)
    fin = np.isfinite(ref).all(1) & np.isfinite(am).all(1) & np.isfinite(as_).all(1)
    sel = on_moved & (m[4 * n:] > SPP) & fin

    def e(a, mask):
        return float(np.sqrt(np.mean((a[mask] - ref[mask]) ** 2)))
    name = "every 7th small sphere" if every == 7 else "every small sphere"
    say("%-28s %9d %9d %12.5f %12.5f %10.1f %10.1f" % (name, int(on_moved.sum()), int(sel.sum()), e(am, sel), e(as_, sel), float(m[4 * n:][sel].mean()),
                                                      float(s[4 * n:][sel].mean())))
    say("%-28s %9s %9s %12.5f %12.5f %10.1f %10.1f" % ("  rectified, defaults", "", "", e(img(mr), sel), e(img(sr), sel), float(mr[4 * n:][sel].mean()),
                                                      float(sr[4 * n:][sel].mean())))
    still = lamb & ~on_moved & (s[4 * n:] > SPP) & (m[4 * n:] > SPP) & fin
    whole = (m[4 * n:] > 0) & fin
    for label, mask in (("  lambertian, NOT moved", still), ("  every non-empty pixel", whole)):
        say("%-28s %9s %9d %12.5f %12.5f %10.1f %10.1f   rectified %9.5f %9.5f  neff %5.1f %5.1f"
            % (label, "", int(mask.sum()), e(am, mask), e(as_, mask), float(m[4 * n:][mask].mean()), float(s[4 * n:][mask].mean()), e(img(mr), mask),
               e(img(sr), mask), float(mr[4 * n:][mask].mean()), float(sr[4 * n:][mask].mean())))
    swept = {}
    for radius, min_count, gamma in settings:
        h = m if gamma == 0 else chain(rt, torch, W, frames, p, True, rt.temporal_rectify(radius=radius, min_count=min_count, gamma=gamma))
        swept[(radius, min_count, gamma)] = e(img(h), whole)
    tree.close()
    W.close()
    return swept


def setup_times(rt, torch, say, n, spl):
    base = rt.World(n, NX, NY)
    spheres, cam = base.spheres.copy(), base.camera.copy()
    moved = torch.from_numpy(small_spheres(spheres)[::7]).cuda()
    keep = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    one, tree, fresh = base.upload(), None, []
    torch.cuda.synchronize()
    t_one, t_fresh = [], []
    for _ in range(REPS + 1):
        # one resident world: keep last frame's geometry, move, set the camera, build the tree on the device
        nxt = one.get_geometry().clone()
        nxt[moved, 0] += STEP                                        # the caller's own animation kernel: outside the timed window
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one.get_geometry(keep)
        one.set_geometry(nxt)
        one.set_camera(cam)
        if tree is not None:
            tree.close()
        tree = rt.Octree(one, spl, gpu=True)
        torch.cuda.synchronize()
        t_one.append((time.perf_counter() - t0) * 1e3)
        # a world per frame, as before: create, upload, build, and free last frame's
        spheres["center"][:, 0] += np.where(np.isin(np.arange(n), moved.cpu().numpy()), np.float32(STEP), np.float32(0))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for h in fresh:
            h.close()
        w = rt.World(n, NX, NY, spheres=spheres, camera=cam).upload()
        fresh = [rt.Octree(w, spl, gpu=True), w]
        torch.cuda.synchronize()
        t_fresh.append((time.perf_counter() - t0) * 1e3)
    for h in fresh + [tree, one]:
        h.close()
    for name, t in (("setters + rt_build_octree_gpu", t_one[1:]), ("world per frame", t_fresh[1:])):
        say("N = %-7d SPL %-4d %-32s median %8.3f ms   min %8.3f   max %8.3f   (%d frames)" % (n, spl, name, float(np.median(t)), min(t), max(t), len(t)))


def main():
    import torch
    import rt_amd as rt
    torch.cuda.set_device(0)
    path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    out = []

    def say(line=""):
        print(line, flush=True)
        out.append(line)

    say("# tools/animate_study.py on %s" % torch.cuda.get_device_name(0))
    say("## quality: %dx%d, N = %d, SPL %d, %d frames of %d spp, static camera, +%g in x per frame, library defaults; RMSE against rt_render(%d)"
        % (NX, NY, N, SPL, FRAMES, SPP, STEP, REF_SPP))
    say("%-28s %9s %9s %12s %12s %10s %10s" % ("moved", "pixels on", "compared", "moving rule", "static rule", "neff mov.", "neff st."))
    for every in (7, 1):
        quality(rt, torch, say, every)
    say()
    say("## set-up of one frame (host clock around a device synchronise): nothing is rendered")
    for n, spl in SETUP:
        setup_times(rt, torch, say, n, spl)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
