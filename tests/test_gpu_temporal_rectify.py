"""GPU tests of rt_temporal_accumulate_rectified (-m gpu).  Every comparison is bit equality through same_any_nan() of
tests/test_gpu_denoise_var.py, except the quality check: the kernel against the numpy model of tests/temporal_rectify_model.py over
chains of three frames of ONE world whose spheres move and whose camera stands or orbits — under the static rule (d_geom_prev NULL) and
under the moving rule (given), at radius 1 and 2, at a biting gamma and at the default —, frames smaller than the window's apron, both
gamma = 0 identities against the two existing entry points, the model's hand-worked 4x4 cases, a captured graph and the refusals.

The scene is create_world at N = 500 (203x77, SPL 30, the adaptive parameters of tests/test_gpu_temporal.py) animated by the Animation of
tests/test_gpu_temporal_moving.py: every 7th small sphere moves, a second set changes radius.  Chains run at position_tolerance 1, for
the reason the docstring of tests/test_gpu_temporal.py gives."""
import numpy as np
import pytest

import temporal_model as tm
import temporal_rectify_model as trm
from bitcmp import same_any_nan
from temporal_paths import Animation

pytestmark = pytest.mark.gpu
NX, NY = 203, 77
N, SPL = 500, 30
ADAPT = (4, 64, 4, 0.1, 0.02)
PATHS = dict(static=0.0, orbit=1.0)            # degrees per frame
F = np.float32


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def gpu_chain(rt, torch, A, p, r, moving, upto=None):
    out = []
    for f in range(len(A.frames[:upto])):
        fr = A.at(f)
        h = rt.alloc_temporal_history(A.nx, A.ny)
        h.fill_(7.0)                                                             # every pixel must be written
        pv = A.frames[f - 1] if f else None
        rt.temporal_accumulate_rectified(h, out[-1] if f else None, fr["d_hits"], pv["d_hits"] if f else None, pv["cam"] if f else None,
                                         fr["state"], A.W, A.nx, A.ny, p, r, d_geom_prev=pv["d_geom"] if f and moving else None)
        out.append(h)
    torch.cuda.synchronize()
    return out


def model_chain(A, p, r, moving, upto=None):
    out, counts = [], []
    for f, fr in enumerate(A.frames[:upto]):
        pv = A.frames[f - 1] if f else None
        c = {}
        out.append(trm.accumulate_rectified(out[-1] if f else None, fr["hits"], pv["hits"] if f else None, pv["cam"] if f else None, fr["h_state"],
                                            A.kind, A.nx, A.ny, p.max_history, p.reuse_specular, p.position_tolerance, p.normal_min_dot,
                                            r.radius, r.min_count, r.gamma, geom=fr["geom"], geom_prev=pv["geom"] if f and moving else None,
                                            counts=c))
        counts.append(c)
    return out, counts


@pytest.fixture(scope="module")
def anims(rt, cuda):
    """three frames at 203x77 on each camera path"""
    trm.self_check()                               # the model follows the rule before the kernel is held to the model
    made = {name: Animation(rt, cuda, N, SPL, NX, NY, [0.0, step, 2 * step], ADAPT) for name, step in PATHS.items()}
    yield made
    for A in made.values():
        A.close()


# ---- 1. kernel == model over the chains ----------------------------------------------------------------------------------------------
CASES = [(path, radius, gamma, moving) for path in PATHS for radius in (1, 2) for gamma in (0.5, None) for moving in (False, True)]
CAUSES = ("rectified", "kept_min_count", "kept_within", "taps_outside", "taps_empty", "taps_sphere")


def rectify_of(rt, radius, gamma):
    """gamma None: the library's default gamma and min_count; the biting gamma tests every window of two pixels or more"""
    return rt.temporal_rectify(radius=radius) if gamma is None else rt.temporal_rectify(radius=radius, gamma=gamma, min_count=2)


@pytest.mark.parametrize("path,radius,gamma,moving", CASES,
                         ids=["%s-r%d-%s-%s" % (c[0], c[1], "default" if c[2] is None else "g%s" % c[2], "moving" if c[3] else "static") for c in CASES])
def test_matches_the_model_over_a_chain(rt, cuda, anims, path, radius, gamma, moving):
    A = anims[path]
    p, r = rt.temporal_params(position_tolerance=1.0), rectify_of(rt, radius, gamma)
    got = gpu_chain(rt, cuda, A, p, r, moving)
    ref, counts = model_chain(A, p, r, moving)
    for f in range(3):
        assert same_any_nan(got[f].cpu().numpy(), ref[f]), (path, radius, gamma, moving, f)
    assert counts[0]["nonempty"] > NX * NY // 2 and counts[0]["took"] == 0 and counts[2]["took"] > 1000
    if gamma is not None:
        assert counts[2]["rectified"] > 100


def test_every_cause_occurs_in_the_chains(rt, cuda, anims):
    """from the model's counts over ALL the chains of the test above: pixels were rectified, kept for a window below min_count, kept
    inside the limit, and window taps were skipped as outside the frame, as EMPTY and as another sphere; the moving rule met pixels on
    translated spheres that took history"""
    p = rt.temporal_params(position_tolerance=1.0)
    seen = dict.fromkeys(CAUSES, 0)
    moved_took = 0
    for path, radius, gamma, moving in CASES:
        _, counts = model_chain(anims[path], p, rectify_of(rt, radius, gamma), moving)
        for c in counts[1:]:
            for key in CAUSES:
                seen[key] += c[key]
            moved_took += c.get("moved_took", 0)
    print(seen, moved_took)
    assert all(v > 0 for v in seen.values()), seen
    assert moved_took > 0


# ---- 2. frames smaller than the apron, and a last tile column of one pixel -------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(1, 1), (3, 2), (16, 17), (33, 17)])
def test_tiny_and_edge_frames_at_radius_2(rt, cuda, nx, ny):
    """(33, 17): the last tile column is one pixel wide and its apron reaches two tiles back; (16, 17) the same for the rows"""
    A = Animation(rt, cuda, 500, 30, nx, ny, [0.0, 0.0, 2.0], (4, 32, 4, 0.1, 0.02))
    p = rt.temporal_params(position_tolerance=1.0, reuse_specular=1)
    for r in (rt.temporal_rectify(radius=2, gamma=0.5, min_count=2), rt.temporal_rectify(radius=2)):
        for moving in (False, True):
            got = gpu_chain(rt, cuda, A, p, r, moving)
            ref, _ = model_chain(A, p, r, moving)
            for f in range(3):
                assert same_any_nan(got[f].cpu().numpy(), ref[f]), (nx, ny, r.gamma, moving, f)
    A.close()


# ---- 3. gamma = 0 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2])
def test_gamma_zero_is_the_two_existing_calls(rt, cuda, anims, radius):
    torch = cuda
    p, off = rt.temporal_params(position_tolerance=1.0), rt.temporal_rectify(radius=radius, gamma=0.0)
    for name, A in anims.items():
        first = gpu_chain(rt, torch, A, p, off, False, upto=1)[0]
        fr, pv = A.at(1), A.frames[0]
        a, b = rt.alloc_temporal_history(NX, NY), rt.alloc_temporal_history(NX, NY)
        a.fill_(5.0)
        rt.temporal_accumulate_rectified(a, first, fr["d_hits"], pv["d_hits"], pv["cam"], fr["state"], A.W, NX, NY, p, off)
        rt.temporal_accumulate(b, first, fr["d_hits"], pv["d_hits"], pv["cam"], fr["state"], A.W, NX, NY, p)
        torch.cuda.synchronize()
        assert same_any_nan(a.cpu().numpy(), b.cpu().numpy()), name
        ref = b.cpu().numpy()
        a.fill_(5.0)
        rt.temporal_accumulate_rectified(a, first, fr["d_hits"], pv["d_hits"], pv["cam"], fr["state"], A.W, NX, NY, p, off, d_geom_prev=pv["d_geom"])
        rt.temporal_accumulate_moving(b, first, fr["d_hits"], pv["d_hits"], pv["cam"], pv["d_geom"], fr["state"], A.W, NX, NY, p)
        torch.cuda.synchronize()
        assert same_any_nan(a.cpu().numpy(), b.cpu().numpy()), name
        assert not same_any_nan(ref, b.cpu().numpy())                                        # the two rules differ on these frames
        b.fill_(9.0)
        rt.temporal_accumulate(b, None, fr["d_hits"], None, None, fr["state"], A.W, NX, NY, p)
        rt.temporal_accumulate_rectified(a, None, fr["d_hits"], None, None, fr["state"], A.W, NX, NY, p, rt.temporal_rectify(radius=radius))
        torch.cuda.synchronize()
        assert same_any_nan(a.cpu().numpy(), b.cpu().numpy()), name                          # a first frame takes no history: nothing to rectify


# ---- 4. the hand-worked cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", trm.hand_cases(), ids=lambda c: c["name"])
def test_hand_worked_cases_on_the_gpu(rt, cuda, case):
    """state, guides and history are built by the model's hand_cases(); nothing is rendered.  The world only supplies its size."""
    torch = cuda
    a = case["args"]
    nx, ny = a["nx"], a["ny"]
    W = rt.World(500, nx, ny)
    kind = W.spheres["material"].astype(np.int32)
    p = rt.temporal_params(max_history=a["max_history"], reuse_specular=a["reuse_specular"], position_tolerance=a["position_tolerance"],
                           normal_min_dot=a["normal_min_dot"])
    r = rt.temporal_rectify(radius=a["radius"], min_count=a["min_count"], gamma=a["gamma"])
    ref = trm.accumulate_rectified(kind=kind, **a)
    trm.check_case(case, ref)
    d = {name: dev(torch, a[name]) for name in ("hist_in", "hits", "hits_prev", "state")}
    geom = W.get_geometry()
    for d_geom_prev in (None, geom):
        out = rt.alloc_temporal_history(nx, ny)
        out.fill_(7.0)
        rt.temporal_accumulate_rectified(out, d["hist_in"], d["hits"], d["hits_prev"], a["cam_prev"], d["state"], W, nx, ny, p, r, d_geom_prev=d_geom_prev)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        trm.check_case(case, got)
        assert same_any_nan(got, ref), case["name"]
    W.close()


# ---- 5. capture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moving", [False, True])
def test_captured_in_a_graph(rt, cuda, anims, moving):
    torch = cuda
    A = anims["orbit"]
    p, r = rt.temporal_params(position_tolerance=1.0), rt.temporal_rectify(radius=2, gamma=0.5)
    h = gpu_chain(rt, torch, A, p, r, moving)
    fr, pv = A.at(2), A.frames[1]
    hist = rt.alloc_temporal_history(NX, NY)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rt.temporal_accumulate_rectified(hist, h[1], fr["d_hits"], pv["d_hits"], pv["cam"], fr["state"], A.W, NX, NY, p, r,
                                         d_geom_prev=pv["d_geom"] if moving else None)
    hist.fill_(3.0)
    g.replay()
    torch.cuda.synchronize()
    assert same_any_nan(hist.cpu().numpy(), h[2].cpu().numpy())


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(rt, cuda, anims):
    torch = cuda
    A = anims["static"]
    a, b = A.frames[0], A.at(1)
    p, r = rt.temporal_params(), rt.temporal_rectify()
    n = NX * NY
    m = (5 * n + 3) // 4 * 4                                                     # floats to the next 16-byte boundary behind one history
    big = torch.zeros(2 * m + 16, dtype=torch.float32, device="cuda")
    first, second = big[:5 * n], big[m:m + 5 * n]                                # both 16-byte aligned, no overlap
    rt.temporal_accumulate_rectified(first, None, a["d_hits"], None, None, a["state"], A.W, NX, NY, p, r)
    rt.temporal_accumulate_rectified(second, first, b["d_hits"], a["d_hits"], a["cam"], b["state"], A.W, NX, NY, p, r, d_geom_prev=a["d_geom"])
    torch.cuda.synchronize()

    def refused(*args, **kw):
        with pytest.raises(rt.RtError) as e:
            rt.temporal_accumulate_rectified(*args, **kw)
        return str(e.value)

    ok = (b["d_hits"], a["d_hits"], a["cam"], b["state"], A.W, NX, NY, p, r)
    for out in (second, big[m + 4:m + 4 + 5 * n], big[m - 4:m - 4 + 5 * n]):       # in place, and aligned overlaps from either side
        assert "failed: -1 " in refused(out, second, *ok)
    assert "failed: -1 " in refused(big[1:5 * n + 1], second, *ok)                 # misaligned histories and guides
    assert "failed: -1 " in refused(second, big[1:5 * n + 1], *ok)
    assert "failed: -1 " in refused(second, first, b["d_hits"][4:], *ok[1:])
    assert "failed: -1 " in refused(second, first, b["d_hits"], a["d_hits"][8:], *ok[2:])
    assert "failed: -1 " in refused(second, first, *ok, d_geom_prev=a["d_geom"].reshape(-1)[1:])                  # misaligned geometry
    assert "failed: -1 " in refused(second, first, *ok[:7], rt.temporal_params(position_tolerance=0.0), r)
    assert "failed: -1 " in refused(second, first, *ok[:8], None)                                                 # no rectify
    for kw in (dict(radius=0), dict(radius=3), dict(min_count=1), dict(min_count=10), dict(gamma=-1.0), dict(gamma=float("nan")), dict(gamma=1e20)):
        assert "failed: -1 " in refused(second, first, *ok[:8], rt.temporal_rectify(**kw)), kw
    half = rt.World(500, NX, NY, precision=rt.FP16)
    assert "failed: -1 " in refused(second, first, *ok[:4], half, NX, NY, p, None)                                # RT_EINVAL first ...
    assert "failed: -4 " in refused(second, first, *ok[:4], half, NX, NY, p, r)                                   # ... then RT_ENOTSUP
    half.close()
    torch.cuda.synchronize()


# ---- 7. quality ------------------------------------------------------------------------------------------------------------------------
FRACTION = 0.2          # two reference luminances differ "by more than a stated fraction": |l_last - l_first| > FRACTION * max(l_first, l_last)
CPU_LOSS_ON_U = 0.0077  # what the CPU run showed on set U (below)


def test_rectified_history_follows_the_light(rt, cuda):
    """203x77, N = 10 000, SPL 32, four frames of 8 spp each (rel_error 0, min_spp = max_spp) of one world under a static camera, RNG
    states carried on, library defaults for the temporal parameters and for the rectification, the moving rule (d_geom_prev given) with
    and without rectification; gamma frames (sqrt of the history) against rt_render(512).  EVERY 7TH small sphere moves +0.5 in x per
    frame: the spheres between them, and the ground, stay where they are while the shadows and reflections on them change.

    Two references: rt_render(512) of the first world and of the last one; l = the sum over the channels of the squared gamma value.
    Set C: lambertian pixels on spheres that did not move, that took history in the last frame under the static and under the moving
    rule, and whose reference luminances differ by more than FRACTION = 0.2 of the larger one.  Set U: the same with luminances that
    agree within that fraction.  Claims: on C the rectified RMSE (against the LAST world's reference) is below the unrectified one; on
    U it is at most the unrectified one times (1 + the loss the CPU showed) x 1.02; the mean neff on C is below the mean neff on U.

    The motion and the fraction were chosen on the CPU before any GPU run, with the oracle's renders (1-spp gamma frames, squared, as
    the per-sample colours; RNG states carried on) and tests/temporal_rectify_model.py: every 7th small sphere, FRACTION 0.2:
    |C| = 904, rectified 0.06315 against 0.06588 (mean neff 25.4 against 26.7); |U| = 5 433, rectified 0.03478 against 0.03451, a loss
    of 0.77 % (mean neff 29.2 against 30.5).  At FRACTION 0.05 / 0.1 / 0.3: |C| 2 253 / 1 557 / 587, 0.05289 / 0.05684 / 0.06770
    against 0.05428 / 0.05874 / 0.07113, the loss on U 1.55 / 1.22 / 0.41 %.  With EVERY small sphere moving only the ground and the
    three large spheres stay: |C| = 68 at 0.2 (157 at 0.05: 0.04706 against 0.05385) — too few to rest on.  A sharper setting repairs
    more and costs more: radius 1, min_count 2, gamma 1 gives 0.05863 on C and a loss of 8.3 % on U.  So rectification at its defaults
    shortens the lighting lag on this scene by 4 %; it does not remove it: the history on C is still twice as far from the reference as on U.

    Measured on one MI355X: C 904 pixels, rectified 0.06315 against 0.06588 (mean neff 25.4 against 26.7); U 5 433 pixels, 0.03478
    against 0.03451 (+0.77 %) — the CPU's figures, as the frames are the oracle's bit for bit (profiles/r19/rectify.txt)."""
    torch = cuda
    A = Animation(rt, torch, 10000, 32, NX, NY, [0.0] * 4, (8, 8, 4, 0.0, 0.0), resize=False, every=7)
    p, r = rt.temporal_params(), rt.temporal_rectify()
    n = NX * NY
    rect = gpu_chain(rt, torch, A, p, r, True)[3].cpu().numpy()
    hm, hs = [], []
    for f in range(4):
        fr, pv = A.at(f), A.frames[f - 1] if f else None
        a, b = rt.alloc_temporal_history(NX, NY), rt.alloc_temporal_history(NX, NY)
        rt.temporal_accumulate_moving(a, hm[-1] if f else None, fr["d_hits"], pv["d_hits"] if f else None, pv["cam"] if f else None,
                                      pv["d_geom"] if f else None, fr["state"], A.W, NX, NY, p)
        rt.temporal_accumulate(b, hs[-1] if f else None, fr["d_hits"], pv["d_hits"] if f else None, pv["cam"] if f else None, fr["state"], A.W, NX, NY, p)
        hm.append(a)
        hs.append(b)
    torch.cuda.synchronize()
    plain, static = hm[3].cpu().numpy(), hs[3].cpu().numpy()
    refs = []
    for f in (0, 3):
        A.at(f)
        A.rebuild()
        fb, st = rt.alloc_fb(NX, NY), rt.alloc_rand_state(NX, NY)
        rt.render_init(NX, NY, st)
        rt.render(fb, NX, NY, 512, A.W, st, A.tree)
        torch.cuda.synchronize()
        refs.append(fb.cpu().numpy().reshape(-1, 3).astype(np.float64))
    first, last = refs
    l0, l3 = (first ** 2).sum(1), (last ** 2).sum(1)
    with np.errstate(all="ignore"):
        differ = np.abs(l3 - l0) > FRACTION * np.maximum(l0, l3)
    xr, nr = tm.history_parts(rect, n)
    xp, npl = tm.history_parts(plain, n)
    _, nst = tm.history_parts(static, n)
    sphere = A.frames[3]["hits"]["sphere"]
    unmoved = (sphere >= 0) & (A.kind[np.clip(sphere, 0, None)] == rt.MAT_LAMBERTIAN) & ~np.isin(sphere, A.moved)
    ar, ap = np.sqrt(xr[:, :3].astype(np.float64)), np.sqrt(xp[:, :3].astype(np.float64))
    ok = unmoved & (npl > 8) & (nst > 8) & np.isfinite(first).all(1) & np.isfinite(last).all(1) & np.isfinite(ar).all(1) & np.isfinite(ap).all(1)
    C, U = ok & differ, ok & ~differ

    def rmse(img, sel):
        return float(np.sqrt(((img[sel] - last[sel]) ** 2).mean()))

    print("C: %d pixels, rectified %.5f unrectified %.5f, mean neff %.1f against %.1f" % (C.sum(), rmse(ar, C), rmse(ap, C), nr[C].mean(), npl[C].mean()))
    print("U: %d pixels, rectified %.5f unrectified %.5f (%+.2f %%), mean neff %.1f against %.1f"
          % (U.sum(), rmse(ar, U), rmse(ap, U), 100 * (rmse(ar, U) / rmse(ap, U) - 1), nr[U].mean(), npl[U].mean()))
    A.close()
    assert (nr <= npl).all()
    assert C.sum() > 100 and U.sum() > 100
    assert rmse(ar, C) < rmse(ap, C)
    assert rmse(ar, U) <= rmse(ap, U) * (1 + CPU_LOSS_ON_U) * 1.02
    assert nr[C].mean() < nr[U].mean()
