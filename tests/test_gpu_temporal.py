"""GPU tests of temporal accumulation (-m gpu): rt_temporal_accumulate and rt_denoise_history.  Every comparison is bit equality through
same_any_nan() of tests/test_gpu_denoise_var.py, except the quality check: the kernel against the numpy float32 model of
tests/temporal_model.py over chains of three frames on camera paths and on fabricated guides and histories; the new prepare against
rt_denoise_adaptive on a first frame; tiny frames; a captured graph, in place, the refusals; and the RMSE against 512 spp.

The camera paths orbit create_world's camera about the y axis.  Their steps were chosen with the oracle's tracer and the model alone on
the CPU: at 203x77 a step of 1 degree moves the image by a median of 1.7 pixels and a step of 60 degrees by 66.  The counts a test
asserts are taken at position_tolerance 1: at this resolution one pixel spans 0.39 degrees, on the ground (seen from a height of 2 at a
distance of 13) more than 0.04 t from its neighbour, so the library's default tolerance of 0.03 t, chosen at 1200x800, accepts too few
taps of a MOVED frame here (the model alone: 33 % of the lambertian pixels take history at 1 degree, against 81 % at tolerance 1, where
14 % take it at 60 degrees)."""
import numpy as np
import pytest

import temporal_model as tm
from bitcmp import same_any_nan
from temporal_paths import gpu_chain, model_chain, Path, PATHS
from world_cases import orbit_camera

pytestmark = pytest.mark.gpu
NX, NY = 203, 77                   # ragged: neither a multiple of the 16x16 tile nor of the 8x8 render tile
N, SPL = 10000, 32
ADAPT = (4, 64, 4, 0.1, 0.02)      # (min_spp, max_spp, batch, rel_error, floor): pixels stop at many different counts


@pytest.fixture(scope="module")
def paths(rt, cuda):
    """three frames at 203x77 on each camera path, at adaptive parameters 4 / 64 / 4"""
    tm.self_check()                                # the model follows the rule before the kernel is held to the model
    made = {name: Path(rt, cuda, N, SPL, NX, NY, [0.0, step, 2 * step], [ADAPT]) for name, step in PATHS.items()}
    yield made
    for P in made.values():
        P.close()


# ---- 1. kernel == model over a chain of three frames -----------------------------------------------------------------------------
PARAMS = [dict(), dict(position_tolerance=1.0), dict(position_tolerance=1e-4), dict(max_history=0), dict(max_history=8, position_tolerance=1.0),
          dict(max_history=1 << 30, position_tolerance=1.0), dict(reuse_specular=1, position_tolerance=1.0), dict(reuse_specular=1),
          dict(normal_min_dot=-1.0, position_tolerance=1.0), dict(normal_min_dot=0.99, position_tolerance=1.0),
          dict(max_history=8, reuse_specular=1, position_tolerance=1e-4, normal_min_dot=-1.0)]


@pytest.mark.parametrize("kw", PARAMS, ids=[",".join("%s=%s" % kv for kv in c.items()) or "defaults" for c in PARAMS])
@pytest.mark.parametrize("path", list(PATHS))
def test_matches_the_model_over_a_chain(rt, cuda, paths, path, kw):
    torch = cuda
    P = paths[path]
    p = rt.temporal_params(**kw)
    k = tm.state_parts(P.frames[0]["h_state"], NX * NY)[3]
    assert len(np.unique(k)) >= 3, np.unique(k)                                  # the frames are not uniform
    got = gpu_chain(rt, torch, P, p)
    ref, counts = model_chain(P, p)
    for f in range(3):
        assert same_any_nan(got[f].cpu().numpy(), ref[f]), (path, kw, f)
    assert counts[0]["nonempty"] > NX * NY // 2 and counts[0]["took"] == 0
    if p.max_history == 0:
        assert same_any_nan(ref[2], tm.accumulate(None, P.frames[2]["hits"], None, None, P.frames[2]["h_state"], P.kind, NX, NY, 0, 0, 1.0, 0.0))
    elif path == "static":
        assert counts[2]["took_lambertian"] >= 0.99 * counts[2]["lambertian"] > 0    # a landing point is its own pixel centre
    if not p.reuse_specular:
        assert all(c["took"] == c["took_lambertian"] for c in counts)
    elif path == "static":
        assert counts[2]["took"] > counts[2]["took_lambertian"]


def test_the_paths_reproject_and_reject(rt, cuda, paths):
    """the model's own counts at position_tolerance 1 (the module's docstring says why): on the small orbit at least half of the non-empty
    lambertian pixels take history and at least one is refused; on the jump fewer take it, and most landing points leave the frame or
    find nothing"""
    p = rt.temporal_params(position_tolerance=1.0)
    took = {}
    for name in ("orbit", "jump"):
        _, counts = model_chain(paths[name], p)
        for c in counts[1:]:
            print(name, {k: v for k, v in c.items() if k != "took_mask"})
        took[name] = [c["took_lambertian"] / c["lambertian"] for c in counts[1:]]
        assert all(c["all_refused"] + c["off_frame"] >= 1 for c in counts[1:])
        assert all(c["sphere"] >= 1 and c["normal"] >= 1 and c["position"] >= 1 for c in counts[1:])
    assert min(took["orbit"]) >= 0.5, took
    assert max(took["jump"]) < min(took["orbit"]) and max(took["jump"]) < 0.5, took
    _, counts = model_chain(paths["jump"], p)
    assert all(c["off_frame"] > 1000 for c in counts[1:])


# ---- 2. fabricated guides and histories on 17x16 ------------------------------------------------------------------------------------
def fabricated(rt, kind, seed=11):
    """guides, previous guides, a history and a state on 17x16 in which every skip cause occurs: landing points spread past all four
    borders, points behind the previous camera, NaN points, history taps with neff = 0 (and a NaN neff), other spheres, turned normals,
    distant points, and pixels all of whose taps are refused.  kind: the world's material tags."""
    nx, ny = 17, 16
    n = nx * ny
    rng = np.random.default_rng(seed)
    cam = orbit_camera(rt, 0.0, nx, ny)
    O, LL = cam[0]["origin"].astype(np.float64), cam[0]["lower_left_corner"].astype(np.float64)
    H, V = cam[0]["horizontal"].astype(np.float64), cam[0]["vertical"].astype(np.float64)
    lamb = np.flatnonzero(kind == rt.MAT_LAMBERTIAN)[:3]
    metal = np.flatnonzero(kind == rt.MAT_METAL)[:1]
    glass = np.flatnonzero(kind == rt.MAT_DIELECTRIC)[:1]
    ids = np.concatenate([lamb, metal, glass]).astype(np.int32)
    assert len(ids) == 5
    normals = np.array([[0, 1, 0], [0, 0.995, 0.0998749], [0.6, 0.8, 0], [0, -1, 0]], np.float32)

    def pick_sphere(size):
        return np.where(rng.random(size) < 0.7, ids[0], rng.choice(ids, size)).astype(np.int32)

    def pick_normal(size):
        return normals[np.where(rng.random(size) < 0.7, 0, rng.integers(0, 4, size))]

    # the previous frame: the centre rays at depth 1, a few much further
    j, i = np.divmod(np.arange(n), nx)
    tau_q = np.where(rng.random(n) < 0.1, 40.0, 1.0)
    prev = np.zeros(n, rt.hit_record_dtype)
    prev["p"] = (O + tau_q[:, None] * ((LL - O) + ((i + 0.5) / nx)[:, None] * H + ((j + 0.5) / ny)[:, None] * V)).astype(np.float32)
    prev["t"] = (tau_q * 10).astype(np.float32)
    prev["sphere"], prev["normal"] = pick_sphere(n), pick_normal(n)
    neff_in = rng.choice(np.array([0, 0.5, 4, 8, 100, 3e9], np.float32), n)
    neff_in[rng.choice(n, 4, replace=False)] = np.float32("nan")
    xv = rng.uniform(0.0, 2.0, (n, 4)).astype(np.float32)
    xv[neff_in == 0] = 0
    # this frame: points on the previous camera's rays through (s, t) spread past all four borders, at depth 1
    s, t = rng.uniform(-0.08, 1.08, n), rng.uniform(-0.08, 1.08, n)
    tau = np.where(rng.random(n) < 0.08, -1.0, 1.0)                                # behind the previous camera
    hits = np.zeros(n, rt.hit_record_dtype)
    hits["p"] = (O + tau[:, None] * ((LL - O) + s[:, None] * H + t[:, None] * V)).astype(np.float32)
    hits["p"][rng.choice(n, 6, replace=False), rng.integers(0, 3, 6)] = np.float32("nan")
    hits["t"] = 10.0
    hits["sphere"], hits["normal"] = pick_sphere(n), pick_normal(n)
    hits["sphere"][rng.choice(n, 5, replace=False)] = -1
    hits["sphere"][rng.choice(n, 3, replace=False)] = 1 << 20                     # not in the world's list: never lambertian, never read
    k = rng.choice(np.array([1, 4, 8, 12], np.int32), n, p=[0.05, 0.3, 0.35, 0.3])
    S = (rng.uniform(0.2, 1.0, (n, 3)) * k[:, None]).astype(np.float32)
    SL = ((S[:, 0] + S[:, 1]) + S[:, 2]).astype(np.float32)
    Q = (SL * SL / k * rng.uniform(1.0, 1.5, n)).astype(np.float32)
    S[rng.choice(n, 3, replace=False), 0] = np.float32("inf")
    return dict(nx=nx, ny=ny, cam=cam, hits=hits, prev=prev, hist=tm.make_history(xv, neff_in), state=tm.make_state(S, SL, Q, k))


@pytest.mark.parametrize("kw", [dict(), dict(reuse_specular=1), dict(position_tolerance=0.05, max_history=8), dict(normal_min_dot=-1.0, reuse_specular=1)],
                         ids=["tol1", "specular", "tight", "any_normal"])
def test_every_skip_cause_on_fabricated_buffers(rt, cuda, kw):
    torch = cuda
    W = rt.World(500, 17, 16)
    kind = W.spheres["material"].astype(np.int32)
    fab = fabricated(rt, kind)
    nx, ny = fab["nx"], fab["ny"]
    p = rt.temporal_params(**dict(dict(position_tolerance=1.0), **kw))
    c = {}
    ref = tm.accumulate(fab["hist"], fab["hits"], fab["prev"], fab["cam"], fab["state"], kind, nx, ny, p.max_history, p.reuse_specular,
                        p.position_tolerance, p.normal_min_dot, counts=c)
    print({k: v for k, v in c.items() if k != "took_mask"})
    causes = ["lam_reject", "nan_p", "off_frame", "out_left", "out_right", "out_bottom", "out_top", "neff0", "sphere", "position", "all_refused",
              "accepted", "took"] + ([] if p.normal_min_dot == -1.0 else ["normal"])
    for name in causes:
        assert c[name] >= 1, name
    dev = {name: torch.from_numpy(np.ascontiguousarray(fab[name]).view(np.uint8).copy()).cuda() for name in ("hits", "prev", "hist", "state")}
    out = rt.alloc_temporal_history(nx, ny)
    out.fill_(7.0)
    rt.temporal_accumulate(out, dev["hist"], dev["hits"], dev["prev"], fab["cam"], dev["state"], W, nx, ny, p)
    torch.cuda.synchronize()
    assert same_any_nan(out.cpu().numpy(), ref)
    W.close()


# ---- 3. a first frame: the new prepare against the old one ---------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2, 3, 5])
def test_first_frame_filters_like_denoise_adaptive(rt, cuda, paths, levels):
    torch = cuda
    fr = paths["static"].frames[0]
    hist = gpu_chain(rt, torch, paths["static"], rt.temporal_params(), upto=1)[0]
    p = rt.denoise_var_params(levels=levels)
    ref, got = torch.full_like(fr["fb"], 7.0), torch.full_like(fr["fb"], 9.0)
    work = rt.alloc_denoise_work(NX, NY)
    rt.denoise_adaptive(ref, fr["fb"], NX, NY, fr["d_hits"], fr["state"], p, work)
    rt.denoise_history(got, fr["fb"], NX, NY, fr["d_hits"], hist, p, work)
    torch.cuda.synchronize()
    assert same_any_nan(got.cpu().numpy(), ref.cpu().numpy())
    assert not np.array_equal(got.cpu().numpy(), fr["fb"].cpu().numpy())           # the filter did something


# ---- 4. tiny frames ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(1, 1), (3, 2), (16, 17)])
def test_tiny_frames(rt, cuda, nx, ny):
    torch = cuda
    P = Path(rt, torch, 500, 30, nx, ny, [0.0, 0.0, 2.0], [(4, 32, 4, 0.1, 0.02)])
    for p in (rt.temporal_params(position_tolerance=1.0), rt.temporal_params(reuse_specular=1, max_history=8)):
        got = gpu_chain(rt, torch, P, p)
        ref, _ = model_chain(P, p)
        for f in range(3):
            assert same_any_nan(got[f].cpu().numpy(), ref[f]), (nx, ny, f)
    fr = P.frames[0]
    hist = gpu_chain(rt, torch, P, rt.temporal_params(), upto=1)[0]
    ref, got = torch.full_like(fr["fb"], 7.0), torch.full_like(fr["fb"], 9.0)
    work = rt.alloc_denoise_work(nx, ny)
    rt.denoise_adaptive(ref, fr["fb"], nx, ny, fr["d_hits"], fr["state"], rt.denoise_var_params(levels=3), work)
    rt.denoise_history(got, fr["fb"], nx, ny, fr["d_hits"], hist, rt.denoise_var_params(levels=3), work)
    torch.cuda.synchronize()
    assert same_any_nan(got.cpu().numpy(), ref.cpu().numpy())
    P.close()


# ---- 5. a graph, in place, refusals ----------------------------------------------------------------------------------------------------
def test_captured_in_a_graph(rt, cuda, paths):
    torch = cuda
    P = paths["orbit"]
    p, dp = rt.temporal_params(position_tolerance=1.0), rt.denoise_var_params(levels=3)
    h = gpu_chain(rt, torch, P, p)
    a, b = P.frames[1], P.frames[2]
    ref = torch.zeros_like(b["fb"])
    work = rt.alloc_denoise_work(NX, NY)
    rt.denoise_history(ref, b["fb"], NX, NY, b["d_hits"], h[2], dp, work)
    torch.cuda.synchronize()
    hist, out = rt.alloc_temporal_history(NX, NY), torch.zeros_like(b["fb"])
    b["W"].upload()                                                              # (already there: the frame was rendered)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rt.temporal_accumulate(hist, h[1], b["d_hits"], a["d_hits"], a["cam"], b["state"], b["W"], NX, NY, p)
        rt.denoise_history(out, b["fb"], NX, NY, b["d_hits"], hist, dp, work)
    for _ in range(2):
        hist.fill_(3.0)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert same_any_nan(hist.cpu().numpy(), h[2].cpu().numpy())
        assert same_any_nan(out.cpu().numpy(), ref.cpu().numpy())


def test_in_place(rt, cuda, paths):
    torch = cuda
    P = paths["static"]
    h = gpu_chain(rt, torch, P, rt.temporal_params())[2]
    fr = P.frames[2]
    dp = rt.denoise_var_params(levels=4)
    work = rt.alloc_denoise_work(NX, NY)
    ref = torch.zeros_like(fr["fb"])
    rt.denoise_history(ref, fr["fb"], NX, NY, fr["d_hits"], h, dp, work)
    buf = fr["fb"].clone()
    rt.denoise_history(buf, buf, NX, NY, fr["d_hits"], h, dp, work)
    torch.cuda.synchronize()
    assert same_any_nan(buf.cpu().numpy(), ref.cpu().numpy())
    assert not np.array_equal(buf.cpu().numpy(), fr["fb"].cpu().numpy())


def test_refusals(rt, cuda, paths):
    torch = cuda
    P = paths["static"]
    a, b = P.frames[0], P.frames[1]
    p = rt.temporal_params()
    n = NX * NY
    m = (5 * n + 3) // 4 * 4                                                     # floats to the next 16-byte boundary behind one history
    big = torch.zeros(2 * m + 16, dtype=torch.float32, device="cuda")
    first, second = big[:5 * n], big[m:m + 5 * n]                                # both 16-byte aligned, no overlap
    rt.temporal_accumulate(first, None, a["d_hits"], None, None, a["state"], a["W"], NX, NY, p)
    rt.temporal_accumulate(second, first, b["d_hits"], a["d_hits"], a["cam"], b["state"], b["W"], NX, NY, p)
    torch.cuda.synchronize()

    def refused(*args):
        with pytest.raises(rt.RtError) as e:
            rt.temporal_accumulate(*args)
        return str(e.value)

    for out in (second, big[m + 4:m + 4 + 5 * n], big[m - 4:m - 4 + 5 * n]):       # the same buffer, and aligned overlaps from either side
        assert "failed: -1 " in refused(out, second, b["d_hits"], a["d_hits"], a["cam"], b["state"], b["W"], NX, NY, p)
    assert "failed: -1 " in refused(big[1:5 * n + 1], second, b["d_hits"], a["d_hits"], a["cam"], b["state"], b["W"], NX, NY, p)      # misaligned
    assert "failed: -1 " in refused(second, big[1:5 * n + 1], b["d_hits"], a["d_hits"], a["cam"], b["state"], b["W"], NX, NY, p)
    assert "failed: -1 " in refused(second, first, b["d_hits"][4:], a["d_hits"], a["cam"], b["state"], b["W"], NX, NY, p)
    assert "failed: -1 " in refused(second, first, b["d_hits"], a["d_hits"][8:], a["cam"], b["state"], b["W"], NX, NY, p)
    half = rt.World(500, NX, NY, precision=rt.FP16)
    assert "failed: -4 " in refused(second, first, b["d_hits"], a["d_hits"], a["cam"], b["state"], half, NX, NY, p)
    half.close()
    work = rt.alloc_denoise_work(NX, NY)
    with pytest.raises(rt.RtError):
        rt.denoise_history(torch.zeros_like(b["fb"]), b["fb"], NX, NY, b["d_hits"], big[1:5 * n + 1], rt.denoise_var_params(), work)
    torch.cuda.synchronize()


# ---- 6. quality --------------------------------------------------------------------------------------------------------------------
def test_four_frames_beat_one(rt, cuda):
    """203x77, N = 10 000, SPL 32, four frames of 8 spp each (rel_error 0, min_spp = max_spp), RNG states carried on, against
    rt_render(512) at the last camera; gamma frames, RMSE over the pixels named.

    Static camera, library defaults: rt_denoise_history of the fourth history has a lower RMSE than rt_denoise_adaptive on the fourth
    frame alone, over the pixels finite in all three frames.  Orbit of 1 degree per frame, position_tolerance 1 (the module's docstring
    says why): over the lambertian pixels whose fourth frame took history, sqrt of the unfiltered history has a lower RMSE than the raw
    fourth frame.  Both bounds are the plain inequality: four frames' samples against one frame's on view-independent surfaces.

    Measured on one MI355X: static 0.03389 against 0.05113 over all 15 631 pixels; orbit 0.04689 against 0.05893 over 6 539 pixels."""
    torch = cuda
    uniform = [(8, 8, 4, 0.0, 0.0)]

    def reference(fr):
        fb, st = rt.alloc_fb(NX, NY), rt.alloc_rand_state(NX, NY)
        rt.render_init(NX, NY, st)
        rt.render(fb, NX, NY, 512, fr["W"], st, fr["O"])
        torch.cuda.synchronize()
        return fb.cpu().numpy().reshape(-1, 3).astype(np.float64)

    def rmse(img, ref, mask):
        return float(np.sqrt(((img[mask] - ref[mask]) ** 2).mean()))

    # static camera: the filtered history against the filtered last frame
    P = Path(rt, torch, N, SPL, NX, NY, [0.0] * 4, uniform)
    last = P.frames[3]
    ref = reference(last)
    h = gpu_chain(rt, torch, P, rt.temporal_params())[3]
    one, four = torch.zeros_like(last["fb"]), torch.zeros_like(last["fb"])
    work = rt.alloc_denoise_work(NX, NY)
    rt.denoise_adaptive(one, last["fb"], NX, NY, last["d_hits"], last["state"], rt.denoise_var_params(), work)
    rt.denoise_history(four, last["fb"], NX, NY, last["d_hits"], h, rt.denoise_var_params(), work)
    torch.cuda.synchronize()
    one, four = (t.cpu().numpy().reshape(-1, 3).astype(np.float64) for t in (one, four))
    fin = np.isfinite(ref).all(1) & np.isfinite(one).all(1) & np.isfinite(four).all(1)
    e_one, e_four = rmse(one, ref, fin), rmse(four, ref, fin)
    print("static: rt_denoise_history %.5f rt_denoise_adaptive %.5f over %d pixels" % (e_four, e_one, fin.sum()))
    P.close()

    # the orbit: the unfiltered history against the raw last frame, where history was taken
    P = Path(rt, torch, N, SPL, NX, NY, [0.0, 1.0, 2.0, 3.0], uniform)
    last = P.frames[3]
    ref = reference(last)
    p = rt.temporal_params(position_tolerance=1.0)
    h = gpu_chain(rt, torch, P, p)[3].cpu().numpy()
    _, counts = model_chain(P, p)
    xv, neff = tm.history_parts(h, NX * NY)
    took = counts[3]["took_mask"] & (P.kind[np.clip(last["hits"]["sphere"], 0, None)] == rt.MAT_LAMBERTIAN)
    assert np.array_equal(neff > 8, counts[3]["took_mask"])                        # the kernel took history exactly where the model did
    raw = last["fb"].cpu().numpy().reshape(-1, 3).astype(np.float64)
    acc = np.sqrt(xv[:, :3].astype(np.float64))
    took &= np.isfinite(ref).all(1) & np.isfinite(raw).all(1) & np.isfinite(acc).all(1)
    e_raw, e_acc = rmse(raw, ref, took), rmse(acc, ref, took)
    print("orbit: unfiltered history %.5f raw %.5f over %d lambertian pixels that took history" % (e_acc, e_raw, took.sum()))
    P.close()
    assert took.sum() > NX * NY // 4
    assert e_four < e_one, (e_four, e_one)
    assert e_acc < e_raw, (e_acc, e_raw)
