"""rt_adaptive_budget_select_temporal / rt_render_adaptive_spend_temporal (-m gpu): every comparison is bit or set equality, no
tolerances, no quality figure and no time.

The key kernel is held to tests/temporal_budget_model.py — temporal_model.accumulate, the key of the merged pixel, the set by a plain
sort — on the second and third frame of the camera paths of tests/test_gpu_temporal.py (static, 1 degree, 60 degrees; 203x77 and 23x11),
on a first frame, on all-sky guides, on a frame whose cut falls between equal keys, on tiny frames, on a frame with more tiles than
blocks and on the fabricated left / right case of tests/test_temporal_budget_host.py.  The last frame's history that the model is fed
is the one rt_temporal_accumulate wrote on the device (tests/test_gpu_temporal.py holds that kernel to the model).  A spend is checked
as tests/test_gpu_adaptive_budget.py checks the raw one, with the frames, scenes and per-pixel exactness check of tests/adaptive_frames.py;
the camera paths and their chains of histories are tests/temporal_paths.py's."""
import ctypes as C

import numpy as np
import pytest

import adaptive_budget_model as B
import denoise_var_model as V
import filtered_budget_model as FM
import temporal_budget_model as M
import temporal_model as tm
from adaptive_frames import (BATCH, FLOOR, MAX_SPP, SENTINEL, Frame, Scene, check_exact, check_round, check_round_filtered, check_round_temporal,
                             model_pick, state_parts)
from bitcmp import assert_same_snapshots, raw_bits, same_any_nan
from temporal_paths import gpu_chain, Path, PATHS

pytestmark = pytest.mark.gpu

NX, NY = 203, 77                   # 203 x 77: 13 x 5 tiles of 16 x 16, ragged on both edges; 15 full selection spans and a rest
N, SPL = 10000, 32
LOOSE = (4, 64, 4, 0.1, FLOOR)     # the frame a spend continues (tests/test_gpu_filtered_budget.py's)
ADAPT = (4, 64, 4, 0.1, 0.02)      # (min_spp, max_spp, batch, rel_error, floor): pixels stop at many different counts
SMALL = (23, 11)
PARAMS = [dict(), dict(position_tolerance=1.0), dict(max_history=0), dict(max_history=8), dict(reuse_specular=1), dict(normal_min_dot=0.99)]


def tup(p):
    return (p.max_history, p.reuse_specular, p.position_tolerance, p.normal_min_dot)


def upload(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def gpu_select(rt, torch, ctx, d_state, W, nx, ny, tin, p, K, batch=BATCH, max_spp=MAX_SPP, floor=FLOOR, want_keys=True):
    """one rt_adaptive_budget_select_temporal: (sorted ids, the float keys or None); nothing may be written behind the count"""
    n = nx * ny
    cap = min(K, n)
    lst = torch.full((cap + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda")
    keys = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda") if want_keys else None
    rt.adaptive_budget_select_temporal(ctx, d_state, W, nx, ny, rt.Budget(0, 1, batch, max_spp, floor), tin, p, K, lst, cnt, keys)
    torch.cuda.synchronize()
    got, c = lst.cpu().numpy().view(np.uint32), int(cnt.cpu().numpy().view(np.uint32)[0])
    assert (got[c:] == SENTINEL).all()
    return np.sort(got[:c]), keys.cpu().numpy().view(np.float32) if want_keys else None


def check_select(rt, torch, ctx, W, kind, nx, ny, p, Ks, hist, hits, prev_hits, prev_cam, state, dev=None):
    """keys and sets of one frame against the model for every K of Ks (a callable gets the number of eligible pixels); the inputs are
    host arrays (hist None: the first frame), dev optionally the device tensors they were read from"""
    dev = dict(dev or {})
    for name, a in (("hist", hist), ("hits", hits), ("prev", prev_hits), ("state", state)):
        if name not in dev:
            dev[name] = upload(torch, a) if a is not None else None
    tin = rt.temporal_inputs(dev["hits"], dev["hist"], dev["prev"], prev_cam)
    key, valid, _ = M.frame_keys(hist, hits, prev_hits, prev_cam, state, kind, nx, ny, FLOOR, *tup(p))
    _, ok, kb = M.select(hist, hits, prev_hits, prev_cam, state, kind, nx, ny, BATCH, MAX_SPP, FLOOR, 0, tup(p))
    assert np.array_equal(kb, B.keybits(key))
    elig = int(ok.sum())
    before = [None if dev[name] is None else dev[name].cpu().numpy().copy() for name in ("hist", "state")]
    for K in (Ks(elig) if callable(Ks) else Ks):
        chosen = FM.pick(ok, kb, K)
        got, keys = gpu_select(rt, torch, ctx, dev["state"], W, nx, ny, tin, p, K)
        assert same_any_nan(keys, key), (nx, ny, K, int((keys.view(np.uint32) != kb).sum()))
        assert len(got) == min(K, elig) and np.array_equal(got, chosen), (nx, ny, K)
    for name, b in zip(("hist", "state"), before):                  # both are only read
        assert b is None or np.array_equal(dev[name].cpu().numpy(), b), name
    return ok, kb, valid


def four_Ks(n):
    return lambda elig: (0, 1, n // 10, n)


@pytest.fixture(scope="module")
def ctx(rt, cuda):
    c = rt.RenderCtx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def paths(rt, cuda):
    """three frames on each camera path of tests/test_gpu_temporal.py: at 203x77 its world (10 000 spheres), at 23x11 500 spheres"""
    M.self_check()                                 # the model follows the rule before the kernel is held to the model
    made = {}
    for size, (n_spheres, spl) in (((NX, NY), (N, SPL)), (SMALL, (500, 30))):
        made[size] = {name: Path(rt, cuda, n_spheres, spl, size[0], size[1], [0.0, step, 2 * step], [ADAPT]) for name, step in PATHS.items()}
    yield made
    for group in made.values():
        for P in group.values():
            P.close()


# ---- 1. kernel == model on the second and third frame of the camera paths ------------------------------------------------------------
@pytest.mark.parametrize("size", [SMALL, (NX, NY)], ids=["23x11", "203x77"])
@pytest.mark.parametrize("kw", PARAMS, ids=[",".join("%s=%s" % kv for kv in c.items()) or "defaults" for c in PARAMS])
@pytest.mark.parametrize("path", list(PATHS))
def test_keys_and_set_match_the_model(rt, cuda, ctx, paths, path, kw, size):
    torch = cuda
    nx, ny = size
    P = paths[size][path]
    p = rt.temporal_params(**kw)
    hist = gpu_chain(rt, torch, P, p, upto=2)                                   # the histories of frames 0 and 1
    took = 0
    for f in (1, 2):
        fr, prev = P.frames[f], P.frames[f - 1]
        h = hist[f - 1].cpu().numpy()
        ok, kb, valid = check_select(rt, torch, ctx, fr["W"], P.kind, nx, ny, p, four_Ks(nx * ny), h, fr["hits"], prev["hits"], prev["cam"],
                                     fr["h_state"], dev=dict(hist=hist[f - 1], hits=fr["d_hits"], prev=prev["d_hits"], state=fr["state"]))
        k = state_parts(fr["h_state"], nx * ny)[3]
        assert 0 < ok.sum() < nx * ny and 0 < valid.sum() < nx * ny and len(np.unique(k)) >= 3
        assert (kb[k + BATCH > MAX_SPP] > 0).any()                                 # the mask is not the key
        c = {}
        M.frame_keys(h, fr["hits"], prev["hits"], prev["cam"], fr["h_state"], P.kind, nx, ny, FLOOR, *tup(p), counts=c)
        took += c["took"]
    if p.max_history == 0:
        assert took == 0
    elif path == "static":
        assert took > 0                                                            # the history entered the keys that were compared


# ---- 2. a first frame ----------------------------------------------------------------------------------------------------------------
def test_first_frame_keys_are_the_filtered_rule_on_this_frame(rt, cuda, ctx, paths):
    torch = cuda
    P = paths[(NX, NY)]["static"]
    fr = P.frames[0]
    n = NX * NY
    p = rt.temporal_params()
    _, keys = gpu_select(rt, torch, ctx, fr["state"], fr["W"], NX, NY, rt.temporal_inputs(fr["d_hits"]), p, n // 10)
    xc, vc, _, empty = tm.frame_values(fr["h_state"], fr["hits"], n)
    _, SL, Q, k = state_parts(fr["h_state"], n)
    with np.errstate(all="ignore"):
        l = (xc[:, 0] + xc[:, 1]) + xc[:, 2]
    want = np.where(empty, B.priority(SL, Q, k, FLOOR), FM.priority_filtered(l, vc, FLOOR))
    assert 0 < empty.sum() < n and same_any_nan(keys, want)
    raw = B.priority(SL, Q, k, FLOOR)
    assert not np.array_equal(raw_bits(want[~empty]), raw_bits(raw[~empty]))                # the same quantity, not the same bits
    assert np.allclose(want[~empty], raw[~empty], rtol=1e-5, atol=0)
    check_select(rt, torch, ctx, fr["W"], P.kind, NX, NY, p, four_Ks(n), None, fr["hits"], None, None, fr["h_state"],
                 dev=dict(hist=None, hits=fr["d_hits"], prev=None, state=fr["state"]))


# ---- 3. all-sky guides: every pixel is EMPTY ----------------------------------------------------------------------------------------
def test_all_sky_guides_select_what_the_raw_key_selects(rt, cuda, ctx):
    torch = cuda
    _, hits, state, _ = V.synthetic_state(NX, NY, 9)
    hits["sphere"] = -1
    n = NX * NY
    rng = np.random.default_rng(3)
    hist = tm.make_history(rng.uniform(0, 1, (n, 4)).astype(np.float32), np.full(n, 16, np.float32))
    W = rt.World(500, NX, NY)
    kind = W.spheres["material"].astype(np.int32)
    d_state, d_hits, d_hist = upload(torch, state), upload(torch, hits), upload(torch, hist)
    _, SL, Q, k = V.state_parts(state, n)
    p = rt.temporal_params(reuse_specular=1)
    ok, kb, valid = check_select(rt, torch, ctx, W, kind, NX, NY, p, four_Ks(n), hist, hits, hits, W.camera, state,
                                 dev=dict(hist=d_hist, hits=d_hits, prev=d_hits, state=d_state))
    assert not valid.any() and np.array_equal(kb, B.keybits(B.priority(SL, Q, k, FLOOR)))
    tin = rt.temporal_inputs(d_hits, d_hist, d_hits, W.camera)
    for K in (1, int(ok.sum()) // 2, n):
        lst = torch.full((min(K, n) + 64,), SENTINEL, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        rt.adaptive_budget_select(ctx, d_state, NX, NY, rt.Budget(0, 1, BATCH, MAX_SPP, FLOOR), K, lst, cnt)
        torch.cuda.synchronize()
        c = int(cnt.cpu().numpy()[0])
        raw = np.sort(lst.cpu().numpy().view(np.uint32)[:c])
        got, _ = gpu_select(rt, torch, ctx, d_state, W, NX, NY, tin, p, K, want_keys=False)
        assert c == min(K, int(ok.sum())) and np.array_equal(got, raw)
    W.close()


# ---- 4. the fabricated left / right case, and a cut between equal keys ------------------------------------------------------------------
def left_right_on_device(rt, torch, nx, ny):
    c = M.left_right_case(nx, ny)
    W = rt.World(500, nx, ny)
    kind = W.spheres["material"].astype(np.int32)
    assert kind[0] == rt.MAT_LAMBERTIAN == tm.LAMBERTIAN           # the case's guides name sphere 0
    return c, W, kind


def test_left_right_case_selects_the_half_without_history(rt, cuda, ctx):
    torch = cuda
    c, W, kind = left_right_on_device(rt, torch, 16, 8)
    nx, ny = c["nx"], c["ny"]
    p = rt.temporal_params(max_history=32, position_tolerance=10.0)
    assert np.array_equal(np.float32(tup(p)), np.float32(c["temporal"]))
    K = int(c["right"].sum())
    ok, kb, valid = check_select(rt, torch, ctx, W, kind, nx, ny, p, (K,), c["hist"], c["hits"], c["prev"], c["cam"], c["state"])
    claim_l, claim_r = c["left"] & ~c["seam"], c["right"] & ~c["seam"]
    assert valid.all() and ok.all() and kb[claim_r].min() > kb[claim_l].max()
    tin = rt.temporal_inputs(upload(torch, c["hits"]), upload(torch, c["hist"]), upload(torch, c["prev"]), c["cam"])
    got, keys = gpu_select(rt, torch, ctx, upload(torch, c["state"]), W, nx, ny, tin, p, K)
    assert np.array_equal(got, np.nonzero(c["right"])[0])          # stated without the model: exactly the right half
    assert keys[claim_r].min() > keys[claim_l].max() > 0
    W.close()


def test_cut_between_equal_keys(rt, cuda, ctx):
    torch = cuda
    c, W, kind = left_right_on_device(rt, torch, 64, 32)           # 4 x 2 tiles, two selection spans; pixel centres exact in binary32
    nx, ny = c["nx"], c["ny"]
    p = rt.temporal_params(max_history=32, position_tolerance=10.0)
    _, ok, kb = M.select(c["hist"], c["hits"], c["prev"], c["cam"], c["state"], kind, nx, ny, BATCH, MAX_SPP, FLOOR, 0, tup(p))
    left, right = c["left"], c["right"]
    assert ok.all() and len(np.unique(kb[left])) == 1 and len(np.unique(kb[right])) == 1 and kb[right][0] > kb[left][0]
    n_r, n_l = int(right.sum()), int(left.sum())
    for K in (n_r // 2, n_r + n_l // 2):                           # inside the upper group, inside the lower one
        assert B.tie_straddles(kb, ok, K)                          # before the GPU is asked
    K = n_r + n_l // 2
    chosen = FM.pick(ok, kb, K)
    ties = np.nonzero(left)[0]
    assert ties[np.isin(ties, chosen)].max() < ties[~np.isin(ties, chosen)].min()      # the lower ids
    check_select(rt, torch, ctx, W, kind, nx, ny, p, (n_r // 2, K, n_r, n_r + 1), c["hist"], c["hits"], c["prev"], c["cam"], c["state"])
    W.close()


# ---- 5. tiny frames, 6. more tiles than blocks -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 37), (41, 1), (17, 2)])
def test_tiny_frames(rt, cuda, ctx, nx, ny):
    torch = cuda
    P = Path(rt, torch, 500, 30, nx, ny, [0.0, 0.0, 1.0], [(4, 32, 4, 0.1, FLOOR)])
    for p in (rt.temporal_params(position_tolerance=1.0), rt.temporal_params(reuse_specular=1, max_history=8)):
        hist = gpu_chain(rt, torch, P, p, upto=2)
        for f in (1, 2):
            fr, prev = P.frames[f], P.frames[f - 1]
            check_select(rt, torch, ctx, fr["W"], P.kind, nx, ny, p, lambda elig: (0, 1, max(elig // 3, 1), elig + 5), hist[f - 1].cpu().numpy(),
                         fr["hits"], prev["hits"], prev["cam"], fr["h_state"],
                         dev=dict(hist=hist[f - 1], hits=fr["d_hits"], prev=prev["d_hits"], state=fr["state"]))
    P.close()


def test_more_tiles_than_blocks(rt, cuda, ctx):
    torch = cuda
    nx, ny = 530, 500                                          # 34 x 32 = 1088 tiles of 16 x 16: a block takes two
    assert ((nx + 15) // 16) * ((ny + 15) // 16) > 1024
    P = Path(rt, torch, 500, 30, nx, ny, [0.0, 0.2], [ADAPT])
    p = rt.temporal_params()
    hist = gpu_chain(rt, torch, P, p, upto=1)[0]
    fr, prev = P.frames[1], P.frames[0]
    c = {}
    h = hist.cpu().numpy()
    M.frame_keys(h, fr["hits"], prev["hits"], prev["cam"], fr["h_state"], P.kind, nx, ny, FLOOR, *tup(p), counts=c)
    assert c["took"] > 1000 and c["asked"] > c["took"]                             # history was taken, and refused
    ok, _, _ = check_select(rt, torch, ctx, fr["W"], P.kind, nx, ny, p, (nx * ny // 5,), h, fr["hits"], prev["hits"], prev["cam"], fr["h_state"],
                            dev=dict(hist=hist, hits=fr["d_hits"], prev=prev["d_hits"], state=fr["state"]))
    assert ok.sum() > nx * ny // 5
    P.close()


# ---- 7. the spend on a rendered frame ------------------------------------------------------------------------------------------------
def temporal_scene(rt, torch, n_spheres, spl, nx, ny, trav=None):
    """Scene (this frame: create_world's camera) with its guides, and the last frame: the same spheres seen from one degree further
    round the orbit, its guides, camera and first-frame history.  position_tolerance 1: the docstring of tests/test_gpu_temporal.py says why."""
    sc = Scene(rt, torch, n_spheres, spl, nx, ny, trav).with_guides()
    sc.last = Path(rt, torch, n_spheres, 30 if spl is None else spl, nx, ny, [1.0], [ADAPT])
    assert np.array_equal(sc.last.kind, sc.W.spheres["material"].astype(np.int32))
    sc.tp = rt.temporal_params(position_tolerance=1.0)
    sc.d_hist = gpu_chain(rt, torch, sc.last, sc.tp)[0]
    sc.hist = sc.d_hist.cpu().numpy().copy()
    prev = sc.last.frames[0]
    sc.tin = rt.temporal_inputs(sc.d_hits, sc.d_hist, prev["d_hits"], prev["cam"])
    sc.model_select = lambda state, K, batch=BATCH, max_spp=MAX_SPP: M.select(sc.hist, sc.hits, prev["hits"], prev["cam"], state, sc.last.kind, nx, ny,
                                                                             batch, max_spp, FLOOR, K, tup(sc.tp))
    return sc


def close_scene(sc):
    sc.last.close()
    sc.close()


@pytest.fixture(scope="module")
def scene(rt, cuda):
    sc = temporal_scene(rt, cuda, N, SPL, NX, NY)
    c = {}
    prev = sc.last.frames[0]
    F = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(sc.W, sc.O, LOOSE)
    M.frame_keys(sc.hist, sc.hits, prev["hits"], prev["cam"], F.snap()["state"], sc.last.kind, NX, NY, FLOOR, *tup(sc.tp), counts=c)
    assert c["took"] > NX * NY // 10 and c["asked"] > c["took"]                     # the history enters the ranking of this scene, and is refused
    yield sc
    close_scene(sc)


def rounds_compose(rt, torch, sc, ctx=None, stream=None):
    A = Frame(rt, torch, sc.nx, sc.ny, rt.WHOLE, ctx, stream).begin(sc.W, sc.O, LOOSE)
    Bf = Frame(rt, torch, sc.nx, sc.ny, rt.WHOLE).begin(sc.W, sc.O, LOOSE)
    n = A.n
    q = n // 4 + 1
    samples, rounds = BATCH * q + 3, 3                       # three rounds of batch 4
    Ks = [B.picks(samples, rounds, BATCH, r) for r in range(rounds)]
    assert sum(Ks) == q and len(set(Ks)) == 2
    picked = A.spend_temporal(sc, samples, rounds)
    singles = []
    for K in Ks:
        before = Bf.snap()
        pk = Bf.spend_temporal(sc, K * BATCH, 1)
        check_round_temporal(sc, Bf, before, Bf.snap(), pk[0], K)
        singles.append(int(pk[0]))
    assert list(picked) == singles and sum(singles) > q // 2
    final = A.snap()
    assert_same_snapshots(final, Bf.snap())
    check_exact(sc, A, final)
    assert len(np.unique(final["spp"])) >= 3
    assert np.array_equal(sc.d_hist.cpu().numpy(), sc.hist)  # d_hist_in is only read
    return A, final


def test_rendered_frame_rounds_compose(rt, cuda, scene):
    rounds_compose(rt, cuda, scene)
    # the history-aware key is another ordering than the raw one on this frame: the first round's sets differ
    F = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(scene.W, scene.O, LOOSE)
    snap = F.snap()
    K = F.n // 6
    h_set = scene.model_select(snap["state"], K)[0]
    r_set = model_pick(snap, F.n, F.inside, K)[0]
    assert len(h_set) == len(r_set) == K and not np.array_equal(h_set, r_set)


def test_list_path(rt, cuda):
    sc = temporal_scene(rt, cuda, 500, None, 131, 71, 0)
    assert rt.render_kernel_name(sc.W, sc.O) == "k_render<false,0,1>"
    rounds_compose(rt, cuda, sc)
    close_scene(sc)


def test_context_on_a_side_stream(rt, cuda, scene):
    torch = cuda
    c = rt.RenderCtx()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    rounds_compose(rt, torch, scene, ctx=c, stream=s.cuda_stream)
    assert len(c.times()) == 2                               # begin and the spend
    c.close()


def test_raw_then_temporal_then_filtered_spend(rt, cuda, scene):
    sc, fp = scene, rt.denoise_var_params()
    F = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(sc.W, sc.O, LOOSE)
    before = F.snap()
    pk = F.spend(sc.W, sc.O, 3000 * BATCH, 1)
    mid = F.snap()
    check_round(sc, F, before, mid, pk[0], 3000)
    pk = F.spend_temporal(sc, 2500 * BATCH, 1)
    after = F.snap()
    check_round_temporal(sc, F, mid, after, pk[0], 2500)
    pk = F.spend_filtered(sc, fp, 1000 * BATCH, 1)
    last = F.snap()
    check_round_filtered(sc, F, after, last, pk[0], 1000, fp)
    check_exact(sc, F, last)
    pk = F.spend_temporal(sc, 500 * BATCH, 1)                # ... and back
    check_round_temporal(sc, F, last, F.snap(), pk[0], 500)
    assert np.array_equal(sc.d_hist.cpu().numpy(), sc.hist)


def test_accumulate_around_a_round_differs_only_in_chosen_pixels(rt, cuda, scene):
    torch, sc = cuda, scene
    n = NX * NY
    prev = sc.last.frames[0]
    F = Frame(rt, torch, NX, NY, rt.WHOLE).begin(sc.W, sc.O, LOOSE)

    def accumulate():
        h = rt.alloc_temporal_history(NX, NY)
        h.fill_(7.0)
        rt.temporal_accumulate(h, sc.d_hist, sc.d_hits, prev["d_hits"], prev["cam"], F.state, sc.W, NX, NY, sc.tp)
        torch.cuda.synchronize()
        return tm.history_parts(h.cpu().numpy(), n)

    xv0, neff0 = accumulate()
    before = F.snap()
    K = 3000
    pk = F.spend_temporal(sc, K * BATCH, 1)
    chosen = check_round_temporal(sc, F, before, F.snap(), pk[0], K)
    xv1, neff1 = accumulate()
    hit = np.zeros(n, bool)
    hit[chosen] = True
    assert len(chosen) == K
    assert np.array_equal(raw_bits(xv0[~hit]), raw_bits(xv1[~hit])) and np.array_equal(raw_bits(neff0[~hit]), raw_bits(neff1[~hit]))
    live = hit & (neff0 > 0)
    assert live.any() and (neff1[live] > neff0[live]).all()                        # m + (n + batch) against m + n
    assert np.array_equal(sc.d_hist.cpu().numpy(), sc.hist)


# ---- 8. errors on the device -----------------------------------------------------------------------------------------------------
def test_binary16_and_contracted_worlds(rt, cuda, scene, ctx):
    torch, sc = cuda, scene
    F = Frame(rt, torch, NX, NY, rt.WHOLE).begin(sc.W, sc.O, LOOSE)
    Bd = rt.Budget(4000, 1, BATCH, MAX_SPP, FLOOR)
    w16 = rt.World(N, NX, NY, precision=rt.FP16)
    wc = rt.World(N, NX, NY)
    wc.set_arith(rt.ARITH_CONTRACT)
    before = F.snap()
    for W in (w16, wc):
        with pytest.raises(rt.RtError, match="-4"):
            rt.render_adaptive_spend_temporal(F.fb, NX, NY, Bd, sc.tin, sc.tp, W, F.st, F.state, None, F.spp)
    lst = torch.full((1064,), SENTINEL, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda")
    with pytest.raises(rt.RtError, match="-4"):
        rt.adaptive_budget_select_temporal(ctx, F.state, w16, NX, NY, Bd, sc.tin, sc.tp, 1000, lst, cnt)
    torch.cuda.synchronize()
    assert_same_snapshots(F.snap(), before)
    assert int(cnt.cpu().numpy()[0]) == SENTINEL
    # the selection renders nothing: a contracted world supplies kind[] like any other
    want, _ = gpu_select(rt, torch, ctx, F.state, sc.W, NX, NY, sc.tin, sc.tp, 1000, want_keys=False)
    got, _ = gpu_select(rt, torch, ctx, F.state, wc, NX, NY, sc.tin, sc.tp, 1000, want_keys=False)
    assert len(want) == 1000 and np.array_equal(got, want)
    w16.close()
    wc.close()


def test_refused_during_a_capture(rt, cuda, scene, ctx):
    torch, sc = cuda, scene
    F = Frame(rt, torch, NX, NY, rt.WHOLE).begin(sc.W, sc.O, LOOSE)
    Bd = rt.Budget(4000, 1, BATCH, MAX_SPP, FLOOR)
    F.spend_temporal(sc, 4000, 1)                            # warm: the workspaces exist, so only the capture can be the reason
    lst = torch.zeros(1064, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    gpu_select(rt, torch, ctx, F.state, sc.W, NX, NY, sc.tin, sc.tp, 1000, want_keys=False)
    marker = torch.zeros(4, device="cuda")
    before = F.snap()
    L = rt.lib()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        marker.add_(1.0)                                     # (the graph is not empty)
        rc_spend = L.rt_render_adaptive_spend_temporal(F.fb.data_ptr(), NX, NY, C.byref(Bd), C.byref(sc.tin), C.byref(sc.tp), sc.W.h,
                                                       F.st.data_ptr(), sc.O.h, F.spp.data_ptr(), F.state.data_ptr(), None, s)
        rc_select = L.rt_adaptive_budget_select_temporal(ctx.h, F.state.data_ptr(), sc.W.h, NX, NY, C.byref(Bd), C.byref(sc.tin), C.byref(sc.tp), 1000,
                                                         lst.data_ptr(), cnt.data_ptr(), None, s)
    assert rc_spend == -1 and rc_select == -1
    g.replay()
    torch.cuda.synchronize()
    assert_same_snapshots(F.snap(), before)
    assert float(marker.sum()) == 4.0 and int(cnt.cpu().numpy()[0]) == 0
