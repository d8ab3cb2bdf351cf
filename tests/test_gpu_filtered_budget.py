"""rt_adaptive_budget_select_filtered / rt_render_adaptive_spend_filtered (-m gpu): every comparison is bit equality except the last
test, which compares three RMSEs.

The key kernel is held to tests/filtered_budget_model.py — level 0 of rt_denoise_adaptive in numpy float32, the key one operation a
line, the set by a plain sort — on states and guides the test writes (ragged against the 16x16 filter tile and the span of the
selection's blocks, with sky, NaN, Inf, k = 1, a clamped d and a zero variance), on a flat patch where the cut falls between equal
keys, on all-sky guides, on tiny frames and on a frame with more tiles than blocks.  A spend is checked as tests/
test_gpu_adaptive_budget.py checks the raw one, with the frames, scenes and per-pixel exactness check of tests/adaptive_frames.py."""
import ctypes as C

import numpy as np
import pytest

import adaptive_budget_model as B
import denoise_var_model as V
import filtered_budget_model as M
from adaptive_frames import BATCH, check_exact, check_round, check_round_filtered, filt_of, FLOOR, Frame, MAX_SPP, model_pick, Scene, SENTINEL
from bitcmp import assert_same_snapshots

pytestmark = pytest.mark.gpu

NX, NY = 203, 77                   # 203 x 77: 13 x 5 filter tiles, ragged on both edges; 15631 pixels = 15 full selection spans and a rest
N, SPL = 10000, 32
LOOSE = (4, 64, 4, 0.1, FLOOR)


def upload_hits(torch, hits):
    return torch.from_numpy(np.ascontiguousarray(hits).view(np.uint8).copy()).cuda()


def gpu_select(rt, torch, ctx, d_state, d_hits, nx, ny, p, K, batch=BATCH, max_spp=MAX_SPP, floor=FLOOR, want_keys=True):
    """one rt_adaptive_budget_select_filtered: (sorted ids, everything behind the count, key bits or None)"""
    n = nx * ny
    cap = min(K, n)
    lst = torch.full((cap + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda")
    keys = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda") if want_keys else None
    rt.adaptive_budget_select_filtered(ctx, d_state, d_hits, nx, ny, rt.Budget(0, 1, batch, max_spp, floor), p, K, lst, cnt, keys)
    torch.cuda.synchronize()
    got, c = lst.cpu().numpy().view(np.uint32), int(cnt.cpu().numpy().view(np.uint32)[0])
    assert (got[c:] == SENTINEL).all()                                   # nothing written past the count
    return np.sort(got[:c]), keys.cpu().numpy().view(np.uint32) if want_keys else None


def check_select(rt, torch, ctx, hits, state, nx, ny, p, Ks=None, d_state=None, d_hits=None):
    """keys and sets of a frame against the model, for K = 0, 1, a middle K and K >= eligible unless Ks says otherwise"""
    d_state = torch.from_numpy(np.ascontiguousarray(state).copy()).cuda() if d_state is None else d_state
    d_hits = upload_hits(torch, hits) if d_hits is None else d_hits
    _, ok, kb = M.select(hits, state, nx, ny, BATCH, MAX_SPP, FLOOR, 0, filt_of(p))
    elig = int(ok.sum())
    for K in (0, 1, max(elig // 3, 1), elig + 5) if Ks is None else Ks:
        chosen = M.pick(ok, kb, K)
        got, keys = gpu_select(rt, torch, ctx, d_state, d_hits, nx, ny, p, K)
        assert np.array_equal(keys, kb), (nx, ny, K, int((keys != kb).sum()))
        assert len(got) == min(K, elig) and np.array_equal(got, chosen), (nx, ny, K)
    assert np.array_equal(d_state.cpu().numpy(), np.ascontiguousarray(state))    # the state is only read
    return ok, kb


@pytest.fixture(scope="module")
def ctx(rt, cuda):
    c = rt.RenderCtx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene(rt, cuda):
    sc = Scene(rt, cuda, N, SPL, NX, NY).with_guides()
    yield sc
    sc.close()


# ---- 1. keys and set on written states and written guides -------------------------------------------------------------------------
FILTERS = {"defaults": {}, "prefilter_0": dict(prefilter=0), "no_normal": dict(normal_pow_log2=-1), "no_position": dict(sigma_position=0.0),
           "no_variance": dict(sigma_variance=0.0)}


@pytest.mark.parametrize("size", [(23, 11), (203, 77)], ids=["23x11", "203x77"])
@pytest.mark.parametrize("name", list(FILTERS))
def test_keys_and_set_on_written_states(rt, cuda, ctx, name, size):
    nx, ny = size
    _, hits, state, special = V.synthetic_state(nx, ny, 7)
    p = rt.denoise_var_params(**FILTERS[name])
    assert p.prefilter == (0 if name == "prefilter_0" else 1)
    ok, kb = check_select(rt, cuda, ctx, hits, state, nx, ny, p)
    k = V.state_parts(state, nx * ny)[3]
    assert 0 < ok.sum() < nx * ny and (kb[k + BATCH > MAX_SPP] > 0).any()        # the mask is not the key
    _, valid = M.frame_keys(hits, state, nx, ny, FLOOR, *filt_of(p))
    for s in ("nan", "k1", "inf"):
        assert not valid[special[s]]
    assert valid[special["neg"]] and valid[special["zero"]] and (~valid).sum() > 3 and len(np.unique(kb)) > nx * ny // 2


def test_levels_beyond_the_first_do_not_enter(rt, cuda, ctx):
    _, hits, state, _ = V.synthetic_state(23, 11, 7)
    check_select(rt, cuda, ctx, hits, state, 23, 11, rt.denoise_var_params(levels=5), Ks=(40,))


# ---- 2. the cut falls between equal keys ------------------------------------------------------------------------------------------
def test_cut_between_equal_keys(rt, cuda, ctx):
    nx, ny = 45, 21
    n = nx * ny
    hits = np.zeros(n, rt.hit_record_dtype)
    hits["sphere"], hits["t"] = 3, 2.0
    hits["normal"] = np.array([0.0, 0.6, 0.8], np.float32)
    hits["p"] = np.arange(3 * n, dtype=np.float32).reshape(n, 3)             # ignored: sigma_position = 0
    S = np.tile(np.array([2.0, 3.0, 1.0], np.float32), (n, 1))
    state = V.make_state(S, np.full(n, 6.0, np.float32), np.full(n, 5.0, np.float32), np.full(n, 8, np.int32))      # d = 8 * 5 - 36 = 4
    p = rt.denoise_var_params(sigma_position=0.0)
    _, ok, kb = M.select(hits, state, nx, ny, BATCH, MAX_SPP, FLOOR, 0, filt_of(p))
    j, i = np.divmod(np.arange(n), nx)
    inner = (i >= 2) & (i < nx - 2) & (j >= 2) & (j < ny - 2)
    assert ok.all() and len(np.unique(kb[inner])) == 1 and (kb[~inner] > kb[inner][0]).all()     # fewer taps at the border: a larger key
    K = int((~inner).sum() + inner.sum() // 2)
    assert B.tie_straddles(kb, ok, K)                                        # before the GPU is asked
    chosen = M.select(hits, state, nx, ny, BATCH, MAX_SPP, FLOOR, K, filt_of(p))[0]
    ties = np.nonzero(inner)[0]
    assert ties[np.isin(ties, chosen)].max() < ties[~np.isin(ties, chosen)].min()                # the lower ids
    check_select(rt, cuda, ctx, hits, state, nx, ny, p, Ks=(K, int((~inner).sum()), int((~inner).sum()) + 1))


# ---- 3. all-sky guides: every pixel is pass-through ------------------------------------------------------------------------------
def test_all_sky_guides_select_what_the_raw_key_selects(rt, cuda, ctx):
    torch = cuda
    _, hits, state, _ = V.synthetic_state(NX, NY, 9)
    hits["sphere"] = -1
    n = NX * NY
    d_state = torch.from_numpy(state.copy()).cuda()
    _, SL, Q, k = V.state_parts(state, n)
    ok, kb = check_select(rt, torch, ctx, hits, state, NX, NY, rt.denoise_var_params(), d_state=d_state)
    assert np.array_equal(kb, B.keybits(B.priority(SL, Q, k, FLOOR)))
    for K in (1, int(ok.sum()) // 2, n):
        lst = torch.full((min(K, n) + 64,), SENTINEL, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        rt.adaptive_budget_select(ctx, d_state, NX, NY, rt.Budget(0, 1, BATCH, MAX_SPP, FLOOR), K, lst, cnt)
        torch.cuda.synchronize()
        c = int(cnt.cpu().numpy()[0])
        raw = np.sort(lst.cpu().numpy().view(np.uint32)[:c])
        got, _ = gpu_select(rt, torch, ctx, d_state, upload_hits(torch, hits), NX, NY, rt.denoise_var_params(), K, want_keys=False)
        assert c == min(K, int(ok.sum())) and np.array_equal(got, raw)


# ---- 4. tiny frames, 5. more tiles than blocks -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 37), (41, 1), (17, 2)])
def test_tiny_frames(rt, cuda, ctx, nx, ny):
    torch = cuda
    W = rt.World(500, nx, ny)
    O = rt.Octree(W, 30)
    F = Frame(rt, torch, nx, ny, rt.WHOLE).begin(W, O, (4, 32, 4, 0.1, FLOOR))
    d_hits = rt.alloc_guides(nx, ny)
    rt.render_guides(W, O, nx, ny, d_hits)
    torch.cuda.synchronize()
    hits = d_hits.cpu().numpy().view(rt.hit_record_dtype)
    for p in (rt.denoise_var_params(), rt.denoise_var_params(prefilter=0, sigma_position=0.0)):
        check_select(rt, torch, ctx, hits, F.state.cpu().numpy(), nx, ny, p, d_state=F.state, d_hits=d_hits)
    O.close()
    W.close()


def test_more_tiles_than_blocks(rt, cuda, ctx):
    nx, ny = 530, 500                                          # 34 x 32 = 1088 tiles of 16 x 16: a block takes two
    assert ((nx + 15) // 16) * ((ny + 15) // 16) > 1024
    _, hits, state, _ = V.synthetic_state(nx, ny, 3)
    ok, _ = check_select(rt, cuda, ctx, hits, state, nx, ny, rt.denoise_var_params(), Ks=(nx * ny // 5,))
    assert ok.sum() > nx * ny // 5


# ---- 6. a rendered frame: rounds compose, every round is the model's, every pixel is exact ------------------------------------------
def rounds_compose(rt, torch, sc, p, ctx=None, stream=None):
    A = Frame(rt, torch, sc.nx, sc.ny, rt.WHOLE, ctx, stream).begin(sc.W, sc.O, LOOSE)
    Bf = Frame(rt, torch, sc.nx, sc.ny, rt.WHOLE).begin(sc.W, sc.O, LOOSE)
    n = A.n
    q = n // 4 + 1
    samples, rounds = BATCH * q + 3, 3                       # three rounds of batch 4
    Ks = [B.picks(samples, rounds, BATCH, r) for r in range(rounds)]
    assert sum(Ks) == q and len(set(Ks)) == 2
    picked = A.spend_filtered(sc, p, samples, rounds)
    singles = []
    for K in Ks:
        before = Bf.snap()
        pk = Bf.spend_filtered(sc, p, K * BATCH, 1)
        check_round_filtered(sc, Bf, before, Bf.snap(), pk[0], K, p)
        singles.append(int(pk[0]))
    assert list(picked) == singles and sum(singles) > q // 2      # (check_round held every count to min(K_r, eligible))
    final = A.snap()
    assert_same_snapshots(final, Bf.snap())
    check_exact(sc, A, final)
    assert len(np.unique(final["spp"])) >= 3
    return A, final


def test_rendered_frame_rounds_compose(rt, cuda, scene):
    p = rt.denoise_var_params()
    A, final = rounds_compose(rt, cuda, scene, p)
    # the filtered key is another ordering than the raw one on this frame: the first round's sets differ
    F = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(scene.W, scene.O, LOOSE)
    snap = F.snap()
    K = F.n // 6
    f_set = M.select(scene.hits, snap["state"], NX, NY, BATCH, MAX_SPP, FLOOR, K, filt_of(p))[0]
    r_set = model_pick(snap, F.n, F.inside, K)[0]
    assert len(f_set) == len(r_set) == K and not np.array_equal(f_set, r_set)


# ---- 7. other paths and mixing ---------------------------------------------------------------------------------------------------
def test_list_path(rt, cuda):
    sc = Scene(rt, cuda, 500, None, 131, 71, 0).with_guides()
    assert rt.render_kernel_name(sc.W, sc.O) == "k_render<false,0,1>"
    rounds_compose(rt, cuda, sc, rt.denoise_var_params())
    sc.close()


def test_context_on_a_side_stream(rt, cuda, scene):
    torch = cuda
    c = rt.RenderCtx()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    A, final = rounds_compose(rt, torch, scene, rt.denoise_var_params(prefilter=0), ctx=c, stream=s.cuda_stream)
    assert len(c.times()) == 2                               # begin and the spend
    c.close()


def test_raw_spend_then_filtered_spend(rt, cuda, scene):
    sc, p = scene, rt.denoise_var_params()
    F = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(sc.W, sc.O, LOOSE)
    before = F.snap()
    pk = F.spend(sc.W, sc.O, 3000 * BATCH, 1)
    mid = F.snap()
    check_round(sc, F, before, mid, pk[0], 3000)
    pk = F.spend_filtered(sc, p, 2500 * BATCH, 1)
    after = F.snap()
    check_round_filtered(sc, F, mid, after, pk[0], 2500, p)
    pk = F.spend(sc.W, sc.O, 1000 * BATCH, 1)                # ... and back
    check_round(sc, F, after, F.snap(), pk[0], 1000)


# ---- 8. errors on the device -----------------------------------------------------------------------------------------------------
def test_binary16_and_contracted_worlds_are_refused(rt, cuda, scene):
    torch = cuda
    F = Frame(rt, torch, NX, NY, rt.WHOLE)
    p, Bd = rt.denoise_var_params(), rt.Budget(4000, 1, BATCH, MAX_SPP, FLOOR)
    w16 = rt.World(N, NX, NY, precision=rt.FP16)
    wc = rt.World(N, NX, NY)
    wc.set_arith(rt.ARITH_CONTRACT)
    before = F.snap()
    for W in (w16, wc):
        with pytest.raises(rt.RtError, match="-4"):
            rt.render_adaptive_spend_filtered(F.fb, NX, NY, Bd, p, scene.d_hits, W, F.st, F.state, None, F.spp)
    assert_same_snapshots(F.snap(), before)
    w16.close()
    wc.close()


def test_refused_during_a_capture(rt, cuda, scene, ctx):
    torch = cuda
    F = Frame(rt, torch, NX, NY, rt.WHOLE).begin(scene.W, scene.O, LOOSE)
    p, Bd = rt.denoise_var_params(), rt.Budget(4000, 1, BATCH, MAX_SPP, FLOOR)
    F.spend_filtered(scene, p, 4000, 1)                      # warm: the workspaces exist, so only the capture can be the reason
    lst = torch.zeros(1064, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    marker = torch.zeros(4, device="cuda")
    before = F.snap()
    L = rt.lib()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        marker.add_(1.0)                                     # (the graph is not empty)
        rc_spend = L.rt_render_adaptive_spend_filtered(F.fb.data_ptr(), NX, NY, C.byref(Bd), C.byref(p), scene.d_hits.data_ptr(), scene.W.h,
                                                       F.st.data_ptr(), scene.O.h, F.spp.data_ptr(), F.state.data_ptr(), None, s)
        rc_select = L.rt_adaptive_budget_select_filtered(ctx.h, F.state.data_ptr(), scene.d_hits.data_ptr(), NX, NY, C.byref(Bd), C.byref(p), 1000,
                                                         lst.data_ptr(), cnt.data_ptr(), None, s)
    assert rc_spend == -1 and rc_select == -1
    g.replay()
    torch.cuda.synchronize()
    assert_same_snapshots(F.snap(), before)
    assert float(marker.sum()) == 4.0 and int(cnt.cpu().numpy()[0]) == 0


# ---- 9. quality on C3 ------------------------------------------------------------------------------------------------------------
def test_c3_filtered_budget_against_uniform(rt, cuda):
    """C3 (1200x800, N = 10 000, SPL 32) at a mean of 32 spp, RMSE against rt_render(1024) after rt_denoise_adaptive with its defaults:
    U = uniform 32 spp, R = begin 8/8 plus rt_render_adaptive_spend (4 rounds of batch 8), F = the same with the filtered spend.
    The bound is the plain inequality F < U (the issue sets no margin); U, R and F are printed."""
    torch = cuda
    nx, ny = 1200, 800
    n = nx * ny
    sc = Scene(rt, torch, 10000, 32, nx, ny).with_guides()
    st, fb = rt.alloc_rand_state(nx, ny), rt.alloc_fb(nx, ny)
    rt.render_init(nx, ny, st)
    rt.render(fb, nx, ny, 1024, sc.W, st, sc.O)
    torch.cuda.synchronize()
    ref = fb.cpu().numpy().reshape(-1, 3).astype(np.float64)
    p = rt.denoise_var_params()
    work = rt.alloc_denoise_work(nx, ny)

    def rmse(F):
        out = torch.zeros_like(F.fb)
        rt.denoise_adaptive(out, F.fb, nx, ny, sc.d_hits, F.state, p, work)
        torch.cuda.synchronize()
        img = out.cpu().numpy().reshape(-1, 3).astype(np.float64)
        m = np.isfinite(ref).all(1) & np.isfinite(img).all(1)
        return float(np.sqrt(np.mean((img[m] - ref[m]) ** 2)))

    U = Frame(rt, torch, nx, ny, rt.WHOLE).begin(sc.W, sc.O, (32, 32, 1, 0.0, FLOOR))
    R = Frame(rt, torch, nx, ny, rt.WHOLE).begin(sc.W, sc.O, (8, 8, 8, 0.0, FLOOR))
    Ff = Frame(rt, torch, nx, ny, rt.WHOLE).begin(sc.W, sc.O, (8, 8, 8, 0.0, FLOOR))
    pr = R.spend(sc.W, sc.O, 24 * n, 4, batch=8, max_spp=1024)
    pf = Ff.spend_filtered(sc, p, 24 * n, 4, batch=8, max_spp=1024)
    kR, kF = R.spp.cpu().numpy(), Ff.spp.cpu().numpy()
    assert int(pr.sum()) * 8 == int(kR.sum()) - 8 * n and int(pf.sum()) * 8 == int(kF.sum()) - 8 * n and not np.array_equal(kR, kF)
    eU, eR, eF = rmse(U), rmse(R), rmse(Ff)
    print("C3, RMSE after rt_denoise_adaptive: U %.5f (32 spp)  R %.5f (mean %.3f, max %d)  F %.5f (mean %.3f, max %d)"
          % (eU, eR, kR.mean(), kR.max(), eF, kF.mean(), kF.max()))
    sc.close()
    assert eF < eU, (eU, eR, eF)
