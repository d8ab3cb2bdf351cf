"""rt_adaptive_budget_select / rt_render_adaptive_spend (-m gpu): every comparison is bit equality, no tolerances.

The selection is held to tests/adaptive_budget_model.py (the priority in numpy float32, the set by a plain sort) on states the test
writes — with ties at the threshold that the model side asserts really occur — and on rendered frames.  A spend is checked through
the per-pixel exactness of adaptive sampling: a pixel that has taken k samples holds, in fb, the RNG state and the
state's sums, exactly what begin((k, k, 1, 0, floor)) leaves there on fresh buffers.  Buffers start out as a sentinel: the padding of
edge tiles in a part must keep it."""
import numpy as np
import pytest

import adaptive_budget_model as M
import denoise_var_model
from adaptive_frames import BATCH, check_exact, check_round, FLOOR, Frame, inside_frame, make_state, MAX_SPP, model_pick, Scene, SENTINEL, state_parts
from bitcmp import assert_same_snapshots, raw_bits

pytestmark = pytest.mark.gpu

NX, NY = 203, 77                   # 26 x 10 = 260 tiles: ragged right and top edges
N, SPL = 10000, 32
LOOSE = (4, 64, 4, 0.2, FLOOR)     # (min_spp, max_spp, batch, rel_error, floor): pixels stop at many different counts


@pytest.fixture(scope="module")
def scene(rt, cuda):
    sc = Scene(rt, cuda, N, SPL, NX, NY)
    yield sc
    sc.close()


# ---- 1. the selection on written states -----------------------------------------------------------------------------------------
KEY_K = 8


def three_groups(rng, n, shares=(0.2, 0.5, 0.3)):
    """SL, Q, k of n elements that share three key values (a > b > c), dealt at random so that every block holds all three"""
    g = rng.choice(3, n, p=shares)
    SL = np.full(n, 4.0, np.float32)
    Q = np.array([4.0, 3.0, 2.5], np.float32)[g]            # d = 8 Q - 16 = 16, 8, 4
    return SL, Q, np.full(n, KEY_K, np.int32), g


def cut_in_ties(kb, ok, near):
    """a K close to `near` that cuts between two equal threshold keys"""
    s = np.sort(kb[ok])[::-1]
    for off in range(len(s)):
        for K in (near - off, near + off):
            if 0 < K < len(s) and s[K - 1] == s[K]:
                return K
    raise AssertionError("the case holds no ties")


def build_case(name, n, inside):
    """(SL, Q, k, K, straddles): the state of a case and its K; straddles = the cut must fall between equal keys"""
    rng = np.random.default_rng(sum(map(ord, name)))
    SL, Q, k, g = three_groups(rng, n)
    ok = lambda: M.eligible(SL, Q, k, BATCH, MAX_SPP, FLOOR, inside)
    if name == "three_groups":
        K = int((g[inside] == 0).sum() + (g[inside] == 1).sum() // 2)
    elif name == "inf_keys":
        Q[rng.random(n) < 0.1] = np.inf                      # n Q = inf: key +inf
        e, kb = ok()
        assert (kb[e] == 0x7F800000).sum() > 1000
        K = int((kb[e] == 0x7F800000).sum() // 2)            # the cut falls inside the +inf keys
    elif name == "inf_keys_all_taken":
        Q[rng.random(n) < 0.1] = np.inf
        e, kb = ok()
        K = int((kb[e] == 0x7F800000).sum() + (g[inside & (Q != np.inf)] == 0).sum() // 2)
    elif name == "nan_sums":
        bad = rng.random(n) < 0.15
        SL[bad & (rng.random(n) < 0.5)] = np.nan
        Q[bad & np.isfinite(SL)] = np.nan
        e, kb = ok()
        assert not e[bad].any() and (bad & inside).sum() > 1000
        K = cut_in_ties(kb, e, int(e.sum()) // 2)
    elif name == "all_zero":
        Q[:] = 2.0                                           # 8 * 2 - 16 = 0: key 0 everywhere
        K = 100
    elif name == "at_cap":
        top = rng.random(n) < 0.2
        Q[top] = 8.0                                         # the largest key, but
        k[top] = MAX_SPP - BATCH + 1                         # k + batch > max_spp
        e, kb = ok()
        assert not e[top].any() and (top & inside).sum() > 1000
        K = cut_in_ties(kb, e, int(e.sum()) // 2)
    elif name == "mixed_k":
        k[:] = rng.choice(np.array([2, 4, 8, 16, 60, 61, 64], np.int32), n)
        SL[:] = k * np.float32(0.5)
        Q[:] = SL * rng.choice(np.array([0.5, 0.75, 1.0, 1.5], np.float32), n)
        e, kb = ok()
        K = cut_in_ties(kb, e, int(e.sum()) // 3)
    elif name == "group_boundary":
        K = int((g[inside] <= 1).sum())                      # exactly the two upper groups: the threshold's ties are all taken
    elif name == "K_zero":
        K = 0
    elif name == "K_eligible":
        K = int(ok()[0].sum())
    elif name == "K_above_eligible":
        k[rng.random(n) < 0.3] = MAX_SPP                     # fewer eligible elements than K
        K = int(ok()[0].sum()) + 1000
    elif name == "one":
        K = 1
    else:
        raise AssertionError(name)
    return SL, Q, k, K, name not in ("all_zero", "group_boundary", "K_zero", "K_eligible", "K_above_eligible")


SELECT_CASES = ["three_groups", "inf_keys", "inf_keys_all_taken", "nan_sums", "all_zero", "at_cap", "mixed_k", "group_boundary", "K_zero",
                "K_eligible", "K_above_eligible", "one"]
SELECT_PARTS = {"whole": (0, 1, 0, 0), "range_lo": (0, 2, 0, 130), "range_hi": (1, 2, 130, 260), "runs": (1, 3, 0, 0)}


def run_select(rt, torch, ctx, name, part):
    P = rt.Partition(*part)
    n = rt.part_pixels(NX, NY, P)
    inside = inside_frame(NX, NY, part, n)
    SL, Q, k, K, straddles = build_case(name, n, inside)
    if not inside.all():
        # the padding would win every round if the selection looked at it: the largest finite key, eligible k
        SL[~inside], Q[~inside], k[~inside] = 4.0, 1.0e30, KEY_K
    chosen, ok, kb = M.select(SL, Q, k, BATCH, MAX_SPP, FLOOR, inside, K)
    assert M.tie_straddles(kb, ok, K) == straddles, name
    if straddles:
        T = kb[chosen].min()
        ties = np.nonzero(ok & (kb == T))[0]
        assert 0 < np.isin(ties, chosen).sum() < len(ties)               # some of the ties are taken, some are not
        assert ties[np.isin(ties, chosen)].max() < ties[~np.isin(ties, chosen)].min()      # the lower ids
    S = np.zeros((n, 3), np.float32)
    state = torch.from_numpy(make_state(S, SL, Q, k).copy()).cuda()
    cap = min(K, n)
    lst = torch.full((cap + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda")
    rt.adaptive_budget_select(ctx, state, NX, NY, rt.Budget(0, 1, BATCH, MAX_SPP, FLOOR), K, lst, cnt, P)
    torch.cuda.synchronize()
    got, c = lst.cpu().numpy().view(np.uint32), int(cnt.cpu().numpy().view(np.uint32)[0])
    assert c == len(chosen) == min(K, int(ok.sum())), (name, c, len(chosen))
    assert np.array_equal(np.sort(got[:c]), chosen), name
    assert (got[c:] == SENTINEL).all()                                   # nothing written past the count
    assert inside[got[:c]].all()
    assert np.array_equal(state.cpu().numpy(), make_state(S, SL, Q, k))  # the state is only read
    return c


@pytest.fixture(scope="module")
def ctx(rt, cuda):
    c = rt.RenderCtx()
    yield c
    c.close()


@pytest.mark.parametrize("name", SELECT_CASES)
def test_selection_on_written_states(rt, cuda, ctx, name):
    c = run_select(rt, cuda, ctx, name, SELECT_PARTS["whole"])
    assert (c == 0) == (name in ("all_zero", "K_zero"))


@pytest.mark.parametrize("part", ["range_lo", "range_hi", "runs"])
@pytest.mark.parametrize("name", ["three_groups", "mixed_k", "K_above_eligible"])
def test_selection_never_lists_padding(rt, cuda, ctx, name, part):
    n = rt.part_pixels(NX, NY, rt.Partition(*SELECT_PARTS[part]))
    assert not inside_frame(NX, NY, SELECT_PARTS[part], n).all()              # ragged: the part has padding
    assert run_select(rt, cuda, ctx, name, SELECT_PARTS[part]) > 0


def test_selection_model_is_what_the_host_export_computes(rt):
    """the model's key is rt_adaptive_priority's, on the values the cases use"""
    for SL, Q, k in ((4.0, 4.0, 8), (4.0, 3.0, 8), (4.0, 2.5, 8), (4.0, np.inf, 8), (np.nan, 3.0, 8), (4.0, 2.0, 8), (4.0, 1.0e30, 8)):
        assert raw_bits(rt.adaptive_priority(SL, Q, k, FLOOR))[()] == raw_bits(M.priority(SL, Q, k, FLOOR))[()]


# ---- 2. one round on a rendered frame ------------------------------------------------------------------------------------------
def one_round(rt, torch, sc, part, ctx=None, stream=None):
    F = Frame(rt, torch, sc.nx, sc.ny, part, ctx, stream).begin(sc.W, sc.O, LOOSE)
    before = F.snap()
    _, ok, _ = model_pick(before, F.n, F.inside, 0)
    K = int(ok.sum()) // 4                                   # never trivial: a quarter of what could be picked
    assert K > 100
    picked = F.spend(sc.W, sc.O, BATCH * K, 1)
    after = F.snap()
    chosen, _ = check_round(sc, F, before, after, picked[0], K)
    assert len(chosen) == K
    return F, before, after


def test_one_round_on_a_rendered_frame(rt, cuda, scene):
    F, before, after = one_round(rt, cuda, scene, rt.WHOLE)
    k0 = state_parts(before["state"], F.n)[3]
    assert len(np.unique(k0)) >= 3                           # the frame the budget continues is not uniform


# ---- 3. rounds compose ------------------------------------------------------------------------------------------------------------
def test_rounds_compose(rt, cuda, scene):
    sc = scene
    A = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(sc.W, sc.O, LOOSE)
    B = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(sc.W, sc.O, LOOSE)
    samples, rounds = BATCH * 5000 + 3, 3                    # q = 5000: 1666, 1667, 1667
    Ks = [M.picks(samples, rounds, BATCH, r) for r in range(rounds)]
    assert sum(Ks) == 5000 and len(set(Ks)) == 2
    picked = A.spend(sc.W, sc.O, samples, rounds)
    singles = []
    for K in Ks:
        before = B.snap()
        p = B.spend(sc.W, sc.O, K * BATCH, 1)
        check_round(sc, B, before, B.snap(), p[0], K)        # the model predicts every single round from the state read back
        singles.append(int(p[0]))
    assert list(picked) == singles == Ks
    assert_same_snapshots(A.snap(), B.snap())


# ---- 4. paths and parts -----------------------------------------------------------------------------------------------------------
PATHS = {
    "list": (500, None, 0, "k_render<false,0,1>"),
    "dense_grid": (100000, 320, 1, "k_render<true,0,2>"),
}


@pytest.mark.parametrize("name", list(PATHS))
def test_other_paths(rt, cuda, name):
    n, spl, trav, kernel = PATHS[name]
    sc = Scene(rt, cuda, n, spl, 131, 71, trav)
    assert rt.render_kernel_name(sc.W, sc.O) == kernel
    one_round(rt, cuda, sc, rt.WHOLE)
    sc.close()


def test_runs_of_three_parts(rt, cuda, scene):
    for p in range(3):
        one_round(rt, cuda, scene, rt.Partition(p, 3))


@pytest.mark.parametrize("band", [0, 1])
def test_range_part_keeps_its_padding(rt, cuda, scene, band):
    starts = [0, 130, 260]
    F, before, after = one_round(rt, cuda, scene, rt.Partition(band, 2, starts[band], starts[band + 1]))
    assert (~F.inside).any()
    init = Frame(rt, cuda, NX, NY, F.part).snap()
    assert np.array_equal(after["st"][~F.inside], init["st"][~F.inside])


def test_context_on_a_side_stream(rt, cuda, scene):
    torch = cuda
    c = rt.RenderCtx()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    F, before, after = one_round(rt, torch, scene, rt.WHOLE, ctx=c, stream=s.cuda_stream)
    assert len(c.times()) == 2                               # begin and the spend
    G, _, ref = one_round(rt, torch, scene, rt.WHOLE)
    assert_same_snapshots(after, ref)
    c.close()


# ---- 5. limits -------------------------------------------------------------------------------------------------------------------
def test_zero_samples_change_nothing(rt, cuda, scene):
    F = Frame(rt, cuda, NX, NY, rt.Partition(1, 3)).begin(scene.W, scene.O, LOOSE)
    before = F.snap()
    picked = F.spend(scene.W, scene.O, 0, 2)
    assert list(picked) == [0, 0]
    assert_same_snapshots(F.snap(), before)
    picked = F.spend(scene.W, scene.O, BATCH - 1, 1)         # less than one batch: q = 0
    assert list(picked) == [0]
    assert_same_snapshots(F.snap(), before)


def test_budget_larger_than_the_frame_can_take(rt, cuda, scene):
    """K_r above the eligible count in every round: every round takes exactly the eligible set, and max_spp is never passed"""
    sc = scene
    cap, rounds = 16, 4
    A = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(sc.W, sc.O, LOOSE)
    B = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(sc.W, sc.O, LOOSE)
    start = B.snap()
    k0 = state_parts(start["state"], B.n)[3].copy()
    K = B.n                                                  # every round may pick the whole frame
    picked = A.spend(sc.W, sc.O, K * BATCH * rounds, rounds, max_spp=cap)
    singles = []
    for r in range(rounds):
        before = B.snap()
        p = B.spend(sc.W, sc.O, K * BATCH, 1, max_spp=cap)
        chosen, ok = check_round(sc, B, before, B.snap(), p[0], K, max_spp=cap)
        assert len(chosen) == int(ok.sum()) < K              # the eligible set, below K_r
        assert np.array_equal(chosen, np.nonzero(ok)[0])
        singles.append(int(p[0]))
    assert list(picked) == singles
    assert singles[0] > singles[-1]                          # pixels became ineligible on the way
    final = A.snap()
    assert_same_snapshots(final, B.snap())
    k1 = state_parts(final["state"], A.n)[3]
    grew = k1 > k0
    assert grew.any() and (k1[grew] <= cap).all() and (k1[~grew] == k0[~grew]).all()
    assert (k0 > cap).any()                                  # pixels beyond the cap existed and were left alone


def test_spend_after_spend(rt, cuda, scene):
    sc = scene
    F = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(sc.W, sc.O, LOOSE)
    for K, batch in ((3000, 4), (2000, 8), (1, 4)):
        before = F.snap()
        p = F.spend(sc.W, sc.O, K * batch, 1, batch=batch, max_spp=128)
        check_round(sc, F, before, F.snap(), p[0], K, batch=batch, max_spp=128)


# ---- 6. with the denoiser -------------------------------------------------------------------------------------------------------
def test_denoiser_accepts_the_state(rt, cuda, scene):
    torch, sc = cuda, scene
    F = Frame(rt, torch, NX, NY, rt.WHOLE).begin(sc.W, sc.O, LOOSE)
    F.spend(sc.W, sc.O, BATCH * 6000, 2)
    d_hits = rt.alloc_guides(NX, NY)
    rt.render_guides(sc.W, sc.O, NX, NY, d_hits)
    torch.cuda.synchronize()
    hits = d_hits.cpu().numpy().view(rt.hit_record_dtype)
    p = rt.denoise_var_params()
    out = torch.full_like(F.fb, 7.0)
    rt.denoise_adaptive(out, F.fb, NX, NY, d_hits, F.state, p, rt.alloc_denoise_work(NX, NY))
    torch.cuda.synchronize()
    ref = denoise_var_model.denoise_adaptive(F.fb.cpu().numpy(), hits, F.state.cpu().numpy(), NX, NY, p.levels, p.normal_pow_log2,
                                             p.prefilter, p.sigma_position, p.sigma_variance)
    got = out.cpu().numpy()
    assert np.array_equal(raw_bits(got), raw_bits(np.asarray(ref, np.float32).reshape(-1)))
    assert not np.array_equal(raw_bits(got), raw_bits(F.fb.cpu().numpy()))


# ---- 7. C3 -----------------------------------------------------------------------------------------------------------------------
def test_c3_spend(rt, cuda):
    nx, ny = 1200, 800
    sc = Scene(rt, cuda, 10000, 32, nx, ny)
    A = Frame(rt, cuda, nx, ny, rt.WHOLE).begin(sc.W, sc.O, (8, 8, 8, 0.0, FLOOR))
    B = Frame(rt, cuda, nx, ny, rt.WHOLE).begin(sc.W, sc.O, (8, 8, 8, 0.0, FLOOR))
    rounds, batch = 4, 8
    samples = batch * (nx * ny // 2) + 5
    picked = A.spend(sc.W, sc.O, samples, rounds, batch=batch)
    Ks = [M.picks(samples, rounds, batch, r) for r in range(rounds)]
    for r, K in enumerate(Ks):
        before = B.snap()
        p = B.spend(sc.W, sc.O, K * batch, 1, batch=batch)
        chosen, ok, kb = model_pick(before, B.n, B.inside, K, batch=batch)
        k0 = state_parts(before["state"], B.n)[3]
        want = k0.copy()
        want[chosen] += batch
        assert int(p[0]) == len(chosen) == int(picked[r])
        assert np.array_equal(B.snap()["spp"], want)
    final = A.snap()
    assert_same_snapshots(final, B.snap())
    check_exact(sc, A, final)
    assert len(np.unique(final["spp"])) >= 3
    sc.close()
