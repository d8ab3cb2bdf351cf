"""CPU tests of history-aware budgets (not gpu): tests/temporal_budget_model.py passes its self-check; the three new calls are declared,
exported and bound with the same signatures and the ABI version has not moved; every refused rt_adaptive_budget_select_temporal /
rt_render_adaptive_spend_temporal call returns before any device work — worlds created on the host and placeholder device pointers
are enough, and every case below holds at least one fault, so nothing here starts the HIP runtime; and the fabricated left / right
case on the model alone: a history of 32 effective samples in the left half, none in the right half, and K = the size of the right
half selects exactly the right half."""
import ctypes as C

import numpy as np
import pytest

import abi_header
import adaptive_budget_model as B
import temporal_budget_model as M
import temporal_model as tm

FAKE = 0x1000                      # 16-byte aligned, never dereferenced: the calls below refuse before they touch a buffer
ODD = 0x1008                       # not 16-byte aligned
NX, NY = 64, 40
EINVAL, ENOTSUP = -1, -4
NEW_CALLS = ("rt_adaptive_budget_select_temporal", "rt_render_adaptive_spend_temporal", "rt_render_adaptive_spend_temporal_on")
NAN, INF = float("nan"), float("inf")


def budget(rt, **kw):
    p = dict(samples=4096, rounds=2, batch=4, max_spp=64, floor=0.01)
    p.update(kw)
    return rt.Budget(**p)


def inputs(rt, hist=FAKE, hits=FAKE, prev=FAKE, cam=FAKE):
    """a TemporalInputs of placeholder pointers (the camera too: a refused call never reads it)"""
    return rt.TemporalInputs(hist, hits, prev, cam)


def _p(x):
    return C.byref(x) if x is not None else None


def select(rt, world, p, t, tin, picks=10, ctx=FAKE, state=FAKE, lst=FAKE, cnt=FAKE, keys=None, nx=NX, ny=NY):
    return rt.lib().rt_adaptive_budget_select_temporal(ctx, state, world.h if world is not None else None, nx, ny, _p(p), _p(tin), _p(t), picks,
                                                       lst, cnt, keys, None)


def spend(rt, world, p, t, tin, on=False, ctx=FAKE, fb=FAKE, rs=FAKE, state=FAKE, nx=NX, ny=NY):
    L = rt.lib()
    w = world.h if world is not None else None
    if on:
        return L.rt_render_adaptive_spend_temporal_on(ctx, fb, nx, ny, _p(p), _p(tin), _p(t), w, rs, None, None, state, None, None)
    return L.rt_render_adaptive_spend_temporal(fb, nx, ny, _p(p), _p(tin), _p(t), w, rs, None, None, state, None, None)


@pytest.fixture(scope="module")
def world(rt):
    W = rt.World(500, NX, NY)
    yield W
    W.close()


def test_model_self_check():
    M.self_check()


# ---- header, library and binding ----------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree(rt):
    abi_header.check_bound(rt, NEW_CALLS)
    assert all(abi_header.PROTOTYPES[name][0] is C.c_int for name in NEW_CALLS)
    abi_header.check_struct(rt.TemporalInputs, "rt_temporal_inputs")
    assert [f[0] for f in rt.TemporalInputs._fields_] == ["d_hist_in", "d_hits", "d_hits_prev", "cam_prev"]
    assert C.sizeof(rt.TemporalInputs) == 4 * C.sizeof(C.c_void_p)
    for name in ("adaptive_budget_select_temporal", "render_adaptive_spend_temporal", "temporal_inputs"):
        assert hasattr(rt, name), name
    assert hasattr(rt.RenderCtx, "render_adaptive_spend_temporal") and hasattr(rt.RenderCtx, "adaptive_budget_select_temporal")


def test_abi_version_is_still_6(rt):
    assert abi_header.DEFINES["RT_ABI_VERSION"] == 6
    assert rt.lib().rt_abi_version() == 6


def test_temporal_inputs_helper(rt):
    cam = np.zeros(1, rt.camera_dtype)
    cam["origin"] = (1, 2, 3)
    t = rt.temporal_inputs(FAKE, 0x2000, 0x3000, cam)
    assert (t.d_hits, t.d_hist_in, t.d_hits_prev) == (FAKE, 0x2000, 0x3000)
    got = np.ctypeslib.as_array(C.cast(t.cam_prev, C.POINTER(C.c_float)), shape=(3,))
    assert list(got) == [1, 2, 3]
    cam["origin"] = 0                                                  # the record holds a copy of its own
    assert list(got) == [1, 2, 3]
    first = rt.temporal_inputs(FAKE)
    assert first.d_hist_in is None and first.d_hits_prev is None and first.cam_prev is None


# ---- refusals ----------------------------------------------------------------------------------------------------------------
BAD_BUDGET = [dict(samples=-1), dict(rounds=0), dict(batch=0), dict(floor=NAN), dict(floor=-0.01), dict(samples=2 ** 32, rounds=1, batch=1)]
BAD_TEMPORAL = [dict(max_history=-1), dict(reuse_specular=2), dict(reuse_specular=-1), dict(position_tolerance=0.0), dict(position_tolerance=-1.0),
                dict(position_tolerance=NAN), dict(position_tolerance=INF), dict(position_tolerance=1e30), dict(normal_min_dot=1.5),
                dict(normal_min_dot=-1.5), dict(normal_min_dot=NAN)]
BAD_INPUTS = [dict(hits=None), dict(hits=ODD), dict(hist=ODD), dict(prev=None), dict(prev=ODD), dict(cam=None), dict(prev=None, cam=None)]


def test_select_refusals(rt, world):
    p, t, tin = budget(rt), rt.temporal_params(), inputs(rt)
    assert select(rt, world, p, t, tin, ctx=None) == EINVAL and select(rt, None, p, t, tin) == EINVAL
    assert select(rt, world, p, t, tin, state=None) == EINVAL and select(rt, world, p, t, tin, lst=None) == EINVAL
    assert select(rt, world, p, t, tin, cnt=None) == EINVAL
    assert select(rt, world, None, t, tin) == EINVAL and select(rt, world, p, None, tin) == EINVAL and select(rt, world, p, t, None) == EINVAL
    assert select(rt, world, p, t, tin, picks=-1) == EINVAL and select(rt, world, p, t, tin, picks=2 ** 32) == EINVAL
    assert select(rt, world, p, t, tin, nx=0) == EINVAL and select(rt, world, p, t, tin, ny=-3) == EINVAL
    assert select(rt, world, p, t, tin, nx=32768, ny=32769) == EINVAL             # above RT_DENOISE_MAX_PIXELS
    for bad in BAD_BUDGET:
        assert select(rt, world, budget(rt, **bad), t, tin) == EINVAL, bad
    for bad in BAD_TEMPORAL:
        assert not rt.temporal_check(NX, NY, rt.temporal_params(**bad)), bad
        assert select(rt, world, p, rt.temporal_params(**bad), tin) == EINVAL, bad
    for bad in BAD_INPUTS:
        assert select(rt, world, p, t, inputs(rt, **bad)) == EINVAL, bad
    # a first frame needs neither the last frame's guides nor its camera: only the other fault is refused
    assert select(rt, world, p, t, inputs(rt, hist=None, prev=None, cam=None), state=None) == EINVAL


@pytest.mark.parametrize("on", [False, True])
def test_spend_refusals(rt, world, on):
    p, t, tin = budget(rt), rt.temporal_params(), inputs(rt)
    assert spend(rt, None, p, t, tin, on) == EINVAL
    assert spend(rt, world, p, t, tin, on, state=None) == EINVAL and spend(rt, world, p, t, tin, on, fb=None) == EINVAL
    assert spend(rt, world, p, t, tin, on, rs=None) == EINVAL
    assert spend(rt, world, None, t, tin, on) == EINVAL and spend(rt, world, p, None, tin, on) == EINVAL and spend(rt, world, p, t, None, on) == EINVAL
    assert spend(rt, world, p, t, tin, on, nx=0) == EINVAL and spend(rt, world, p, t, tin, on, nx=32768, ny=32769) == EINVAL
    for bad in BAD_BUDGET:
        assert spend(rt, world, budget(rt, **bad), t, tin, on) == EINVAL, bad
    for bad in BAD_TEMPORAL:
        assert spend(rt, world, p, rt.temporal_params(**bad), tin, on) == EINVAL, bad
    for bad in BAD_INPUTS:
        assert spend(rt, world, p, t, inputs(rt, **bad), on) == EINVAL, bad
    if on:
        assert spend(rt, world, p, t, tin, True, ctx=None) == EINVAL


def test_binary16_and_contracted_worlds_are_not_supported(rt):
    p, t, tin = budget(rt), rt.temporal_params(), inputs(rt)
    w16 = rt.World(500, NX, NY, precision=rt.FP16)
    wc = rt.World(500, NX, NY)
    wc.set_arith(rt.ARITH_CONTRACT)
    for on in (False, True):
        assert spend(rt, w16, p, t, tin, on) == ENOTSUP and spend(rt, wc, p, t, tin, on) == ENOTSUP          # after the parameter checks ...
        for W in (w16, wc):                                                                                  # ... which come first
            assert spend(rt, W, p, rt.temporal_params(max_history=-1), tin, on) == EINVAL
            assert spend(rt, W, p, t, inputs(rt, hits=ODD), on) == EINVAL and spend(rt, W, p, t, inputs(rt, cam=None), on) == EINVAL
            assert spend(rt, W, p, t, tin, on, state=None) == EINVAL
    # the selection renders nothing: binary16 alone is refused (kind[] is read from an fp32 world's upload)
    assert select(rt, w16, p, t, tin) == ENOTSUP
    assert select(rt, w16, p, t, inputs(rt, prev=ODD)) == EINVAL and select(rt, w16, p, t, tin, picks=-1) == EINVAL
    assert select(rt, wc, p, t, tin, state=None) == EINVAL
    w16.close()
    wc.close()


# ---- the fabricated left / right case, on the model alone ---------------------------------------------------------------------------
def test_left_right_case_selects_the_half_without_history():
    """one lambertian sphere, a static camera, one (S, SL, Q, k) with v_c > 0 everywhere; the last frame's history holds neff = 32 and
    v = v_c in the left half and neff = 0 in the right half.  A left pixel merges at a = n / (32 + n) < 1, so its v is
    ((1 - a)^2 + a^2) v_c < v_c at the same colour: every key of the right half is strictly above every key of the left half (the
    columns next to the seam left out of the claim), and K = the size of the right half selects exactly it."""
    c = M.left_right_case()
    nx, ny, n = c["nx"], c["ny"], c["nx"] * c["ny"]
    assert c["vc"] > 0 and c["left"].sum() == c["right"].sum() == n // 2 and c["seam"].sum() == 2 * ny
    for floor in (0.02, 0.0, 5.0):                                   # the mean above the floor, no floor, the floor divides
        counts = {}
        key, valid, hist = M.frame_keys(c["hist"], c["hits"], c["prev"], c["cam"], c["state"], c["kind"], nx, ny, floor, *c["temporal"],
                                        counts=counts)
        xv, neff = tm.history_parts(hist, n)
        k = tm.state_parts(c["state"], n)[3]
        assert valid.all() and counts["took"] == n // 2 and np.array_equal(counts["took_mask"], c["left"])
        assert np.array_equal(neff, np.where(c["left"], np.float32(32 + k[0]), np.float32(k[0])))
        a = np.float32(k[0]) / (np.float32(32) + np.float32(k[0]))
        assert a < 1 and (xv[c["left"], 3] < c["vc"]).all() and (xv[c["right"], 3] == c["vc"]).all()
        claim_l, claim_r = c["left"] & ~c["seam"], c["right"] & ~c["seam"]
        assert claim_l.sum() == claim_r.sum() == n // 2 - ny > 0
        assert key[claim_r].min() > key[claim_l].max() > 0
        K = int(c["right"].sum())
        chosen, ok, kb = M.select(c["hist"], c["hits"], c["prev"], c["cam"], c["state"], c["kind"], nx, ny, 4, 64, floor, K, c["temporal"])
        assert ok.all() and np.array_equal(chosen, np.nonzero(c["right"])[0])
        assert not B.tie_straddles(kb, ok, K)
    # without the history, or with nothing taken from it, both halves rank alike: the selection falls back on the pixel ids
    for hist, temporal in ((None, c["temporal"]), (c["hist"], (0,) + c["temporal"][1:])):
        chosen, ok, kb = M.select(hist, c["hits"], c["prev"] if hist is not None else None, c["cam"] if hist is not None else None, c["state"],
                                  c["kind"], nx, ny, 4, 64, 0.02, n // 2, temporal)
        assert len(np.unique(kb)) == 1 and np.array_equal(chosen, np.arange(n // 2))
