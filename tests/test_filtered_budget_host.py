"""CPU tests of filter-aware budgets (not gpu): the new calls are declared, exported and bound with the same signatures, the ABI version
has not moved, tests/filtered_budget_model.py passes its self-check, rt_adaptive_priority_filtered equals the model's key bit for bit,
and every refused rt_adaptive_budget_select_filtered / rt_render_adaptive_spend_filtered call returns before any device work — a world
created on the host and placeholder device pointers are enough."""
import ctypes as C

import numpy as np
import pytest

import abi_header
import filtered_budget_model as M
from bitcmp import f32_bits

FAKE = C.c_void_p(0x1000)          # 16-byte aligned, never dereferenced: the calls below refuse before they touch a buffer
ODD = C.c_void_p(0x1008)           # not 16-byte aligned
NX, NY = 64, 40
EINVAL, ENOTSUP = -1, -4
INT_CALLS = ("rt_adaptive_budget_select_filtered", "rt_render_adaptive_spend_filtered", "rt_render_adaptive_spend_filtered_on")
NAN, INF = float("nan"), float("inf")


def budget(rt, **kw):
    p = dict(samples=4096, rounds=2, batch=4, max_spp=64, floor=0.01)
    p.update(kw)
    return rt.Budget(**p)


def select(rt, p, f, picks=10, ctx=FAKE, state=FAKE, hits=FAKE, lst=FAKE, cnt=FAKE, keys=None, nx=NX, ny=NY):
    return rt.lib().rt_adaptive_budget_select_filtered(ctx, state, hits, nx, ny, C.byref(p) if p is not None else None,
                                                       C.byref(f) if f is not None else None, picks, lst, cnt, keys, None)


def spend(rt, world, p, f, on=False, ctx=FAKE, hits=FAKE, state=FAKE, nx=NX, ny=NY):
    L = rt.lib()
    pp, ff = (C.byref(p) if p is not None else None), (C.byref(f) if f is not None else None)
    if on:
        return L.rt_render_adaptive_spend_filtered_on(ctx, FAKE, nx, ny, pp, ff, hits, world.h, FAKE, None, None, state, None, None)
    return L.rt_render_adaptive_spend_filtered(FAKE, nx, ny, pp, ff, hits, world.h, FAKE, None, None, state, None, None)


@pytest.fixture(scope="module")
def world(rt):
    W = rt.World(500, NX, NY)
    yield W
    W.close()


def test_header_and_binding_agree(rt):
    abi_header.check_bound(rt, INT_CALLS + ("rt_adaptive_priority_filtered",))
    assert all(abi_header.PROTOTYPES[name][0] is C.c_int for name in INT_CALLS)
    assert abi_header.PROTOTYPES["rt_adaptive_priority_filtered"][0] is C.c_float
    for name in ("adaptive_priority_filtered", "adaptive_budget_select_filtered", "render_adaptive_spend_filtered"):
        assert hasattr(rt, name), name
    assert hasattr(rt.RenderCtx, "render_adaptive_spend_filtered") and hasattr(rt.RenderCtx, "adaptive_budget_select_filtered")


def test_abi_version_is_still_6(rt):
    assert abi_header.DEFINES["RT_ABI_VERSION"] == 6
    assert rt.lib().rt_abi_version() == 6


def test_model_self_check():
    M.self_check()


# ---- the key -----------------------------------------------------------------------------------------------------------------
def test_priority_filtered_equals_the_model(rt):
    tiny = float(np.float32(1e-45))                                   # the smallest denormal
    vals = [0.0, -0.0, tiny, 1e-40, 1.1754944e-38, 1e-20, 0.02, 0.3, 1.0, 1.5, 3.0e19, 3.0e38, INF, NAN, -1.0, -INF]
    floors = [0.0, tiny, 1e-20, 0.02, 1.0, 3.0e38]
    l, v, f = (a.reshape(-1).astype(np.float32) for a in np.meshgrid(vals, vals, floors, indexing="ij"))
    assert (f == 0).any() and (l < f).any() and np.isnan(l).any() and np.isnan(v).any() and np.isinf(v).any()
    L = rt.lib()
    got = np.array([L.rt_adaptive_priority_filtered(C.c_float(l[i]), C.c_float(v[i]), C.c_float(f[i])) for i in range(len(l))], np.float32)
    ref = M.priority_filtered(l, v, f)
    assert np.array_equal(f32_bits(got), f32_bits(ref))
    assert not np.isnan(got).any() and (f32_bits(got) < 0x80000000).all()         # never NaN, never negative (not even -0)
    assert np.isinf(got).any() and (got == 0).any() and len(np.unique(got)) > 30       # the table is not degenerate
    # random pairs in the range a frame produces
    rng = np.random.default_rng(20240611)
    l = rng.uniform(0.0, 3.0, 4000).astype(np.float32)
    v = (rng.uniform(0.0, 1.0, 4000) ** 4).astype(np.float32)
    f = rng.choice(np.array([0.0, 0.02, 1.0], np.float32), 4000)
    got = np.array([rt.adaptive_priority_filtered(l[i], v[i], f[i]) for i in range(4000)], np.float32)
    assert np.array_equal(f32_bits(got), f32_bits(M.priority_filtered(l, v, f)))


def test_priority_filtered_edge_values(rt):
    """what the header promises, stated without the model"""
    P = lambda *a: float(rt.adaptive_priority_filtered(*a))
    assert P(0.0, 0.0, 0.0) == 0.0                                    # 0 / 0 becomes 0
    assert P(0.0, 1.0, 0.0) == INF                                    # v / 0 stays +inf
    assert P(NAN, 1.0, 0.5) == 4.0                                    # a NaN l takes the floor
    assert P(NAN, 1.0, 0.0) == INF
    assert P(1.0, NAN, 0.02) == 0.0 and P(INF, INF, 0.02) == 0.0
    assert P(1.0, INF, 0.02) == INF
    assert P(0.01, 0.5, 0.5) == 2.0                                   # l below the floor
    assert P(2.0, 1.0, 0.02) == 0.25 and P(1.0, -1.0, 0.02) == 0.0


# ---- refusals ----------------------------------------------------------------------------------------------------------------
BAD_BUDGET = [dict(samples=-1), dict(rounds=0), dict(batch=0), dict(floor=NAN), dict(floor=-0.01), dict(samples=2 ** 32, rounds=1, batch=1)]
BAD_FILTER = [dict(levels=0), dict(levels=9), dict(normal_pow_log2=-2), dict(normal_pow_log2=11), dict(prefilter=2), dict(sigma_position=-1.0),
              dict(sigma_position=NAN), dict(sigma_position=1e-30), dict(sigma_variance=-1.0), dict(sigma_variance=NAN), dict(sigma_variance=1e30)]


def test_select_refusals(rt):
    p, f = budget(rt), rt.denoise_var_params()
    assert select(rt, p, f, ctx=None) == EINVAL
    assert select(rt, p, f, hits=None) == EINVAL and select(rt, p, f, hits=ODD) == EINVAL
    assert select(rt, p, f, state=None) == EINVAL and select(rt, p, f, lst=None) == EINVAL and select(rt, p, f, cnt=None) == EINVAL
    assert select(rt, None, f) == EINVAL and select(rt, p, None) == EINVAL
    assert select(rt, p, f, picks=-1) == EINVAL and select(rt, p, f, picks=2 ** 32) == EINVAL
    assert select(rt, p, f, nx=0) == EINVAL and select(rt, p, f, ny=-3) == EINVAL
    assert select(rt, p, f, nx=32768, ny=32769) == EINVAL             # above RT_DENOISE_MAX_PIXELS
    for bad in BAD_BUDGET:
        assert select(rt, budget(rt, **bad), f) == EINVAL, bad
    for bad in BAD_FILTER:
        assert not rt.denoise_adaptive_check(NX, NY, rt.denoise_var_params(**bad)), bad
        assert select(rt, p, rt.denoise_var_params(**bad)) == EINVAL, bad


@pytest.mark.parametrize("on", [False, True])
def test_spend_refusals(rt, world, on):
    p, f = budget(rt), rt.denoise_var_params()
    assert spend(rt, world, p, f, on, hits=None) == EINVAL and spend(rt, world, p, f, on, hits=ODD) == EINVAL
    assert spend(rt, world, p, f, on, state=None) == EINVAL
    assert spend(rt, world, None, f, on) == EINVAL and spend(rt, world, p, None, on) == EINVAL
    assert spend(rt, world, p, f, on, nx=32768, ny=32769) == EINVAL
    for bad in BAD_BUDGET:
        assert spend(rt, world, budget(rt, **bad), f, on) == EINVAL, bad
    for bad in BAD_FILTER:
        assert spend(rt, world, p, rt.denoise_var_params(**bad), on) == EINVAL, bad
    if on:
        assert spend(rt, world, p, f, True, ctx=None) == EINVAL


@pytest.mark.parametrize("on", [False, True])
def test_binary16_and_contracted_worlds_are_not_supported(rt, on):
    p, f = budget(rt), rt.denoise_var_params()
    w16 = rt.World(500, NX, NY, precision=rt.FP16)
    assert spend(rt, w16, p, f, on) == ENOTSUP                         # after the parameter checks ...
    assert spend(rt, w16, p, rt.denoise_var_params(levels=0), on) == EINVAL and spend(rt, w16, p, f, on, hits=ODD) == EINVAL      # ... which come first
    w16.close()
    wc = rt.World(500, NX, NY)
    wc.set_arith(rt.ARITH_CONTRACT)
    assert spend(rt, wc, p, f, on) == ENOTSUP
    wc.close()
