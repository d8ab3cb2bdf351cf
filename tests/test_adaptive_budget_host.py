"""CPU tests of adaptive sample budgets (not gpu): the new calls are declared, exported and bound with the same signatures,
rt_adaptive_priority equals the numpy model bit for bit, rt_adaptive_budget_picks deals q = samples / batch over the rounds, and every
refused rt_render_adaptive_spend / rt_adaptive_budget_select call returns before any device work — a world created on the host and
placeholder device pointers are enough."""
import ctypes as C

import numpy as np
import pytest

import abi_header
import adaptive_budget_model as M

FAKE = C.c_void_p(0x1000)          # never dereferenced: the calls below refuse before they touch a buffer
NX, NY = 64, 40                    # 8 x 5 = 40 tiles
WHOLE = (0, 1, 0, 0)
INT_CALLS = ("rt_adaptive_budget_check", "rt_adaptive_budget_picks", "rt_adaptive_budget_select", "rt_render_adaptive_spend",
             "rt_render_adaptive_spend_on")
I64MAX = 2 ** 63 - 1


def budget(rt, **kw):
    p = dict(samples=4096, rounds=2, batch=4, max_spp=64, floor=0.01)
    p.update(kw)
    return rt.Budget(**p)


def spend(rt, world, p, part=WHOLE, on=False, state=FAKE, ctx=FAKE):
    L = rt.lib()
    ptr = C.byref(p) if p is not None else None
    if on:
        return L.rt_render_adaptive_spend_on(ctx, FAKE, NX, NY, ptr, world.h, FAKE, None, None, state, rt.Partition(*part), None, None)
    return L.rt_render_adaptive_spend(FAKE, NX, NY, ptr, world.h, FAKE, None, None, state, rt.Partition(*part), None, None)


def select(rt, p, picks=10, part=WHOLE, ctx=FAKE, state=FAKE, lst=FAKE, cnt=FAKE, nx=NX, ny=NY):
    ptr = C.byref(p) if p is not None else None
    return rt.lib().rt_adaptive_budget_select(ctx, state, nx, ny, rt.Partition(*part), ptr, picks, lst, cnt, None)


@pytest.fixture(scope="module")
def world(rt):
    W = rt.World(500, NX, NY)
    yield W
    W.close()


@pytest.fixture(scope="module")
def w16(rt):
    W = rt.World(500, NX, NY, precision=rt.FP16)
    yield W
    W.close()


def test_header_and_binding_agree(rt):
    abi_header.check_bound(rt, INT_CALLS + ("rt_adaptive_priority",))
    assert all(abi_header.PROTOTYPES[name][0] is C.c_int for name in INT_CALLS) and abi_header.PROTOTYPES["rt_adaptive_priority"][0] is C.c_float
    abi_header.check_struct(rt.Budget, "rt_budget")           # rt_budget as the header lays it out
    assert C.sizeof(rt.Budget) == 24
    assert abi_header.DEFINES["RT_ABI_VERSION"] == 6
    assert rt.lib().rt_abi_version() == 6
    for name in ("Budget", "adaptive_priority", "adaptive_budget_check", "adaptive_budget_picks", "adaptive_budget_select",
                 "render_adaptive_spend"):
        assert hasattr(rt, name), name
    assert hasattr(rt.RenderCtx, "render_adaptive_spend") and hasattr(rt.RenderCtx, "adaptive_budget_select")


# ---- the priority -------------------------------------------------------------------------------------------------------------
def f32(x):
    return np.float32(x)


def bits(x):
    return int(np.asarray(x, np.float32).view(np.uint32))


NAN, INF = float("nan"), float("inf")
# (SL, Q, k, floor)
EDGE = {
    "equal_samples": (f32(0.3) * f32(8), f32(0.3) * f32(0.3) * f32(8), 8, 0.01),          # d == 0 or a rounding away from it
    "d_negative_by_rounding": (f32(3.3000002), f32(1.21), 9, 0.0),                          # 9 * 1.21 < 3.3000002^2 in binary32
    "zero_sum_zero_floor": (0.0, 0.0, 8, 0.0),                                              # 0 / 0 becomes 0
    "zero_sum_zero_floor_q": (0.0, 1.0, 8, 0.0),                                            # d / 0 = +inf stays
    "zero_sum_floor": (0.0, 0.0, 8, 0.02),
    "zero_sum_floor_q": (0.0, 0.5, 8, 0.02),
    "below_floor": (0.01, 0.002, 8, 0.05),
    "nan_sl": (NAN, 1.0, 8, 0.01),
    "nan_sl_zero_floor": (NAN, 1.0, 8, 0.0),
    "nan_q": (1.0, NAN, 8, 0.01),
    "inf_sl": (INF, 1.0, 8, 0.01),
    "inf_q": (1.0, INF, 8, 0.01),
    "inf_both": (INF, INF, 8, 0.01),
    "overflow_nq": (1.0, 3.0e38, 16, 0.01),
    "overflow_both": (3.0e20, 3.0e38, 16, 0.01),
    "k2": (1.0, 0.9, 2, 0.01),
    "k2_equal": (1.0, 0.5, 2, 0.01),
    "k1": (1.0, 2.0, 1, 0.01),                                                              # n - 1 == 0
    "tiny": (1.0e-30, 1.0e-38, 4, 0.0),                                                     # subnormal products
    "huge_floor": (1.0, 1.0, 4, 3.0e38),
}


@pytest.mark.parametrize("name", list(EDGE))
def test_priority_edge_cases(rt, name):
    SL, Q, k, floor = EDGE[name]
    got = rt.lib().rt_adaptive_priority(C.c_float(SL), C.c_float(Q), k, C.c_float(floor))
    ref = M.priority(f32(SL), f32(Q), k, floor)
    assert bits(got) == bits(ref), (name, got, ref)
    assert not np.isnan(got) and bits(got) < 0x80000000                 # never NaN, never negative (not even -0)


def test_priority_edge_values(rt):
    """what the header promises for the cases above, stated without the model"""
    P = lambda *a: float(rt.adaptive_priority(*a))
    assert P(0.0, 0.0, 8, 0.0) == 0.0 and P(0.0, 1.0, 8, 0.0) == INF
    assert P(NAN, 1.0, 8, 0.01) == 0.0 and P(1.0, NAN, 8, 0.01) == 0.0 and P(INF, INF, 8, 0.01) == 0.0
    assert P(1.0, INF, 8, 0.01) == INF and P(1.0, 3.0e38, 16, 0.01) == INF
    assert P(*EDGE["d_negative_by_rounding"]) == 0.0
    SL, Q, k, fl = EDGE["d_negative_by_rounding"]
    assert f32(k) * f32(Q) - f32(SL) * f32(SL) < 0                       # the case is what its name says
    assert P(1.0, 0.9, 2, 0.01) == float((f32(2) * f32(0.9) - f32(1)) / (f32(1) * f32(1)))


def test_priority_random_triples(rt):
    rng = np.random.default_rng(20240607)
    n = 4000
    k = rng.integers(2, 200, n).astype(np.int32)
    mean = rng.uniform(0.0, 2.0, n).astype(np.float32)
    spread = (rng.uniform(0.0, 1.0, n) ** 3).astype(np.float32)
    SL = (mean * k).astype(np.float32)
    Q = (SL * mean * (np.float32(1) + spread)).astype(np.float32)
    floor = rng.choice(np.array([0.0, 0.01, 0.05, 1.0], np.float32), n)
    L = rt.lib()
    got = np.array([L.rt_adaptive_priority(C.c_float(SL[i]), C.c_float(Q[i]), int(k[i]), C.c_float(floor[i])) for i in range(n)], np.float32)
    ref = np.array([M.priority(SL[i], Q[i], k[i], floor[i]) for i in range(n)], np.float32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert (got > 0).sum() > n // 2 and len(np.unique(got)) > n // 2     # the table is not degenerate


# ---- the parameters -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples,rounds,batch", [(0, 1, 1), (4096, 2, 4), (1000, 3, 7), (10, 4, 3), (5, 8, 1), (12345678901, 7, 5),
                                                  ((2 ** 32 - 1) * 3, 3, 1), ((2 ** 32 - 1) * (2 ** 31 - 1) + 5, 1, 2 ** 31 - 1)])
def test_picks_sum_to_the_budget(rt, samples, rounds, batch):
    p = budget(rt, samples=samples, rounds=rounds, batch=batch)
    assert rt.adaptive_budget_check(p)
    ks = [rt.adaptive_budget_picks(p, r) for r in range(rounds)]
    assert ks == [M.picks(samples, rounds, batch, r) for r in range(rounds)]
    assert sum(ks) == samples // batch and max(ks) - min(ks) <= 1
    k = C.c_int64(-7)
    L = rt.lib()
    assert L.rt_adaptive_budget_picks(C.byref(p), rounds, C.byref(k)) == -1 and L.rt_adaptive_budget_picks(C.byref(p), -1, C.byref(k)) == -1
    assert L.rt_adaptive_budget_picks(C.byref(p), 0, None) == -1 and L.rt_adaptive_budget_picks(None, 0, C.byref(k)) == -1
    assert k.value == -7


BAD = {
    "negative_samples": dict(samples=-1),
    "no_rounds": dict(rounds=0),
    "negative_rounds": dict(rounds=-3),
    "no_batch": dict(batch=0),
    "negative_batch": dict(batch=-4),
    "nan_floor": dict(floor=NAN),
    "negative_floor": dict(floor=-0.01),
    "inf_floor": dict(floor=INF),
    "product_overflows": dict(samples=I64MAX, rounds=2, batch=1),                   # q * rounds
    "product_overflows_far": dict(samples=I64MAX // 2, rounds=2 ** 31 - 1, batch=1),
    "picks_past_32_bits": dict(samples=2 ** 32, rounds=1, batch=1),                 # K_0 = 2^32
    "picks_past_32_bits_rounded_up": dict(samples=2 * (2 ** 32 - 1) + 1, rounds=2, batch=1),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_parameters_are_refused(rt, world, w16, name):
    p = budget(rt, **BAD[name])
    assert not rt.adaptive_budget_check(p)
    k = C.c_int64(0)
    assert rt.lib().rt_adaptive_budget_picks(C.byref(p), 0, C.byref(k)) == -1
    for on in (False, True):
        assert spend(rt, world, p, on=on) == -1
        assert spend(rt, w16, p, on=on) == -1                                        # before the precision is looked at
    assert select(rt, p) == -1


def test_the_largest_accepted_picks(rt):
    p = budget(rt, samples=2 ** 32 - 1, rounds=1, batch=1)
    assert rt.adaptive_budget_check(p) and rt.adaptive_budget_picks(p, 0) == 2 ** 32 - 1
    assert rt.lib().rt_adaptive_budget_check(None) == -1


@pytest.mark.parametrize("on", [False, True])
def test_missing_state_and_arguments_are_refused(rt, world, on):
    p = budget(rt)
    assert spend(rt, world, p, on=on, state=None) == -1
    assert spend(rt, world, None, on=on) == -1
    assert spend(rt, world, p, part=(2, 2, 0, 0), on=on) == -1                       # invalid partition
    assert spend(rt, world, p, part=(0, 2, 30, 41), on=on) == -1                     # a range past the frame's 40 tiles
    if on:
        assert spend(rt, world, p, on=True, ctx=None) == -1


def test_select_refusals(rt):
    p = budget(rt)
    assert select(rt, p, ctx=None) == -1
    assert select(rt, None) == -1
    assert select(rt, p, state=None) == -1 and select(rt, p, lst=None) == -1 and select(rt, p, cnt=None) == -1
    assert select(rt, p, picks=-1) == -1 and select(rt, p, picks=2 ** 32) == -1
    assert select(rt, p, part=(2, 2, 0, 0)) == -1 and select(rt, p, part=(0, 2, 30, 41)) == -1
    assert select(rt, p, nx=0) == -1
    assert select(rt, p, part=(2, 3, 0, 0), nx=8, ny=8, state=None, lst=None, cnt=None) == 0      # a part without tiles


def test_part_without_tiles_is_a_no_op(rt):
    """more parts than tiles: a part that owns none returns 0 before it looks at a buffer (8x8 frame: one tile)"""
    L = rt.lib()
    W = rt.World(22, 8, 8)
    p = budget(rt)
    part = rt.Partition(2, 3)
    assert L.rt_render_adaptive_spend(None, 8, 8, C.byref(p), W.h, None, None, None, None, part, None, None) == 0
    W.close()


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("part", [(0, 1, 0, 0), (0, 3, 0, 0), (1, 2, 20, 40)], ids=["whole", "runs", "range"])
def test_binary16_and_contracted_worlds_are_not_supported(rt, w16, part, on):
    p = budget(rt)
    assert spend(rt, w16, p, part, on) == -4                                         # RT_ENOTSUP, after the parameter checks
    wc = rt.World(500, NX, NY)
    wc.set_arith(rt.ARITH_CONTRACT)
    assert spend(rt, wc, p, part, on) == -4
    wc.close()
