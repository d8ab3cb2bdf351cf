"""CPU tests of rt_render_adaptive_begin / rt_render_adaptive_refine (not gpu): the four calls are declared, exported and bound with
the same signatures, and every refused call returns before any device work — a world created on the host and placeholder device
pointers are enough.  A binary16 world answers RT_ENOTSUP only after the parameter checks, so it shows which pairs the rule accepts."""
import ctypes as C

import pytest

import abi_header

FAKE = C.c_void_p(0x1000)          # never dereferenced: the calls below refuse before they touch a buffer
NX, NY = 64, 40                    # 8 x 5 = 40 tiles
NEW = ("rt_render_adaptive_begin", "rt_render_adaptive_begin_on", "rt_render_adaptive_refine", "rt_render_adaptive_refine_on")
WHOLE = (0, 1, 0, 0)


def params(rt, **kw):
    p = dict(min_spp=4, max_spp=32, batch=4, rel_error=0.2, floor=0.01)
    p.update(kw)
    return rt.Adaptive(**p)


def begin(rt, world, p, part=WHOLE, on=False, state=FAKE):
    L = rt.lib()
    ptr = C.byref(p) if p is not None else None
    if on:
        return L.rt_render_adaptive_begin_on(FAKE, FAKE, NX, NY, ptr, world.h, FAKE, None, None, state, rt.Partition(*part), None)
    return L.rt_render_adaptive_begin(FAKE, NX, NY, ptr, world.h, FAKE, None, None, state, rt.Partition(*part), None)


def refine(rt, world, frm, to, part=WHOLE, on=False, state=FAKE):
    L = rt.lib()
    a = C.byref(frm) if frm is not None else None
    b = C.byref(to) if to is not None else None
    if on:
        return L.rt_render_adaptive_refine_on(FAKE, FAKE, NX, NY, a, b, world.h, FAKE, None, None, state, rt.Partition(*part), None)
    return L.rt_render_adaptive_refine(FAKE, NX, NY, a, b, world.h, FAKE, None, None, state, rt.Partition(*part), None)


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
    abi_header.check_bound(rt, NEW)
    assert all(abi_header.PROTOTYPES[name][0] is C.c_int for name in NEW)
    assert abi_header.DEFINES["RT_ADAPTIVE_STATE_BYTES"] == 24
    assert rt.ADAPTIVE_STATE_BYTES == 24
    assert rt.lib().rt_abi_version() == 6


# (from, to) pairs the rule refuses: to.rel raised, a zero target followed by a positive one, min_spp or batch changed, max_spp
# lowered, floor raised, from.rel^2 * (max_spp - 1) overflowing (with t finite, and with t itself inf), and an underflowing rel^2
# (t == 0) followed by a lower floor, where 0 * inf = NaN on the `from` side would let the lower floor stop a pixel `from` kept going
BAD = {
    "rel_raised": (dict(), dict(rel_error=0.3)),
    "rel_from_zero": (dict(rel_error=0.0), dict(rel_error=0.1)),
    "min_spp_changed": (dict(), dict(min_spp=8, max_spp=32)),
    "batch_changed": (dict(), dict(batch=2)),
    "max_spp_lowered": (dict(), dict(max_spp=28)),
    "floor_raised": (dict(), dict(floor=0.02)),
    "rel_overflow_tn": (dict(rel_error=1.0e19), dict(rel_error=0.1)),
    "rel_overflow_t": (dict(rel_error=1.0e20), dict(rel_error=0.1)),
    "rel_underflow_floor_lowered": (dict(rel_error=1.0e-30, floor=1.0e20), dict(rel_error=1.0e-30, floor=0.0)),
    "from_invalid": (dict(batch=0), dict(batch=0)),
    "to_invalid": (dict(), dict(rel_error=float("nan"))),
}


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("name", list(BAD))
def test_pairs_that_do_not_refine_are_refused(rt, world, w16, name, on):
    frm, to = BAD[name]
    assert refine(rt, world, params(rt, **frm), params(rt, **to), on=on) == -1           # RT_EINVAL
    assert refine(rt, w16, params(rt, **frm), params(rt, **to), on=on) == -1            # before the precision is looked at


GOOD = {
    "same": (dict(), dict()),
    "tighter": (dict(rel_error=0.2), dict(rel_error=0.1)),
    "longer": (dict(max_spp=32), dict(max_spp=128)),
    "to_zero": (dict(), dict(rel_error=0.0, max_spp=64)),
    "zero_to_zero": (dict(rel_error=0.0), dict(rel_error=0.0, max_spp=64)),
    "floor_lowered": (dict(floor=0.05), dict(floor=0.0)),
    "rel_underflow_same_floor": (dict(rel_error=1.0e-30, floor=1.0e20), dict(rel_error=1.0e-31, floor=1.0e20)),
    "rel_underflow_to_zero": (dict(rel_error=1.0e-30, floor=1.0e20), dict(rel_error=0.0, floor=0.0)),
}


@pytest.mark.parametrize("name", list(GOOD))
def test_pairs_that_refine_pass_the_checks(rt, w16, name):
    """a binary16 world answers RT_ENOTSUP, not RT_EINVAL: the pair passed the rule"""
    frm, to = GOOD[name]
    assert refine(rt, w16, params(rt, **frm), params(rt, **to)) == -4


@pytest.mark.parametrize("on", [False, True])
def test_missing_state_and_arguments_are_refused(rt, world, on):
    p, q = params(rt), params(rt, rel_error=0.1)
    assert begin(rt, world, p, on=on, state=None) == -1
    assert refine(rt, world, p, q, on=on, state=None) == -1
    assert begin(rt, world, None, on=on) == -1
    assert refine(rt, world, None, q, on=on) == -1
    assert refine(rt, world, p, None, on=on) == -1
    assert begin(rt, world, p, part=(2, 2, 0, 0), on=on) == -1                       # invalid partition
    assert refine(rt, world, p, q, part=(0, 2, 30, 41), on=on) == -1                 # a range past the frame's 40 tiles
    L = rt.lib()
    assert L.rt_render_adaptive_begin_on(None, FAKE, NX, NY, C.byref(p), world.h, FAKE, None, None, FAKE, rt.Partition(*WHOLE), None) == -1
    assert L.rt_render_adaptive_refine_on(None, FAKE, NX, NY, C.byref(p), C.byref(q), world.h, FAKE, None, None, FAKE,
                                          rt.Partition(*WHOLE), None) == -1


def test_part_without_tiles_is_a_no_op(rt):
    """more parts than tiles: a part that owns none returns 0 before it looks at a buffer (8x8 frame: one tile)"""
    L = rt.lib()
    W = rt.World(22, 8, 8)
    p, q = params(rt), params(rt, rel_error=0.1)
    part = rt.Partition(2, 3)
    assert L.rt_render_adaptive_begin(None, 8, 8, C.byref(p), W.h, None, None, None, None, part, None) == 0
    assert L.rt_render_adaptive_refine(None, 8, 8, C.byref(p), C.byref(q), W.h, None, None, None, None, part, None) == 0
    W.close()


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("part", [(0, 1, 0, 0), (0, 3, 0, 0), (1, 2, 20, 40)], ids=["whole", "runs", "range"])
def test_binary16_and_contracted_worlds_are_not_supported(rt, w16, part, on):
    p, q = params(rt), params(rt, rel_error=0.1)
    assert begin(rt, w16, p, part, on) == -4                                         # RT_ENOTSUP
    assert refine(rt, w16, p, q, part, on) == -4
    wc = rt.World(500, NX, NY)
    wc.set_arith(rt.ARITH_CONTRACT)
    assert begin(rt, wc, p, part, on) == -4
    assert refine(rt, wc, p, q, part, on) == -4
    wc.close()
