"""CPU tests of rt_render_adaptive's argument checks (not gpu): every refused call returns before any device work, so a world
created on the host and placeholder device pointers are enough.  The binding's rt_adaptive and the header's agree."""
import ctypes as C

import pytest

import abi_header

FAKE = C.c_void_p(0x1000)          # never dereferenced: the calls below refuse before they touch a buffer
NX, NY = 64, 40


def good(rt, **kw):
    p = dict(min_spp=4, max_spp=32, batch=4, rel_error=0.05, floor=0.01)
    p.update(kw)
    return rt.Adaptive(**p)


def call(rt, world, params, on=False):
    L = rt.lib()
    ptr = C.byref(params) if params is not None else None
    if on:      # (a context is created on a device; the handle, too, is never dereferenced before these refusals)
        return L.rt_render_adaptive_on(FAKE, FAKE, NX, NY, ptr, world.h, FAKE, None, None, None)
    return L.rt_render_adaptive(FAKE, NX, NY, ptr, world.h, FAKE, None, None, None)


@pytest.fixture(scope="module")
def world(rt):
    return rt.World(500, NX, NY)


BAD = [
    dict(min_spp=1, max_spp=5, batch=4),           # min_spp < 2
    dict(min_spp=0, max_spp=4, batch=4),
    dict(batch=0),                                 # batch < 1
    dict(batch=-4),
    dict(min_spp=8, max_spp=4),                    # max < min
    dict(min_spp=4, max_spp=30, batch=4),          # (max - min) % batch != 0
    dict(rel_error=-0.01),                         # negative rel_error
    dict(floor=-1.0),                              # negative floor
    dict(rel_error=float("nan")),
    dict(floor=float("nan")),
]


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("bad", BAD, ids=[",".join("%s=%s" % kv for kv in b.items()) for b in BAD])
def test_bad_parameters_are_refused(rt, world, bad, on):
    assert call(rt, world, good(rt, **bad), on) == -1          # RT_EINVAL


def test_missing_arguments_are_refused(rt, world):
    L = rt.lib()
    p = good(rt)
    assert call(rt, world, None) == -1                         # NULL params
    assert L.rt_render_adaptive(None, NX, NY, C.byref(p), world.h, FAKE, None, None, None) == -1          # no fb
    assert L.rt_render_adaptive(FAKE, NX, NY, C.byref(p), world.h, None, None, None, None) == -1          # no RNG states
    assert L.rt_render_adaptive(FAKE, NX, NY, C.byref(p), None, FAKE, None, None, None) == -1             # no world
    assert L.rt_render_adaptive(FAKE, 0, NY, C.byref(p), world.h, FAKE, None, None, None) == -1           # empty frame
    assert L.rt_render_adaptive_on(None, FAKE, NX, NY, C.byref(p), world.h, FAKE, None, None, None) == -1  # no context


def test_edge_parameters_pass_the_checks(rt, world):
    """min == max (round 0 only), batch 1, rel_error 0 and floor 0 are valid: a binary16 world then answers RT_ENOTSUP, not RT_EINVAL"""
    w16 = rt.World(500, NX, NY, precision=rt.FP16)
    for kw in (dict(min_spp=2, max_spp=2, batch=1), dict(min_spp=2, max_spp=3, batch=1), dict(rel_error=0.0, floor=0.0)):
        assert call(rt, w16, good(rt, **kw)) == -4
    w16.close()


@pytest.mark.parametrize("on", [False, True])
def test_binary16_world_is_not_supported(rt, on):
    w16 = rt.World(500, NX, NY, precision=rt.FP16)
    assert call(rt, w16, good(rt), on) == -4                   # RT_ENOTSUP
    w16.close()


def test_binding_and_header_agree(rt):
    abi_header.check_struct(rt.Adaptive, "rt_adaptive")
    assert C.sizeof(rt.Adaptive) == 20
    abi_header.check_bound(rt, ("rt_render_adaptive", "rt_render_adaptive_on"))
    assert abi_header.PROTOTYPES["rt_render_adaptive"][0] is abi_header.PROTOTYPES["rt_render_adaptive_on"][0] is C.c_int
    assert rt.lib().rt_abi_version() == 6
