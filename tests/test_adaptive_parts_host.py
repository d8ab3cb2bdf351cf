"""CPU tests of rt_render_adaptive_part / rt_multi_render_adaptive (not gpu): the new symbols are declared, exported and bound, and
every refused call returns before any device work — a world created on the host and placeholder device pointers are enough.
(A refused root without fb_full needs an rt_multi, which lives on a device: tests/test_gpu_multi_adaptive.py checks it.)"""
import ctypes as C

import pytest

import abi_header

FAKE = C.c_void_p(0x1000)          # never dereferenced: the calls below refuse before they touch a buffer
NX, NY = 64, 40                    # 8 x 5 = 40 tiles
NEW = ("rt_render_adaptive_part", "rt_render_adaptive_part_on", "rt_multi_render_adaptive")


def good(rt, **kw):
    p = dict(min_spp=4, max_spp=32, batch=4, rel_error=0.05, floor=0.01)
    p.update(kw)
    return rt.Adaptive(**p)


def call(rt, world, params, part, on=False, nx=NX, ny=NY):
    L = rt.lib()
    ptr = C.byref(params) if params is not None else None
    if on:
        return L.rt_render_adaptive_part_on(FAKE, FAKE, nx, ny, ptr, world.h, FAKE, None, None, part, None)
    return L.rt_render_adaptive_part(FAKE, nx, ny, ptr, world.h, FAKE, None, None, part, None)


@pytest.fixture(scope="module")
def world(rt):
    W = rt.World(500, NX, NY)
    yield W
    W.close()


def test_new_symbols_are_declared_exported_and_bound(rt):
    abi_header.check_bound(rt, NEW)
    assert all(abi_header.PROTOTYPES[name][0] is C.c_int for name in NEW)
    assert rt.lib().rt_abi_version() == 6


BAD_PARTS = [
    (3, 2, 0, 0),            # part >= nparts
    (-1, 2, 0, 0),
    (0, 0, 0, 0),            # no parts
    (0, 2, 10, 5),           # an empty / reversed range
    (0, 2, 30, 41),          # a range past the frame's 40 tiles
]


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("bad", BAD_PARTS, ids=[str(b) for b in BAD_PARTS])
def test_bad_partitions_are_refused(rt, world, bad, on):
    assert call(rt, world, good(rt), rt.Partition(*bad), on) == -1          # RT_EINVAL


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("bad", [dict(min_spp=1), dict(batch=0), dict(max_spp=30), dict(rel_error=-1.0), dict(floor=float("nan"))],
                         ids=["min_spp", "batch", "max_spp", "rel_error", "floor"])
def test_bad_parameters_are_refused(rt, world, bad, on):
    assert call(rt, world, good(rt, **bad), rt.Partition(0, 2), on) == -1


def test_missing_arguments_are_refused(rt, world):
    L = rt.lib()
    p = good(rt)
    part = rt.Partition(0, 2)
    assert call(rt, world, None, part) == -1                                                                 # NULL params
    assert L.rt_render_adaptive_part(None, NX, NY, C.byref(p), world.h, FAKE, None, None, part, None) == -1    # no fb
    assert L.rt_render_adaptive_part(FAKE, NX, NY, C.byref(p), world.h, None, None, None, part, None) == -1    # no RNG states
    assert L.rt_render_adaptive_part(FAKE, NX, NY, C.byref(p), None, FAKE, None, None, part, None) == -1       # no world
    assert L.rt_render_adaptive_part_on(None, FAKE, NX, NY, C.byref(p), world.h, FAKE, None, None, part, None) == -1   # no context


def test_part_without_tiles_is_a_no_op(rt, world):
    """more parts than tiles: a part that owns none returns 0 before it looks at a buffer (8x8 frame: one tile)"""
    L = rt.lib()
    W = rt.World(22, 8, 8)
    p = good(rt)
    for part in (rt.Partition(1, 3), rt.Partition(2, 3)):
        assert L.rt_render_adaptive_part(None, 8, 8, C.byref(p), W.h, None, None, None, part, None) == 0
    assert L.rt_render_adaptive_part(None, 8, 8, C.byref(p), W.h, None, None, None, rt.Partition(0, 3), None) == -1   # part 0 has pixels
    W.close()


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("part", [(0, 1, 0, 0), (0, 3, 0, 0), (1, 2, 20, 40)], ids=["whole", "runs", "range"])
def test_binary16_and_contracted_worlds_are_not_supported(rt, part, on):
    w16 = rt.World(500, NX, NY, precision=rt.FP16)
    assert call(rt, w16, good(rt), rt.Partition(*part), on) == -4                  # RT_ENOTSUP
    w16.close()
    wc = rt.World(500, NX, NY)
    wc.set_arith(rt.ARITH_CONTRACT)
    assert call(rt, wc, good(rt), rt.Partition(*part), on) == -4
    wc.close()


def test_multi_without_a_handle_is_refused(rt, world):
    L = rt.lib()
    p = good(rt)
    assert L.rt_multi_render_adaptive(None, FAKE, NX, NY, C.byref(p), world.h, None, 0, 0, None, None) == -1
