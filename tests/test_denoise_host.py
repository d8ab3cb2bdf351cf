"""CPU tests of rt_render_guides / rt_denoise (not gpu): both are declared, exported and bound with the same signatures, and every
refused call returns its code before any device work — placeholder device pointers are enough.  A binary16 world answers
RT_ENOTSUP from rt_render_guides only after the argument checks, which pins the frame-size limit of the guides; rt_denoise_check
(the host-only size and parameter checks that rt_denoise runs) pins the filter's limit and shows which parameters are accepted."""
import ctypes as C

import pytest

import abi_header

FAKE = C.c_void_p(0x1000)          # never dereferenced: the calls below refuse before they touch a buffer
NX, NY = 64, 40
EINVAL, ENOTSUP = -1, -4


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
    names = {"rt_render_guides": ["world", "d_octree", "max_x", "max_y", "d_hits", "stream"],
             "rt_denoise": ["fb_out", "fb_in", "max_x", "max_y", "d_hits", "params", "d_work", "stream"],
             "rt_denoise_check": ["max_x", "max_y", "params"]}
    abi_header.check_bound(rt, names)
    for name in names:
        assert abi_header.PARAM_NAMES[name] == names[name] and abi_header.PROTOTYPES[name][0] is C.c_int, name
    # the struct as the header defines it (its constants and defaults: tests/test_host_and_abi.py::test_constants_equal_the_header)
    abi_header.check_struct(rt.DenoiseParams, "rt_denoise_params")


def guides(rt, world, octree=None, nx=NX, ny=NY, hits=FAKE):
    return rt.lib().rt_render_guides(world.h if world is not None else None, octree, nx, ny, hits, None)


def test_guides_refuse_bad_arguments(rt, world):
    assert guides(rt, None) == EINVAL
    assert guides(rt, world, hits=None) == EINVAL
    for nx, ny in ((0, NY), (NX, 0), (-1, NY), (NX, -5), (1 << 16, 1 << 15)):     # the last: 2^31 pixels
        assert guides(rt, world, nx=nx, ny=ny) == EINVAL, (nx, ny)


def test_guides_refuse_a_tree_of_the_other_precision(rt, world, w16):
    O16 = rt.Octree(w16, 30)                                      # a host-built tree: nothing is uploaded
    O32 = rt.Octree(world, 30)
    assert guides(rt, world, O16.h) == EINVAL
    assert guides(rt, w16, O32.h) == EINVAL
    O16.close()
    O32.close()


def test_guides_of_a_binary16_world_are_not_supported_after_the_checks(rt, w16):
    assert guides(rt, w16, hits=None) == EINVAL
    assert guides(rt, w16, nx=0) == EINVAL
    assert guides(rt, w16) == ENOTSUP
    O16 = rt.Octree(w16, 30)
    assert guides(rt, w16, O16.h) == ENOTSUP
    O16.close()


def test_guides_frame_limit(rt, w16):
    """frames of exactly DENOISE_MAX_PIXELS pixels pass the size check (a binary16 world then answers RT_ENOTSUP), one pixel more does not"""
    lim = rt.DENOISE_MAX_PIXELS
    for nx, ny in ((1 << 15, 1 << 15), (lim, 1), (1, lim), (1 << 10, 1 << 20)):
        assert nx * ny == lim
        assert guides(rt, w16, nx=nx, ny=ny) == ENOTSUP, (nx, ny)
    for nx, ny in ((lim + 1, 1), (1, lim + 1), (1 << 15, (1 << 15) + 1), (3 * 11 * 331, 331 * 331)):
        assert nx * ny > lim
        assert guides(rt, w16, nx=nx, ny=ny) == EINVAL, (nx, ny)


def params(rt, **kw):
    p = dict(input=rt.DENOISE_INPUT_GAMMA, samples=1, levels=5, normal_pow_log2=5, sigma_position=0.05, sigma_color=0.5)
    p.update(kw)
    return rt.DenoiseParams(**p)


def denoise(rt, p, out=FAKE, inp=FAKE, nx=NX, ny=NY, hits=FAKE, work=FAKE, byref=True):
    return rt.lib().rt_denoise(out, inp, nx, ny, hits, C.byref(p) if (byref and p is not None) else None, work, None)


def test_denoise_refuses_null_pointers_and_bad_sizes(rt):
    p = params(rt)
    assert denoise(rt, p, out=None) == EINVAL
    assert denoise(rt, p, inp=None) == EINVAL
    assert denoise(rt, p, hits=None) == EINVAL
    assert denoise(rt, p, work=None) == EINVAL
    assert denoise(rt, None) == EINVAL
    for nx, ny in ((0, NY), (NX, 0), (-3, NY), (NX, -1), (1 << 15, (1 << 15) + 1), (46341, 46341)):
        assert denoise(rt, p, nx=nx, ny=ny) == EINVAL, (nx, ny)
    # misaligned guide or workspace (read and written as float4)
    assert denoise(rt, p, hits=C.c_void_p(0x1004)) == EINVAL
    assert denoise(rt, p, work=C.c_void_p(0x1008)) == EINVAL


def check(rt, p, nx=NX, ny=NY):
    return rt.lib().rt_denoise_check(nx, ny, C.byref(p) if p is not None else None)


def test_denoise_frame_limit(rt):
    """the filter's kernels index pixels and guide halves (2 * p + 1) in int: frames of exactly DENOISE_MAX_PIXELS pixels are accepted,
    one pixel more is refused — by rt_denoise_check and, before any device work, by rt_denoise"""
    p = params(rt)
    lim = rt.DENOISE_MAX_PIXELS
    for nx, ny in ((1 << 15, 1 << 15), (lim, 1), (1, lim), (1 << 10, 1 << 20)):
        assert nx * ny == lim
        assert check(rt, p, nx, ny) == 0, (nx, ny)
        assert rt.denoise_check(nx, ny, p)
    # frames whose last colour offset 3 * p + 2 is past 2^31 (p >= 715 827 883) are inside the limit: the kernels compute it in 64 bits
    for nx, ny in ((28000, 28000), (30000, 30000), (715827883, 1)):
        assert 3 * (nx * ny - 1) + 2 > 0x7FFFFFFF and nx * ny <= lim
        assert check(rt, p, nx, ny) == 0, (nx, ny)
    for nx, ny in ((lim + 1, 1), (1, lim + 1), (1 << 15, (1 << 15) + 1), (3 * 11 * 331, 331 * 331)):
        assert nx * ny > lim
        assert check(rt, p, nx, ny) == EINVAL, (nx, ny)
        assert denoise(rt, p, nx=nx, ny=ny) == EINVAL, (nx, ny)
    assert check(rt, p, 1, 1) == 0
    for nx, ny in ((0, 1), (1, 0), (-1, 5), (5, -1)):
        assert check(rt, p, nx, ny) == EINVAL, (nx, ny)
    assert check(rt, None) == EINVAL


def test_denoise_refuses_bad_parameters(rt):
    bad = [dict(input=2), dict(input=-1), dict(input=rt.DENOISE_INPUT_SUM, samples=0), dict(input=rt.DENOISE_INPUT_SUM, samples=-4),
           dict(levels=0), dict(levels=rt.DENOISE_MAX_LEVELS + 1), dict(levels=-1),
           dict(normal_pow_log2=-2), dict(normal_pow_log2=11),
           dict(sigma_position=-0.1), dict(sigma_position=float("nan")), dict(sigma_position=float("inf")),
           dict(sigma_color=-1e-3), dict(sigma_color=float("nan")), dict(sigma_color=float("-inf")),
           dict(sigma_position=1e-20),                                   # 1 / sigma^2 overflows: 0 * inf at the centre tap
           dict(sigma_color=1e-18, levels=8)]                            # 4^7 / sigma^2 overflows at the last level
    for kw in bad:
        assert denoise(rt, params(rt, **kw)) == EINVAL, kw
        assert check(rt, params(rt, **kw)) == EINVAL, kw
    # the mirror images of those limits are accepted
    good = [dict(), dict(input=rt.DENOISE_INPUT_SUM, samples=1), dict(levels=1), dict(levels=rt.DENOISE_MAX_LEVELS),
            dict(normal_pow_log2=-1), dict(normal_pow_log2=10), dict(sigma_position=0.0), dict(sigma_color=0.0),
            dict(sigma_color=1e-18, levels=1), dict(sigma_position=1e-18), dict(sigma_color=1e-16, levels=8),
            dict(input=rt.DENOISE_INPUT_GAMMA, samples=0), dict(input=rt.DENOISE_INPUT_GAMMA, samples=-7),
            dict(normal_pow_log2=-1, sigma_position=0.0, sigma_color=0.0, levels=8)]
    for kw in good:
        assert check(rt, params(rt, **kw)) == 0, kw
    assert check(rt, rt.denoise_params()) == 0
    assert check(rt, rt.denoise_params(rt.DENOISE_INPUT_SUM, 1, levels=rt.DENOISE_MAX_LEVELS)) == 0


def test_python_defaults_are_valid(rt):
    p = rt.denoise_params()
    assert (p.input, p.levels, p.normal_pow_log2) == (rt.DENOISE_INPUT_GAMMA, rt.DENOISE_DEFAULTS["levels"], rt.DENOISE_DEFAULTS["normal_pow_log2"])
    q = rt.denoise_params(rt.DENOISE_INPUT_SUM, 8, levels=3)
    assert (q.input, q.samples, q.levels) == (rt.DENOISE_INPUT_SUM, 8, 3)
