"""CPU tests of history rectification (not gpu): the numpy model of rt_temporal_accumulate_rectified (tests/temporal_rectify_model.py) on
its hand-worked cases and against both parent models, the new symbols in header, library and binding, rt_temporal_rectify_check, and
the refusals of the entry point that come before any device call."""
import ctypes as C

import numpy as np
import pytest

import abi_header
import temporal_rectify_model as trm

tm, tmm = trm.tm, trm.tmm
F = np.float32
NEW = ("rt_temporal_rectify_check", "rt_temporal_accumulate_rectified")


def test_the_rectify_model_on_its_hand_worked_cases():
    trm.self_check()


def random_inputs(seed):
    """fabricated 9x7 buffers as tests/test_animate_host.py builds them, with a varied colour per pixel, some EMPTY pixels and two
    window-sized patches of one sphere so that windows hold more than their centre"""
    rng = np.random.default_rng(seed)
    nx, ny = 9, 7
    n = nx * ny
    cam = tm.simple_camera()
    j, i = np.divmod(np.arange(n), nx)
    pts = np.stack([-1 + 2 * (i + 0.5) / nx, -1 + 2 * (j + 0.5) / ny, -np.ones(n)], 1) * rng.uniform(1.5, 2.5, n)[:, None]
    prev, state = trm.coloured_frame(nx, ny, pts, rng.uniform(0.1, 1.0, n))
    prev["sphere"] = np.where(i < 5, 0, 1 + (j > 3))
    prev["sphere"][rng.choice(n, 6, replace=False)] = rng.integers(3, 12, 6)
    hits = prev.copy()
    hits["sphere"][rng.choice(n, 3, replace=False)] = [-1, 12, 1 << 20]
    S, SL, Q, k = (a.copy() for a in tm.state_parts(state, n))
    k[rng.choice(n, 4, replace=False)] = 1
    state = trm.make_state(S, SL, Q, k)
    g0 = rng.uniform(-1, 1, (12, 4)).astype(F)
    g1 = g0.copy()
    g1[1::3, :3] += F(0.3)
    g1[2::3, 3] *= F(1.25)
    hist = tm.make_history(rng.uniform(0, 1, (n, 4)).astype(F), rng.choice(np.array([0, 4, 8, 100], F), n))
    args = dict(kind=np.zeros(12, np.int32), nx=nx, ny=ny, max_history=32, reuse_specular=0, position_tolerance=1.0, normal_min_dot=0.9)
    return hist, hits, prev, cam, state, g0, g1, args


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_gamma_zero_is_both_parent_models_bit_for_bit(seed):
    hist, hits, prev, cam, state, g0, g1, args = random_inputs(seed)
    for radius, min_count in ((1, 2), (2, 25)):
        off = dict(args, radius=radius, min_count=min_count, gamma=0.0)
        c = {}
        got = trm.accumulate_rectified(hist, hits, prev, cam, state, counts=c, **off)
        assert np.array_equal(got.view(np.uint32), tm.accumulate(hist, hits, prev, cam, state, **args).view(np.uint32))
        assert c["took"] > 10 and c["rectified"] == 0
        got = trm.accumulate_rectified(hist, hits, prev, cam, state, geom=g1, geom_prev=g0, counts=c, **off)
        assert np.array_equal(got.view(np.uint32), tmm.accumulate_moving(hist, hits, prev, cam, g1, g0, state, **args).view(np.uint32))
        assert c["moved_asked"] > 0 and c["rectified"] == 0
        first = trm.accumulate_rectified(None, hits, None, None, state, geom=g1, geom_prev=None, **off)
        assert np.array_equal(first.view(np.uint32), tm.accumulate(None, hits, None, None, state, **args).view(np.uint32))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_neff_never_rises_and_untaken_pixels_are_untouched(seed):
    hist, hits, prev, cam, state, g0, g1, args = random_inputs(seed)
    n = args["nx"] * args["ny"]
    seen = dict(rectified=0, kept_min_count=0, kept_within=0, taps_outside=0, taps_empty=0, taps_sphere=0)
    for moving in (False, True):
        geo = dict(geom=g1, geom_prev=g0) if moving else {}
        plain = tmm.accumulate_moving(hist, hits, prev, cam, g1, g0, state, **args) if moving else tm.accumulate(hist, hits, prev, cam, state, **args)
        xp, npl = tm.history_parts(plain, n)
        for radius, min_count, gamma in ((1, 2, 0.5), (1, 4, 1.5), (2, 2, 1.0), (2, 6, 3.0)):
            c = {}
            got = trm.accumulate_rectified(hist, hits, prev, cam, state, radius=radius, min_count=min_count, gamma=gamma, counts=c, **geo, **args)
            x, neff = tm.history_parts(got, n)
            assert (neff <= npl).all()
            assert np.array_equal(c["neff_unrectified"], npl)
            same = ~c["rectified_mask"]
            assert np.array_equal(x[same].view(np.uint32), xp[same].view(np.uint32)) and np.array_equal(neff[same], npl[same])
            assert (neff[c["rectified_mask"]] < npl[c["rectified_mask"]]).all() and not (c["rectified_mask"] & ~c["took_mask"]).any()
            for key in seen:
                seen[key] += c[key]
    assert all(v > 0 for v in seen.values()), seen


def test_header_library_and_binding_name_the_new_symbols(rt):
    abi_header.check_bound(rt, NEW)
    assert all(abi_header.PROTOTYPES[name][0] is C.c_int for name in NEW)
    abi_header.check_struct(rt.TemporalRectify, "rt_temporal_rectify")
    assert C.sizeof(rt.TemporalRectify) == 12
    for name in ("TemporalRectify", "temporal_rectify", "temporal_rectify_check", "temporal_accumulate_rectified"):
        assert hasattr(rt, name), name
    for key in ("RADIUS", "MIN_COUNT", "GAMMA"):
        assert abi_header.DEFINES["RT_TEMPORAL_RECTIFY_DEFAULT_" + key] == rt.TEMPORAL_RECTIFY_DEFAULTS[key.lower()], key
    d = rt.temporal_rectify()
    assert (d.radius, d.min_count) == (rt.TEMPORAL_RECTIFY_DEFAULTS["radius"], rt.TEMPORAL_RECTIFY_DEFAULTS["min_count"])
    assert rt.temporal_rectify_check(d) and rt.temporal_rectify(gamma=0.0).gamma == 0.0
    assert rt.lib().rt_abi_version() == 6 and abi_header.DEFINES["RT_ABI_VERSION"] == 6


BAD = [dict(radius=0), dict(radius=3), dict(min_count=1), dict(radius=1, min_count=10), dict(radius=2, min_count=26), dict(gamma=-1.0),
       dict(gamma=float("nan")), dict(gamma=float("inf")), dict(gamma=1e20)]


def test_rectify_check(rt):
    L = rt.lib()
    assert L.rt_temporal_rectify_check(None) == -1
    assert not rt.temporal_rectify_check(None)
    for kw in BAD:
        assert not rt.temporal_rectify_check(rt.temporal_rectify(**kw)), kw
    for kw in (dict(radius=1, min_count=2), dict(radius=1, min_count=9), dict(radius=2, min_count=25), dict(gamma=0.0), dict(gamma=1e19),
               dict(gamma=1e-30)):
        assert rt.temporal_rectify_check(rt.temporal_rectify(**kw)), kw


def test_the_entry_point_refuses_before_any_device_call(rt):
    """a world that is never uploaded and pointers that are never followed: every refusal here comes from the host checks"""
    L = rt.lib()
    W = rt.World(22, 8, 8)
    p, r = rt.temporal_params(), rt.temporal_rectify()
    a = lambda v: C.c_void_p(v)
    cam = W.get_camera()
    camp = cam.ctypes.data_as(C.c_void_p)

    def call(out=a(1 << 20), hin=a(2 << 20), hits=a(3 << 20), prev=a(4 << 20), cam=camp, geom=None, state=a(5 << 20), world=W.h, nx=8, ny=8,
             params=C.byref(p), rect=C.byref(r)):
        return L.rt_temporal_accumulate_rectified(out, hin, hits, prev, cam, geom, state, world, nx, ny, params, rect, None)

    assert call(rect=None) == -1
    for kw in BAD:
        assert call(rect=C.byref(rt.temporal_rectify(**kw))) == -1, kw
    assert call(geom=a((6 << 20) + 4)) == -1 and call(geom=a((6 << 20) + 8)) == -1       # misaligned, with a history ...
    assert call(hin=None, prev=None, cam=None, geom=a((6 << 20) + 4)) == -1               # ... and without one
    # everything rt_temporal_accumulate refuses
    assert call(out=None) == -1 and call(hits=None) == -1 and call(state=None) == -1 and call(world=None) == -1
    assert call(prev=None) == -1 and call(cam=None) == -1
    assert call(out=a((1 << 20) + 4)) == -1 and call(hin=a((2 << 20) + 4)) == -1 and call(hits=a((3 << 20) + 8)) == -1
    assert call(prev=a((4 << 20) + 4)) == -1
    assert call(hin=a((1 << 20) + 16)) == -1                                              # overlapping histories
    assert call(nx=0) == -1 and call(params=None) == -1 and call(params=C.byref(rt.temporal_params(position_tolerance=0.0))) == -1
    half = rt.World(22, 8, 8, precision=rt.FP16)
    assert call(world=half.h, rect=None) == -1                                            # RT_EINVAL comes first ...
    assert call(world=half.h) == -4                                                       # ... then RT_ENOTSUP, still without a device
    half.close()
    W.close()
