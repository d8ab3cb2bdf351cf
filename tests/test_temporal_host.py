"""CPU tests of temporal accumulation (not gpu): the numpy model of the rule passes its hand-worked cases; rt_temporal_accumulate,
rt_temporal_check and rt_denoise_history are declared, exported and bound with the same signatures, structure and constants;
rt_temporal_check refuses every out-of-range field and accepts the defaults; every refused call returns RT_EINVAL before any device
work (placeholder device pointers are enough); and the ABI version is still 6 (the feature only adds symbols)."""
import ctypes as C

import numpy as np

import abi_header
import temporal_model

FAKE, FAKE2 = C.c_void_p(0x100000), C.c_void_p(0x900000)      # never dereferenced: the calls below refuse before they touch a buffer
NX, NY = 64, 40
EINVAL, ENOTSUP = -1, -4
NEW = ("rt_temporal_check", "rt_temporal_accumulate", "rt_denoise_history")


def test_the_model_follows_the_rule():
    temporal_model.self_check()


def test_header_library_and_binding_agree(rt):
    names = {"rt_temporal_check": ["max_x", "max_y", "params"],
             "rt_temporal_accumulate": ["d_hist_out", "d_hist_in", "d_hits", "d_hits_prev", "cam_prev", "d_state", "world", "max_x", "max_y",
                                        "params", "stream"],
             "rt_denoise_history": ["fb_out", "fb_in", "max_x", "max_y", "d_hits", "d_hist", "params", "d_work", "stream"]}
    abi_header.check_bound(rt, NEW)
    for name in NEW:
        assert abi_header.PARAM_NAMES[name] == names[name] and abi_header.PROTOTYPES[name][0] is C.c_int, name
    abi_header.check_struct(rt.TemporalParams, "rt_temporal_params")
    assert C.sizeof(rt.TemporalParams) == 16
    # (the header's constants and defaults against the binding's: tests/test_host_and_abi.py::test_constants_equal_the_header)
    assert abi_header.DEFINES["RT_TEMPORAL_HISTORY_BYTES"] == rt.TEMPORAL_HISTORY_BYTES == 20
    assert set(rt.TEMPORAL_DEFAULTS) == {n for n, _ in rt.TemporalParams._fields_}
    assert temporal_model.hit_record_dtype == rt.hit_record_dtype and temporal_model.camera_dtype == rt.camera_dtype
    for fn in ("temporal_params", "alloc_temporal_history", "temporal_check", "temporal_accumulate", "denoise_history"):
        assert callable(getattr(rt, fn)), fn


def test_abi_version_is_unchanged(rt):
    assert rt.lib().rt_abi_version() == 6


def check(rt, p, nx=NX, ny=NY):
    return rt.lib().rt_temporal_check(nx, ny, C.byref(p) if p is not None else None)


def test_check_refuses_every_field_out_of_range_and_accepts_the_defaults(rt):
    assert check(rt, rt.temporal_params()) == 0 and rt.temporal_check(NX, NY, rt.temporal_params())
    bad = [dict(max_history=-1), dict(max_history=-(1 << 31)), dict(reuse_specular=-1), dict(reuse_specular=2),
           dict(position_tolerance=0.0), dict(position_tolerance=-0.01), dict(position_tolerance=float("nan")),
           dict(position_tolerance=float("inf")), dict(position_tolerance=2e19),                 # tol^2 overflows
           dict(normal_min_dot=-1.0001), dict(normal_min_dot=1.0001), dict(normal_min_dot=float("nan")), dict(normal_min_dot=float("inf"))]
    for kw in bad:
        assert check(rt, rt.temporal_params(**kw)) == EINVAL, kw
        assert not rt.temporal_check(NX, NY, rt.temporal_params(**kw)), kw
    good = [dict(max_history=0), dict(max_history=(1 << 31) - 1), dict(reuse_specular=1), dict(position_tolerance=1e-30),
            dict(position_tolerance=1e19), dict(normal_min_dot=-1.0), dict(normal_min_dot=1.0), dict(normal_min_dot=0.0)]
    for kw in good:
        assert check(rt, rt.temporal_params(**kw)) == 0, kw
    assert check(rt, None) == EINVAL
    lim = rt.DENOISE_MAX_PIXELS
    for nx, ny in ((0, NY), (NX, 0), (-3, NY), (NX, -1), (lim + 1, 1), (1 << 15, (1 << 15) + 1)):
        assert check(rt, rt.temporal_params(), nx, ny) == EINVAL, (nx, ny)
    for nx, ny in ((1, 1), (lim, 1), (1 << 15, 1 << 15)):
        assert check(rt, rt.temporal_params(), nx, ny) == 0, (nx, ny)


def accumulate(rt, world, p, out=FAKE, inp=FAKE2, hits=FAKE, prev=FAKE, cam="cam", state=FAKE, nx=NX, ny=NY):
    camera = np.zeros(1, rt.camera_dtype)
    cam = camera.ctypes.data_as(C.c_void_p) if cam == "cam" else cam
    return rt.lib().rt_temporal_accumulate(out, inp, hits, prev, cam, state, world, nx, ny, C.byref(p) if p is not None else None, None)


def test_accumulate_refuses_before_any_device_work(rt):
    W = rt.World(500, NX, NY)
    H = rt.World(500, NX, NY, precision=rt.FP16)
    p = rt.temporal_params()
    try:
        assert accumulate(rt, W.h, p, out=None) == EINVAL
        assert accumulate(rt, W.h, p, hits=None) == EINVAL
        assert accumulate(rt, W.h, p, state=None) == EINVAL
        assert accumulate(rt, None, p) == EINVAL
        assert accumulate(rt, W.h, None) == EINVAL
        assert accumulate(rt, W.h, p, prev=None) == EINVAL                   # a history without the guides or the camera it belongs to
        assert accumulate(rt, W.h, p, cam=None) == EINVAL
        for kw in (dict(out=C.c_void_p(0x100004)), dict(inp=C.c_void_p(0x900008)), dict(hits=C.c_void_p(0x10000c)), dict(prev=C.c_void_p(0x100010 + 4))):
            assert accumulate(rt, W.h, p, **kw) == EINVAL, kw
        assert accumulate(rt, W.h, p, inp=FAKE) == EINVAL                     # d_hist_in == d_hist_out
        n = NX * NY
        for off in (16, 20 * n - 16, -16, -(20 * n - 16)):                     # any overlap of the two histories
            assert accumulate(rt, W.h, p, inp=C.c_void_p(FAKE.value + off)) == EINVAL, off
        for kw in (dict(max_history=-1), dict(reuse_specular=2), dict(position_tolerance=0.0), dict(normal_min_dot=2.0)):
            assert accumulate(rt, W.h, rt.temporal_params(**kw)) == EINVAL, kw
        assert accumulate(rt, W.h, p, nx=0) == EINVAL and accumulate(rt, W.h, p, ny=-1) == EINVAL
        # after those checks, an fp16 world is RT_ENOTSUP — and a refused argument still comes first
        assert accumulate(rt, H.h, p) == ENOTSUP
        assert accumulate(rt, H.h, p, inp=None, prev=None, cam=None) == ENOTSUP
        assert accumulate(rt, H.h, p, out=None) == EINVAL
        assert accumulate(rt, H.h, rt.temporal_params(max_history=-1)) == EINVAL
    finally:
        W.close()
        H.close()


def test_denoise_history_refuses_like_denoise_adaptive(rt):
    def call(p, out=FAKE, inp=FAKE, nx=NX, ny=NY, hits=FAKE, hist=FAKE, work=FAKE):
        return rt.lib().rt_denoise_history(out, inp, nx, ny, hits, hist, C.byref(p) if p is not None else None, work, None)
    p = rt.denoise_var_params()
    for kw in (dict(out=None), dict(inp=None), dict(hits=None), dict(hist=None), dict(work=None)):
        assert call(p, **kw) == EINVAL, kw
    assert call(None) == EINVAL
    for kw in (dict(hits=C.c_void_p(0x100004)), dict(hist=C.c_void_p(0x100008)), dict(work=C.c_void_p(0x10000c))):
        assert call(p, **kw) == EINVAL, kw
    for nx, ny in ((0, NY), (NX, 0), (1 << 15, (1 << 15) + 1)):
        assert call(p, nx=nx, ny=ny) == EINVAL, (nx, ny)
    for kw in (dict(levels=0), dict(levels=rt.DENOISE_MAX_LEVELS + 1), dict(prefilter=2), dict(sigma_variance=-1.0), dict(sigma_position=1e-20)):
        assert call(rt.denoise_var_params(**kw)) == EINVAL, kw


def test_python_defaults(rt):
    p = rt.temporal_params()
    d = rt.TEMPORAL_DEFAULTS
    assert (p.max_history, p.reuse_specular) == (d["max_history"], d["reuse_specular"])
    assert np.float32(p.position_tolerance) == np.float32(d["position_tolerance"]) and np.float32(p.normal_min_dot) == np.float32(d["normal_min_dot"])
    q = rt.temporal_params(max_history=8, reuse_specular=1, position_tolerance=1.0)
    assert (q.max_history, q.reuse_specular, q.position_tolerance) == (8, 1, 1.0)
