"""CPU tests of rt_denoise_adaptive (not gpu): declared, exported and bound with the same signatures, structure and constants; every
refused call returns RT_EINVAL before any device work (placeholder device pointers are enough) and the mirror image of every limit is
accepted; the frame limit sits at exactly RT_DENOISE_MAX_PIXELS; the numpy model of the rule passes its own check against the float64
restatement; and the ABI version is still 6 (the feature only adds symbols)."""
import ctypes as C
import os

import numpy as np

import abi_header
import denoise_var_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = C.c_void_p(0x1000)          # never dereferenced: the calls below refuse before they touch a buffer
NX, NY = 64, 40
EINVAL = -1


def test_header_and_binding_agree(rt):
    names = {"rt_denoise_adaptive": ["fb_out", "fb_in", "max_x", "max_y", "d_hits", "d_state", "params", "d_work", "stream"],
             "rt_denoise_adaptive_check": ["max_x", "max_y", "params"]}
    abi_header.check_bound(rt, names)
    for name in names:
        assert abi_header.PARAM_NAMES[name] == names[name] and abi_header.PROTOTYPES[name][0] is C.c_int, name
    abi_header.check_struct(rt.DenoiseVarParams, "rt_denoise_var_params")
    # (the header's constants and defaults against the binding's: tests/test_host_and_abi.py::test_constants_equal_the_header)
    assert np.float32(abi_header.DEFINES["RT_DENOISE_VAR_EPS"]) == denoise_var_model.EPS
    assert set(rt.DENOISE_VAR_DEFAULTS) == {n for n, _ in rt.DenoiseVarParams._fields_}


def test_abi_version_is_unchanged(rt):
    assert rt.lib().rt_abi_version() == 6


def params(rt, **kw):
    p = dict(levels=5, normal_pow_log2=5, prefilter=1, sigma_position=0.05, sigma_variance=2.0)
    p.update(kw)
    return rt.DenoiseVarParams(**p)


def denoise(rt, p, out=FAKE, inp=FAKE, nx=NX, ny=NY, hits=FAKE, state=FAKE, work=FAKE):
    return rt.lib().rt_denoise_adaptive(out, inp, nx, ny, hits, state, C.byref(p) if p is not None else None, work, None)


def check(rt, p, nx=NX, ny=NY):
    return rt.lib().rt_denoise_adaptive_check(nx, ny, C.byref(p) if p is not None else None)


def test_refuses_null_pointers_misalignment_and_bad_sizes(rt):
    p = params(rt)
    assert denoise(rt, p, out=None) == EINVAL
    assert denoise(rt, p, inp=None) == EINVAL
    assert denoise(rt, p, hits=None) == EINVAL
    assert denoise(rt, p, state=None) == EINVAL
    assert denoise(rt, p, work=None) == EINVAL
    assert denoise(rt, None) == EINVAL
    for nx, ny in ((0, NY), (NX, 0), (-3, NY), (NX, -1), (1 << 15, (1 << 15) + 1), (46341, 46341)):
        assert denoise(rt, p, nx=nx, ny=ny) == EINVAL, (nx, ny)
        assert check(rt, p, nx, ny) == EINVAL, (nx, ny)
    assert denoise(rt, p, hits=C.c_void_p(0x1004)) == EINVAL                      # read and written as float4
    assert denoise(rt, p, work=C.c_void_p(0x1008)) == EINVAL
    assert check(rt, None) == EINVAL


def test_frame_limit(rt):
    """frames of exactly DENOISE_MAX_PIXELS pixels are accepted, one pixel more is refused — by the check and, before any device
    work, by the call"""
    p = params(rt)
    lim = rt.DENOISE_MAX_PIXELS
    for nx, ny in ((1 << 15, 1 << 15), (lim, 1), (1, lim), (1 << 10, 1 << 20), (28000, 28000), (715827883, 1)):
        assert nx * ny <= lim
        assert check(rt, p, nx, ny) == 0, (nx, ny)
        assert rt.denoise_adaptive_check(nx, ny, p)
    for nx, ny in ((lim + 1, 1), (1, lim + 1), (1 << 15, (1 << 15) + 1), (3 * 11 * 331, 331 * 331)):
        assert nx * ny > lim
        assert check(rt, p, nx, ny) == EINVAL, (nx, ny)
        assert not rt.denoise_adaptive_check(nx, ny, p)
        assert denoise(rt, p, nx=nx, ny=ny) == EINVAL, (nx, ny)
    assert check(rt, p, 1, 1) == 0


def test_refuses_bad_parameters_and_accepts_their_mirror_images(rt):
    bad = [dict(levels=0), dict(levels=rt.DENOISE_MAX_LEVELS + 1), dict(levels=-1),
           dict(normal_pow_log2=-2), dict(normal_pow_log2=11),
           dict(prefilter=-1), dict(prefilter=2),
           dict(sigma_position=-0.1), dict(sigma_position=float("nan")), dict(sigma_position=float("inf")),
           dict(sigma_variance=-1e-3), dict(sigma_variance=float("nan")), dict(sigma_variance=float("inf")), dict(sigma_variance=float("-inf")),
           dict(sigma_position=1e-20),                                   # 1 / sigma^2 overflows: 0 * inf at the centre tap
           dict(sigma_variance=2e19)]                                    # sigma^2 overflows
    for kw in bad:
        assert denoise(rt, params(rt, **kw)) == EINVAL, kw
        assert check(rt, params(rt, **kw)) == EINVAL, kw
    good = [dict(), dict(levels=1), dict(levels=rt.DENOISE_MAX_LEVELS), dict(normal_pow_log2=-1), dict(normal_pow_log2=10),
            dict(prefilter=0), dict(prefilter=1), dict(sigma_position=0.0), dict(sigma_variance=0.0), dict(sigma_position=1e-18),
            dict(sigma_variance=1e19), dict(sigma_variance=1e-30),
            dict(normal_pow_log2=-1, sigma_position=0.0, sigma_variance=0.0, prefilter=0, levels=8)]
    for kw in good:
        assert check(rt, params(rt, **kw)) == 0, kw
    assert check(rt, rt.denoise_var_params()) == 0
    assert check(rt, rt.denoise_var_params(levels=rt.DENOISE_MAX_LEVELS, sigma_variance=0.0)) == 0


def test_python_defaults(rt):
    p = rt.denoise_var_params()
    d = rt.DENOISE_VAR_DEFAULTS
    assert (p.levels, p.normal_pow_log2, p.prefilter) == (d["levels"], d["normal_pow_log2"], d["prefilter"])
    assert np.float32(p.sigma_position) == np.float32(d["sigma_position"]) and np.float32(p.sigma_variance) == np.float32(d["sigma_variance"])
    q = rt.denoise_var_params(levels=3, prefilter=0, sigma_variance=8.0)
    assert (q.levels, q.prefilter, q.sigma_variance) == (3, 0, 8.0)


def test_the_model_follows_the_rule():
    denoise_var_model.self_check()


def test_rt_main_refuses_sigma_variance_without_adaptive_or_denoise(tmp_path):
    """the argument check comes before any device work, so the host program answers it without a GPU"""
    import subprocess
    exe = os.path.join(ROOT, "dd2360-raytracing_amd", "rt_main")
    base = [exe, "1", "500", "64", "40", "8", "1", "30", "0.1", "0", "0"]
    for tail in (["0", "4", "4", "0", "2", "2.0"],        # REL_ERROR 0
                 ["0.1", "4", "4", "0", "0", "2.0"]):     # DENOISE 0
        p = subprocess.run(base + tail, cwd=tmp_path, capture_output=True, timeout=60)
        assert p.returncode != 0 and "DENOISE_SIGMA_VARIANCE" in p.stderr.decode(), tail
