"""rt_frame_levels / rt_frame_compare without a GPU: the ABI's new names, the host-only checks and size functions, the
three host metrics on hand-filled records, and the numpy model (tests/frame_metrics_model.py) against tools/image_metrics (scipy)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import abi_header
import frame_metrics_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW = {"rt_frame_levels", "rt_frame_levels_check", "rt_frame_levels_bytes", "rt_frame_compare_work_bytes", "rt_frame_compare",
       "rt_frame_psnr", "rt_frame_ssim", "rt_frame_rmse"}
EINVAL, ENOTSUP = -1, -4
MAX_PIXELS = 1 << 30


def test_header_binding_and_library_agree_on_the_new_names(rt):
    assert NEW <= set(abi_header.PROTOTYPES) and NEW <= set(rt.SYMBOLS)
    assert set(abi_header.PROTOTYPES) == set(rt.SYMBOLS)
    abi_header.check_bound(rt, NEW)
    assert rt.lib().rt_abi_version() == 6 and abi_header.DEFINES["RT_ABI_VERSION"] == 6
    for name, value in (("RT_LEVELS_RGB8", 0), ("RT_LEVELS_RGBA8", 1), ("RT_LEVELS_GRAY8", 2)):
        assert abi_header.DEFINES[name] == value
    assert (rt.LEVELS_RGB8, rt.LEVELS_RGBA8, rt.LEVELS_GRAY8) == (0, 1, 2)
    abi_header.check_struct(rt.FrameMetrics, "rt_frame_metrics")
    abi_header.check_struct(rt.LevelsParams, "rt_levels_params")
    assert C.sizeof(rt.FrameMetrics) == 64 and C.sizeof(rt.LevelsParams) == 16
    assert [f[0] for f in rt.FrameMetrics._fields_] == ["pixels", "gray_sse", "gray_differ", "windows", "ssim_sum", "finite_pixels", "sq_err",
                                                        "reserved"]


def test_levels_check_accepts_and_refuses(rt):
    L = rt.lib()

    def chk(nx, ny, prec, *p):
        return L.rt_frame_levels_check(nx, ny, prec, C.byref(rt.LevelsParams(*p)))

    for fmt in (0, 1, 2):
        for top in (0, 1):
            assert chk(37, 23, rt.FP32, rt.DENOISE_INPUT_GAMMA, 0, fmt, top) == 0
            assert chk(37, 23, rt.FP16, rt.DENOISE_INPUT_GAMMA, -5, fmt, top) == 0          # GAMMA ignores samples
            assert chk(37, 23, rt.FP32, rt.DENOISE_INPUT_SUM, 1, fmt, top) == 0
    assert chk(1 << 15, 1 << 15, rt.FP32, 0, 1, 0, 1) == 0                                   # exactly RT_DENOISE_MAX_PIXELS
    assert chk((1 << 15) + 1, 1 << 15, rt.FP32, 0, 1, 0, 1) == EINVAL
    assert L.rt_frame_levels_check(8, 8, rt.FP32, None) == EINVAL
    for nx, ny in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert chk(nx, ny, rt.FP32, 0, 1, 0, 1) == EINVAL
    assert chk(8, 8, 2, 0, 1, 0, 1) == EINVAL and chk(8, 8, -1, 0, 1, 0, 1) == EINVAL      # precision
    assert chk(8, 8, rt.FP32, 2, 1, 0, 1) == EINVAL and chk(8, 8, rt.FP32, -1, 1, 0, 1) == EINVAL      # input
    assert chk(8, 8, rt.FP32, 0, 1, 3, 1) == EINVAL and chk(8, 8, rt.FP32, 0, 1, -1, 1) == EINVAL      # format
    assert chk(8, 8, rt.FP32, rt.DENOISE_INPUT_SUM, 0, 0, 1) == EINVAL                      # samples < 1 with SUM
    assert chk(8, 8, rt.FP32, 0, 1, 0, 2) == EINVAL and chk(8, 8, rt.FP32, 0, 1, 0, -1) == EINVAL      # top_first
    assert chk(8, 8, rt.FP16, rt.DENOISE_INPUT_SUM, 4, 0, 1) == ENOTSUP
    assert chk(8, 8, rt.FP16, rt.DENOISE_INPUT_SUM, 0, 0, 1) == EINVAL                      # a bad argument comes first


def test_size_functions(rt):
    L = rt.lib()
    assert L.rt_frame_levels_bytes(37, 23, 0) == 3 * 37 * 23
    assert L.rt_frame_levels_bytes(37, 23, 1) == 4 * 37 * 23
    assert L.rt_frame_levels_bytes(37, 23, 2) == 37 * 23
    assert L.rt_frame_levels_bytes(1 << 15, 1 << 15, 1) == 4 << 30
    assert rt.frame_levels_bytes(3840, 2160, rt.LEVELS_RGBA8) == 4 * 3840 * 2160
    for args in ((0, 23, 0), (37, 0, 0), (-4, 23, 0), (37, 23, 3), (37, 23, -1), ((1 << 15) + 1, 1 << 15, 0)):
        assert L.rt_frame_levels_bytes(*args) == -1
    with pytest.raises(rt.RtError):
        rt.frame_levels_bytes(0, 1)
    sizes = {}
    for nx, ny in ((1, 1), (7, 7), (6, 20), (131, 67), (1200, 800), (3840, 2160), (1 << 30, 1), (1, 1 << 30)):
        n = L.rt_frame_compare_work_bytes(nx, ny)
        assert n > 0 and n % 8 == 0
        sizes[(nx, ny)] = n
    assert sizes[(1, 1)] == sizes[(7, 7)] and sizes[(3840, 2160)] > sizes[(1200, 800)] > sizes[(131, 67)] > sizes[(1, 1)]
    assert sizes[(1200, 800)] < 1200 * 800                 # partial records, not a per-pixel buffer
    for nx, ny in ((0, 8), (8, 0), (-1, -1), ((1 << 15) + 1, 1 << 15)):
        assert L.rt_frame_compare_work_bytes(nx, ny) == -1


def test_compare_refuses_bad_arguments_on_the_host(rt):
    """everything rt_frame_compare and rt_frame_levels refuse is refused before any device work (the pointers are never dereferenced)"""
    L = rt.lib()
    a, b, m, w = 0x1000, 0x2000, 0x3000, 0x4000
    assert L.rt_frame_compare(None, 0, b, 0, 8, 8, m, None, w, None) == EINVAL
    assert L.rt_frame_compare(a, 0, None, 0, 8, 8, m, None, w, None) == EINVAL
    assert L.rt_frame_compare(a, 0, b, 0, 8, 8, None, None, w, None) == EINVAL
    assert L.rt_frame_compare(a, 0, b, 0, 8, 8, m, None, None, None) == EINVAL
    for nx, ny in ((0, 8), (8, 0), (-8, 8), ((1 << 15) + 1, 1 << 15)):
        assert L.rt_frame_compare(a, 0, b, 0, nx, ny, m, None, w, None) == EINVAL
    assert L.rt_frame_compare(a, 2, b, 0, 8, 8, m, None, w, None) == EINVAL
    assert L.rt_frame_compare(a, 0, b, -1, 8, 8, m, None, w, None) == EINVAL
    assert L.rt_frame_compare(a, 0, b, 0, 8, 8, m, None, w + 4, None) == EINVAL
    assert L.rt_frame_compare(a, 0, b, 0, 8, 8, m, 0x5004, w, None) == EINVAL
    p = rt.LevelsParams(0, 1, 0, 1)
    assert L.rt_frame_levels(None, a, 8, 8, 0, C.byref(p), None) == EINVAL
    assert L.rt_frame_levels(a, None, 8, 8, 0, C.byref(p), None) == EINVAL
    assert L.rt_frame_levels(a, b, 8, 8, 0, None, None) == EINVAL
    assert L.rt_frame_levels(a, b, 0, 8, 0, C.byref(p), None) == EINVAL
    assert L.rt_frame_levels(a, b, 8, 8, 0, C.byref(rt.LevelsParams(0, 1, 7, 1)), None) == EINVAL
    assert L.rt_frame_levels(a, b, 8, 8, 1, C.byref(rt.LevelsParams(1, 4, 0, 1)), None) == ENOTSUP


RECORDS = [dict(pixels=960000, gray_sse=123456789, gray_differ=700000, windows=1194 * 794, ssim_sum=881234.56789, finite_pixels=959990,
                sq_err=1234.5678),
           dict(pixels=49, gray_sse=1, gray_differ=1, windows=1, ssim_sum=0.999, finite_pixels=49, sq_err=1e-12),
           dict(pixels=1 << 30, gray_sse=65025 << 30, gray_differ=1 << 30, windows=1, ssim_sum=-0.25, finite_pixels=1 << 30, sq_err=3e77),
           dict(pixels=120, gray_sse=0, gray_differ=0, windows=0, ssim_sum=0.0, finite_pixels=0, sq_err=0.0)]


@pytest.mark.parametrize("rec", RECORDS, ids=["c3-like", "one-window", "extremes", "zeros"])
def test_host_metrics_on_hand_filled_records(rt, rec):
    m = rt.FrameMetrics(rec["pixels"], rec["gray_sse"], rec["gray_differ"], rec["windows"], rec["ssim_sum"], rec["finite_pixels"], rec["sq_err"], 0)
    if rec["gray_sse"] == 0:
        assert m.psnr == math.inf
    else:
        ref = 10.0 * np.log10(65025.0 * np.float64(rec["pixels"]) / np.float64(rec["gray_sse"]))
        print("psnr", m.psnr, ref)
        assert abs(m.psnr - ref) <= 1e-12 * abs(ref) or (ref == 0 and abs(m.psnr) <= 1e-12)
    if rec["windows"] == 0:
        assert math.isnan(m.ssim)
    else:
        assert m.ssim == rec["ssim_sum"] / rec["windows"]
    if rec["finite_pixels"] == 0:
        assert math.isnan(m.rmse)
    else:
        assert m.rmse == math.sqrt(rec["sq_err"] / (3.0 * rec["finite_pixels"]))
    assert m.psnr == fm.psnr(rec) or abs(m.psnr - fm.psnr(rec)) <= 1e-12 * abs(fm.psnr(rec))
    L = rt.lib()
    assert math.isnan(L.rt_frame_psnr(None)) and math.isnan(L.rt_frame_ssim(None)) and math.isnan(L.rt_frame_rmse(None))


def greys(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w)), rng.integers(0, 256, (h, w))
    if kind == "gradient":
        a = (np.add.outer(np.arange(h) * 3, np.arange(w) * 2) % 256).astype(np.int64)
        return a, np.clip(a + rng.integers(-6, 7, (h, w)), 0, 255)
    a = ((np.add.outer(np.arange(h), np.arange(w)) & 1) * 255).astype(np.int64)      # 0/255 checker against its shifted copy
    return a, np.roll(a, 1, axis=1) if w > 1 else a


@pytest.mark.parametrize("kind", ["random", "gradient", "checker"])
@pytest.mark.parametrize("h,w", [(67, 131), (45, 70), (7, 7)])
def test_model_reproduces_the_scipy_metrics(kind, h, w):
    import image_metrics as im
    a, b = greys(kind, h, w, 11)
    s, p = fm.gray_metrics(a, b)
    s_ref, p_ref = im.ssim(a.astype(np.float64), b.astype(np.float64)), im.psnr(a.astype(np.float64), b.astype(np.float64))
    print(kind, h, w, "ssim", s, s_ref, abs(s - s_ref), "psnr", p, p_ref)
    assert abs(s - s_ref) <= 1e-9
    assert abs(p - p_ref) <= 1e-9 or (math.isinf(p) and math.isinf(p_ref))


@pytest.mark.parametrize("h,w", [(67, 131), (7, 7), (9, 40)])
def test_model_gives_exactly_one_for_identical_images(h, w):
    for kind in ("random", "gradient", "checker"):
        a, _ = greys(kind, h, w, 5)
        S = fm.ssim_map(a, a)
        assert S.shape == (h - 6, w - 6) and (S == 1.0).all()
        assert fm.gray_metrics(a, a) == (1.0, math.inf)
    for v in (0, 255):
        assert (fm.ssim_map(np.full((h, w), v), np.full((h, w), v)) == 1.0).all()


def test_model_levels_follow_the_p6_writer(rt, tmp_path):
    """the model's levels are the bytes rt_write_image's P6 holds, on the awkward values too"""
    nx, ny = 19, 5
    rng = np.random.default_rng(3)
    fb = rng.uniform(-0.1, 1.1, (ny, nx, 3)).astype(np.float32)
    flat = fb.reshape(-1)
    flat[:9] = [np.nan, np.inf, -np.inf, -0.3, 1.7, 8e6, 1e10, -1e10, 0.0]
    k = np.arange(1, 40, dtype=np.float64)
    edge = (k / 255.99).astype(np.float32)
    flat[20:59], flat[60:99], flat[100:139] = edge, np.nextafter(edge, np.float32(2)), np.nextafter(edge, np.float32(-2))
    path = tmp_path / "m.ppm"
    rt.write_image(path, fb, nx, ny, rt.FP32, rt.IMAGE_P6)
    raw = open(path, "rb").read()
    body = np.frombuffer(raw[len(raw) - nx * ny * 3:], np.uint8)
    assert np.array_equal(fm.frame_levels(fb, nx, ny, fm.RGB8, 1), body)
    assert np.array_equal(fm.frame_levels(fb, nx, ny, fm.RGB8, 0).reshape(ny, nx, 3)[::-1].reshape(-1), body)
    lv = fm.levels(fb)
    assert lv[0, 0].tolist() == [0, 0, 0] and lv[0, 1].tolist() == [0, 255, 255] and lv[0, 2].tolist() == [0, 0, 0]
    assert np.array_equal(fm.frame_levels(fb, nx, ny, fm.GRAY8, 0), fm.gray(lv).reshape(-1))
