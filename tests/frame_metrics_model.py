"""numpy model of rt_frame_levels / rt_frame_compare (include/rt_amd.h), operation by operation, without scipy:
the P6 quantisation of host/rt_image.hpp, cv2's fixed-point grey, the 7x7 window sums by a double cumsum in int64, S exactly as the
header writes it (integers until two binary64 multiplies and one division), and math.fsum for the two double sums — the correctly
rounded sums the device's fixed-order sums are bounded against."""
import math

import numpy as np

RGB8, RGBA8, GRAY8 = 0, 1, 2
GAMMA, SUM = 0, 1
K, C1, C2 = 10000, 65025, 585225


def channels(fb, max_x, max_y):
    """the frame as binary32 (max_y, max_x, 3); a binary16 frame converts exactly"""
    return np.asarray(fb).reshape(max_y, max_x, 3).astype(np.float32)


def levels(c):
    """rt::image_level and the P6 clamp: v = 255.99 * (double)c; INT32_MIN unless -2147483649 < v < 2147483648, else trunc; 0..255"""
    v = 255.99 * np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = (v > -2147483649.0) & (v < 2147483648.0)
    lv = np.full(v.shape, -2**31, np.int64)
    lv[ok] = np.trunc(v[ok]).astype(np.int64)
    return np.clip(lv, 0, 255)


def gray(lv):
    """cv2's RGB -> gray on three levels"""
    return (lv[..., 0] * 4899 + lv[..., 1] * 9617 + lv[..., 2] * 1868 + 8192) >> 14


def display(fb, max_x, max_y, input=GAMMA, samples=1):
    """the channel value rt_frame_levels quantises: GAMMA the frame, SUM sqrtf(fb / (float)samples), each one binary32 rounding"""
    c = channels(fb, max_x, max_y)
    if input == SUM:
        with np.errstate(invalid="ignore", divide="ignore"):
            c = np.sqrt(c / np.float32(samples))
        assert c.dtype == np.float32
    return c


def frame_levels(fb, max_x, max_y, fmt=RGB8, top_first=1, input=GAMMA, samples=1):
    """the bytes rt_frame_levels writes, as a flat uint8 array"""
    lv = levels(display(fb, max_x, max_y, input, samples))
    if top_first:
        lv = lv[::-1]
    if fmt == GRAY8:
        out = gray(lv)
    elif fmt == RGBA8:
        out = np.concatenate([lv, np.full(lv.shape[:2] + (1,), 255, np.int64)], axis=2)
    else:
        out = lv
    return np.ascontiguousarray(out).astype(np.uint8).reshape(-1)


def window_sums(a, win=7):
    """the sum of every win x win window of an int64 image, anchored at its lowest-index pixel: (H-win+1, W-win+1)"""
    c = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
    c[1:, 1:] = np.cumsum(np.cumsum(a.astype(np.int64), axis=0), axis=1)
    return c[win:, win:] - c[:-win, win:] - c[win:, :-win] + c[:-win, :-win]


def ssim_map(ga, gb):
    """S of every window of two grey images (int levels), (H-6, W-6) binary64; an empty array when a side is below 7"""
    ga, gb = np.asarray(ga, np.int64), np.asarray(gb, np.int64)
    if ga.shape[0] < 7 or ga.shape[1] < 7:
        return np.zeros((0, 0), np.float64)
    Sx, Sy = window_sums(ga), window_sums(gb)
    Sxx, Syy, Sxy = window_sums(ga * ga), window_sums(gb * gb), window_sums(ga * gb)
    P = Sx * Sy
    A1 = K * 2 * P + 2401 * C1
    B1 = K * (Sx * Sx + Sy * Sy) + 2401 * C1
    A2 = K * 2 * (49 * Sxy - P) + 2352 * C2
    B2 = K * ((49 * Sxx - Sx * Sx) + (49 * Syy - Sy * Sy)) + 2352 * C2
    for t in (A1, A2, B1, B2):
        assert np.abs(t).max() < 2**53                    # the conversions below are exact
    assert B1.min() > 0 and B2.min() > 0
    return (A1.astype(np.float64) * A2.astype(np.float64)) / (B1.astype(np.float64) * B2.astype(np.float64))


def compare(fb_a, fb_b, max_x, max_y):
    """the record rt_frame_compare leaves (a dict of rt_frame_metrics' fields), plus `ssim_map` and `sq_terms` (the addends of sq_err)"""
    a, b = channels(fb_a, max_x, max_y), channels(fb_b, max_x, max_y)
    ga, gb = gray(levels(a)), gray(levels(b))
    d = ga - gb
    S = ssim_map(ga, gb)
    fin = np.isfinite(a).all(axis=2) & np.isfinite(b).all(axis=2)
    e = a[fin].astype(np.float64) - b[fin].astype(np.float64)
    terms = (e * e).reshape(-1)
    return dict(pixels=max_x * max_y, gray_sse=int((d * d).sum()), gray_differ=int((d != 0).sum()), windows=int(S.size),
                ssim_sum=math.fsum(S.reshape(-1).tolist()), finite_pixels=int(fin.sum()), sq_err=math.fsum(terms.tolist()), reserved=0,
                ssim_map=S, sq_terms=terms)


def psnr(m):
    return math.inf if m["gray_sse"] == 0 else 10.0 * math.log10(65025.0 * m["pixels"] / m["gray_sse"])


def ssim(m):
    return math.nan if m["windows"] == 0 else m["ssim_sum"] / m["windows"]


def rmse(m):
    return math.nan if m["finite_pixels"] == 0 else math.sqrt(m["sq_err"] / (3.0 * m["finite_pixels"]))


def gray_metrics(ga, gb):
    """SSIM and PSNR of two grey images given as levels: what tools/image_metrics.ssim / psnr compute with scipy"""
    ga, gb = np.asarray(ga, np.int64), np.asarray(gb, np.int64)
    S = ssim_map(ga, gb)
    d = ga - gb
    m = dict(pixels=ga.size, gray_sse=int((d * d).sum()), windows=int(S.size), ssim_sum=math.fsum(S.reshape(-1).tolist()))
    return ssim(m), psnr(m)
