"""The premise of csrc/rt_sampling.h, checked on the host for EVERY value a 32-bit draw can convert to.

rng_uniform is (float)X * 2^-32 + 2^-33 and the rejection loops form 2.0f * x - 1.0f.  The kernels compute each with one fused
multiply-add.  That gives the reference's bits if (a) the product is exact in binary32 and (b) rounding the exact sum once gives what
the two-step form gives.  (float)X takes 2^24 + 8 * 2^23 + 1 distinct values for X in 0 .. 2^32 - 1; all of them are enumerated here."""
import numpy as np

P32 = np.float32(2.0 ** -32)
P33 = np.float32(2.0 ** -33)


def _converted_draws():
    """every distinct value of (float)X, X in 0 .. 2^32 - 1, in chunks: the integers up to 2^24, then 2^23 significands for each
    of the exponents 24 .. 31 (round-to-nearest of X lands on these and on 2^32), then 2^32"""
    step = 1 << 22
    for lo in range(0, 1 << 24, step):
        yield np.arange(lo, lo + step, dtype=np.float64).astype(np.float32)
    for e in range(24, 32):
        for lo in range(1 << 23, 1 << 24, step):
            yield (np.arange(lo, lo + step, dtype=np.float64) * float(1 << (e - 23))).astype(np.float32)
    yield np.array([2.0 ** 32], dtype=np.float32)


def test_enumeration_matches_the_conversion_on_random_and_edge_draws():
    """the chunks above are exactly the image of uint32 -> float32: spot-check the conversion itself"""
    rng = np.random.default_rng(7)
    X = np.concatenate([rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64),
                        np.array([0, 1, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 1 << 31, (1 << 32) - 1], dtype=np.uint64)])
    xf = X.astype(np.uint32).astype(np.float32)
    v = xf.astype(np.float64)
    assert np.all((v == 0) | (v >= 1)) and np.all(v <= 2.0 ** 32)
    # each is an integer with at most 24 significant bits: an integer < 2^24, or a multiple of 2^(e-23) in [2^e, 2^(e+1)]
    m, e = np.frexp(v)
    assert np.all(np.ldexp(m, 24) == np.floor(np.ldexp(m, 24)))
    n = 0
    for c in _converted_draws():
        n += c.size
    assert n == (1 << 24) + 8 * (1 << 23) + 1


def test_single_rounding_forms_equal_the_two_step_forms_for_every_draw():
    lo, hi = np.inf, -np.inf
    for xf in _converted_draws():
        x64 = xf.astype(np.float64)
        # (a) the product is exact
        prod32 = xf * P32
        assert prod32.dtype == np.float32
        assert np.array_equal(prod32.astype(np.float64), x64 * 2.0 ** -32)
        # (b) the exact sum (it fits binary64: at most 34 significant bits) rounded once == the two-step result
        two_step = prod32 + P33
        once = (x64 * 2.0 ** -32 + 2.0 ** -33).astype(np.float32)
        assert np.array_equal(two_step.view(np.uint32), once.view(np.uint32))
        u = two_step
        lo = min(lo, float(u.min())); hi = max(hi, float(u.max()))
        # 2x - 1 on every value the draw can return: 2x exact, one rounding of the exact difference == the two-step result
        u64 = u.astype(np.float64)
        dbl32 = np.float32(2.0) * u
        assert np.array_equal(dbl32.astype(np.float64), 2.0 * u64)
        two_step_s = dbl32 - np.float32(1.0)
        once_s = (2.0 * u64 - 1.0).astype(np.float32)
        assert np.array_equal(two_step_s.view(np.uint32), once_s.view(np.uint32))
    assert lo == 2.0 ** -33 and hi == 1.0
