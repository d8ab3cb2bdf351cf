"""Bit views and bit comparisons of the tests, each written once.  numpy only.

Two views: f32_bits converts what it is given to float32 first (a list, a float64 model result, an integer array by VALUE);
raw_bits reinterprets the bytes of a 4-byte array (float32, int32, uint32) and converts nothing.  Three comparisons: the reference's
NaNs (got must be NaN exactly there, any payload), any NaN equals any NaN, and snapshot dicts key by key."""
import numpy as np


def f32_bits(a):
    """the binary32 patterns of a's values: a is converted to float32 first"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def raw_bits(a):
    """a 4-byte array's own bytes as uint32: nothing is converted (an int32 count stays its integer pattern)"""
    return np.ascontiguousarray(a).view(np.uint32)


def same_nan_as_ref(got, ref):
    """same shape, bit-equal where the reference is a number, NaN (any payload) where the reference has NaN"""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    nan = np.isnan(ref)
    return got.shape == ref.shape and np.array_equal(f32_bits(got)[~nan], f32_bits(ref)[~nan]) and bool(np.isnan(got[nan]).all())


def same_any_nan(a, b):
    """bit equality, except that any two NaNs are equal (sqrtf of a NaN need not keep its payload)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(f32_bits(a[~na]), f32_bits(b[~nb])))


def assert_same_snapshots(a, b, what=""):
    """two snapshot dicts (Frame.snap) hold equal arrays under every key of a; a failure names the key"""
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)
