"""The numpy model of adaptive sample budgets (include/rt_amd.h, DESIGN.md §5.9 "Budgets"): the priority key in binary32, one
operation per line, the eligibility mask, the picks of a round, and the selection as a plain sort."""
import numpy as np


def priority(SL, Q, k, floor):
    """rt_adaptive_priority for arrays (or scalars): float32 in, float32 out, one rounding per operation"""
    SL = np.asarray(SL, np.float32)
    Q = np.asarray(Q, np.float32)
    floor = np.float32(floor)
    with np.errstate(all="ignore"):
        n = np.asarray(k, np.int32).astype(np.float32)
        nq = n * Q
        ss = SL * SL
        d = nq - ss
        d = np.where(d > 0, d, np.float32(0))                # a NaN d becomes 0
        nf = n * floor
        m = np.where(SL > nf, SL, nf)
        mm = m * m
        n1 = n - np.float32(1)
        den = n1 * mm
        e = d / den
        key = np.where(e > 0, e, np.float32(0))              # NaN becomes 0, +inf stays
    return key.astype(np.float32)


def keybits(key):
    return np.ascontiguousarray(key, np.float32).view(np.uint32)


def picks(samples, rounds, batch, r):
    """K_r: integer divisions (Python ints, never negative here, so // is C's /)"""
    q = samples // batch
    return q * (r + 1) // rounds - q * r // rounds


def eligible(SL, Q, k, batch, max_spp, floor, in_frame):
    """(mask, key bits) of the elements a round may pick"""
    kb = keybits(priority(SL, Q, k, floor))
    ok = in_frame & (np.asarray(k, np.int64) + batch <= max_spp) & (kb > 0)
    return ok, kb


def select(SL, Q, k, batch, max_spp, floor, in_frame, K):
    """the sorted ids of the first min(K, eligible) eligible elements by key descending, id ascending; also the mask and the key bits"""
    ok, kb = eligible(SL, Q, k, batch, max_spp, floor, in_frame)
    ids = np.nonzero(ok)[0].astype(np.int64)
    order = np.lexsort((ids, ~kb[ids]))
    chosen = ids[order][:K]
    return np.sort(chosen).astype(np.uint32), ok, kb


def tie_straddles(kb, ok, K):
    """True when at least two eligible elements share the threshold key and the cut falls between them"""
    ids = np.nonzero(ok)[0]
    if K <= 0 or K >= len(ids):
        return False
    s = np.sort(kb[ids])[::-1]
    return bool(s[K - 1] == s[K])
