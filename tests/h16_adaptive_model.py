"""The numpy model of adaptive sampling for binary16 worlds (include/rt_amd_h16_adaptive.h, DESIGN.md §5.9 "Binary16"), for the CPU
and the GPU tests.  Per sample: the colour sum in binary16 (one rounding of the exact sum), the luminance l = ((float)c.x + (float)c.y)
+ (float)c.z and the sums SL, Q in binary32, one rounding per operation; at the checkpoints adapt_rule's arithmetic; at a pixel's end
rt_render's colour for ns = k: real_t(1.0 / (double)float(real_t(k))), the product and the root each rounded once to binary16.
numpy only."""
import numpy as np

F = np.float32
H = np.float16


def bits16(a):
    """the binary16 patterns of an array of binary16 values (float16, or float32 / float64 images of them)"""
    return np.ascontiguousarray(a).astype(H).view(np.uint16)


def add16(col, c):
    """col + c with ONE rounding to binary16 of the exact sum (binary64 holds it); numpy's own float16 addition gives the same bits"""
    with np.errstate(over="ignore", invalid="ignore"):
        s = (col.astype(np.float64) + c.astype(np.float64)).astype(H)
        own = col + c
    assert np.array_equal(s.view(np.uint16), own.view(np.uint16)) or np.isnan(s).any()
    return s


def end_colour(col, k):
    """what k_render_h MODE 0 writes for the binary16 sums col [n, 3] after ns = k samples (k: a scalar or [n]); float16"""
    kh = np.asarray(k, F).astype(H)                                     # real_t(k)
    scale = F(1.0) / kh.astype(F).astype(np.float64)                    # 1.0 / (double)float(real_t(k))
    scale = scale.astype(F).astype(H)                                   # real_t(double): double -> float -> binary16
    if scale.ndim:
        scale = scale[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt((col * scale).astype(F)).astype(H)


def rule(SL, Q, k, rel_error, floor):
    """adapt_rule (csrc/rt_adapt_rule.h) on arrays of binary32 sums after k samples"""
    rel, fl, n = F(rel_error), F(floor), F(k)
    if not rel > 0:
        return np.zeros(SL.shape, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        d = n * Q - SL * SL
        nf = n * fl
        m = np.where(SL > nf, SL, nf)
        return d <= ((rel * rel) * (n - F(1))) * (m * m)


def run(samples, rel_error, floor, lo, step, hi):
    """samples [>= hi, n, 3]: the per-sample colours (float32 images of binary16 values, zero for an absorbed path).  Every pixel of the
    frame rt_render_adaptive_h16((lo, hi, step, rel_error, floor)) leaves: spp [n] int32, fb [n, 3] float16, and the state's S [n, 3]
    (float32 images of the binary16 sums), SL, Q [n] float32 at the pixel's end."""
    n = samples.shape[1]
    col = np.zeros((n, 3), H)
    SL, Q = np.zeros(n, F), np.zeros(n, F)
    out = dict(spp=np.zeros(n, np.int32), fb=np.zeros((n, 3), H), S=np.zeros((n, 3), F), SL=np.zeros(n, F), Q=np.zeros(n, F))
    for k in range(1, hi + 1):
        c = samples[k - 1].astype(F)
        assert np.array_equal(c.astype(H).astype(F), c), "the samples are binary16 values"
        col = add16(col, c.astype(H))
        with np.errstate(invalid="ignore", over="ignore"):
            l = (c[:, 0] + c[:, 1]) + c[:, 2]
            SL = SL + l
            Q = Q + l * l
        if k < lo or (k - lo) % step:
            continue
        stop = (out["spp"] == 0) & (rule(SL, Q, k, rel_error, floor) | (k == hi))
        out["fb"][stop] = end_colour(col[stop], k)
        out["S"][stop] = col[stop].astype(F)
        out["SL"][stop], out["Q"][stop] = SL[stop], Q[stop]
        out["spp"][stop] = k
    return out


def mixed(spp, hi):
    """the condition of a frame that says something: >= 3 distinct counts, an early stop, a capped pixel"""
    return len(np.unique(spp)) >= 3 and bool((spp < hi).any()) and bool((spp == hi).any())


SWEEP = (0.02, 0.03, 0.05, 0.07, 0.1, 0.15, 0.2, 0.3, 0.5)


def mixed_targets(samples, lo, step, hi, floor):
    """the targets of the sweep whose frames are mixed (adaptive_frames.pick_rel_error's sweep and condition, on this model), from the
    loosest down: a later one refines an earlier one"""
    return [rel for rel in reversed(SWEEP) if mixed(run(samples, rel, floor, lo, step, hi)["spp"], hi)]


def pick_rel_error(samples, lo, step, hi, floor):
    """the first target of the sweep, from the tightest up, whose frame is mixed"""
    ok = mixed_targets(samples, lo, step, hi, floor)
    assert ok, "no rel_error in the sweep gives a mixed frame"
    return ok[-1]
