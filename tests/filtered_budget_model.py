"""numpy float32 model of the filter-aware budget key (include/rt_amd.h "Filter-aware budgets"): level 0 of
rt_denoise_adaptive on the state — the filtered mean y and the variance v' of that mean — the key of a filtered pixel one operation
per line, the keys of a frame (pass-through pixels keep the raw key of adaptive_budget_model) and the selection by lexsort.

Built like tests/denoise_var_model.py and tied to it: self_check() holds sqrt(y) to denoise_var_model.denoise_adaptive(levels=1) bit
for bit, and the key to a per-pixel float64 restatement (python tests/filtered_budget_model.py runs it alone)."""
import numpy as np

import adaptive_budget_model as B
import denoise_var_model as V
from denoise_model import F, K

WHOLE = (0, 1, 0, 0)


def level0(hits, state, nx, ny, normal_pow_log2, prefilter, sigma_position, sigma_variance):
    """(y [ny, nx, 3], v' [ny, nx], valid [ny, nx]) of level L = 0 (step 1) of rt_denoise_adaptive; y and v' hold the level's input
    (x, v) where valid is False — a pass-through pixel"""
    n = nx * ny
    S, SL, Q, k = V.state_parts(state, n)
    sph = np.asarray(hits["sphere"]).reshape(ny, nx)
    t = np.asarray(hits["t"], F).reshape(ny, nx)
    P = np.asarray(hits["p"], F).reshape(ny, nx, 3)
    N = np.asarray(hits["normal"], F).reshape(ny, nx, 3)
    sp, sv = F(sigma_position), F(sigma_variance)
    with np.errstate(all="ignore"):
        nf = k.astype(F)
        x = (S / nf[:, None]).reshape(ny, nx, 3)
        d = nf * Q - SL * SL
        d = np.where(d > F(0), d, F(0)).astype(F)
        v = (d / ((nf * nf) * (nf - F(1)))).reshape(ny, nx)
        valid = (sph != -1) & (k.reshape(ny, nx) >= 2) & np.isfinite(x).all(axis=2) & np.isfinite(v)
        tt = t * t
        inv_sp2 = F(1) / (sp * sp) if sp > 0 else None
        sv2 = sv * sv if sv > 0 else None
        lum = (x[..., 0] + x[..., 1]) + x[..., 2]
        vb = v
        if prefilter:
            sg = np.zeros((ny, nx), F)
            sgv = np.zeros((ny, nx), F)
            for dy in range(-1, 2):
                jq, in_j = V.shifted(ny, dy)
                for dx in range(-1, 2):
                    iq, in_i = V.shifted(nx, dx)
                    sel = np.ix_(jq, iq)
                    ok = valid & in_j[:, None] & in_i[None, :] & valid[sel] & (sph[sel] == sph)
                    g = V.K3[dx + 1] * V.K3[dy + 1]
                    sg = np.where(ok, sg + g, sg)
                    sgv = np.where(ok, sgv + g * v[sel], sgv)
            vb = sgv / sg
        den = (sv2 * vb + V.EPS) if sv2 is not None else None
        sw = np.zeros((ny, nx), F)
        s = np.zeros((ny, nx, 3), F)
        s3 = np.zeros((ny, nx), F)
        for dy in range(-2, 3):
            jq, in_j = V.shifted(ny, dy)
            for dx in range(-2, 3):
                iq, in_i = V.shifted(nx, dx)
                sel = np.ix_(jq, iq)
                xq, Nq, Pq = x[sel], N[sel], P[sel]
                ok = valid & in_j[:, None] & in_i[None, :] & valid[sel] & (sph[sel] == sph)
                wn = np.ones((ny, nx), F)
                if normal_pow_log2 >= 0:
                    dn = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
                    wn = np.where(dn > F(0), dn, F(0)).astype(F)
                    for _ in range(normal_pow_log2):
                        wn = wn * wn
                apos = np.zeros((ny, nx), F)
                if inv_sp2 is not None:
                    e = P - Pq
                    apos = (((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) / tt) * inv_sp2
                avar = np.zeros((ny, nx), F)
                if den is not None:
                    dl = lum - lum[sel]
                    avar = (dl * dl) / den
                w = ((K[dx + 2] * K[dy + 2]) * wn) / ((F(1) + apos) * (F(1) + avar))
                sw = np.where(ok, sw + w, sw)
                s = np.where(ok[..., None], s + w[..., None] * xq, s)
                s3 = np.where(ok, s3 + (w * w) * v[sel], s3)
        y = np.where(valid[..., None], s / sw[..., None], x)
        vy = np.where(valid, s3 / (sw * sw), v)
    assert y.dtype == F and vy.dtype == F
    return y, vy, valid


def priority_filtered(l, v, floor):
    """rt_adaptive_priority_filtered for arrays (or scalars): float32 in, float32 out, one rounding per operation"""
    l = np.asarray(l, np.float32)
    v = np.asarray(v, np.float32)
    floor = np.float32(floor)
    with np.errstate(all="ignore"):
        m = np.where(l > floor, l, floor)                     # a NaN l takes the floor
        mm = m * m
        e = v / mm
        key = np.where(e > 0, e, np.float32(0))               # NaN becomes 0, +inf stays
    return key.astype(np.float32)


def frame_keys(hits, state, nx, ny, floor, normal_pow_log2, prefilter, sigma_position, sigma_variance):
    """the key of every pixel (float32 [nx * ny], before the eligibility mask) and which pixels the filter touches"""
    n = nx * ny
    y, vy, valid = level0(hits, state, nx, ny, normal_pow_log2, prefilter, sigma_position, sigma_variance)
    _, SL, Q, k = V.state_parts(state, n)
    with np.errstate(all="ignore"):
        l = (y[..., 0] + y[..., 1]) + y[..., 2]
    filtered = priority_filtered(l, vy, floor).reshape(-1)
    raw = B.priority(SL, Q, k, floor)
    valid = valid.reshape(-1)
    return np.where(valid, filtered, raw).astype(np.float32), valid


def select(hits, state, nx, ny, batch, max_spp, floor, K_picks, filt):
    """the sorted ids of the first min(K, eligible) eligible pixels by key descending, id ascending; the mask, the key bits before the
    mask; filt = (normal_pow_log2, prefilter, sigma_position, sigma_variance)"""
    n = nx * ny
    key, _ = frame_keys(hits, state, nx, ny, floor, *filt)
    kb = B.keybits(key)
    k = V.state_parts(state, n)[3]
    ok = (k.astype(np.int64) + batch <= max_spp) & (kb > 0)
    return pick(ok, kb, K_picks), ok, kb


def pick(ok, kb, K_picks):
    """the sorted ids of the first min(K, eligible) pixels of the mask by key bits descending, id ascending"""
    ids = np.nonzero(ok)[0].astype(np.int64)
    order = np.lexsort((ids, ~kb[ids]))
    return np.sort(ids[order][:K_picks]).astype(np.uint32)


def slow_keys(hits, state, nx, ny, floor, normal_pow_log2, prefilter, sigma_position, sigma_variance):
    """the rule restated per pixel in float64 on the level-0 values of the model: key = v' / max(l, floor)^2"""
    y, vy, valid = level0(hits, state, nx, ny, normal_pow_log2, prefilter, sigma_position, sigma_variance)
    out = np.zeros(nx * ny)
    y64, v64 = y.reshape(-1, 3).astype(np.float64), vy.reshape(-1).astype(np.float64)
    for p in np.nonzero(valid.reshape(-1))[0]:
        l = float(np.float32(np.float32(y.reshape(-1, 3)[p, 0] + y.reshape(-1, 3)[p, 1]) + y.reshape(-1, 3)[p, 2]))
        m = max(l, float(np.float32(floor)))
        out[p] = v64[p] / (m * m) if m > 0 else (np.inf if v64[p] > 0 else 0.0)
        assert abs(l - y64[p].sum()) <= 1e-6 * abs(l)
    return out, valid.reshape(-1)


def self_check():
    """level 0 against denoise_var_model (bit for bit through sqrt), the key against the float64 restatement, pass-through pixels
    against the raw rule — on the synthetic state that holds sky, NaN, Inf, k = 1, a clamped d and a zero variance.  Raises
    AssertionError."""
    nx, ny = 23, 11
    n = nx * ny
    for seed in (5, 11):
        fb, hits, state, special = V.synthetic_state(nx, ny, seed)
        _, SL, Q, k = V.state_parts(state, n)
        keep = hits["sphere"] == -1
        for name in ("nan", "k1", "inf"):
            keep[special[name]] = True
        for npow, pre, sp, sv in ((4, 1, 0.01, 4.0), (5, 1, 0.05, 2.0), (2, 0, 0.3, 4.0), (-1, 1, 0.0, 0.0), (4, 0, 0.0, 1.0)):
            y, vy, valid = level0(hits, state, nx, ny, npow, pre, sp, sv)
            assert np.array_equal(~valid.reshape(-1), keep)
            ref = V.denoise_adaptive(fb, hits, state, nx, ny, 1, npow, pre, sp, sv).reshape(-1, 3)
            with np.errstate(all="ignore"):
                got = np.sqrt(y).reshape(-1, 3)
            vm = valid.reshape(-1)
            assert np.array_equal(got[vm].view(np.uint32), ref[vm].view(np.uint32)), (seed, npow, pre, sp, sv)
            assert np.isfinite(vy[valid]).all() and (vy[valid] >= 0).all()
            for floor in (0.02, 0.0, 5.0):
                key, v2 = frame_keys(hits, state, nx, ny, floor, npow, pre, sp, sv)
                assert key.dtype == np.float32 and np.array_equal(v2, vm)
                slow, _ = slow_keys(hits, state, nx, ny, floor, npow, pre, sp, sv)
                assert np.allclose(key[vm], slow[vm], rtol=1e-6, atol=0.0), (seed, floor)
                assert np.array_equal(key[~vm].view(np.uint32), B.priority(SL, Q, k, floor)[~vm].view(np.uint32))
                assert not np.isnan(key).any() and (B.keybits(key) < 0x80000000).all()
            # the filter lowers the error of most pixels it touches: the key is a different ordering, not the raw one
            key, _ = frame_keys(hits, state, nx, ny, 0.02, npow, pre, sp, sv)
            raw = B.priority(SL, Q, k, 0.02)
            assert (key[vm] < raw[vm]).mean() > 0.5
            assert key[special["zero"]] >= 0 and raw[special["zero"]] == 0
    # the selection is a plain sort: K = 0, one, all
    fb, hits, state, special = V.synthetic_state(nx, ny, 5)
    filt = (4, 1, 0.01, 4.0)
    chosen, ok, kb = select(hits, state, nx, ny, 4, 64, 0.02, 10 ** 9, filt)
    assert np.array_equal(chosen, np.nonzero(ok)[0]) and 0 < ok.sum() < n
    assert len(select(hits, state, nx, ny, 4, 64, 0.02, 0, filt)[0]) == 0
    one = select(hits, state, nx, ny, 4, 64, 0.02, 1, filt)[0]
    assert len(one) == 1 and kb[one[0]] == kb[ok].max()


if __name__ == "__main__":
    self_check()
    print("filtered_budget_model: self-check passed")
