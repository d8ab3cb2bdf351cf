"""numpy float32 model of rt_denoise_adaptive (include/rt_amd.h): the variance-guided filter bit for bit.

Built like tests/denoise_model.py, whose kernel K, float type and synthetic guides it imports: every value is np.float32, every
constant an np.float32 scalar, one rounding per operation in the order the header states, a skipped tap leaves the running sums
untouched (np.where on the sum, never a multiplication by 0).  Test infrastructure only: self_check() holds the model to a per-pixel
float64 restatement of the rule before the GPU tests hold the kernels to the model (python tests/denoise_var_model.py runs it alone)."""
import numpy as np

from denoise_model import F, K, synthetic_frame

K3 = (F(0.25), F(0.5), F(0.25))
EPS = F(1e-8)                      # rt_amd.h RT_DENOISE_VAR_EPS


def state_parts(state, n):
    """the state's structure of arrays: S_rgb [n, 3], SL [n], Q [n] (float32), k [n] (int32); state is a byte array"""
    s = np.ascontiguousarray(state).view(np.uint8)
    f = s.view(np.float32)
    return f[:3 * n].reshape(n, 3), f[3 * n:4 * n], f[4 * n:5 * n], s.view(np.int32)[5 * n:6 * n]


def make_state(S, SL, Q, k):
    """the bytes of a whole-frame state from its four arrays"""
    n = len(k)
    out = np.empty(6 * n, np.float32)
    out[:3 * n] = np.asarray(S, np.float32).reshape(-1)
    out[3 * n:4 * n] = SL
    out[4 * n:5 * n] = Q
    out[5 * n:].view(np.int32)[:] = k
    return out.view(np.uint8)


def shifted(n, step):
    """indices of the row or column `step` further on, clipped to the frame, and which of them lie inside it"""
    q = np.arange(n) + step
    return np.clip(q, 0, n - 1), (q >= 0) & (q < n)


def denoise_adaptive(fb_in, hits, state, nx, ny, levels, normal_pow_log2, prefilter, sigma_position, sigma_variance):
    """fb_out of rt_denoise_adaptive for a host frame fb_in (nx*ny*3 float32, row-major), host guides (hit_record_dtype, nx*ny) and
    the host copy of the whole-frame state; the parameters are those of rt_denoise_var_params, all of them explicit"""
    n = nx * ny
    c = np.asarray(fb_in, F).reshape(ny, nx, 3)
    S, SL, Q, k = state_parts(state, n)
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
        for L in range(levels):
            h = 1 << L
            lum = (x[..., 0] + x[..., 1]) + x[..., 2]
            vb = v
            if prefilter:
                sg = np.zeros((ny, nx), F)
                sgv = np.zeros((ny, nx), F)
                for dy in range(-1, 2):
                    jq, in_j = shifted(ny, dy)
                    for dx in range(-1, 2):
                        iq, in_i = shifted(nx, dx)
                        sel = np.ix_(jq, iq)
                        ok = valid & in_j[:, None] & in_i[None, :] & valid[sel] & (sph[sel] == sph)
                        g = K3[dx + 1] * K3[dy + 1]
                        sg = np.where(ok, sg + g, sg)
                        sgv = np.where(ok, sgv + g * v[sel], sgv)
                vb = sgv / sg
            den = (sv2 * vb + EPS) if sv2 is not None else None
            sw = np.zeros((ny, nx), F)
            s = np.zeros((ny, nx, 3), F)
            s3 = np.zeros((ny, nx), F)
            for dy in range(-2, 3):
                jq, in_j = shifted(ny, h * dy)
                for dx in range(-2, 3):
                    iq, in_i = shifted(nx, h * dx)
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
            x = np.where(valid[..., None], s / sw[..., None], x)
            v = np.where(valid, s3 / (sw * sw), v)
        out = np.where(valid[..., None], np.sqrt(x), c)
    assert out.dtype == F and x.dtype == F and v.dtype == F
    return out.reshape(-1)


def slow_reference(fb, hits, state, nx, ny, levels, npow, prefilter, sp, sv):
    """the rule of the header restated per pixel and per tap in float64 — the float32 model must stay close to it"""
    n = nx * ny
    S, SL, Q, k = state_parts(state, n)
    sph, t = hits["sphere"].reshape(ny, nx), hits["t"].reshape(ny, nx).astype(np.float64)
    P, N = hits["p"].reshape(ny, nx, 3).astype(np.float64), hits["normal"].reshape(ny, nx, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        nf = k.astype(np.float64)
        x = (S.astype(np.float64) / nf[:, None]).reshape(ny, nx, 3)
        # the clamp is decided in binary32, as the rule states it: a d that rounds below 0 there is 0 here too
        nf32 = k.astype(F)
        neg = ~((nf32 * Q - SL * SL) > 0)
        d = nf * Q.astype(np.float64) - SL.astype(np.float64) ** 2
        d[neg] = 0.0
        v = (d / (nf * nf * (nf - 1))).reshape(ny, nx)
        valid = (sph != -1) & (k.reshape(ny, nx) >= 2) & np.isfinite(x.astype(F)).all(axis=2) & np.isfinite(v.astype(F))
    k5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
    k3 = (1 / 4, 1 / 2, 1 / 4)

    def tap(j, i, qj, qi):
        return 0 <= qj < ny and 0 <= qi < nx and valid[qj, qi] and sph[qj, qi] == sph[j, i]

    for L in range(levels):
        h = 1 << L
        y, vy = x.copy(), v.copy()
        for j in range(ny):
            for i in range(nx):
                if not valid[j, i]:
                    continue
                vb = v[j, i]
                if prefilter:
                    sg = sgv = 0.0
                    for dy in range(-1, 2):
                        for dx in range(-1, 2):
                            if tap(j, i, j + dy, i + dx):
                                sg += k3[dx + 1] * k3[dy + 1]
                                sgv += k3[dx + 1] * k3[dy + 1] * v[j + dy, i + dx]
                    vb = sgv / sg
                sw, s, s3 = 0.0, np.zeros(3), 0.0
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        qj, qi = j + h * dy, i + h * dx
                        if not tap(j, i, qj, qi):
                            continue
                        wn = max(float(N[j, i] @ N[qj, qi]), 0.0) ** (2 ** npow) if npow >= 0 else 1.0
                        apos = float(((P[j, i] - P[qj, qi]) ** 2).sum()) / t[j, i] ** 2 / sp ** 2 if sp > 0 else 0.0
                        avar = (x[j, i].sum() - x[qj, qi].sum()) ** 2 / (sv ** 2 * vb + 1e-8) if sv > 0 else 0.0
                        w = k5[dx + 2] * k5[dy + 2] * wn / ((1 + apos) * (1 + avar))
                        sw += w
                        s += w * x[qj, qi]
                        s3 += w * w * v[qj, qi]
                y[j, i] = s / sw
                vy[j, i] = s3 / (sw * sw)
        x, v = y, vy
    c = fb.reshape(ny, nx, 3).astype(np.float64)
    return np.where(valid[..., None], np.sqrt(x), c).reshape(-1), valid


def synthetic_state(nx, ny, seed):
    """a synthetic adaptive frame on denoise_model's guides: per-pixel k that differ, sums of k noisy samples around a smooth colour,
    the gamma frame they give, and five special pixels (returned by name) — sky comes with the guides"""
    rng = np.random.default_rng(seed)
    _, hits = synthetic_frame(nx, ny, seed)
    n = nx * ny
    j, i = np.divmod(np.arange(n), nx)
    k = rng.choice(np.array([4, 8, 12, 16, 64], np.int32), n)
    base = np.stack([0.4 + 0.3 * np.sin(0.2 * i), 0.5 + 0.2 * np.cos(0.3 * j), 0.3 + 0.01 * i], 1)
    S = np.zeros((n, 3), F)
    SL = np.zeros(n, F)
    Q = np.zeros(n, F)
    for s in range(int(k.max())):
        live = s < k
        col = (base * rng.uniform(0.5, 1.5, (n, 1))).astype(F)
        lum = (col[:, 0] + col[:, 1]) + col[:, 2]
        S[live] = S[live] + col[live]
        SL[live] = SL[live] + lum[live]
        Q[live] = Q[live] + (lum * lum)[live]
    special = dict(nan=40, k1=57, neg=93, inf=120, zero=101)
    S[special["nan"], 1] = F("nan")                               # a NaN sample colour: pass-through, not sky
    k[special["k1"]] = 1                                          # one sample: no variance
    S[special["inf"], 2] = F("inf")
    # identical samples: n*Q - SL*SL is 0 in exact arithmetic and rounds below 0 in binary32 for this luminance
    p = special["neg"]
    k[p] = 12
    lum = F(1.1)
    SL[p], Q[p] = F(0), F(0)
    for _ in range(12):
        SL[p] = SL[p] + lum
        Q[p] = Q[p] + lum * lum
    S[p] = SL[p] / F(3)
    assert F(12) * Q[p] - SL[p] * SL[p] < 0, "the synthetic pixel must exercise the clamp of d"
    # a converged pixel: variance exactly 0 (the epsilon keeps its centre tap from 0 / 0)
    p = special["zero"]
    k[p] = 4
    SL[p], Q[p], S[p] = F(2), F(1), F(2) / F(3)
    for name, p in special.items():
        assert hits["sphere"][p] != -1, name
    with np.errstate(all="ignore"):
        fb = np.sqrt(S / k.astype(F)[:, None]).astype(F).reshape(-1)
    return fb, hits, make_state(S, SL, Q, k), special


def self_check():
    """the model against slow_reference on a synthetic frame that contains sky, a NaN pixel, an Inf pixel, a k = 1 pixel, a pixel whose
    d rounds below 0, a pixel of variance 0 and per-pixel k that differ: finite where the restatement is finite and close to it, and the
    pass-through pixels keep their exact input bits.  Raises AssertionError."""
    nx, ny = 23, 11
    fb, hits, state, special = synthetic_state(nx, ny, 5)
    k = state_parts(state, nx * ny)[3]
    assert len(np.unique(k)) >= 5 and (hits["sphere"] == -1).any()
    keep = hits["sphere"] == -1
    for name in ("nan", "k1", "inf"):
        keep[special[name]] = True
    for levels, npow, pre, sp, sv in ((1, 5, 1, 0.05, 2.0), (3, 2, 0, 0.3, 4.0), (2, 7, 1, 1.0, 8.0), (2, -1, 1, 0.0, 0.0), (4, 4, 0, 0.0, 1.0)):
        got = denoise_adaptive(fb, hits, state, nx, ny, levels, npow, pre, sp, sv)
        ref, valid = slow_reference(fb, hits, state, nx, ny, levels, npow, pre, sp, sv)
        assert np.array_equal(~valid.reshape(-1), keep)
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(got))
        assert np.allclose(got[fin], ref[fin], rtol=1e-4, atol=1e-5), (levels, npow, pre, sp, sv, np.abs(got[fin] - ref[fin]).max())
        k3 = np.repeat(keep, 3)
        assert np.array_equal(got[k3].view(np.uint32), fb[k3].view(np.uint32))
        assert np.isfinite(got[~k3]).all()
        assert not np.array_equal(got[~k3], fb[~k3])
    # the variance term does something, and so does the prefilter
    a = denoise_adaptive(fb, hits, state, nx, ny, 2, 4, 1, 0.01, 2.0)
    assert not np.array_equal(a, denoise_adaptive(fb, hits, state, nx, ny, 2, 4, 1, 0.01, 0.0))
    assert not np.array_equal(a, denoise_adaptive(fb, hits, state, nx, ny, 2, 4, 0, 0.01, 2.0))


if __name__ == "__main__":
    self_check()
    print("denoise_var_model: self-check passed")
