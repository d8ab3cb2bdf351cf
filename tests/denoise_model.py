"""numpy float32 model of rt_denoise (include/rt_amd.h): the filter bit for bit.

Every value is np.float32 and every constant an np.float32 scalar, so nothing is promoted to float64; numpy's float32 +, -, *, /
and sqrt are the IEEE binary32 operations the kernels perform, one rounding each, in the order the header states.  A skipped tap
leaves the running sums untouched (np.where on the sum, never a multiplication by 0: 0 * inf is NaN).  Test infrastructure only:
self_check() holds the model to a per-pixel float64 restatement of the rule before the GPU tests hold the kernels to the model
(python tests/denoise_model.py runs it alone)."""
import numpy as np

F = np.float32
K = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))
GAMMA, SUM = 0, 1


def guide_rays(cam, nx, ny):
    """rt_render_guides' pixel-centre rays (origin, direction), row-major, as an (nx*ny, 6) float32 array; cam is a camera_dtype record"""
    j, i = np.divmod(np.arange(nx * ny), nx)
    u = (i.astype(F) + F(0.5)) / F(nx)
    v = (j.astype(F) + F(0.5)) / F(ny)
    rays = np.empty((nx * ny, 6), F)
    o = np.asarray(cam["origin"], F).reshape(3)
    llc = np.asarray(cam["lower_left_corner"], F).reshape(3)
    hor = np.asarray(cam["horizontal"], F).reshape(3)
    ver = np.asarray(cam["vertical"], F).reshape(3)
    for c in range(3):
        rays[:, c] = o[c]
        rays[:, 3 + c] = ((llc[c] + u * hor[c]) + v * ver[c]) - o[c]
    return rays


def denoise(fb_in, hits, nx, ny, input, samples, levels, normal_pow_log2, sigma_position, sigma_color):
    """fb_out of rt_denoise for a host frame fb_in (nx*ny*3 float32, row-major) and host guides (hit_record_dtype, nx*ny); the
    parameters are those of rt_denoise_params, all of them explicit (the library's defaults live in the library)"""
    c = np.asarray(fb_in, F).reshape(ny, nx, 3)
    sph = np.asarray(hits["sphere"]).reshape(ny, nx)
    t = np.asarray(hits["t"], F).reshape(ny, nx)
    P = np.asarray(hits["p"], F).reshape(ny, nx, 3)
    N = np.asarray(hits["normal"], F).reshape(ny, nx, 3)
    sp, sc = F(sigma_position), F(sigma_color)
    with np.errstate(all="ignore"):
        x = c * c if input == GAMMA else c / F(samples)
        valid = (sph != -1) & np.isfinite(x).all(axis=2)
        display = c.copy() if input == GAMMA else np.sqrt(x)
        tt = t * t
        inv_sp2 = F(1) / (sp * sp) if sp > 0 else None
        for L in range(levels):
            h = 1 << L
            col = F(4 ** L) / (sc * sc) if sc > 0 else None
            sw = np.zeros((ny, nx), F)
            s = np.zeros((ny, nx, 3), F)
            for dy in range(-2, 3):
                jq = np.arange(ny) + h * dy
                in_j = (jq >= 0) & (jq < ny)
                jq = np.clip(jq, 0, ny - 1)
                for dx in range(-2, 3):
                    iq = np.arange(nx) + h * dx
                    in_i = (iq >= 0) & (iq < nx)
                    iq = np.clip(iq, 0, nx - 1)
                    sel = np.ix_(jq, iq)
                    xq, Nq, Pq = x[sel], N[sel], P[sel]
                    ok = valid & in_j[:, None] & in_i[None, :] & valid[sel] & (sph[sel] == sph)
                    wn = np.ones((ny, nx), F)
                    if normal_pow_log2 >= 0:
                        d = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
                        wn = np.where(d > F(0), d, F(0)).astype(F)
                        for _ in range(normal_pow_log2):
                            wn = wn * wn
                    apos = np.zeros((ny, nx), F)
                    if inv_sp2 is not None:
                        e = P - Pq
                        apos = (((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) / tt) * inv_sp2
                    acol = np.zeros((ny, nx), F)
                    if col is not None:
                        e = x - xq
                        acol = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) * col
                    w = ((K[dx + 2] * K[dy + 2]) * wn) / ((F(1) + apos) * (F(1) + acol))
                    sw = np.where(ok, sw + w, sw)
                    s = np.where(ok[..., None], s + w[..., None] * xq, s)
            x = np.where(valid[..., None], s / sw[..., None], x)
        out = np.where(valid[..., None], np.sqrt(x), display)
    assert out.dtype == F
    return out.reshape(-1)


def slow_reference(fb, hits, nx, ny, levels, npow, sp, sc):
    """the rule of the header restated per pixel and per tap in float64 (GAMMA input) — the float32 model must stay close to it"""
    c = fb.reshape(ny, nx, 3).astype(np.float64)
    sph, t = hits["sphere"].reshape(ny, nx), hits["t"].reshape(ny, nx).astype(np.float64)
    P, N = hits["p"].reshape(ny, nx, 3).astype(np.float64), hits["normal"].reshape(ny, nx, 3).astype(np.float64)
    x = c * c
    valid = (sph != -1) & np.isfinite(x).all(axis=2)
    k = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
    for L in range(levels):
        h = 1 << L
        y = x.copy()
        for j in range(ny):
            for i in range(nx):
                if not valid[j, i]:
                    continue
                sw, s = 0.0, np.zeros(3)
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        qj, qi = j + h * dy, i + h * dx
                        if not (0 <= qj < ny and 0 <= qi < nx) or not valid[qj, qi] or sph[qj, qi] != sph[j, i]:
                            continue
                        wn = max(float(N[j, i] @ N[qj, qi]), 0.0) ** (2 ** npow)
                        apos = float(((P[j, i] - P[qj, qi]) ** 2).sum()) / t[j, i] ** 2 / sp ** 2
                        acol = float(((x[j, i] - x[qj, qi]) ** 2).sum()) * 4 ** L / sc ** 2
                        w = k[dx + 2] * k[dy + 2] * wn / ((1 + apos) * (1 + acol))
                        sw += w
                        s += w * x[qj, qi]
                y[j, i] = s / sw
        x = y
    return np.where(valid[..., None], np.sqrt(x), c).reshape(-1)


def synthetic_frame(nx, ny, seed):
    """a noisy frame on two spheres and some sky, with guides that vary smoothly: enough to exercise every branch of the rule"""
    rng = np.random.default_rng(seed)
    hits = np.zeros(nx * ny, [("t", "<f4"), ("p", "<f4", 3), ("normal", "<f4", 3), ("sphere", "<i4")])
    j, i = np.divmod(np.arange(nx * ny), nx)
    hits["sphere"] = np.where(i < nx // 2, 0, 7)
    hits["sphere"][(j == ny - 1) & (i % 3 == 0)] = -1
    hits["t"] = (2.0 + 0.05 * i + 0.02 * j).astype(np.float32)
    hits["p"] = np.stack([0.1 * i, 0.05 * j, np.sin(0.3 * i)], 1).astype(np.float32)
    n = np.stack([np.sin(0.2 * i), np.cos(0.2 * i), 0.1 * np.ones(nx * ny)], 1)
    hits["normal"] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    fb = rng.uniform(0.0, 1.0, nx * ny * 3).astype(np.float32)
    return fb, hits


def self_check():
    """the model against slow_reference on a small synthetic frame (three weight settings, a NaN pixel and sky): finite where the
    restatement is finite and close to it, and the pass-through pixels keep their exact input bits.  Raises AssertionError."""
    nx, ny = 23, 11
    fb, hits = synthetic_frame(nx, ny, 5)
    fb[3 * 40 + 1] = np.float32("nan")                             # a pass-through pixel that is not sky
    for levels, npow, sp, sc in ((1, 5, 0.05, 0.5), (3, 2, 0.3, 0.2), (2, 7, 1.0, 2.0)):
        got = denoise(fb, hits, nx, ny, GAMMA, 1, levels, npow, sp, sc)
        ref = slow_reference(fb, hits, nx, ny, levels, npow, sp, sc)
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(got))
        assert np.allclose(got[fin], ref[fin], rtol=2e-5, atol=1e-6), (levels, npow, sp, sc)
    got = denoise(fb, hits, nx, ny, GAMMA, 1, 2, 4, 0.01, 0.3)
    keep = np.repeat((hits["sphere"] == -1) | (np.arange(nx * ny) == 40), 3)
    assert np.array_equal(got[keep].view(np.uint32), fb[keep].view(np.uint32))
    assert not np.array_equal(got[~keep], fb[~keep])
    assert np.isfinite(got[~keep]).all()


if __name__ == "__main__":
    self_check()
    print("denoise_model: self-check passed")
