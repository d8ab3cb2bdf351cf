"""numpy float32 model of rt_temporal_accumulate (include/rt_amd.h, DESIGN.md §5.10 "Temporal accumulation"): the rule bit for bit.

Built like tests/denoise_var_model.py, whose state layout it imports: every value is np.float32, every constant an np.float32 scalar,
one rounding per operation in the order the header states, a skipped tap leaves the running sums untouched (np.where on the sum,
never a multiplication by 0).  A history is a float32 array of 5 n values: (x.r, x.g, x.b, v) [n], then neff [n].  accumulate() also
counts what happened to the pixels and taps, so that a test can assert that the cases it means to cover occurred.  Test
infrastructure only: self_check() holds the model to hand-worked cases (python tests/temporal_model.py runs it alone)."""
import numpy as np

from denoise_var_model import make_state, state_parts

F = np.float32
LAMBERTIAN = 0                     # rt_amd.h RT_MAT_LAMBERTIAN
hit_record_dtype = np.dtype([("t", "<f4"), ("p", "<f4", 3), ("normal", "<f4", 3), ("sphere", "<i4")])
camera_dtype = np.dtype([("origin", "<f4", 3), ("lower_left_corner", "<f4", 3), ("horizontal", "<f4", 3), ("vertical", "<f4", 3),
                         ("u", "<f4", 3), ("v", "<f4", 3), ("w", "<f4", 3), ("lens_radius", "<f4")])


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def history_parts(hist, n):
    """(x, v) as [n, 4] and neff [n] of a history"""
    h = np.ascontiguousarray(hist).view(np.float32).reshape(-1)
    return h[:4 * n].reshape(n, 4), h[4 * n:5 * n]


def make_history(xv, neff):
    return np.concatenate([np.asarray(xv, F).reshape(-1), np.asarray(neff, F).reshape(-1)])


def frame_values(state, hits, n):
    """x_c [n, 3], v_c [n], n [n] (float32) and which pixels are empty: the "per pixel" line of rt_denoise_adaptive"""
    S, SL, Q, k = state_parts(state, n)
    with np.errstate(all="ignore"):
        nf = k.astype(F)
        xc = S / nf[:, None]
        d = nf * Q - SL * SL
        d = np.where(d > F(0), d, F(0)).astype(F)
        vc = d / ((nf * nf) * (nf - F(1)))
    empty = (np.asarray(hits["sphere"]) == -1) | (k < 2) | ~np.isfinite(xc).all(axis=1) | ~np.isfinite(vc)
    return xc, vc, nf, empty


def reproject(P, cam, nx, ny):
    """lam, fx, fy of the points P [n, 3] through the camera `cam` (a camera_dtype record)"""
    O, LL = np.asarray(cam["origin"], F).reshape(3), np.asarray(cam["lower_left_corner"], F).reshape(3)
    H, V = np.asarray(cam["horizontal"], F).reshape(3), np.asarray(cam["vertical"], F).reshape(3)
    with np.errstate(all="ignore"):
        A = LL - O
        D = P - O
        W = np.array([H[1] * V[2] - H[2] * V[1], H[2] * V[0] - H[0] * V[2], H[0] * V[1] - H[1] * V[0]], F)
        lam = dot(D, W) / dot(A, W)
        s = (dot(D, H) / lam - dot(A, H)) / dot(H, H)
        t = (dot(D, V) / lam - dot(A, V)) / dot(V, V)
        fx = s * F(nx) - F(0.5)
        fy = t * F(ny) - F(0.5)
    assert lam.dtype == F and fx.dtype == F and fy.dtype == F
    return lam, fx, fy


def accumulate(hist_in, hits, hits_prev, cam_prev, state, kind, nx, ny, max_history, reuse_specular, position_tolerance, normal_min_dot,
               counts=None):
    """d_hist_out of rt_temporal_accumulate for host copies of its inputs (hist_in None: the first frame); kind is the world list's
    material tags (int32).  counts (a dict) receives what happened: pixels nonempty / lambertian / asked / took / took_lambertian /
    lam_reject / nan_p / off_frame / all_refused, and taps out_left / out_right / out_bottom / out_top / neff0 / sphere / normal /
    position / accepted"""
    n = nx * ny
    hits = np.asarray(hits).reshape(n)
    xc, vc, nf, empty = frame_values(state, hits, n)
    sph = np.asarray(hits["sphere"])
    kind = np.asarray(kind, np.int32)
    known = (sph >= 0) & (sph < len(kind))
    lamb = known & (kind[np.clip(sph, 0, len(kind) - 1)] == LAMBERTIAN)
    x = np.where(empty[:, None], F(0), xc).astype(F)
    v = np.where(empty, F(0), vc).astype(F)
    neff = np.where(empty, F(0), nf).astype(F)
    c = dict(nonempty=int((~empty).sum()), lambertian=int((~empty & lamb).sum()), asked=0, took=0, took_lambertian=0, lam_reject=0, nan_p=0,
             off_frame=0, all_refused=0, out_left=0, out_right=0, out_bottom=0, out_top=0, neff0=0, sphere=0, normal=0, position=0, accepted=0)
    took = np.zeros(n, bool)
    if hist_in is not None and max_history != 0:
        ask = ~empty & (lamb if not reuse_specular else True)
        xv_in, neff_in = history_parts(hist_in, n)
        prev = np.asarray(hits_prev).reshape(n)
        t = np.asarray(hits["t"], F)
        P, N = np.asarray(hits["p"], F), np.asarray(hits["normal"], F)
        Pq_all, Nq_all, sq_all = np.asarray(prev["p"], F), np.asarray(prev["normal"], F), np.asarray(prev["sphere"])
        lam, fx, fy = reproject(P, np.asarray(cam_prev).reshape(1)[0], nx, ny)
        with np.errstate(all="ignore"):
            front = lam > F(0)
            inside = (fx > F(-1)) & (fx < F(nx)) & (fy > F(-1)) & (fy < F(ny))
            land = ask & front & inside
            i0 = np.where(land, np.floor(fx), F(0)).astype(np.int64)
            j0 = np.where(land, np.floor(fy), F(0)).astype(np.int64)
            ax, ay = fx - i0.astype(F), fy - j0.astype(F)
            lim = (F(position_tolerance) * F(position_tolerance)) * (t * t)
            sg = np.zeros(n, F)
            sx = np.zeros((n, 3), F)
            sv = np.zeros(n, F)
            sn = np.zeros(n, F)
            for b in (0, 1):
                for a in (0, 1):
                    qi, qj = i0 + a, j0 + b
                    q = np.clip(qj, 0, ny - 1) * nx + np.clip(qi, 0, nx - 1)
                    in_frame = (qi >= 0) & (qi < nx) & (qj >= 0) & (qj < ny)
                    has = neff_in[q] > F(0)
                    same = sq_all[q] == sph
                    facing = dot(N, Nq_all[q]) >= F(normal_min_dot)
                    e = P - Pq_all[q]
                    near = ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) <= lim
                    c["out_left"] += int((land & (qi < 0)).sum())
                    c["out_right"] += int((land & (qi >= nx)).sum())
                    c["out_bottom"] += int((land & (qj < 0)).sum())
                    c["out_top"] += int((land & (qj >= ny)).sum())
                    live = land & in_frame
                    c["neff0"] += int((live & ~has).sum())
                    live = live & has
                    c["sphere"] += int((live & ~same).sum())
                    live = live & same
                    c["normal"] += int((live & ~facing).sum())
                    live = live & facing
                    c["position"] += int((live & ~near).sum())
                    ok = live & near
                    c["accepted"] += int(ok.sum())
                    g = (ax if a else F(1) - ax) * (ay if b else F(1) - ay)
                    sg = np.where(ok, sg + g, sg)
                    sx = np.where(ok[:, None], sx + g[:, None] * xv_in[q, :3], sx)
                    sv = np.where(ok, sv + g * xv_in[q, 3], sv)
                    sn = np.where(ok, sn + g * neff_in[q], sn)
            took = land & (sg > F(0))
            hx, hv, hn = sx / sg[:, None], sv / sg, sn / sg
            mh = F(max_history)
            m = np.where(hn < mh, hn, mh).astype(F)
            al = nf / (m + nf)
            mx = hx + al[:, None] * (xc - hx)
            mv = ((F(1) - al) * (F(1) - al)) * hv + (al * al) * vc
            x = np.where(took[:, None], mx, x)
            v = np.where(took, mv, v)
            neff = np.where(took, m + nf, neff)
        nan_p = ask & ~np.isfinite(P).all(axis=1)
        c.update(asked=int(ask.sum()), took=int(took.sum()), took_lambertian=int((took & lamb).sum()), nan_p=int(nan_p.sum()),
                 lam_reject=int((ask & ~nan_p & ~front).sum()), off_frame=int((ask & front & ~inside).sum()),
                 all_refused=int((land & ~took).sum()))
    assert x.dtype == F and v.dtype == F and neff.dtype == F
    if counts is not None:
        counts.update(c)
        counts["took_mask"] = took
    return make_history(np.concatenate([x, v[:, None]], axis=1), neff)


# ---- hand-worked cases --------------------------------------------------------------------------------------------------------------
def simple_camera():
    """origin 0, looking down -z at the square (-1, -1, -1) .. (1, 1, -1): the ray of (s, t) is (-1 + 2s, -1 + 2t, -1)"""
    cam = np.zeros(1, camera_dtype)
    cam["lower_left_corner"] = (-1, -1, -1)
    cam["horizontal"] = (2, 0, 0)
    cam["vertical"] = (0, 2, 0)
    return cam


def simple_frame(nx, ny, points, k=8, colour=1.0):
    """guides whose P are `points` [n, 3] (sphere 0, normal +z, t = |P|) and a state of k samples of `colour` each, luminance variance > 0"""
    n = nx * ny
    hits = np.zeros(n, hit_record_dtype)
    hits["p"] = np.asarray(points, F)
    hits["t"] = np.sqrt((np.asarray(points, np.float64) ** 2).sum(axis=1)).astype(F)
    hits["normal"] = (0, 0, 1)
    S = np.full((n, 3), k * colour, F)
    SL = np.full(n, 3 * k * colour, F)
    Q = np.full(n, k * (3 * colour) ** 2 + k, F)              # n*Q - SL^2 = k*k: v_c = 1 / (k - 1)
    return hits, make_state(S, SL, Q, np.full(n, k, np.int32))


def self_check():
    """hand-worked cases on a 4x4 frame behind simple_camera(): a point on a pixel centre, a point behind the camera, landing points at
    fx just under max_x and at max_x, a capped n_h, max_history 0, a specular first hit, an empty pixel.  Raises AssertionError."""
    nx = ny = 4
    n = nx * ny
    cam = simple_camera()
    j, i = np.divmod(np.arange(n), nx)
    centres = np.stack([-1 + 2 * (i + 0.5) / nx, -1 + 2 * (j + 0.5) / ny, -np.ones(n)], 1) * 2.0       # the centre rays at distance 2 along them
    hits, state = simple_frame(nx, ny, centres)
    prev = hits.copy()
    xv = np.zeros((n, 4), F)
    xv[:, :3] = F(0.5)
    xv[:, 3] = F(0.25)
    kind = np.array([LAMBERTIAN, 1], np.int32)
    args = dict(kind=kind, nx=nx, ny=ny, reuse_specular=0, position_tolerance=10.0, normal_min_dot=0.9)
    vc = F(1) / F(7)

    # 1. every point lands exactly on its own pixel centre: fx = i, ax = 0; neff_q = 8 and n = 8 give a = 1/2
    lam, fx, fy = reproject(np.asarray(hits["p"], F), cam[0], nx, ny)
    assert np.array_equal(lam, np.full(n, 2, F)) and np.array_equal(fx, i.astype(F)) and np.array_equal(fy, j.astype(F))
    c = {}
    out, neff = history_parts(accumulate(make_history(xv, np.full(n, 8, F)), hits, prev, cam, state, max_history=64, counts=c, **args), n)
    assert np.array_equal(out[:, :3], np.full((n, 3), 0.75, F)), out
    assert np.array_equal(out[:, 3], np.full(n, F(0.25) * F(0.25) + F(0.25) * vc, F))
    assert np.array_equal(neff, np.full(n, 16, F))
    assert c["took"] == n == c["asked"] and c["out_right"] == 2 * ny and c["out_top"] == 2 * nx and c["out_left"] == 0

    # 2. a point behind the previous camera: lam <= 0, this frame's values alone
    behind, _ = simple_frame(nx, ny, centres * np.array([1, 1, -1.0]))
    c = {}
    out, neff = history_parts(accumulate(make_history(xv, np.full(n, 8, F)), behind, prev, cam, state, max_history=64, counts=c, **args), n)
    assert c["lam_reject"] == n and c["took"] == 0
    assert np.array_equal(out[:, :3], np.ones((n, 3), F)) and np.array_equal(out[:, 3], np.full(n, vc, F)) and np.array_equal(neff, np.full(n, 8, F))

    # 3. fx just under max_x: s = 1.12 gives fx = 3.98, column 3 with weight 1 - ax and column 4 outside; s = 1.125 gives fx = 4: rejected
    pts = centres.copy()
    pts[:, 0] = 2.0 * (-1 + 2 * 1.12)
    edge, _ = simple_frame(nx, ny, pts)
    lam, fx, _ = reproject(np.asarray(edge["p"], F), cam[0], nx, ny)
    assert (fx > F(3.9)).all() and (fx < F(4)).all()
    c = {}
    out, neff = history_parts(accumulate(make_history(xv, np.full(n, 8, F)), edge, prev, cam, state, max_history=64, counts=c, **args), n)
    assert c["took"] == n and c["out_right"] == 2 * n and c["accepted"] == 2 * n - nx
    assert np.array_equal(out[:, :3], np.full((n, 3), 0.75, F)) and np.array_equal(neff, np.full(n, 16, F))
    pts[:, 0] = 2.0 * (-1 + 2 * 1.125)
    edge, _ = simple_frame(nx, ny, pts)
    lam, fx, _ = reproject(np.asarray(edge["p"], F), cam[0], nx, ny)
    assert np.array_equal(fx, np.full(n, 4, F))
    c = {}
    out, neff = history_parts(accumulate(make_history(xv, np.full(n, 8, F)), edge, prev, cam, state, max_history=64, counts=c, **args), n)
    assert c["off_frame"] == n and c["took"] == 0 and np.array_equal(neff, np.full(n, 8, F))

    # 4. a capped n_h: neff_q = 100 against max_history 8 is m = 8, a = 1/2, neff = 16; uncapped it is a = 8/108
    out, neff = history_parts(accumulate(make_history(xv, np.full(n, 100, F)), hits, prev, cam, state, max_history=8, **args), n)
    assert np.array_equal(out[:, :3], np.full((n, 3), 0.75, F)) and np.array_equal(neff, np.full(n, 16, F))
    out, neff = history_parts(accumulate(make_history(xv, np.full(n, 100, F)), hits, prev, cam, state, max_history=1 << 30, **args), n)
    a = F(8) / F(108)
    assert np.array_equal(neff, np.full(n, 108, F)) and np.array_equal(out[:, 0], np.full(n, F(0.5) + a * F(0.5), F))

    # 5. nothing is asked: no history, max_history 0, a specular first hit (unless reuse_specular); an empty pixel writes zeros
    first = accumulate(None, hits, None, None, state, max_history=64, **args)
    zero = accumulate(make_history(xv, np.full(n, 8, F)), hits, prev, cam, state, max_history=0, **args)
    assert np.array_equal(first, zero) and np.array_equal(history_parts(first, n)[1], np.full(n, 8, F))
    metal, prev_metal = hits.copy(), prev.copy()
    metal["sphere"] = 1
    prev_metal["sphere"] = 1
    assert np.array_equal(accumulate(make_history(xv, np.full(n, 8, F)), metal, prev_metal, cam, state, max_history=64, **args), first)
    spec = dict(args, reuse_specular=1)
    out, neff = history_parts(accumulate(make_history(xv, np.full(n, 8, F)), metal, prev_metal, cam, state, max_history=64, **spec), n)
    assert np.array_equal(neff, np.full(n, 16, F))
    sky = hits.copy()
    sky["sphere"][5] = -1
    S, SL, Q, k = (a.copy() for a in state_parts(state, n))
    k[6] = 1
    S[7, 1] = F("nan")
    out, neff = history_parts(accumulate(make_history(xv, np.full(n, 8, F)), sky, prev, cam, make_state(S, SL, Q, k), max_history=64, **args), n)
    for p in (5, 6, 7):
        assert not out[p].any() and neff[p] == 0, p
    assert (neff[[4, 8]] == 16).all()


if __name__ == "__main__":
    self_check()
    print("temporal_model: self-check passed")
