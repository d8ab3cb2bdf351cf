"""numpy float32 model of rt_temporal_accumulate_rectified (include/rt_amd.h, DESIGN.md §5.10 "History rectification"): the rule bit
for bit.

Built on tests/temporal_model.py and tests/temporal_moving_model.py, both imported unchanged.  What the unrectified call writes comes
from their accumulate(): every pixel that took no history keeps exactly those values.  For the pixels that took history this module
gathers the history once more (gather(): temporal_model's four taps without the bookkeeping — with gamma 0 the result must equal the
parent models bit for bit, which tests/test_temporal_rectify_host.py asserts on random inputs), computes the window statistics of
THIS frame, scales m and merges.  The moving rule enters as in temporal_moving_model: the gather runs on guides whose p fields hold P',
and a pixel whose sphere changed its radius took nothing.  Every value is np.float32, one rounding per operation in the order the header
states, a skipped window pixel leaves the running sums untouched.  accumulate_rectified() counts what happened.  Test infrastructure
only: self_check() holds the model to the hand-worked cases of hand_cases() (python tests/temporal_rectify_model.py runs it alone)."""
import numpy as np

import temporal_model as tm
import temporal_moving_model as tmm
from denoise_var_model import make_state

F = tm.F


def gather(hist_in, hits, hits_prev, cam_prev, nx, ny, position_tolerance, normal_min_dot):
    """sg [n], x_h [n, 3], v_h [n], n_h [n] and the landing mask of every pixel, asked or not: the "where it was" and "four taps" lines"""
    n = nx * ny
    hits = np.asarray(hits).reshape(n)
    prev = np.asarray(hits_prev).reshape(n)
    xv_in, neff_in = tm.history_parts(hist_in, n)
    sph = np.asarray(hits["sphere"])
    t = np.asarray(hits["t"], F)
    P, N = np.asarray(hits["p"], F), np.asarray(hits["normal"], F)
    Pq_all, Nq_all, sq_all = np.asarray(prev["p"], F), np.asarray(prev["normal"], F), np.asarray(prev["sphere"])
    lam, fx, fy = tm.reproject(P, np.asarray(cam_prev).reshape(1)[0], nx, ny)
    with np.errstate(all="ignore"):
        land = (lam > F(0)) & (fx > F(-1)) & (fx < F(nx)) & (fy > F(-1)) & (fy < F(ny))
        i0 = np.where(land, np.floor(fx), F(0)).astype(np.int64)
        j0 = np.where(land, np.floor(fy), F(0)).astype(np.int64)
        ax, ay = fx - i0.astype(F), fy - j0.astype(F)
        lim = (F(position_tolerance) * F(position_tolerance)) * (t * t)
        sg, sx, sv, sn = np.zeros(n, F), np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F)
        for b in (0, 1):
            for a in (0, 1):
                qi, qj = i0 + a, j0 + b
                q = np.clip(qj, 0, ny - 1) * nx + np.clip(qi, 0, nx - 1)
                e = P - Pq_all[q]
                ok = (land & (qi >= 0) & (qi < nx) & (qj >= 0) & (qj < ny) & (neff_in[q] > F(0)) & (sq_all[q] == sph)
                      & (tm.dot(N, Nq_all[q]) >= F(normal_min_dot)) & (((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) <= lim))
                g = (ax if a else F(1) - ax) * (ay if b else F(1) - ay)
                sg = np.where(ok, sg + g, sg)
                sx = np.where(ok[:, None], sx + g[:, None] * xv_in[q, :3], sx)
                sv = np.where(ok, sv + g * xv_in[q, 3], sv)
                sn = np.where(ok, sn + g * neff_in[q], sn)
        hx, hv, hn = sx / sg[:, None], sv / sg, sn / sg
    return sg, hx, hv, hn, land


def window(state, hits, nx, ny, radius, counted=None, counts=None):
    """cnt, ml, s2 [n] of this frame's (2 radius + 1)^2 windows: "the window", "first pass" and "second pass"; counts receives the
    skipped taps of the pixels in the mask `counted`: taps_outside / taps_empty / taps_sphere, and taps_accepted"""
    n = nx * ny
    hits = np.asarray(hits).reshape(n)
    xc, _, _, empty = tm.frame_values(state, hits, n)
    with np.errstate(all="ignore"):
        l = (xc[:, 0] + xc[:, 1]) + xc[:, 2]
    sph = np.asarray(hits["sphere"])
    j, i = np.divmod(np.arange(n), nx)
    offsets = [(dx, dy) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]
    c = dict(taps_outside=0, taps_empty=0, taps_sphere=0, taps_accepted=0)
    cnt, s1, oks, lqs = np.zeros(n, F), np.zeros(n, F), [], []
    with np.errstate(all="ignore"):
        for dx, dy in offsets:
            qi, qj = i + dx, j + dy
            inside = (qi >= 0) & (qi < nx) & (qj >= 0) & (qj < ny)
            q = np.clip(qj, 0, ny - 1) * nx + np.clip(qi, 0, nx - 1)
            ok = inside & ~empty[q] & (sph[q] == sph)
            if counted is not None:
                c["taps_outside"] += int((counted & ~inside).sum())
                c["taps_empty"] += int((counted & inside & empty[q]).sum())
                c["taps_sphere"] += int((counted & inside & ~empty[q] & (sph[q] != sph)).sum())
                c["taps_accepted"] += int((counted & ok).sum())
            cnt = np.where(ok, cnt + F(1), cnt)
            s1 = np.where(ok, s1 + l[q], s1)
            oks.append(ok)
            lqs.append(l[q])
        ml = s1 / cnt
        ss = np.zeros(n, F)
        for ok, lq in zip(oks, lqs):
            ss = np.where(ok, ss + (lq - ml) * (lq - ml), ss)
        s2 = ss / (cnt - F(1))
    assert cnt.dtype == F and ml.dtype == F and s2.dtype == F
    if counts is not None:
        counts.update(c)
    return cnt, ml, s2


def accumulate_rectified(hist_in, hits, hits_prev, cam_prev, state, kind, nx, ny, max_history, reuse_specular, position_tolerance,
                         normal_min_dot, radius, min_count, gamma, geom=None, geom_prev=None, counts=None):
    """d_hist_out of rt_temporal_accumulate_rectified for host copies of its inputs.  geom_prev None: the static rule; given (with
    geom, this frame's geometry): the moving rule.  counts receives the parent model's counts and: rectified (pixels whose m was
    scaled), kept_min_count (pixels with history whose window held fewer than min_count pixels), kept_within (tested, e2 <= lim or a
    NaN), taps_outside / taps_empty / taps_sphere / taps_accepted (window taps of the pixels that took history), the masks took_mask
    and rectified_mask, and neff_unrectified [n]"""
    n = nx * ny
    moving = geom_prev is not None and hist_in is not None
    c = {}
    if moving:
        base = tmm.accumulate_moving(hist_in, hits, hits_prev, cam_prev, geom, geom_prev, state, kind, nx, ny, max_history, reuse_specular,
                                     position_tolerance, normal_min_dot, counts=c)
    else:
        base = tm.accumulate(hist_in, hits, hits_prev, cam_prev, state, kind, nx, ny, max_history, reuse_specular, position_tolerance,
                             normal_min_dot, counts=c)
    took = c["took_mask"]
    xb, nb = tm.history_parts(base, n)
    x, v, neff = xb[:, :3].copy(), xb[:, 3].copy(), nb.copy()
    extra = dict(rectified=0, kept_min_count=0, kept_within=0, taps_outside=0, taps_empty=0, taps_sphere=0, taps_accepted=0,
                 rectified_mask=np.zeros(n, bool), neff_unrectified=nb.copy())
    if took.any():
        guides = tmm.patched_guides(hits, geom, geom_prev) if moving else np.asarray(hits).reshape(n)
        sg, hx, hv, hn, land = gather(hist_in, guides, hits_prev, cam_prev, nx, ny, position_tolerance, normal_min_dot)
        assert (land & (sg > F(0)))[took].all()
        xc, vc, nf, _ = tm.frame_values(state, np.asarray(hits).reshape(n), n)
        w = {}
        cnt, ml, s2 = window(state, hits, nx, ny, radius, counted=took, counts=w)
        with np.errstate(all="ignore"):
            mh = F(max_history)
            m = np.where(hn < mh, hn, mh).astype(F)
            tested = took & (F(gamma) != F(0)) & (cnt >= F(min_count))
            lh = (hx[:, 0] + hx[:, 1]) + hx[:, 2]
            dl = lh - ml
            e2 = dl * dl
            lim = (F(gamma) * F(gamma)) * s2
            scale = tested & (e2 > lim)
            m = np.where(scale, m * (lim / e2), m).astype(F)
            al = nf / (m + nf)
            mx = hx + al[:, None] * (xc - hx)
            mv = ((F(1) - al) * (F(1) - al)) * hv + (al * al) * vc
            x = np.where(took[:, None], mx, x)
            v = np.where(took, mv, v)
            neff = np.where(took, m + nf, neff)
        extra.update(w, rectified=int(scale.sum()), rectified_mask=scale, kept_within=int((tested & ~scale).sum()),
                     kept_min_count=int((took & (F(gamma) != F(0)) & ~(cnt >= F(min_count))).sum()))
    assert x.dtype == F and v.dtype == F and neff.dtype == F
    if counts is not None:
        counts.update(c)
        counts.update(extra)
    return tm.make_history(np.concatenate([x, v[:, None]], axis=1), neff)


# ---- hand-worked cases --------------------------------------------------------------------------------------------------------------
def coloured_frame(nx, ny, points, colour, k=8):
    """tm.simple_frame with a colour per pixel: x_c = (colour, colour, colour), l = 3 colour, v_c = 1 / (k - 1)"""
    n = nx * ny
    hits, _ = tm.simple_frame(nx, ny, points, k=k)
    col = np.broadcast_to(np.asarray(colour, F), (n,)).astype(F)
    S = np.repeat((F(k) * col)[:, None], 3, axis=1)
    SL = F(3 * k) * col
    Q = F(k) * (F(3) * col) ** 2 + F(k)
    return hits, make_state(S, SL, Q, np.full(n, k, np.int32))


def hand_cases():
    """the hand-worked cases on the 4x4 frame behind tm.simple_camera(): every point on its own pixel centre at distance 2 (tap (0, 0)
    with weight 1: x_h, v_h, n_h are the history's own values at the pixel), k = 8 samples, v_c = 1/7, history variance 0.25,
    reuse_specular 1 (no material is looked at), radius 1.  Each case: a name, the arguments of accumulate_rectified (without kind)
    and `expect`, {pixel: (neff, x)} with the hand-computed values, exact in binary32.  The frame's colour is c per channel, so
    l = 3c; pixel p = 4 j + i.

    on_mean     colour by column 0.25, 0.5, 0.75, 1: l = 0.75, 1.5, 2.25, 3.  The 3x3 window of pixel 5 (column 1) holds each of the
                columns 0..2 three times: s1 = 13.5, ml = 1.5; ss = 6 * 0.75^2 = 3.375, s2 = 3.375 / 8 = 0.421875.  History colour 0.5:
                lh = 1.5 = ml, e2 = 0: untouched.  n_h = 128 uncapped: a = 8 / 136, neff = 136.
    two_sigma   the same frame, history colour 1: lh = 3, dl = 1.5, e2 = 2.25; gamma 1: lim = 0.421875; lim / e2 = 0.1875;
                m = 128 * 0.1875 = 24; neff = 32; a = 0.25; x = 1 + 0.25 * (0.5 - 1) = 0.875; v = 0.5625 * 0.25 + 0.0625 / 7.
                Pixel 6 (column 2, ml = 2.25, the same s2): dl = 0.75, e2 = 0.5625, lim / e2 = 0.75, m = 96, neff = 104.
    flat        every pixel colour 1: s2 = 0 everywhere (s1 = 3 cnt, exact), lim = 0; history colour 0.5: e2 = 2.25 > 0, m = 8 * 0 = 0:
                this frame alone — a = 1, x = 0.5 + 1 * (1 - 0.5) = 1, neff = 8.
    min_count   the same with min_count 5: a corner's window holds 4 pixels and keeps its history (neff 16, x = 0.75), an edge's 6 and
                the interior's 9 are tested.
    skipped     the flat frame, but pixel 6 is EMPTY (k = 1) and pixel 9 lies on another sphere; both carry the colour 100.  The
                window of pixel 5 accepts the other 7 pixels, all of colour 1: s2 = 0, m = 0, neff = 8.  Were either of the two
                accepted, s2 would exceed 1000 and the history (e2 = 2.25) would be kept at neff 16."""
    nx = ny = 4
    n = nx * ny
    cam = tm.simple_camera()
    j, i = np.divmod(np.arange(n), nx)
    centres = np.stack([-1 + 2 * (i + 0.5) / nx, -1 + 2 * (j + 0.5) / ny, -np.ones(n)], 1) * 2.0
    base = dict(nx=nx, ny=ny, cam_prev=cam, reuse_specular=1, position_tolerance=10.0, normal_min_dot=0.9, radius=1, min_count=2, gamma=1.0)

    def hist(colour, neff):
        xv = np.zeros((n, 4), F)
        xv[:, :3] = F(colour)
        xv[:, 3] = F(0.25)
        return tm.make_history(xv, np.full(n, neff, F))

    cases = []
    ramp = np.array([0.25, 0.5, 0.75, 1.0], F)[i]
    hits, state = coloured_frame(nx, ny, centres, ramp)
    a = F(8) / F(136)
    cases.append(dict(name="on_mean", args=dict(base, hist_in=hist(0.5, 128), hits=hits, hits_prev=hits.copy(), state=state, max_history=1 << 30),
                      expect={5: (F(136), F(0.5) + a * (F(0.5) - F(0.5))), 9: (F(136), F(0.5))}, rectified_at={5: False, 9: False}))
    cases.append(dict(name="two_sigma", args=dict(base, hist_in=hist(1.0, 128), hits=hits, hits_prev=hits.copy(), state=state, max_history=1 << 30),
                      expect={5: (F(32), F(0.875)), 9: (F(32), F(0.875)), 6: (F(104), F(1) + (F(8) / F(104)) * (F(0.75) - F(1)))},
                      rectified_at={5: True, 6: True}, v={5: F(0.5625) * F(0.25) + F(0.0625) * (F(1) / F(7))}))
    hits, state = coloured_frame(nx, ny, centres, 1.0)
    cases.append(dict(name="flat", args=dict(base, hist_in=hist(0.5, 8), hits=hits, hits_prev=hits.copy(), state=state, max_history=64),
                      expect={p: (F(8), F(1)) for p in range(n)}, rectified_at={p: True for p in range(n)}, v={5: F(1) / F(7)}))
    cases.append(dict(name="min_count", args=dict(base, hist_in=hist(0.5, 8), hits=hits, hits_prev=hits.copy(), state=state, max_history=64, min_count=5),
                      expect={0: (F(16), F(0.75)), 3: (F(16), F(0.75)), 12: (F(16), F(0.75)), 15: (F(16), F(0.75)), 1: (F(8), F(1)), 5: (F(8), F(1))},
                      rectified_at={0: False, 15: False, 1: True, 5: True}, kept_min_count=4))
    col = np.ones(n, F)
    col[[6, 9]] = F(100)
    hits, state = coloured_frame(nx, ny, centres, col)
    S, SL, Q, k = (a.copy() for a in tm.state_parts(state, n))
    k[6] = 1
    hits["sphere"][9] = 1
    prev = hits.copy()
    cases.append(dict(name="skipped", args=dict(base, hist_in=hist(0.5, 8), hits=hits, hits_prev=prev, state=make_state(S, SL, Q, k), max_history=64),
                      expect={5: (F(8), F(1)), 0: (F(8), F(1))}, rectified_at={5: True}, min_taps=dict(taps_empty=1, taps_sphere=1, taps_outside=1)))
    return cases


def check_case(case, out, counts=None):
    """hold one result (a history, from the model or from the GPU) to the case's hand-computed values"""
    n = case["args"]["nx"] * case["args"]["ny"]
    x, neff = tm.history_parts(out, n)
    for p, (want_neff, want_x) in case["expect"].items():
        assert neff[p] == want_neff, (case["name"], p, neff[p], want_neff)
        assert np.array_equal(x[p, :3], np.full(3, want_x, F)), (case["name"], p, x[p], want_x)
    for p, want_v in case.get("v", {}).items():
        assert x[p, 3] == want_v, (case["name"], p, x[p, 3], want_v)
    if counts is not None:
        for p, want in case["rectified_at"].items():
            assert bool(counts["rectified_mask"][p]) == want, (case["name"], p)
        if "kept_min_count" in case:
            assert counts["kept_min_count"] == case["kept_min_count"], (case["name"], counts["kept_min_count"])
        for key, least in case.get("min_taps", {}).items():
            assert counts[key] >= least, (case["name"], key)


def self_check():
    """the parent models' self-checks, then the hand-worked cases; gamma 0 on each case is the parent model.  Raises AssertionError."""
    tmm.self_check()
    kind = np.array([tm.LAMBERTIAN, tm.LAMBERTIAN], np.int32)
    for case in hand_cases():
        c = {}
        out = accumulate_rectified(kind=kind, counts=c, **case["args"])
        check_case(case, out, c)
        a = dict(case["args"], gamma=0.0)
        off = accumulate_rectified(kind=kind, counts=c, **a)
        for key in ("radius", "min_count", "gamma"):
            a.pop(key)
        assert np.array_equal(off.view(np.uint32), tm.accumulate(kind=kind, **a).view(np.uint32)), case["name"]
        assert c["rectified"] == 0 and c["kept_min_count"] == 0 and c["kept_within"] == 0
        _, n_on = tm.history_parts(out, 16)
        _, n_off = tm.history_parts(off, 16)
        assert (n_on <= n_off).all(), case["name"]
    # the skipped case with the two pixels accepted instead (no EMPTY pixel, one sphere): the history is kept
    case = [c for c in hand_cases() if c["name"] == "skipped"][0]
    a = dict(case["args"])
    hits = a["hits"].copy()
    hits["sphere"] = 0
    S, SL, Q, k = (z.copy() for z in tm.state_parts(a["state"], 16))
    k[:] = 8
    a.update(hits=hits, hits_prev=hits.copy(), state=make_state(S, SL, Q, k))
    _, neff = tm.history_parts(accumulate_rectified(kind=kind, **a), 16)
    assert neff[5] == 16


if __name__ == "__main__":
    self_check()
    print("temporal_rectify_model: self-check passed")
