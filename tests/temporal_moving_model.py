"""numpy float32 model of rt_temporal_accumulate_moving (include/rt_amd.h, DESIGN.md §5.10 "Moving scenes"): the rule bit for bit.

The static rule is tests/temporal_model.py, imported unchanged; this module adds the two changes, in the form of the header's second
identity: where the sphere of a pixel kept its radius, the moving call is the static call on guides whose p fields hold
P' = (P - c1) + c0 — everything else of the rule reads t, the normal and the sphere, which a translation leaves alone — and where the
radius changed its bits the pixel is not asked, which writes what a first frame writes.  moved_points() is the only new arithmetic.
Test infrastructure only: self_check() holds the model to hand-worked cases (python tests/temporal_moving_model.py runs it alone)."""
import numpy as np

import temporal_model as tm
from bitcmp import f32_bits

F = tm.F


def moved_points(hits, geom, geom_prev):
    """P' [n, 3] of the guides, and per pixel: its sphere is in the list, its centre changed bits, its radius changed bits"""
    hits = np.asarray(hits).reshape(-1)
    geom, geom_prev = np.asarray(geom, F).reshape(-1, 4), np.asarray(geom_prev, F).reshape(-1, 4)
    assert geom.shape == geom_prev.shape
    s = np.asarray(hits["sphere"])
    known = (s >= 0) & (s < len(geom))
    sc = np.clip(s, 0, len(geom) - 1)
    c1, c0 = geom[sc], geom_prev[sc]
    moved = known & (f32_bits(c0[:, :3]) != f32_bits(c1[:, :3])).any(axis=1)
    resized = known & (f32_bits(c0[:, 3]) != f32_bits(c1[:, 3]))
    P = np.asarray(hits["p"], F)
    with np.errstate(all="ignore"):
        back = (P - c1[:, :3]) + c0[:, :3]
    assert back.dtype == F
    return np.where(moved[:, None], back, P), known, moved, resized


def patched_guides(hits, geom, geom_prev):
    """a copy of the guides whose p fields hold P'"""
    out = np.asarray(hits).reshape(-1).copy()
    out["p"] = moved_points(hits, geom, geom_prev)[0]
    return out


def accumulate_moving(hist_in, hits, hits_prev, cam_prev, geom, geom_prev, state, kind, nx, ny, max_history, reuse_specular, position_tolerance,
                      normal_min_dot, counts=None):
    """d_hist_out of rt_temporal_accumulate_moving for host copies of its inputs (hist_in None: the first frame, geom_prev unused).
    counts receives temporal_model's counts of the static call on the patched guides and, on top: moved_asked / moved_took (pixels
    on a translated sphere that were asked / took history), resized_not_asked (pixels the static rule would have asked, dropped for
    their radius), moved_refused (asked pixels on a translated sphere that landed in the frame and had every tap refused), and the
    masks took_mask / moved_mask / resized_mask"""
    n = nx * ny
    if hist_in is None:
        c = {}
        out = tm.accumulate(None, hits, None, None, state, kind, nx, ny, max_history, reuse_specular, position_tolerance, normal_min_dot, counts=c)
        if counts is not None:
            counts.update(c, moved_asked=0, moved_took=0, resized_not_asked=0, moved_refused=0, moved_mask=np.zeros(n, bool),
                          resized_mask=np.zeros(n, bool))
        return out
    assert len(np.asarray(geom).reshape(-1, 4)) == len(kind)
    _, known, moved, resized = moved_points(hits, geom, geom_prev)
    c = {}
    asked = tm.accumulate(hist_in, patched_guides(hits, geom, geom_prev), hits_prev, cam_prev, state, kind, nx, ny, max_history, reuse_specular,
                          position_tolerance, normal_min_dot, counts=c)
    alone = tm.accumulate(None, hits, None, None, state, kind, nx, ny, max_history, reuse_specular, position_tolerance, normal_min_dot)
    xa, na = tm.history_parts(asked, n)
    x0, n0 = tm.history_parts(alone, n)
    out = tm.make_history(np.where(resized[:, None], x0, xa), np.where(resized, n0, na))
    if counts is not None:
        took = c["took_mask"] & ~resized
        # which pixels the rule asks: not empty, and lambertian unless reuse_specular (temporal_model.accumulate's `ask`)
        _, _, _, empty = tm.frame_values(state, np.asarray(hits).reshape(n), n)
        s = np.asarray(np.asarray(hits).reshape(n)["sphere"])
        k = np.asarray(kind, np.int32)
        lamb = known & (k[np.clip(s, 0, len(k) - 1)] == tm.LAMBERTIAN)
        ask = ~empty & (lamb if not reuse_specular else True) & (max_history != 0)
        lam, fx, fy = tm.reproject(moved_points(hits, geom, geom_prev)[0], np.asarray(cam_prev).reshape(1)[0], nx, ny)
        with np.errstate(all="ignore"):
            land = (lam > F(0)) & (fx > F(-1)) & (fx < F(nx)) & (fy > F(-1)) & (fy < F(ny))
        counts.update(c, took=int(took.sum()), took_mask=took, moved_mask=moved, resized_mask=resized,
                      moved_asked=int((ask & moved & ~resized).sum()), moved_took=int((took & moved).sum()),
                      resized_not_asked=int((ask & resized).sum()), moved_refused=int((ask & moved & ~resized & land & ~took).sum()))
    return out


# ---- hand-worked cases --------------------------------------------------------------------------------------------------------------
def self_check():
    """hand-worked cases on the 4x4 frame of temporal_model.self_check (every point on its own pixel centre at distance 2, a history of
    0.25 / 0.5 / 0.75 / 1 by column with neff 8 against a frame of 1.0 with k = 8): both identities, the radius rule, a sphere outside the list, a sphere moved so
    that P' leaves the previous frame, a sphere moved onto a pixel that held another sphere.  Raises AssertionError."""
    tm.self_check()
    nx = ny = 4
    n = nx * ny
    cam = tm.simple_camera()
    j, i = np.divmod(np.arange(n), nx)
    centres = np.stack([-1 + 2 * (i + 0.5) / nx, -1 + 2 * (j + 0.5) / ny, -np.ones(n)], 1) * 2.0
    prev, state = tm.simple_frame(nx, ny, centres)
    prev["sphere"] = np.where(i < 2, 0, 1)                          # sphere 0 covers the left half of the last frame, sphere 1 the right
    xv = np.zeros((n, 4), F)
    xv[:, :3] = np.array([0.25, 0.5, 0.75, 1.0], F)[i][:, None]    # the history's colour names the column it was written at
    xv[:, 3] = F(0.25)
    hist = tm.make_history(xv, np.full(n, 8, F))
    kind = np.array([tm.LAMBERTIAN, tm.LAMBERTIAN, 1], np.int32)
    g0 = np.array([[0, 0, -2, 0.5], [3, 0, -2, 0.5], [0, 5, -2, 0.5]], F)
    args = dict(kind=kind, nx=nx, ny=ny, max_history=64, reuse_specular=0, position_tolerance=0.01, normal_min_dot=0.9)
    first = tm.accumulate(None, prev, None, None, state, **args)

    # 1. nothing moved: the bytes of the static call, also with geometry that is NaN (bits are compared, not values)
    hits = prev.copy()
    static = tm.accumulate(hist, hits, prev, cam, state, **args)
    c = {}
    assert np.array_equal(accumulate_moving(hist, hits, prev, cam, g0, g0, state, counts=c, **args), static)
    assert c["took"] == n and c["moved_asked"] == 0 and c["resized_not_asked"] == 0
    gn = g0.copy()
    gn[0] = F("nan")
    assert np.array_equal(accumulate_moving(hist, hits, prev, cam, gn, gn, state, **args), static)
    assert np.array_equal(accumulate_moving(None, hits, None, None, g0, None, state, **args), first)

    # 2. sphere 0 moved by one pixel to the right (+1 in x at distance 2) and now covers columns 0..2.  Every value is dyadic, so
    #    P' = P - (1, 0, 0) is last frame's pixel centre one column to the left, exactly: column 0 lands at fx = -1 (off the frame,
    #    rejected), column 1 takes column 0's history, column 2 — which held sphere 1 — takes column 1's.  The static rule looks at
    #    the pixel's own place instead: another column's colour, or (column 2) another sphere.
    g1 = g0.copy()
    g1[0, 0] += F(1)
    hits = prev.copy()
    hits["sphere"] = np.where(i < 3, 0, 1)
    Pb, known, moved, resized = moved_points(hits, g1, g0)
    assert moved[i < 3].all() and not moved[i == 3].any() and not resized.any() and known.all()
    assert np.array_equal(Pb[i == 1], prev["p"][i == 0]) and np.array_equal(Pb[i == 2], prev["p"][i == 1])
    c = {}
    got = accumulate_moving(hist, hits, prev, cam, g1, g0, state, counts=c, **args)
    x, neff = tm.history_parts(got, n)
    assert (neff[i == 0] == 8).all() and c["off_frame"] == ny and np.array_equal(x[i == 0, :3], np.ones((ny, 3), F))
    assert (neff[i >= 1] == 16).all()
    for col, h in ((1, 0.25), (2, 0.5), (3, 1.0)):                                 # h + (1 - h) / 2 with the history of the column it came from
        assert np.array_equal(x[i == col, :3], np.full((ny, 3), h + (1 - h) / 2, F)), col
    assert c["moved_took"] == 2 * ny and c["moved_asked"] == 3 * ny and c["moved_refused"] == 0
    s_x, s_neff = tm.history_parts(tm.accumulate(hist, hits, prev, cam, state, **args), n)
    assert np.array_equal(s_x[i == 1, :3], np.full((ny, 3), 0.75, F)) and (s_neff[i == 2] == 8).all()   # its own column; another sphere
    assert np.array_equal(got, tm.accumulate(hist, patched_guides(hits, g1, g0), prev, cam, state, **args))      # the second identity

    # 3. moved onto a pixel that held another sphere: sphere 0 (columns 0 and 1) moved one pixel to the LEFT, so P' lies one column to
    #    the right — column 0 lands on last frame's column 1 (sphere 0: taken), column 1 on column 2, which held sphere 1: refused
    g2 = g0.copy()
    g2[0, 0] -= F(1)
    hits = prev.copy()
    c = {}
    got = accumulate_moving(hist, hits, prev, cam, g2, g0, state, counts=c, **args)
    x, neff = tm.history_parts(got, n)
    assert (neff[i == 1] == 8).all() and c["sphere"] >= ny and c["moved_refused"] == ny and c["all_refused"] == ny
    assert (neff[i == 0] == 16).all() and np.array_equal(x[i == 0, :3], np.full((ny, 3), 0.75, F))
    assert (neff[i >= 2] == 16).all() and c["moved_took"] == ny

    # 4. the radius rule: the bits of the radius, whatever the centre does
    g3 = g0.copy()
    g3[1, 3] = np.nextafter(g0[1, 3], F(1))
    hits = prev.copy()
    c = {}
    got = accumulate_moving(hist, hits, prev, cam, g3, g0, state, counts=c, **args)
    x, neff = tm.history_parts(got, n)
    x1, n1 = tm.history_parts(first, n)
    assert (neff[i >= 2] == 8).all() and np.array_equal(x[i >= 2], x1[i >= 2]) and (neff[i < 2] == 16).all()
    assert c["resized_not_asked"] == 2 * ny and c["took"] == 2 * ny
    gz = g0.copy()
    gz[1, 3] = F(-0.5)
    gz0 = g0.copy()
    gz0[1, 3] = F(0.5)
    assert moved_points(hits, gz, gz0)[3][i >= 2].all()                           # -0.5 against 0.5: other bits
    gm, gp = g0.copy(), g0.copy()
    gm[1, 3], gp[1, 3] = F(-0.0), F(0.0)
    assert moved_points(hits, gm, gp)[3][i >= 2].all()                            # -0 against +0: other bits, though equal values

    # 5. a sphere index outside the list reads no geometry: P' = P bit for bit, and with reuse_specular it is reprojected as it is
    hits = prev.copy()
    hits["sphere"] = 7
    prev7 = prev.copy()
    prev7["sphere"] = 7
    spec = dict(args, reuse_specular=1)
    Pb, known, moved, resized = moved_points(hits, g1, g0)
    assert not known.any() and not moved.any() and not resized.any() and np.array_equal(f32_bits(Pb), f32_bits(hits["p"]))
    assert np.array_equal(accumulate_moving(hist, hits, prev7, cam, g1, g0, state, **spec), tm.accumulate(hist, hits, prev7, cam, state, **spec))
    assert np.array_equal(accumulate_moving(hist, hits, prev7, cam, g1, g0, state, **args), first)       # not lambertian: not asked
    hits["sphere"] = -1
    assert not moved_points(hits, g1, g0)[1].any()


if __name__ == "__main__":
    self_check()
    print("temporal_moving_model: self-check passed")
