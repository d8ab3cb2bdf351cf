"""numpy float32 model of the history-aware budget key (include/rt_amd.h "History-aware budgets"): what
rt_temporal_accumulate would write for every pixel (temporal_model.accumulate, bit for bit), the key of the merged pixel
(filtered_budget_model.priority_filtered on its luminance and variance), the raw key of adaptive_budget_model for the pixels that
accumulate nothing (neff == 0), and the selection by filtered_budget_model.pick.

It composes the existing models and restates none of them.  self_check() holds it to hand-worked cases on temporal_model's 4x4 frame
(python tests/temporal_budget_model.py runs it alone)."""
import numpy as np

import adaptive_budget_model as B
import filtered_budget_model as FM
import temporal_model as tm
from denoise_var_model import make_state, state_parts

F = np.float32


def frame_keys(hist_in, hits, hits_prev, cam_prev, state, kind, nx, ny, floor, max_history, reuse_specular, position_tolerance, normal_min_dot,
               counts=None):
    """the key of every pixel (float32 [nx * ny], before the eligibility mask), which pixels are ranked by the merged values
    (neff > 0), and the history rt_temporal_accumulate would write"""
    n = nx * ny
    hist = tm.accumulate(hist_in, hits, hits_prev, cam_prev, state, kind, nx, ny, max_history, reuse_specular, position_tolerance, normal_min_dot,
                         counts=counts)
    xv, neff = tm.history_parts(hist, n)
    _, SL, Q, k = state_parts(state, n)
    with np.errstate(all="ignore"):
        l = (xv[:, 0] + xv[:, 1]) + xv[:, 2]
    merged = FM.priority_filtered(l, xv[:, 3], floor)
    raw = B.priority(SL, Q, k, floor)
    valid = neff != F(0)
    key = np.where(valid, merged, raw).astype(F)
    assert l.dtype == F and key.dtype == F
    return key, valid, hist


def select(hist_in, hits, hits_prev, cam_prev, state, kind, nx, ny, batch, max_spp, floor, K_picks, temporal):
    """the sorted ids of the first min(K, eligible) eligible pixels by key descending, id ascending; the mask, the key bits before the
    mask; temporal = (max_history, reuse_specular, position_tolerance, normal_min_dot)"""
    key, _, _ = frame_keys(hist_in, hits, hits_prev, cam_prev, state, kind, nx, ny, floor, *temporal)
    kb = B.keybits(key)
    k = state_parts(state, nx * ny)[3]
    ok = (k.astype(np.int64) + batch <= max_spp) & (kb > 0)
    return FM.pick(ok, kb, K_picks), ok, kb


def left_right_case(nx=16, ny=8, k=8, colour=0.5, neff_left=32):
    """The fabricated left / right frame: guides of one lambertian sphere (index 0) on the centre rays of temporal_model.simple_camera(),
    a static camera, one (S, SL, Q, k) in every pixel with v_c > 0.  The last frame's history holds (x_c, v_c) at neff = neff_left in the
    left half and nothing (neff = 0) in the right half.  Returns a dict of the inputs, v_c and the masks `left`, `right` and `seam` (the
    pixels within one column of the seam: their taps are their own column alone — every point lands on its own pixel centre, ax = ay = 0
    — but the claim below leaves them out all the same).

    Why every key of the right half lies strictly above every key of the left half: a left pixel merges with a = n / (32 + n) < 1 a
    history of the same colour, so x stays x_c up to rounding and v = ((1 - a)^2 + a^2) v_c < v_c (for n = 8: 0.68 v_c); a right pixel
    finds neff_q = 0 in its tap, takes nothing and keeps (x_c, v_c).  Both keys divide by the same max(l, floor)^2 up to rounding."""
    n = nx * ny
    j, i = np.divmod(np.arange(n), nx)
    centres = np.stack([-1 + 2 * (i + 0.5) / nx, -1 + 2 * (j + 0.5) / ny, -np.ones(n)], 1) * 2.0
    hits, state = tm.simple_frame(nx, ny, centres, k=k, colour=colour)
    xc, vc, _, empty = tm.frame_values(state, hits, n)
    assert not empty.any() and (vc > 0).all() and len(np.unique(vc)) == 1
    left = i < nx // 2
    xv = np.concatenate([xc, vc[:, None]], axis=1).astype(F)
    xv[~left] = 0
    neff = np.where(left, F(neff_left), F(0)).astype(F)
    seam = (i == nx // 2 - 1) | (i == nx // 2)
    return dict(nx=nx, ny=ny, cam=tm.simple_camera(), hits=hits, prev=hits.copy(), hist=tm.make_history(xv, neff), state=state,
                kind=np.array([tm.LAMBERTIAN, 1], np.int32), vc=vc[0], left=left, right=~left, seam=seam,
                temporal=(32, 0, 10.0, 0.9))


def self_check():
    """hand-worked keys on 4x4: a first frame (the filtered rule on (x_c, v_c)), max_history 0, a merge at a = 1/2, an empty pixel (the
    raw rule), a specular first hit, the eligibility mask and the pick.  Raises AssertionError."""
    tm.self_check()
    nx = ny = 4
    n = nx * ny
    cam = tm.simple_camera()
    j, i = np.divmod(np.arange(n), nx)
    centres = np.stack([-1 + 2 * (i + 0.5) / nx, -1 + 2 * (j + 0.5) / ny, -np.ones(n)], 1) * 2.0
    hits, state = tm.simple_frame(nx, ny, centres)             # k = 8, colour 1: x_c = 1, l = 3, v_c = 1/7
    prev = hits.copy()
    kind = np.array([tm.LAMBERTIAN, 1], np.int32)
    args = dict(kind=kind, nx=nx, ny=ny, reuse_specular=0, position_tolerance=10.0, normal_min_dot=0.9)
    vc = F(1) / F(7)
    floor = 0.02

    # 1. a first frame, and max_history = 0: v_c / (l * l) with l = 3, not the raw key's bits necessarily, the same quantity
    key, valid, _ = frame_keys(None, hits, None, None, state, floor=floor, max_history=64, **args)
    assert valid.all() and np.array_equal(key, np.full(n, vc / (F(3) * F(3)), F))
    _, SL, Q, k = state_parts(state, n)
    raw = B.priority(SL, Q, k, floor)
    assert np.allclose(key, raw, rtol=1e-6, atol=0)
    xv = np.zeros((n, 4), F)
    xv[:, :3] = F(0.5)
    xv[:, 3] = F(0.25)
    hist = tm.make_history(xv, np.full(n, 8, F))
    key0, _, _ = frame_keys(hist, hits, prev, cam, state, floor=floor, max_history=0, **args)
    assert np.array_equal(key0, key)

    # 2. a merge at a = 1/2 (neff_q = 8, n = 8): x = 0.75, l = 2.25, v = 0.25 * 0.25 + 0.25 * v_c
    keym, valid, h = frame_keys(hist, hits, prev, cam, state, floor=floor, max_history=64, **args)
    v = F(0.25) * F(0.25) + F(0.25) * vc
    assert valid.all() and np.array_equal(keym, np.full(n, v / (F(2.25) * F(2.25)), F))
    assert np.array_equal(tm.history_parts(h, n)[1], np.full(n, 16, F))
    # ... below the floor the floor divides
    keyf, _, _ = frame_keys(hist, hits, prev, cam, state, floor=5.0, max_history=64, **args)
    assert np.array_equal(keyf, np.full(n, v / (F(5) * F(5)), F))

    # 3. empty pixels keep the raw rule: sky, k = 1 (key 0: n - 1 = 0 divides), a NaN colour sum (SL and Q are fine: the raw key stands)
    sky = hits.copy()
    sky["sphere"][5] = -1
    S, SL, Q, k = (a.copy() for a in state_parts(state, n))
    k[6] = 1
    S[7, 1] = F("nan")
    st2 = make_state(S, SL, Q, k)
    key, valid, _ = frame_keys(hist, sky, prev, cam, st2, floor=floor, max_history=64, **args)
    raw2 = B.priority(SL, Q, k, floor)
    assert not valid[[5, 6, 7]].any() and valid.sum() == n - 3
    assert np.array_equal(key[[5, 6, 7]].view(np.uint32), raw2[[5, 6, 7]].view(np.uint32)) and key[5] == raw[5] and key[7] == raw[7]
    assert np.array_equal(key[valid], keym[valid])
    assert not np.isnan(key).any() and (B.keybits(key) < 0x80000000).all()

    # 4. a specular first hit is ranked by this frame alone unless reuse_specular; against a history of this frame's own colour and
    #    variance the merged pixel (a = 1/2: v = v_c / 2) ranks below it
    metal, prev_metal = hits.copy(), prev.copy()
    metal["sphere"][:8] = 1
    prev_metal["sphere"][:8] = 1
    xv = np.ones((n, 4), F)
    xv[:, 3] = vc
    hist = tm.make_history(xv, np.full(n, 8, F))
    first = vc / (F(3) * F(3))
    half = (F(0.25) * vc + F(0.25) * vc) / (F(3) * F(3))
    key, _, _ = frame_keys(hist, metal, prev_metal, cam, state, floor=floor, max_history=64, **args)
    assert np.array_equal(key[:8], np.full(8, first, F)) and np.array_equal(key[8:], np.full(8, half, F)) and first > half > 0
    key, _, _ = frame_keys(hist, metal, prev_metal, cam, state, floor=floor, max_history=64, **dict(args, reuse_specular=1))
    assert np.array_equal(key, np.full(n, half, F))

    # 5. the selection: the specular half first, the lower ids at the cut, the mask is not the key
    t = (64, 0, 10.0, 0.9)
    chosen, ok, kb = select(hist, metal, prev_metal, cam, state, kind, nx, ny, 4, 64, floor, 8, t)
    assert ok.all() and np.array_equal(chosen, np.arange(8))
    assert np.array_equal(select(hist, metal, prev_metal, cam, state, kind, nx, ny, 4, 64, floor, 10, t)[0], np.arange(10))
    assert len(select(hist, metal, prev_metal, cam, state, kind, nx, ny, 4, 64, floor, 0, t)[0]) == 0
    chosen, ok, kb2 = select(hist, metal, prev_metal, cam, state, kind, nx, ny, 4, 11, floor, 10 ** 9, t)       # 8 + 4 > 11
    assert not ok.any() and len(chosen) == 0 and np.array_equal(kb2, kb)

    # 6. the left / right case: the claim of its docstring
    c = left_right_case()
    key, valid, _ = frame_keys(c["hist"], c["hits"], c["prev"], c["cam"], c["state"], c["kind"], c["nx"], c["ny"], floor, *c["temporal"])
    claim_l, claim_r = c["left"] & ~c["seam"], c["right"] & ~c["seam"]
    assert valid.all() and key[claim_r].min() > key[claim_l].max() > 0


if __name__ == "__main__":
    self_check()
    print("temporal_budget_model: self-check passed")
