"""What the GPU tests of adaptive sampling share (begin / refine / the three spends): the layout of a part's buffers, the state's
arrays, ONE Frame of sentinel-filled buffers, the Scene that keeps the k-sample reference frames, and the checks of a budget round
against the numpy models.  Every comparison is bit equality.  torch is the caller's (the cuda fixture): importing this needs no GPU."""
import numpy as np

import adaptive_budget_model as M
import filtered_budget_model as FM
from bitcmp import raw_bits
from denoise_var_model import make_state, state_parts      # the state's structure of arrays, written once

RUN = 64                           # rt_amd.h RT_PART_RUN
SENTINEL = 0x7FC0DEAD              # a NaN pattern nothing renders
STATE_FILL = 0xA5                  # every byte of a fresh state (padding elements keep it)
FLOOR = 0.02
BATCH, MAX_SPP = 4, 64             # the budget the tests spend unless they say otherwise


def part_tuple(P):
    return (P.part, P.nparts, P.tile_begin, P.tile_end)


def part_tile(lt, part, nparts, begin, end):
    """global tile of a part's local tile (rt_amd.h: runs of RT_PART_RUN dealt round-robin, or a range)"""
    if end > begin:
        return begin + lt
    return ((lt // RUN) * nparts + part) * RUN + lt % RUN


def part_layout(nx, ny, part, n):
    """for every element of a part's buffer: its row-major pixel index and whether it lies inside the frame; part = (part, nparts,
    tile_begin, tile_end), n = rt_part_pixels.  A part's buffer is tile-major (local_tile * 64 + ly * 8 + lx) with padded edge tiles;
    nparts == 1 without a range is the whole frame in the reference's row-major layout, where every element is a pixel."""
    e = np.arange(n, dtype=np.int64)
    p, nparts, begin, end = part
    if nparts == 1 and not end > begin:
        return e, np.ones(n, bool)
    tile = part_tile(e // 64, *part)
    tiles_x = (nx + 7) // 8
    i = (tile % tiles_x) * 8 + (e % 64) % 8
    j = (tile // tiles_x) * 8 + (e % 64) // 8
    inside = (i < nx) & (j < ny)
    return np.where(inside, j * nx + i, 0), inside


def inside_frame(nx, ny, part, n):
    """for every element of a part's buffer: whether it holds a pixel of the frame (the rest is the padding of edge tiles)"""
    return part_layout(nx, ny, part, n)[1]


def stop_rule_model(samples, rel_error, floor, lo, step, hi):
    """the stop rule of rt_render_adaptive on per-sample colours samples[s, pixel, 3] (float32): (spp, fb) of every pixel"""
    F = np.float32
    npx = samples.shape[1]
    S = np.zeros((npx, 3), F)
    SL = np.zeros(npx, F)
    Q = np.zeros(npx, F)
    spp = np.zeros(npx, np.int32)
    fb = np.zeros((npx, 3), F)
    rel, fl = F(rel_error), F(floor)
    for k in range(1, hi + 1):
        c = samples[k - 1]
        S = S + c
        l = (c[:, 0] + c[:, 1]) + c[:, 2]
        SL = SL + l
        Q = Q + l * l
        if k < lo or (k - lo) % step:
            continue
        n = F(k)
        d = n * Q - SL * SL
        m = np.where(SL > n * fl, SL, n * fl)
        t = rel * rel
        with np.errstate(invalid="ignore", over="ignore"):
            conv = (d <= (t * (n - F(1))) * (m * m)) if rel > 0 else np.zeros(npx, bool)
        stop = (spp == 0) & (conv | (k == hi))
        kk = F(1.0 / float(F(k)))
        fb[stop] = np.sqrt(S[stop] * kk)
        spp[stop] = k
    return spp, fb


def pick_rel_error(samples, lo, step, hi, floor):
    """the first target of a sweep whose frame mixes >= 3 distinct counts, early stops and capped pixels"""
    for rel in (0.02, 0.03, 0.05, 0.07, 0.1, 0.15, 0.2, 0.3, 0.5):
        spp, _ = stop_rule_model(samples, rel, floor, lo, step, hi)
        if len(np.unique(spp)) >= 3 and (spp < hi).any() and (spp == hi).any():
            return rel
    raise AssertionError("no rel_error in the sweep gives a mixed frame")


def progressive_samples(rt, torch, W, O, nx, ny, count):
    """per-sample colours [count, pixels, 3] and the RNG state after every pass [count, pixels, 12], from one-sample passes"""
    st = rt.alloc_rand_state(nx, ny)
    fb = rt.alloc_fb(nx, ny)
    rt.render_init(nx, ny, st)
    cols, states = [], []
    for _ in range(count):
        rt.render_progressive(fb, nx, ny, 1, W, st, O)
        cols.append(fb.clone())
        states.append(st.clone())
    torch.cuda.synchronize()
    return (np.stack([c.cpu().numpy().reshape(-1, 3) for c in cols]),
            np.stack([s.cpu().numpy().view(np.uint32).reshape(-1, 12) for s in states]))


def adaptive_frame(rt, torch, W, O, nx, ny, params, ctx=None, stream=None):
    """(spp [n], fb [n, 3], RNG states [n, 12]) of one whole-frame rt_render_adaptive on fresh buffers"""
    st = rt.alloc_rand_state(nx, ny)
    fb = rt.alloc_fb(nx, ny)
    spp = torch.full((nx * ny,), -1, dtype=torch.int32, device="cuda")
    rt.render_init(nx, ny, st)
    if ctx is None:
        rt.render_adaptive(fb, nx, ny, params, W, st, O, spp)
    else:
        ctx.render_adaptive(fb, nx, ny, params, W, st, O, spp, stream=stream)
    torch.cuda.synchronize()
    return spp.cpu().numpy(), fb.cpu().numpy().reshape(-1, 3), st.cpu().numpy().view(np.uint32).reshape(-1, 12)


def filt_of(p):
    """the filter arguments of tests/filtered_budget_model.py from rt_denoise_var_params"""
    return (p.normal_pow_log2, p.prefilter, p.sigma_position, p.sigma_variance)


class Frame:
    """the buffers of one part: fb and d_spp pre-filled with SENTINEL, RNG states from rt_render_init(part), a fresh state.  With a
    context every call goes through it, on `stream`."""

    def __init__(self, rt, torch, nx, ny, part, ctx=None, stream=None):
        self.rt, self.torch, self.nx, self.ny, self.part, self.ctx, self.stream = rt, torch, nx, ny, part, ctx, stream
        n = self.n = rt.part_pixels(nx, ny, part)
        self.fb = torch.full((n * 3,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        self.spp = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
        self.st = rt.alloc_rand_state(nx, ny, part)
        rt.render_init(nx, ny, self.st, part)
        self.state = torch.full((n * rt.ADAPTIVE_STATE_BYTES,), STATE_FILL, dtype=torch.uint8, device="cuda")
        self.inside = inside_frame(nx, ny, part_tuple(part), n)
        torch.cuda.synchronize()

    def _call(self, name, *args):
        if self.ctx is not None:
            getattr(self.ctx, name)(*args, stream=self.stream)
        else:
            getattr(self.rt, name)(*args)

    def begin(self, W, O, P):
        self._call("render_adaptive_begin", self.fb, self.nx, self.ny, self.rt.Adaptive(*P), W, self.st, self.state, O, self.spp, self.part)
        return self

    def refine(self, W, O, frm, to):
        self._call("render_adaptive_refine", self.fb, self.nx, self.ny, self.rt.Adaptive(*frm), self.rt.Adaptive(*to), W, self.st, self.state, O,
                   self.spp, self.part)
        return self

    def _spend(self, name, budget, head, W, O, tail=()):
        """one spend call of any kind; returns d_picked read back.  The order is fill, synchronize, spend: the fill runs on the current
        stream, a context's spend on the context's, and without the wait the spend may find d_picked not yet filled."""
        samples, rounds = budget[:2]
        picked = self.torch.full((rounds,), SENTINEL, dtype=self.torch.int32, device="cuda")
        self.torch.cuda.synchronize()
        self._call(name, self.fb, self.nx, self.ny, self.rt.Budget(*budget), *head, W, self.st, self.state, O, self.spp, *tail, picked)
        self.torch.cuda.synchronize()
        return picked.cpu().numpy().view(np.uint32)

    def spend(self, W, O, samples, rounds, batch=BATCH, max_spp=MAX_SPP, floor=FLOOR):
        """one rt_render_adaptive_spend"""
        return self._spend("render_adaptive_spend", (samples, rounds, batch, max_spp, floor), (), W, O, (self.part,))

    def spend_filtered(self, sc, p, samples, rounds, batch=BATCH, max_spp=MAX_SPP, floor=FLOOR):
        """one rt_render_adaptive_spend_filtered on the scene's guides (whole frames only)"""
        return self._spend("render_adaptive_spend_filtered", (samples, rounds, batch, max_spp, floor), (p, sc.d_hits), sc.W, sc.O)

    def spend_temporal(self, sc, samples, rounds, batch=BATCH, max_spp=MAX_SPP, floor=FLOOR):
        """one rt_render_adaptive_spend_temporal on the scene's temporal inputs and parameters (whole frames only)"""
        return self._spend("render_adaptive_spend_temporal", (samples, rounds, batch, max_spp, floor), (sc.tin, sc.tp), sc.W, sc.O)

    def snap(self):
        self.torch.cuda.synchronize()
        return dict(fb=raw_bits(self.fb.cpu().numpy()).reshape(-1, 3), spp=self.spp.cpu().numpy(),
                    st=self.st.cpu().numpy().view(np.uint32).reshape(-1, 12), state=self.state.cpu().numpy().copy())


class Scene:
    """a world and tree, and for every k the frame begin((k, k, 1, 0, floor)) leaves on fresh buffers of a part (the reference of a
    pixel that has taken exactly k samples)"""

    def __init__(self, rt, torch, n, spl, nx, ny, trav=None):
        self.rt, self.torch, self.nx, self.ny = rt, torch, nx, ny
        self.W = rt.World(n, nx, ny)
        self.O = rt.Octree(self.W, spl) if spl else None
        if trav is not None:
            (self.O.set_traversal if self.O is not None else self.W.set_list_traversal)(trav)
        self.refs = {}

    def with_guides(self):
        """rt_render_guides of the whole frame: d_hits on the device, hits on the host"""
        self.d_hits = self.rt.alloc_guides(self.nx, self.ny)
        self.rt.render_guides(self.W, self.O, self.nx, self.ny, self.d_hits)
        self.torch.cuda.synchronize()
        self.hits = self.d_hits.cpu().numpy().view(self.rt.hit_record_dtype)
        return self

    def at_k(self, part, k, floor=FLOOR):
        key = (part_tuple(part), int(k), floor)
        if key not in self.refs:
            self.refs[key] = Frame(self.rt, self.torch, self.nx, self.ny, part).begin(self.W, self.O, (int(k), int(k), 1, 0.0, floor)).snap()
        return self.refs[key]

    def close(self):
        if self.O is not None:
            self.O.close()
        self.W.close()


def model_pick(snap, n, inside, K, batch=BATCH, max_spp=MAX_SPP, floor=FLOOR):
    """the raw model's choice for the state of a snapshot: (sorted ids, eligible mask, key bits)"""
    S, SL, Q, k = state_parts(snap["state"], n)
    kk = np.where(inside, k, 0)                              # (padding holds the fill pattern: any k, never eligible)
    return M.select(SL, Q, kk, batch, max_spp, floor, inside, K)


def check_exact(sc, F, snap, floor=FLOOR):
    """for every distinct k of the frame: fb, the RNG state and the state's sums at the pixels with that k are the k-sample frame's"""
    n, inside = F.n, F.inside
    S, SL, Q, k = state_parts(snap["state"], n)
    for kv in np.unique(k[inside]):
        ref = sc.at_k(F.part, kv, floor)
        at = inside & (k == kv)
        rS, rSL, rQ, rk = state_parts(ref["state"], n)
        assert (rk[inside] == kv).all()
        assert np.array_equal(snap["fb"][at], ref["fb"][at]), kv
        assert np.array_equal(snap["st"][at], ref["st"][at]), kv
        assert (np.array_equal(raw_bits(S[at]), raw_bits(rS[at])) and np.array_equal(raw_bits(SL[at]), raw_bits(rSL[at]))
                and np.array_equal(raw_bits(Q[at]), raw_bits(rQ[at]))), kv


def check_round(sc, F, before, after, picked, K, batch=BATCH, max_spp=MAX_SPP, floor=FLOOR):
    """one raw round of a part from `before` to `after` against the model: the chosen set through the counts, untouched pixels, the
    padding, every pixel at its k"""
    n, inside = F.n, F.inside
    chosen, ok, kb = model_pick(before, n, inside, K, batch, max_spp, floor)
    assert int(picked) == len(chosen) == min(K, int(ok.sum()))
    k0 = state_parts(before["state"], n)[3]
    S1, SL1, Q1, k1 = state_parts(after["state"], n)
    want = k0.copy()
    want[chosen] += batch
    assert np.array_equal(k1[inside], want[inside])
    assert np.array_equal(after["spp"][inside], want[inside])
    # every untouched element — the padding included — keeps all its bits
    hit = np.zeros(n, bool)
    hit[chosen] = True
    S0, SL0, Q0, _ = state_parts(before["state"], n)
    for a, b in ((before["fb"], after["fb"]), (before["st"], after["st"]), (before["spp"], after["spp"]), (raw_bits(S0), raw_bits(S1)),
                 (raw_bits(SL0), raw_bits(SL1)), (raw_bits(Q0), raw_bits(Q1)), (k0, k1)):
        assert np.array_equal(a[~hit], b[~hit])
    assert (after["spp"][~inside] == SENTINEL).all() and (after["fb"][~inside] == SENTINEL).all()
    assert (after["state"].view(np.uint32).reshape(6, n)[3:, ~inside] == 0xA5A5A5A5).all() and (raw_bits(S1)[~inside] == 0xA5A5A5A5).all()
    check_exact(sc, F, after)
    return chosen, ok


def _check_whole_frame_round(F, before, after, picked, chosen, ok, K, batch):
    """a round of a whole frame whose set a model gave: the count, the chosen set through the counts, untouched pixels keep every bit"""
    n = F.n
    assert int(picked) == len(chosen) == min(K, int(ok.sum()))
    S0, SL0, Q0, k0 = state_parts(before["state"], n)
    S1, SL1, Q1, k1 = state_parts(after["state"], n)
    want = k0.copy()
    want[chosen] += batch
    assert np.array_equal(k1, want) and np.array_equal(after["spp"], want)
    hit = np.zeros(n, bool)
    hit[chosen] = True
    for a, b in ((before["fb"], after["fb"]), (before["st"], after["st"]), (raw_bits(S0), raw_bits(S1)), (raw_bits(SL0), raw_bits(SL1)),
                 (raw_bits(Q0), raw_bits(Q1))):
        assert np.array_equal(a[~hit], b[~hit])
    return chosen


def check_round_filtered(sc, F, before, after, picked, K, p, batch=BATCH, max_spp=MAX_SPP):
    """one filtered round from `before` to `after`: the set of tests/filtered_budget_model.py on the snapshot and the scene's guides"""
    chosen, ok, _ = FM.select(sc.hits, before["state"], F.nx, F.ny, batch, max_spp, FLOOR, K, filt_of(p))
    return _check_whole_frame_round(F, before, after, picked, chosen, ok, K, batch)


def check_round_temporal(sc, F, before, after, picked, K, batch=BATCH, max_spp=MAX_SPP):
    """one history-aware round from `before` to `after`: the set of sc.model_select (tests/temporal_budget_model.py on the scene's
    history) on the snapshot, and every pixel holds what its k samples give"""
    chosen, ok, _ = sc.model_select(before["state"], K, batch, max_spp)
    _check_whole_frame_round(F, before, after, picked, chosen, ok, K, batch)
    check_exact(sc, F, after)
    return chosen
