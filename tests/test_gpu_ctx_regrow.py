"""One render context through every way its workspaces grow (-m gpu): the scheduling workspace (and with it the kept schedule), the
progressive tile order, the adaptive lists and per-round counts, the budget workspace from its unfiltered to its filtered size, and at
the end a smaller frame in the workspace a larger one left.  After every step the buffers the call wrote — frame, sample counts, RNG
states, refinement state, pick counts — and what the call added to schedule_reuse() equal, byte for byte, what the same call with the
same inputs gives on a context created for it.  Consecutive scheduled steps differ in world or frame, so none of them meets a kept
schedule that a fresh context would not have."""
import pytest

pytestmark = pytest.mark.gpu
SMALL, LARGE = (16, 16), (72, 40)          # 2 x 2 tiles; 9 x 5 tiles with a ragged right edge


def test_every_regrow_path_of_one_context_matches_a_fresh_context(rt, cuda):
    torch = cuda
    worlds = {22: (rt.World(22, *LARGE), None)}
    w500 = rt.World(500, *LARGE)
    worlds[500] = (w500, rt.Octree(w500, 30))
    hits = rt.alloc_guides(*LARGE)
    rt.render_guides(worlds[22][0], None, LARGE[0], LARGE[1], hits)

    def start(size):
        fb, st = rt.alloc_fb(*size), rt.alloc_rand_state(*size)
        rt.render_init(size[0], size[1], st)
        return dict(fb=fb, st=st)

    def render(n, size, ns):
        def step(ctx, _):
            b, (W, O) = start(size), worlds[n]
            ctx.render(b["fb"], size[0], size[1], ns, W, b["st"], O)
            return b
        return step

    def progressive(n, size, passes):
        def step(ctx, _):
            b, (W, O) = start(size), worlds[n]
            for s in range(1, passes + 1):
                rt.check(rt.lib().rt_render_progressive_on(ctx.h, rt._dev(b["fb"]), size[0], size[1], s, W.h, rt._dev(b["st"]),
                                                           O.h if O is not None else None, rt.WHOLE, rt._stream()), "rt_render_progressive_on")
            return b
        return step

    def adaptive(n, size, P, begin=False):
        def step(ctx, _):
            b, (W, O) = start(size), worlds[n]
            b["spp"] = torch.zeros(size[0] * size[1], dtype=torch.int32, device="cuda")
            if begin:
                b["state"] = rt.alloc_adaptive_state(*size)
                ctx.render_adaptive_begin(b["fb"], size[0], size[1], P, W, b["st"], b["state"], O, b["spp"])
            else:
                ctx.render_adaptive(b["fb"], size[0], size[1], P, W, b["st"], O, b["spp"])
            return b
        return step

    def spend(n, size, B, filt=None):
        def step(ctx, prev):                     # continues the frame the previous step left: a copy of its buffers
            b, (W, O) = {k: v.clone() for k, v in prev.items()}, worlds[n]
            b["picked"] = torch.zeros(B.rounds, dtype=torch.int32, device="cuda")
            if filt is None:
                ctx.render_adaptive_spend(b["fb"], size[0], size[1], B, W, b["st"], b["state"], O, b["spp"], None, b["picked"])
            else:
                ctx.render_adaptive_spend_filtered(b["fb"], size[0], size[1], B, filt, hits, W, b["st"], b["state"], O, b["spp"], b["picked"])
            return b
        return step

    A1, A3 = rt.Adaptive(4, 8, 4, 0.05, 0.01), rt.Adaptive(4, 16, 4, 0.05, 0.01)
    B = rt.Budget(2000, 2, 4, 64, 0.01)
    steps = [
        ("render 16x16", render(22, SMALL, 16)),
        ("render 72x40: the scheduling workspace grows, the kept schedule is dropped", render(500, LARGE, 16)),
        ("progressive 16x16", progressive(22, SMALL, 3)),
        ("progressive 72x40: the kept tile order grows", progressive(500, LARGE, 3)),
        ("adaptive, 1 round", adaptive(22, SMALL, A1)),
        ("adaptive, 3 rounds: the lists and the per-round counts grow", adaptive(500, LARGE, A3)),
        ("adaptive begin", adaptive(22, LARGE, A1, begin=True)),
        ("spend: the budget workspace", spend(22, LARGE, B)),
        ("filtered spend: the budget workspace grows to the filtered size", spend(22, LARGE, B, rt.denoise_var_params())),
        ("render 16x16 in the larger workspace", render(22, SMALL, 16)),
    ]
    ctx, prev, before = rt.RenderCtx(), None, (0, 0)
    try:
        for name, step in steps:
            got = step(ctx, prev)
            after = ctx.schedule_reuse()
            fresh = rt.RenderCtx()
            try:
                want = step(fresh, prev)
                torch.cuda.synchronize()
                assert (after[0] - before[0], after[1] - before[1]) == fresh.schedule_reuse(), name
            finally:
                fresh.close()
            assert got.keys() == want.keys()
            for k in got:
                assert torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8)), "%s: %s differs from a fresh context's" % (name, k)
            assert bool((got["fb"] != 0).any()), name
            prev, before = got, after
    finally:
        ctx.close()
        for W, O in worlds.values():
            if O is not None:
                O.close()
            W.close()
