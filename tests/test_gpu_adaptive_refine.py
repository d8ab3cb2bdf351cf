"""rt_render_adaptive_begin / rt_render_adaptive_refine (-m gpu): every comparison is bit equality, no tolerances.

begin(P) is rt_render_adaptive_part(P) that also keeps every pixel's sums and count in a state of the caller's; refine(P -> Q)
continues that state and must leave fb, d_spp, the RNG states and the state bytes exactly as begin(Q) leaves them (include/rt_amd.h,
DESIGN.md §5.9 "Refinement").  Buffers start out as a sentinel: the padding of edge tiles in a part must keep it."""
import numpy as np
import pytest

from adaptive_frames import Frame, SENTINEL, state_parts
from bitcmp import assert_same_snapshots, raw_bits
from gpu_frames import frame_rows, render_frame

pytestmark = pytest.mark.gpu

NX, NY = 203, 77                   # 26 x 10 = 260 tiles: ragged right and top edges
N, SPL = 10000, 32
FLOOR = 0.02

P0 = (4, 64, 4, 0.2, FLOOR)        # (min_spp, max_spp, batch, rel_error, floor)
P1 = (4, 64, 4, 0.1, FLOOR)
P2 = (4, 128, 4, 0.05, FLOOR)


def chain(rt, torch, W, O, nx, ny, part, steps=(P0, P1, P2)):
    """begin(steps[0]) -> refine -> ... on one set of buffers, against begin(steps[-1]) on fresh ones; returns the snapshots"""
    F = Frame(rt, torch, nx, ny, part).begin(W, O, steps[0])
    seen = [F.snap()]
    for a, b in zip(steps, steps[1:]):
        F.refine(W, O, a, b)
        seen.append(F.snap())
    ref = Frame(rt, torch, nx, ny, part).begin(W, O, steps[-1]).snap()
    assert_same_snapshots(seen[-1], ref, part)
    inside = F.inside
    for x, y in zip(seen, seen[1:]):
        assert (y["spp"][inside] >= x["spp"][inside]).all()          # a refinement never takes a sample back
    return seen, ref, inside


@pytest.fixture(scope="module")
def scene(rt, cuda):
    W = rt.World(N, NX, NY)
    O = rt.Octree(W, SPL)
    yield W, O
    O.close()
    W.close()


# ---- 1. begin is rt_render_adaptive_part plus the state -----------------------------------------------------------------
@pytest.mark.parametrize("nparts", [1, 3])
def test_begin_equals_adaptive_part(rt, cuda, scene, nparts):
    W, O = scene
    for p in range(nparts):
        part = rt.Partition(p, nparts)
        F = Frame(rt, cuda, NX, NY, part).begin(W, O, P1)
        got = F.snap()
        R = Frame(rt, cuda, NX, NY, part)
        rt.render_adaptive_part(R.fb, NX, NY, rt.Adaptive(*P1), W, R.st, O, R.spp, part)
        ref = R.snap()
        for k in ("fb", "spp", "st"):
            assert np.array_equal(got[k], ref[k]), (part, k)
        # the state's layout: k is the count, sqrtf(S_rgb * (1/k)) the colour (the reciprocal in double, as rt_render)
        inside = F.inside
        S, SL, Q, k = state_parts(got["state"], F.n)
        assert np.array_equal(k[inside], got["spp"][inside])
        assert len(np.unique(k[inside])) >= 2
        kk = np.array([np.float32(1.0 / float(np.float32(x))) for x in k[inside]], np.float32)
        assert np.array_equal(raw_bits(np.sqrt(S[inside] * kk[:, None])), got["fb"][inside])
        assert (SL[inside] >= 0).all() and (Q[inside] >= 0).all()


# ---- 2. begin(P0) -> refine(P0 -> P1) -> refine(P1 -> P2) equals begin(P2) ------------------------------------------------
def test_chain_tree(rt, cuda, scene):
    W, O = scene
    seen, ref, inside = chain(rt, cuda, W, O, NX, NY, rt.WHOLE)
    assert (seen[2]["spp"] > seen[0]["spp"]).any() and (seen[2]["spp"] == seen[0]["spp"]).any()
    assert (ref["spp"] > 64).any() and len(np.unique(ref["spp"])) >= 3


# (spheres, SPL or None = no octree, traversal, kernel that rt_render launches for the scene)
PATHS = {
    "list": (500, None, 0, "k_render<false,0,1>"),
    "dense_grid": (100000, 320, 1, "k_render<true,0,2>"),
}


@pytest.mark.parametrize("name", list(PATHS))
def test_chain_other_paths(rt, cuda, name):
    n, spl, trav, kernel = PATHS[name]
    nx, ny = 131, 71
    W = rt.World(n, nx, ny)
    O = rt.Octree(W, spl) if spl else None
    if O is not None:
        O.set_traversal(trav)
    else:
        W.set_list_traversal(trav)
    assert rt.render_kernel_name(W, O) == kernel
    seen, ref, _ = chain(rt, cuda, W, O, nx, ny, rt.WHOLE)
    assert (seen[2]["spp"] > seen[0]["spp"]).any()
    if O is not None:
        O.close()
    W.close()


def test_chain_runs_of_three_parts(rt, cuda, scene):
    W, O = scene
    grew = False
    for p in range(3):
        seen, ref, inside = chain(rt, cuda, W, O, NX, NY, rt.Partition(p, 3))
        grew |= bool((seen[2]["spp"][inside] > seen[0]["spp"][inside]).any())
        assert (seen[2]["spp"][~inside] == SENTINEL).all() and (seen[2]["fb"][~inside] == SENTINEL).all()
    assert grew


@pytest.mark.parametrize("band", [0, 1])
def test_chain_range_part_keeps_its_padding(rt, cuda, scene, band):
    W, O = scene
    starts = [0, 130, 260]
    part = rt.Partition(band, 2, starts[band], starts[band + 1])
    seen, ref, inside = chain(rt, cuda, W, O, NX, NY, part)
    assert (~inside).any()
    n = rt.part_pixels(NX, NY, part)
    init = Frame(rt, cuda, NX, NY, part).snap()
    for got in seen:
        assert (got["spp"][~inside] == SENTINEL).all() and (got["fb"][~inside] == SENTINEL).all()
        assert np.array_equal(got["st"][~inside], init["st"][~inside])
        S, SL, Q, k = state_parts(got["state"], n)
        for a in (S[~inside], SL[~inside], Q[~inside], k[~inside]):
            assert (raw_bits(a) == 0xA5A5A5A5).all()


# ---- 3. refine reads only the state ----------------------------------------------------------------------------------------
def test_refine_ignores_fb_and_spp(rt, cuda, scene):
    W, O = scene
    F = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(W, O, P0)
    cuda.cuda.synchronize()
    F.fb.view(cuda.int32).fill_(SENTINEL)
    F.spp.fill_(SENTINEL)
    got = F.refine(W, O, P0, P2).snap()
    assert_same_snapshots(got, Frame(rt, cuda, NX, NY, rt.WHOLE).begin(W, O, P2).snap())


# ---- 4./5. zero targets: the uniform render --------------------------------------------------------------------------------
def test_zero_target_raising_max_spp_is_the_uniform_render(rt, cuda, scene):
    W, O = scene
    got = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(W, O, (4, 16, 4, 0.0, FLOOR)).refine(W, O, (4, 16, 4, 0.0, FLOOR), (4, 40, 4, 0.0, FLOOR)).snap()
    fb, st = frame_rows(*render_frame(rt, cuda, W, O, NX, NY, 40))
    assert (got["spp"] == 40).all()
    assert np.array_equal(got["fb"], raw_bits(fb)) and np.array_equal(got["st"], st)


def test_refine_to_zero_target_is_the_uniform_render(rt, cuda, scene):
    W, O = scene
    F = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(W, O, (4, 32, 4, 0.2, FLOOR))
    first = F.snap()
    assert (first["spp"] < 32).any()
    got = F.refine(W, O, (4, 32, 4, 0.2, FLOOR), (4, 48, 4, 0.0, FLOOR)).snap()
    fb, st = frame_rows(*render_frame(rt, cuda, W, O, NX, NY, 48))
    assert (got["spp"] == 48).all()
    assert np.array_equal(got["fb"], raw_bits(fb)) and np.array_equal(got["st"], st)


# ---- 6. refining to the same target changes nothing ------------------------------------------------------------------------
def test_refine_to_the_same_target_changes_nothing(rt, cuda, scene):
    W, O = scene
    F = Frame(rt, cuda, NX, NY, rt.Partition(1, 3)).begin(W, O, P1)
    before = F.snap()
    assert_same_snapshots(F.refine(W, O, P1, P1).snap(), before)


# ---- 7. C3 ---------------------------------------------------------------------------------------------------------------
def test_c3_refinement(rt, cuda):
    W = rt.World(10000, 1200, 800)
    O = rt.Octree(W, 32)
    a, b = (8, 64, 8, 0.2, FLOOR), (8, 128, 8, 0.1, FLOOR)
    seen, ref, _ = chain(rt, cuda, W, O, 1200, 800, rt.WHOLE, steps=(a, b))
    assert (seen[1]["spp"] > seen[0]["spp"]).any() and (seen[1]["spp"] == seen[0]["spp"]).any()
    O.close()
    W.close()


# ---- 8. the _on forms ----------------------------------------------------------------------------------------------------
def test_context_on_a_side_stream(rt, cuda, scene):
    torch = cuda
    W, O = scene
    ctx = rt.RenderCtx()
    s = torch.cuda.Stream()
    F = Frame(rt, torch, NX, NY, rt.WHOLE)
    torch.cuda.synchronize()
    ctx.render_adaptive_begin(F.fb, NX, NY, rt.Adaptive(*P0), W, F.st, F.state, O, F.spp, stream=s.cuda_stream)
    ctx.render_adaptive_refine(F.fb, NX, NY, rt.Adaptive(*P0), rt.Adaptive(*P1), W, F.st, F.state, O, F.spp, stream=s.cuda_stream)
    ctx.render_adaptive_refine(F.fb, NX, NY, rt.Adaptive(*P1), rt.Adaptive(*P2), W, F.st, F.state, O, F.spp, stream=s.cuda_stream)
    s.synchronize()
    assert len(ctx.times()) == 3
    assert_same_snapshots(F.snap(), Frame(rt, torch, NX, NY, rt.WHOLE).begin(W, O, P2).snap())
    ctx.close()

