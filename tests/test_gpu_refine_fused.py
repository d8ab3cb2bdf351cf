"""rt_render_adaptive_refine_fused (-m gpu): a refinement from the seed pass and ONE render launch, k_render<*,4,*> over the seed's list.
Every comparison is bit equality, no tolerances: the call leaves fb, d_spp, the RNG states and the state bytes exactly as
rt_render_adaptive_refine(from -> to) leaves them, which is what rt_render_adaptive_begin(to) leaves (include/rt_amd_refine_fused.h,
DESIGN.md §5.9 "Fused refinement").  Buffers start out as a sentinel (adaptive_frames.Frame): the padding of edge tiles in a part
must keep it.  The shapes are those of tests/test_gpu_adaptive_refine.py."""
import ctypes as C

import numpy as np
import pytest

from adaptive_frames import Frame, SENTINEL, progressive_samples, state_parts, stop_rule_model
from bitcmp import assert_same_snapshots, raw_bits
from gpu_frames import frame_rows, render_frame
import material_edge_worlds as mw

pytestmark = pytest.mark.gpu

NX, NY = 203, 77                   # 26 x 10 = 260 tiles: ragged right and top edges
N, SPL = 10000, 32
FLOOR = 0.02

P0 = (4, 64, 4, 0.2, FLOOR)        # (min_spp, max_spp, batch, rel_error, floor)
P1 = (4, 64, 4, 0.1, FLOOR)
P2 = (4, 128, 4, 0.05, FLOOR)


def refine_fused(F, W, O, frm, to):
    """rt_render_adaptive_refine_fused on the Frame's buffers (through its context and stream, if it has one)"""
    F._call("render_adaptive_refine_fused", F.fb, F.nx, F.ny, F.rt.Adaptive(*frm), F.rt.Adaptive(*to), W, F.st, F.state, O, F.spp, F.part)
    return F


def begin_fused(F, W, O, params):
    """rt_render_adaptive_fused with a state"""
    F._call("render_adaptive_fused", F.fb, F.nx, F.ny, F.rt.Adaptive(*params), W, F.st, F.state, O, F.spp, F.part)
    return F


def says_something(before, after, batch, cap):
    """the four conditions of a refinement that exercises the kernel, on count maps of in-frame pixels: a pixel gained samples, a pixel
    kept its count, a pixel passed at least two checkpoints and stopped below the cap, a pixel reached the cap in this refinement"""
    gained = after - before
    return (bool((gained > 0).any()), bool((gained == 0).any()), bool(((gained >= 2 * batch) & (after < cap)).any()),
            bool(((after == cap) & (gained > 0)).any()))


@pytest.fixture(scope="module")
def scene(rt, cuda):
    W = rt.World(N, NX, NY)
    O = rt.Octree(W, SPL)
    refs = {}

    def begun(part, params):
        """what begin(params) leaves on fresh buffers of the part: computed once, never written"""
        key = ((part.part, part.nparts, part.tile_begin, part.tile_end), params)
        if key not in refs:
            refs[key] = Frame(rt, cuda, NX, NY, part).begin(W, O, params).snap()
        return refs[key]

    yield W, O, begun
    O.close()
    W.close()


# ---- 1. against the rounds and against begin(to), on every path MODE 2 serves -----------------------------------------------------
# (spheres, SPL or None = no octree, traversal or None = the default, frame, the kernel of the path): test_gpu_adaptive_fused.py's PATHS
PATHS = {
    "sparse_tree": (10000, 32, None, (203, 77), "k_render<true,4,4>"),
    "solo_chains": (500, 30, None, (203, 77), "k_render<true,4,5>"),
    "list": (500, None, 0, (131, 71), "k_render<false,4,1>"),
    "dense_grid": (100000, 320, 1, (131, 71), "k_render<true,4,2>"),
    "per_lane_tree": (500, 30, 0, (131, 71), "k_render<true,4,1>"),
}
SWEEP = (0.02, 0.03, 0.05, 0.07, 0.1, 0.15, 0.2, 0.3, 0.5)          # adaptive_frames.pick_rel_error's targets


def pick_pair(samples, lo, step, hi):
    """the first (from, to) of the sweep, tightest `to` first, whose refinement meets the four conditions by the model of the rule"""
    spp = {rel: stop_rule_model(samples, rel, FLOOR, lo, step, hi)[0] for rel in SWEEP}
    for to in SWEEP:
        for frm in SWEEP:
            if frm > to and all(says_something(spp[frm], spp[to], step, hi)):
                return frm, to
    raise AssertionError("no pair of the sweep gives a refinement that meets the four conditions")


@pytest.mark.parametrize("name", list(PATHS))
def test_equals_the_rounds_and_begin_on_every_path(rt, cuda, name):
    n, spl, trav, (nx, ny), kernel = PATHS[name]
    W = rt.World(n, nx, ny)
    O = rt.Octree(W, spl) if spl else None
    if trav is not None:
        (O.set_traversal if O is not None else W.set_list_traversal)(trav)
    assert rt.render_kernel_name(W, O, 4) == kernel
    assert rt.render_kernel_name(W, O, 0) == kernel.replace(",4,", ",0,")
    frm, to = P0, P1

    def rounds(frm, to):
        F = Frame(rt, cuda, nx, ny, rt.WHOLE).begin(W, O, frm)
        before = F.snap()
        return before, F.refine(W, O, frm, to).snap()

    before, ref = rounds(frm, to)
    if not all(says_something(before["spp"], ref["spp"], to[2], to[1])):           # the conditions are the rounds' own count maps'
        samples, _ = progressive_samples(rt, cuda, W, O, nx, ny, 64)
        a, b = pick_pair(samples, 4, 4, 64)
        frm, to = (4, 64, 4, a, FLOOR), (4, 64, 4, b, FLOOR)
        before, ref = rounds(frm, to)
    print(name, "rel_error", frm[3], "->", to[3], "counts", np.unique(before["spp"]).tolist(), "->", np.unique(ref["spp"]).tolist(),
          "listed", int((ref["spp"] > before["spp"]).sum()))
    assert says_something(before["spp"], ref["spp"], to[2], to[1]) == (True, True, True, True)
    got = refine_fused(Frame(rt, cuda, nx, ny, rt.WHOLE).begin(W, O, frm), W, O, frm, to).snap()
    assert_same_snapshots(got, ref, name + ": the rounds")
    assert_same_snapshots(got, Frame(rt, cuda, nx, ny, rt.WHOLE).begin(W, O, to).snap(), name + ": begin(to)")
    if O is not None:
        O.close()
    W.close()


# ---- 2. chains, on the same buffers each time ------------------------------------------------------------------------------------
CHAINS = {
    "fused_fused": (Frame.begin, (refine_fused, refine_fused)),
    "rounds_fused": (Frame.begin, (Frame.refine, refine_fused)),
    "fused_rounds": (Frame.begin, (refine_fused, Frame.refine)),
    "fused_begin": (begin_fused, (refine_fused, refine_fused)),
}


@pytest.mark.parametrize("name", list(CHAINS))
def test_chains_equal_begin(rt, cuda, scene, name):
    W, O, begun = scene
    first, steps = CHAINS[name]
    ref = begun(rt.WHOLE, P2)
    assert (ref["spp"] > 64).any() and len(np.unique(ref["spp"])) >= 3
    F = first(Frame(rt, cuda, NX, NY, rt.WHOLE), W, O, P0)
    seen = [F.snap()]
    for step, (a, b) in zip(steps, ((P0, P1), (P1, P2))):
        step(F, W, O, a, b)
        seen.append(F.snap())
    assert_same_snapshots(seen[1], begun(rt.WHOLE, P1), name + ": P1")
    assert_same_snapshots(seen[2], ref, name + ": P2")
    for x, y in zip(seen, seen[1:]):
        assert (y["spp"] >= x["spp"]).all() and (y["spp"] > x["spp"]).any()        # never a sample back, and each step had work


def test_a_refinement_may_skip_a_target(rt, cuda, scene):
    """P0 -> P2 directly, from a fused begin: pixels resume from 4 .. 64 samples and run up to 128"""
    W, O, begun = scene
    got = refine_fused(begin_fused(Frame(rt, cuda, NX, NY, rt.WHOLE), W, O, P0), W, O, P0, P2).snap()
    assert_same_snapshots(got, begun(rt.WHOLE, P2))


# ---- 3. parts --------------------------------------------------------------------------------------------------------------------
def check_part(rt, cuda, scene, part):
    W, O, begun = scene
    F = refine_fused(Frame(rt, cuda, NX, NY, part).begin(W, O, P0), W, O, P0, P1)
    got = F.snap()
    assert_same_snapshots(got, Frame(rt, cuda, NX, NY, part).begin(W, O, P0).refine(W, O, P0, P1).snap(), (part, "the rounds"))
    assert_same_snapshots(got, begun(part, P1), (part, "begin(to)"))
    inside = F.inside
    init = Frame(rt, cuda, NX, NY, part).snap()
    assert (got["spp"][~inside] == SENTINEL).all() and (got["fb"][~inside] == SENTINEL).all()
    assert np.array_equal(got["st"][~inside], init["st"][~inside])
    for a in state_parts(got["state"], F.n):
        assert (raw_bits(a[~inside]) == 0xA5A5A5A5).all()
    assert (got["spp"][inside] > begun(part, P0)["spp"][inside]).any()
    return inside


def test_runs_of_three_parts(rt, cuda, scene):
    padded = False
    for p in range(3):
        padded |= bool((~check_part(rt, cuda, scene, rt.Partition(p, 3))).any())
    assert padded


@pytest.mark.parametrize("band", [0, 1])
def test_range_part_keeps_its_padding(rt, cuda, scene, band):
    starts = [0, 130, 260]
    inside = check_part(rt, cuda, scene, rt.Partition(band, 2, starts[band], starts[band + 1]))
    assert (~inside).any()


# ---- 4. limits -------------------------------------------------------------------------------------------------------------------
def test_to_zero_target_is_the_uniform_render(rt, cuda, scene):
    W, O, _ = scene
    fb, st = frame_rows(*render_frame(rt, cuda, W, O, NX, NY, 24))
    # (1e18: the largest power of ten whose square times max_spp - 1 is finite in binary32 - the refinement rule refuses 1e30 as a
    # `from`, in both refines - and under it every pixel stops at min_spp)
    for frm_rel, all_at_min in ((0.1, False), (1e18, True)):
        frm, to = (4, 24, 4, frm_rel, FLOOR), (4, 24, 4, 0.0, FLOOR)
        F = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(W, O, frm)
        first = F.snap()["spp"]
        assert (first == 4).all() if all_at_min else ((first < 24).any() and (first > 4).any())
        got = refine_fused(F, W, O, frm, to).snap()
        assert (got["spp"] == 24).all(), frm
        assert np.array_equal(got["fb"], raw_bits(fb)) and np.array_equal(got["st"], st), frm
    F = Frame(rt, cuda, NX, NY, rt.WHOLE)
    a, b = rt.Adaptive(4, 24, 4, 1e30, FLOOR), rt.Adaptive(4, 24, 4, 0.0, FLOOR)
    args = (F.fb.data_ptr(), NX, NY, C.byref(a), C.byref(b), W.h, F.st.data_ptr(), O.h, F.spp.data_ptr(), F.state.data_ptr(), rt.WHOLE, rt._stream())
    assert rt.lib().rt_render_adaptive_refine(*args) == rt.lib().rt_render_adaptive_refine_fused(*args) == -1


def test_the_same_target_changes_nothing(rt, cuda, scene):
    """an empty list: the render kernel is launched on zero slots and every lane retires"""
    W, O, begun = scene
    for part in (rt.WHOLE, rt.Partition(1, 3)):
        F = Frame(rt, cuda, NX, NY, part).begin(W, O, P1)
        before = F.snap()
        assert_same_snapshots(before, begun(part, P1))
        assert_same_snapshots(refine_fused(F, W, O, P1, P1).snap(), before, part)


def test_only_the_cap_moves(rt, cuda, scene):
    W, O, _ = scene
    frm, to = (4, 32, 4, 0.1, FLOOR), (4, 128, 4, 0.1, FLOOR)
    F = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(W, O, frm)
    first = F.snap()["spp"]
    got = refine_fused(F, W, O, frm, to).snap()
    assert_same_snapshots(got, Frame(rt, cuda, NX, NY, rt.WHOLE).begin(W, O, to).snap())
    assert np.array_equal(got["spp"][first < 32], first[first < 32]) and (got["spp"][first == 32] > 32).any()


def test_fb_and_spp_are_never_read(rt, cuda, scene):
    W, O, begun = scene
    F = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(W, O, P0)
    cuda.cuda.synchronize()
    F.fb.view(cuda.int32).fill_(SENTINEL)
    F.spp.fill_(SENTINEL)
    assert_same_snapshots(refine_fused(F, W, O, P0, P2).snap(), begun(rt.WHOLE, P2))


# ---- 5. a NaN sample runs to the cap ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", [True, False])
def test_nan_samples_run_to_the_cap(rt, cuda, tree):
    nx, ny, frm, to = 64, 40, (4, 16, 4, 0.1, FLOOR), (4, 32, 4, 0.1, FLOOR)
    sp, cam = mw.world("extremes", nx, ny, None, rt=rt)
    W = mw.gpu_world(rt, sp, cam, nx, ny)
    O = rt.Octree(W, 30) if tree else None
    ref = Frame(rt, cuda, nx, ny, rt.WHOLE).begin(W, O, to).snap()
    S, SL, Q, k = state_parts(ref["state"], nx * ny)
    nan = np.isnan(SL) | np.isnan(Q)
    print("extremes tree=%s: %d pixels hold a NaN sum" % (tree, nan.sum()))
    assert nan.sum() >= 1 and (k[nan] == to[1]).all() and (k < to[1]).any()
    assert_same_snapshots(refine_fused(Frame(rt, cuda, nx, ny, rt.WHOLE).begin(W, O, frm), W, O, frm, to).snap(), ref)
    if O is not None:
        O.close()
    W.close()


# ---- 6. a context on a side stream -----------------------------------------------------------------------------------------------
def test_context_on_a_side_stream(rt, cuda, scene):
    torch = cuda
    W, O, begun = scene
    ctx = rt.RenderCtx()
    s = torch.cuda.Stream()
    snaps = []
    for _ in range(2):
        F = Frame(rt, torch, NX, NY, rt.WHOLE).begin(W, O, P0)          # (begun on the world's own context: the context's times are the refinements')
        torch.cuda.synchronize()
        ctx.render_adaptive_refine_fused(F.fb, NX, NY, rt.Adaptive(*P0), rt.Adaptive(*P1), W, F.st, F.state, O, F.spp, stream=s.cuda_stream)
        s.synchronize()
        snaps.append(F.snap())
    assert_same_snapshots(snaps[1], snaps[0])
    assert len(ctx.times()) == 2
    assert_same_snapshots(snaps[0], refine_fused(Frame(rt, torch, NX, NY, rt.WHOLE).begin(W, O, P0), W, O, P0, P1).snap(), "the default context")
    assert_same_snapshots(snaps[0], begun(rt.WHOLE, P1))
    ctx.close()


# ---- 7. the state continues ------------------------------------------------------------------------------------------------------
def test_the_state_spends_as_the_rounds_state(rt, cuda, scene):
    W, O, _ = scene
    part = rt.Partition(1, 3)
    A = refine_fused(Frame(rt, cuda, NX, NY, part).begin(W, O, P0), W, O, P0, P1)
    B = Frame(rt, cuda, NX, NY, part).begin(W, O, P0).refine(W, O, P0, P1)
    K = 2000
    pa, pb = A.spend(W, O, K, 1), B.spend(W, O, K, 1)
    assert np.array_equal(pa, pb) and int(pa[0]) > 0
    assert_same_snapshots(A.snap(), B.snap(), "spend")


# ---- 8. refusals on the device ---------------------------------------------------------------------------------------------------
def test_refusals_on_the_device(rt, cuda, scene):
    torch = cuda
    W, O, _ = scene
    L = rt.lib()
    F = Frame(rt, torch, NX, NY, rt.WHOLE).begin(W, O, P0)
    a, b = rt.Adaptive(*P0), rt.Adaptive(*P1)

    def both(world=W, stream=None):
        s = rt._stream() if stream is None else stream
        args = (F.fb.data_ptr(), NX, NY, C.byref(a), C.byref(b), world.h, F.st.data_ptr(), O.h, F.spp.data_ptr(), F.state.data_ptr(), rt.WHOLE, s)
        return L.rt_render_adaptive_refine(*args), L.rt_render_adaptive_refine_fused(*args)

    before = F.snap()
    # a tree of another precision
    w16 = rt.World(500, NX, NY, precision=rt.FP16)
    assert both(world=w16) == (-1, -1)
    w16.close()
    # a capturing stream (the graph is captured and never replayed)
    marker = torch.zeros(4, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        marker.add_(1.0)                                                    # (the graph is not empty)
        rc = both(stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == (-1, -1)
    assert_same_snapshots(F.snap(), before)
