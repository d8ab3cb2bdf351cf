"""rt_render_adaptive_fused (-m gpu): the adaptive frame from ONE render launch, the stop rule inside k_render<*,3,*>.  Every comparison
is bit equality, no tolerances: with a state the call leaves fb, d_spp, the RNG states and the state bytes exactly as
rt_render_adaptive_begin leaves them, without one what rt_render_adaptive_part leaves (include/rt_amd_fused.h, DESIGN.md §5.9 "Fused").
Buffers start out as a sentinel (adaptive_frames.Frame): the padding of edge tiles in a part must keep it."""
import ctypes as C

import numpy as np
import pytest

from adaptive_frames import Frame, SENTINEL, pick_rel_error, progressive_samples, state_parts, stop_rule_model
from bitcmp import assert_same_snapshots, raw_bits
from gpu_frames import frame_rows, render_frame
import material_edge_worlds as mw

pytestmark = pytest.mark.gpu

NX, NY = 203, 77                   # 26 x 10 = 260 tiles: ragged right and top edges
FLOOR = 0.02
P = (4, 64, 4, 0.1, FLOOR)         # (min_spp, max_spp, batch, rel_error, floor)


def fused(F, W, O, params, state=True):
    """rt_render_adaptive_fused on the Frame's buffers (through its context and stream, if it has one)"""
    F._call("render_adaptive_fused", F.fb, F.nx, F.ny, F.rt.Adaptive(*params), W, F.st, F.state if state else None, O, F.spp, F.part)
    return F


def mixed(spp, lo, hi):
    """the condition of a frame that says something: >= 3 distinct counts, an early stop, a capped pixel"""
    return len(np.unique(spp)) >= 3 and bool((spp < hi).any()) and bool((spp == hi).any())


@pytest.fixture(scope="module")
def scene(rt, cuda):
    W = rt.World(10000, NX, NY)
    O = rt.Octree(W, 32)
    yield W, O
    O.close()
    W.close()


# ---- 1. against begin, on every path MODE 2 serves -------------------------------------------------------------------------
# (spheres, SPL or None = no octree, traversal or None = the default, frame, the fused kernel of the path)
PATHS = {
    "sparse_tree": (10000, 32, None, (203, 77), "k_render<true,3,4>"),
    "solo_chains": (500, 30, None, (203, 77), "k_render<true,3,5>"),
    "list": (500, None, 0, (131, 71), "k_render<false,3,1>"),               # (the reference's list scan: without it the list takes a grid of its own)
    "dense_grid": (100000, 320, 1, (131, 71), "k_render<true,3,2>"),
    "per_lane_tree": (500, 30, 0, (131, 71), "k_render<true,3,1>"),         # (the reference's tree walk: no candidate grid)
}


@pytest.mark.parametrize("name", list(PATHS))
def test_equals_begin_on_every_path(rt, cuda, name):
    n, spl, trav, (nx, ny), kernel = PATHS[name]
    W = rt.World(n, nx, ny)
    O = rt.Octree(W, spl) if spl else None
    if trav is not None:
        (O.set_traversal if O is not None else W.set_list_traversal)(trav)
    assert rt.render_kernel_name(W, O, 3) == kernel
    assert rt.render_kernel_name(W, O, 0) == kernel.replace(",3,", ",0,")
    params = P
    ref = Frame(rt, cuda, nx, ny, rt.WHOLE).begin(W, O, params).snap()
    if not mixed(ref["spp"], params[0], params[1]):                   # the condition is begin's own count map's
        samples, _ = progressive_samples(rt, cuda, W, O, nx, ny, params[1])
        params = (4, 64, 4, pick_rel_error(samples, 4, 4, 64, FLOOR), FLOOR)
        ref = Frame(rt, cuda, nx, ny, rt.WHOLE).begin(W, O, params).snap()
    print(name, "rel_error", params[3], "counts", np.unique(ref["spp"]).tolist())
    assert mixed(ref["spp"], params[0], params[1])
    got = fused(Frame(rt, cuda, nx, ny, rt.WHOLE), W, O, params).snap()
    assert_same_snapshots(got, ref, name)
    if O is not None:
        O.close()
    W.close()


# ---- 2. against the rule itself ---------------------------------------------------------------------------------------------
def test_equals_the_model_of_the_rule(rt, cuda):
    nx, ny, lo, hi, step = 64, 40, 4, 24, 4
    W = rt.World(10000, nx, ny)
    O = rt.Octree(W, 32)
    samples, states = progressive_samples(rt, cuda, W, O, nx, ny, hi)
    rel = pick_rel_error(samples, lo, step, hi, FLOOR)
    m_spp, m_fb = stop_rule_model(samples, rel, FLOOR, lo, step, hi)
    got = fused(Frame(rt, cuda, nx, ny, rt.WHOLE), W, O, (lo, hi, step, rel, FLOOR)).snap()
    assert np.array_equal(got["spp"], m_spp)
    assert np.array_equal(got["fb"], raw_bits(m_fb))
    assert np.array_equal(got["st"], states[m_spp - 1, np.arange(m_spp.size)])
    O.close()
    W.close()


# ---- 3. parts ---------------------------------------------------------------------------------------------------------------
def check_part(rt, cuda, W, O, part):
    F = fused(Frame(rt, cuda, NX, NY, part), W, O, P)
    got = F.snap()
    assert_same_snapshots(got, Frame(rt, cuda, NX, NY, part).begin(W, O, P).snap(), part)
    inside = F.inside
    init = Frame(rt, cuda, NX, NY, part).snap()
    assert (got["spp"][~inside] == SENTINEL).all() and (got["fb"][~inside] == SENTINEL).all()
    assert np.array_equal(got["st"][~inside], init["st"][~inside])
    for a in state_parts(got["state"], F.n):
        assert (raw_bits(a[~inside]) == 0xA5A5A5A5).all()
    return inside


def test_runs_of_three_parts(rt, cuda, scene):
    W, O = scene
    padded = False
    for p in range(3):
        padded |= bool((~check_part(rt, cuda, W, O, rt.Partition(p, 3))).any())
    assert padded


@pytest.mark.parametrize("band", [0, 1])
def test_range_part_keeps_its_padding(rt, cuda, scene, band):
    W, O = scene
    starts = [0, 130, 260]
    inside = check_part(rt, cuda, W, O, rt.Partition(band, 2, starts[band], starts[band + 1]))
    assert (~inside).any()


# ---- 4. no state ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nparts", [1, 3])
def test_without_a_state_equals_adaptive_part(rt, cuda, scene, nparts):
    W, O = scene
    part = rt.Partition(nparts - 1, nparts)
    got = fused(Frame(rt, cuda, NX, NY, part), W, O, P, state=False).snap()
    R = Frame(rt, cuda, NX, NY, part)
    rt.render_adaptive_part(R.fb, NX, NY, rt.Adaptive(*P), W, R.st, O, R.spp, part)
    ref = R.snap()
    assert_same_snapshots(got, ref, part)                                   # (the state bytes: the fill, untouched, in both)
    assert (got["state"] == 0xA5).all()
    # ... and d_spp is optional
    F = Frame(rt, cuda, NX, NY, part)
    rt.render_adaptive_fused(F.fb, NX, NY, rt.Adaptive(*P), W, F.st, None, O, None, part)
    again = F.snap()
    assert np.array_equal(again["fb"], ref["fb"]) and np.array_equal(again["st"], ref["st"]) and (again["spp"] == SENTINEL).all()


# ---- 5. limits --------------------------------------------------------------------------------------------------------------
def test_limits(rt, cuda, scene):
    W, O = scene
    for params, ns in (((4, 24, 4, 0.0, FLOOR), 24), ((4, 24, 4, 1e30, FLOOR), 4), ((12, 12, 4, 0.1, FLOOR), 12)):
        got = fused(Frame(rt, cuda, NX, NY, rt.WHOLE), W, O, params).snap()
        fb, st = frame_rows(*render_frame(rt, cuda, W, O, NX, NY, ns))
        assert (got["spp"] == ns).all(), params
        assert np.array_equal(got["fb"], raw_bits(fb)) and np.array_equal(got["st"], st), params
    F = Frame(rt, cuda, NX, NY, rt.WHOLE)
    bad = rt.Adaptive(4, 18, 4, 0.1, FLOOR)
    assert rt.lib().rt_render_adaptive_fused(F.fb.data_ptr(), NX, NY, C.byref(bad), W.h, F.st.data_ptr(), O.h, F.spp.data_ptr(), F.state.data_ptr(),
                                             rt.WHOLE, rt._stream()) == -1


# ---- 6. a NaN sample runs to the cap ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", [True, False])
def test_nan_samples_run_to_the_cap(rt, cuda, tree):
    """`extremes` at the size of its own GPU test (64x40, SPHERES_PER_LEAF 30), (4, 16, 4): the frame equals begin's; the condition,
    on begin's output: pixels whose state holds a NaN sum, all of them at max_spp"""
    nx, ny, params = 64, 40, (4, 16, 4, 0.1, FLOOR)
    sp, cam = mw.world("extremes", nx, ny, None, rt=rt)
    W = mw.gpu_world(rt, sp, cam, nx, ny)
    O = rt.Octree(W, 30) if tree else None
    ref = Frame(rt, cuda, nx, ny, rt.WHOLE).begin(W, O, params).snap()
    S, SL, Q, k = state_parts(ref["state"], nx * ny)
    nan = np.isnan(SL) | np.isnan(Q)
    print("extremes tree=%s: %d pixels hold a NaN sum" % (tree, nan.sum()))
    assert nan.sum() >= 1 and (k[nan] == params[1]).all() and (k < params[1]).any()
    assert_same_snapshots(fused(Frame(rt, cuda, nx, ny, rt.WHOLE), W, O, params).snap(), ref)
    if O is not None:
        O.close()
    W.close()


# ---- 7. the state continues -------------------------------------------------------------------------------------------------
def test_the_state_refines_and_spends_as_begins(rt, cuda, scene):
    W, O = scene
    P0, P1 = (4, 64, 4, 0.2, FLOOR), (4, 64, 4, 0.1, FLOOR)
    got = fused(Frame(rt, cuda, NX, NY, rt.WHOLE), W, O, P0).refine(W, O, P0, P1).snap()
    assert_same_snapshots(got, Frame(rt, cuda, NX, NY, rt.WHOLE).begin(W, O, P1).snap(), "refine")
    part = rt.Partition(1, 3)
    A, B = fused(Frame(rt, cuda, NX, NY, part), W, O, P1), Frame(rt, cuda, NX, NY, part).begin(W, O, P1)
    K = 2000
    pa, pb = A.spend(W, O, K, 1), B.spend(W, O, K, 1)
    assert np.array_equal(pa, pb) and int(pa[0]) > 0
    assert_same_snapshots(A.snap(), B.snap(), "spend")


# ---- 8. a context on a side stream ------------------------------------------------------------------------------------------
def test_context_on_a_side_stream_reuses_the_schedule(rt, cuda, scene):
    torch = cuda
    W, O = scene
    ctx = rt.RenderCtx()
    s = torch.cuda.Stream()
    snaps = []
    reuse = []
    for _ in range(2):
        F = Frame(rt, torch, NX, NY, rt.WHOLE, ctx=ctx, stream=s.cuda_stream)
        fused(F, W, O, P)
        s.synchronize()
        snaps.append(F.snap())
        reuse.append(ctx.schedule_reuse())
    assert reuse[1] == (reuse[0][0] + 1, reuse[0][1]), reuse
    assert_same_snapshots(snaps[1], snaps[0])
    assert_same_snapshots(snaps[0], Frame(rt, torch, NX, NY, rt.WHOLE).begin(W, O, P).snap())
    assert len(ctx.times()) == 2
    counters, sched = ctx.counters(), ctx.schedule()
    assert counters["slots"] >= 260 * 64 and counters["thin_waves"] == 0, counters
    assert len(sched) == len(rt.SCHEDULE_FIELDS)
    # begin shares the record: the same key, one more reuse
    F = Frame(rt, torch, NX, NY, rt.WHOLE, ctx=ctx, stream=s.cuda_stream).begin(W, O, P)
    s.synchronize()
    assert ctx.schedule_reuse() == (reuse[1][0] + 1, reuse[1][1])
    assert_same_snapshots(F.snap(), snaps[0])
    ctx.close()


# ---- 9. refusals: begin's codes ---------------------------------------------------------------------------------------------
def test_refusals_are_begins(rt, cuda, scene):
    torch = cuda
    W, O = scene
    L = rt.lib()
    F = Frame(rt, torch, NX, NY, rt.WHOLE)
    ok = rt.Adaptive(*P)

    def both(fb=F.fb.data_ptr(), nx=NX, ny=NY, params=ok, world=W, st=F.st.data_ptr(), octree=O, part=rt.WHOLE, stream=None):
        s = rt._stream() if stream is None else stream
        pp = None if params is None else C.byref(params)
        wh, oh = (None if world is None else world.h), (None if octree is None else octree.h)
        a = L.rt_render_adaptive_begin(fb, nx, ny, pp, wh, st, oh, F.spp.data_ptr(), F.state.data_ptr(), part, s)
        b = L.rt_render_adaptive_fused(fb, nx, ny, pp, wh, st, oh, F.spp.data_ptr(), F.state.data_ptr(), part, s)
        return a, b

    before = F.snap()
    for kw in (dict(params=rt.Adaptive(4, 18, 4, 0.1, FLOOR)), dict(params=rt.Adaptive(0, 16, 4, 0.1, FLOOR)), dict(params=rt.Adaptive(4, 16, 0, 0.1, FLOOR)),
               dict(params=rt.Adaptive(4, 16, 4, -0.1, FLOOR)), dict(params=rt.Adaptive(4, 16, 4, 0.1, -1.0)), dict(params=None), dict(world=None),
               dict(fb=None), dict(st=None), dict(nx=0), dict(ny=-3), dict(part=rt.Partition(3, 3)), dict(part=rt.Partition(0, 0)),
               dict(part=rt.Partition(0, 2, 0, 261)), dict(nx=1 << 17, ny=1 << 17)):
        a, b = both(**kw)
        assert a == b == -1, (kw, a, b)
    # a part without tiles: 0, nothing launched (NULL buffers are not even looked at)
    a, b = both(part=rt.Partition(7, 8), fb=None, st=None)
    assert a == b == 0
    # a tree of another precision, a binary16 world, a contracted world
    w16 = rt.World(500, NX, NY, precision=rt.FP16)
    assert both(world=w16) == (-1, -1)
    assert both(world=w16, octree=None) == (-4, -4)
    w16.close()
    wc = rt.World(500, NX, NY)
    wc.set_arith(rt.ARITH_CONTRACT)
    assert both(world=wc, octree=None) == (-4, -4)
    wc.close()
    # a capturing stream
    marker = torch.zeros(4, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        marker.add_(1.0)                                                    # (the graph is not empty)
        rc = both(stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == (-1, -1)
    assert_same_snapshots(F.snap(), before)
    # the _on forms without a context
    args = (F.fb.data_ptr(), NX, NY, C.byref(ok), W.h, F.st.data_ptr(), O.h, F.spp.data_ptr(), F.state.data_ptr(), rt.WHOLE, rt._stream())
    assert L.rt_render_adaptive_begin_on(None, *args) == L.rt_render_adaptive_fused_on(None, *args) == -1
