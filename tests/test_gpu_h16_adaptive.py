"""rt_render_adaptive_h16 (-m gpu): the adaptive frame of a binary16 world from ONE render launch, the stop rule inside k_render_h<*,3>
(include/rt_amd_h16_adaptive.h, DESIGN.md §5.9 "Binary16").  Every comparison is bit equality, no tolerances.  The property the kernel
is held to: a pixel that stopped after k samples is rt_render(ns = k)'s pixel — colour and RNG state — and its count, its stop and
its state's record are those of tests/h16_adaptive_model.py on the GPU's own one-sample passes.  Buffers start out as sentinels
(h16_adaptive_frames.Frame): the padding of edge tiles in a part must keep them."""
import ctypes as C

import numpy as np
import pytest

import h16_adaptive_model as M
from adaptive_frames import SENTINEL, state_parts
from bitcmp import assert_same_snapshots, raw_bits
from h16_adaptive_frames import FLOOR, HI, LO, STEP, Frame, Scene16, check_model, check_padding, check_part_of_whole

pytestmark = pytest.mark.gpu

NX, NY = 64, 40                    # the model's frame
PX, PY = 203, 77                   # the parts' frame: 26 x 10 = 260 tiles, ragged right and top edges
WORLDS = {"tree": (10000, 32, False), "list": (500, None, False), "tree_gpu": (10000, 32, True)}      # spheres, SPL, rt_build_octree_gpu


@pytest.fixture(scope="module", params=list(WORLDS))
def scene(request, rt, cuda):
    n, spl, gpu = WORLDS[request.param]
    sc = Scene16(rt, cuda, n, spl, NX, NY, gpu=gpu, count=32)
    sc.name = request.param
    yield sc
    sc.close()


@pytest.fixture(scope="module")
def tree(rt, cuda):
    sc = Scene16(rt, cuda, *WORLDS["tree"][:2], NX, NY)
    yield sc
    sc.close()


@pytest.fixture(scope="module")
def parts(rt, cuda):
    """the 203x77 frame of the tree world, its swept target and the whole frame's snapshot"""
    sc = Scene16(rt, cuda, 10000, 32, PX, PY)
    assert sc.targets, "no rel_error of the sweep gives a mixed 203x77 frame"
    sc.P = (LO, HI, STEP, sc.targets[-1], FLOOR)
    sc.whole = Frame(rt, cuda, PX, PY, rt.WHOLE).first(sc.W, sc.O, sc.P).snap()
    assert M.mixed(sc.whole["spp"], HI)
    yield sc
    sc.close()


# ---- 1. the rule, 2. the truncation ----------------------------------------------------------------------------------------
def test_the_rule_and_the_truncation(rt, cuda, scene):
    sc = scene
    assert rt.render_kernel_name(sc.W, sc.O, 3) == "k_render_h<%s,3>" % ("true" if sc.O is not None else "false")
    assert sc.targets, "no rel_error of the sweep gives a mixed frame"
    between = 0
    for rel in sc.targets:                                                  # every mixed frame of the sweep is the model's
        P = (LO, HI, STEP, rel, FLOOR)
        snap = Frame(rt, cuda, NX, NY, rt.WHOLE).first(sc.W, sc.O, P).snap()
        check_model(sc, snap, P)
        between = max(between, int(((snap["spp"] > LO) & (snap["spp"] < HI)).sum()))
    # (the tightest mixed target may be mixed by a handful of pixels: some frame of the sweep stops at least a twentieth of the
    # pixels at an intermediate checkpoint, or the checkpoints between min_spp and max_spp are not exercised)
    assert between >= NX * NY // 20, between
    print(sc.name, "rel_error", P[3], "counts", dict(zip(*(a.tolist() for a in np.unique(snap["spp"], return_counts=True)))))
    assert M.mixed(snap["spp"], HI)
    # the pixels with count k hold rt_render(ns = k)'s colour and state; S the images of the binary16 sums of the first k colours
    for k in np.unique(snap["spp"]):
        at = snap["spp"] == k
        fb, st = sc.at_k(k)
        assert np.array_equal(snap["fb"][at], fb[at]) and np.array_equal(snap["st"][at], st[at]), k
        col = np.zeros((NX * NY, 3), np.float16)
        for s in range(k):
            col = M.add16(col, sc.samples[s].astype(np.float16))
        assert np.array_equal(raw_bits(state_parts(snap["state"], NX * NY)[0][at]), raw_bits(col.astype(np.float32)[at])), k
        assert np.array_equal(M.bits16(M.end_colour(col, k))[at], fb[at]), k                    # (the model's end of a pixel is rt_render's)


# ---- 3. limits -------------------------------------------------------------------------------------------------------------
def test_limits(rt, cuda, scene):
    sc = scene
    rel = sc.targets[-1]
    # rel_error = 0: rt_render(max_spp), byte for byte; min = max: no checkpoint; a huge finite rel_error: every pixel stops at min_spp
    for P, ns in (((LO, HI, STEP, 0.0, FLOOR), HI), ((12, 12, 4, rel, FLOOR), 12), ((LO, HI, STEP, 1e30, FLOOR), LO)):
        snap = Frame(rt, cuda, NX, NY, rt.WHOLE).first(sc.W, sc.O, P).snap()
        fb, st = sc.at_k(ns)
        assert (snap["spp"] == ns).all(), P
        assert np.array_equal(snap["fb"], fb) and np.array_equal(snap["st"], st), P
        check_model(sc, snap, P)
    # below every scheduling threshold; batch = 1; a cap past 24 (the binary16 sum's ulp grows, the binary32 statistics go on)
    for P in ((2, 6, 2, rel, FLOOR), (LO, HI, 1, rel, FLOOR), (LO, 32, STEP, rel, FLOOR)):
        snap = Frame(rt, cuda, NX, NY, rt.WHOLE).first(sc.W, sc.O, P).snap()
        check_model(sc, snap, P)
        assert len(np.unique(snap["spp"])) >= 2, P


# ---- 4. parts --------------------------------------------------------------------------------------------------------------
def check_part(rt, cuda, sc, part):
    F = Frame(rt, cuda, PX, PY, part).first(sc.W, sc.O, sc.P)
    snap = F.snap()
    check_part_of_whole(F, snap, sc.whole)
    out = check_padding(F, snap)
    # without a state (and without d_spp): the same fb, d_spp and RNG bytes, the state's bytes untouched
    G = Frame(rt, cuda, PX, PY, part).first(sc.W, sc.O, sc.P, state=False)
    bare = G.snap()
    for key in ("fb", "spp", "st"):
        assert np.array_equal(bare[key], snap[key]), key
    assert (bare["state"] == 0xA5).all()
    H = Frame(rt, cuda, PX, PY, part).first(sc.W, sc.O, sc.P, state=False, spp=False).snap()
    assert np.array_equal(H["fb"], snap["fb"]) and np.array_equal(H["st"], snap["st"]) and (H["spp"] == SENTINEL).all()
    return out


def test_runs_of_three_parts(rt, cuda, parts):
    padded = False
    for p in range(3):
        padded |= bool(check_part(rt, cuda, parts, rt.Partition(p, 3)).any())
    assert padded


@pytest.mark.parametrize("band", [0, 1])
def test_a_range_band(rt, cuda, parts, band):
    starts = [0, 130, 260]
    assert check_part(rt, cuda, parts, rt.Partition(band, 2, starts[band], starts[band + 1])).any()


def test_the_whole_frame_of_the_parts_is_the_truncation(rt, cuda, parts):
    snap = parts.whole
    check_model(parts, snap, parts.P)
    for k in np.unique(snap["spp"]):
        at = snap["spp"] == k
        fb, st = parts.at_k(k)
        assert np.array_equal(snap["fb"][at], fb[at]) and np.array_equal(snap["st"][at], st[at]), k


# ---- 5. scheduling does not change the pixel -------------------------------------------------------------------------------
def test_context_on_a_side_stream_reuses_the_schedule(rt, cuda, parts):
    torch = cuda
    ctx = rt.RenderCtx()
    s = torch.cuda.Stream()
    snaps, reuse = [], []
    for _ in range(2):
        F = Frame(rt, torch, PX, PY, rt.WHOLE, ctx=ctx, stream=s.cuda_stream).first(parts.W, parts.O, parts.P)
        s.synchronize()
        snaps.append(F.snap())
        reuse.append(ctx.schedule_reuse())
    assert reuse[1] == (reuse[0][0] + 1, reuse[0][1]), reuse
    assert_same_snapshots(snaps[1], snaps[0])
    assert_same_snapshots(snaps[0], parts.whole)
    assert len(ctx.times()) == 2
    counters = ctx.counters()
    assert counters["slots"] >= 260 * 64, counters
    assert len(ctx.schedule()) == len(rt.SCHEDULE_FIELDS)
    ctx.close()


# ---- 6. the refusals that need a GPU ---------------------------------------------------------------------------------------
def test_gpu_refusals(rt, cuda, tree):
    torch = cuda
    sc = tree
    L = rt.lib()
    F = Frame(rt, torch, NX, NY, rt.WHOLE)
    ok = rt.Adaptive(LO, HI, STEP, 0.1, FLOOR)
    before = F.snap()

    def call(world=sc.W, octree=sc.O, stream=None):
        s = rt._stream() if stream is None else stream
        return L.rt_render_adaptive_h16(F.fb.data_ptr(), NX, NY, C.byref(ok), world.h, F.st.data_ptr(), None if octree is None else octree.h,
                                        F.spp.data_ptr(), F.state.data_ptr(), rt.WHOLE, s)

    w32 = rt.World(500, NX, NY)
    t32 = rt.Octree(w32, 30)
    assert call(world=w32, octree=None) == -4 and call(world=w32, octree=t32) == -4          # the binary32 calls exist
    assert call(world=w32, octree=sc.O) == -1 and call(octree=t32) == -1                      # a tree of the other precision
    marker = torch.zeros(4, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        marker.add_(1.0)                                                                        # (the graph is not empty)
        rc = call(stream=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -1
    assert_same_snapshots(F.snap(), before)
    t32.close()
    w32.close()
    # ... and the call itself works on these buffers afterwards
    assert call() == 0
    check_model(sc, F.snap(), (LO, HI, STEP, 0.1, FLOOR))
