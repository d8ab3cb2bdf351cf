"""rt_render_adaptive_part (-m gpu): adaptive sampling on parts of a frame, every comparison bit equality through the C ABI.

Every pixel has its own XORWOW stream keyed by its absolute pixel_index, so a part's adaptive render is the whole-frame
rt_render_adaptive re-placed into the part's compact tile-major buffers (include/rt_amd.h, rt_partition): element
local_tile * 64 + ly * 8 + lx.  Colours are compared after rt_assemble / rt_assemble_split; counts and RNG states through that
layout, mapped here in numpy.  The buffers start out as a sentinel: the padding of edge tiles must keep it (and the RNG states
what rt_render_init(part) wrote)."""
import numpy as np
import pytest

from adaptive_frames import adaptive_frame, part_layout, part_tuple
from bitcmp import raw_bits

pytestmark = pytest.mark.gpu

NX, NY = 203, 77                   # 26 x 10 = 260 tiles: ragged right and top edges; 5 runs of 64 tiles, the last one of 4
N, SPL = 10000, 32
MIN, BATCH, MAX = 4, 4, 32
FLOOR = 0.02
SENTINEL = 0x7FC0DEAD              # a NaN pattern nothing renders


def part_render(rt, torch, W, O, nx, ny, params, P, ctx=None, stream=None):
    """(fb [n, 3] float32, spp [n], state [n, 12] uint32, state after render_init [n, 12]) of one part, buffers pre-filled with SENTINEL"""
    n = rt.part_pixels(nx, ny, P)
    fb = torch.full((n * 3,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    spp = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    st = rt.alloc_rand_state(nx, ny, P)
    rt.render_init(nx, ny, st, P)
    torch.cuda.synchronize()
    st0 = st.cpu().numpy().view(np.uint32).reshape(-1, 12)
    if ctx is None:
        rt.render_adaptive_part(fb, nx, ny, params, W, st, O, spp, P)
    else:
        ctx.render_adaptive_part(fb, nx, ny, params, W, st, O, spp, P, stream=stream)
    torch.cuda.synchronize()
    return fb, spp.cpu().numpy(), st.cpu().numpy().view(np.uint32).reshape(-1, 12), st0


def check_part(rt, ref, nx, ny, P, got):
    """a part's counts and states against the whole frame through the layout; padding untouched"""
    r_spp, r_fb, r_st = ref
    fb, spp, st, st0 = got
    pix, inside = part_layout(nx, ny, part_tuple(P), rt.part_pixels(nx, ny, P))
    f = raw_bits(fb.cpu().numpy()).reshape(-1, 3)
    assert np.array_equal(spp[inside], r_spp[pix[inside]]), P
    assert np.array_equal(f[inside], raw_bits(r_fb)[pix[inside]]), P
    assert np.array_equal(st[inside], r_st[pix[inside]]), P
    assert (spp[~inside] == SENTINEL).all() and (f[~inside] == SENTINEL).all(), P
    assert np.array_equal(st[~inside], st0[~inside]), P


def runs_case(rt, torch, W, O, nx, ny, params, nparts, ref):
    """every part of an nparts runs split, checked one by one, and the colours through rt_assemble"""
    per = rt.part_pixels(nx, ny, rt.Partition(0, nparts))
    staged = torch.zeros(per * 3 * nparts, dtype=torch.float32, device="cuda")
    for p in range(nparts):
        P = rt.Partition(p, nparts)
        n = rt.part_pixels(nx, ny, P)
        if n == 0:
            continue
        got = part_render(rt, torch, W, O, nx, ny, params, P)
        check_part(rt, ref, nx, ny, P, got)
        staged[p * per * 3:(p * per + n) * 3] = got[0]
    full = rt.alloc_fb(nx, ny)
    rt.assemble(full, staged, nx, ny, nparts)
    torch.cuda.synchronize()
    assert np.array_equal(raw_bits(full.cpu().numpy()).reshape(-1, 3), raw_bits(ref[1])), nparts


def pick_rel_error(rt, torch, W, O, nx, ny, lo, step, hi):
    """the first target of a sweep whose frame mixes >= 3 distinct counts, early stops and capped pixels"""
    for rel in (0.02, 0.03, 0.05, 0.07, 0.1, 0.15, 0.2, 0.3, 0.5):
        P = rt.Adaptive(lo, hi, step, rel, FLOOR)
        ref = adaptive_frame(rt, torch, W, O, nx, ny, P)
        spp = ref[0]
        if len(np.unique(spp)) >= 3 and (spp < hi).any() and (spp == hi).any():
            return P, ref
    raise AssertionError("no rel_error in the sweep gives a mixed frame")


@pytest.fixture(scope="module")
def scene(rt, cuda):
    W = rt.World(N, NX, NY)
    O = rt.Octree(W, SPL)
    P, ref = pick_rel_error(rt, cuda, W, O, NX, NY, MIN, BATCH, MAX)
    yield dict(W=W, O=O, P=P, ref=ref)
    O.close()
    W.close()


@pytest.mark.parametrize("nparts", [2, 3, 8])
def test_runs_parts_equal_the_whole_frame(rt, cuda, scene, nparts):
    runs_case(rt, cuda, scene["W"], scene["O"], NX, NY, scene["P"], nparts, scene["ref"])


@pytest.mark.parametrize("starts", [[0, 130, 260], [0, 77, 200, 260]])
def test_range_parts_equal_the_whole_frame(rt, cuda, scene, starts):
    torch = cuda
    nparts = len(starts) - 1
    stride = max(b - a for a, b in zip(starts, starts[1:])) * 64
    staged = torch.zeros(stride * 3 * nparts, dtype=torch.float32, device="cuda")
    for p in range(nparts):
        P = rt.Partition(p, nparts, starts[p], starts[p + 1])
        got = part_render(rt, torch, scene["W"], scene["O"], NX, NY, scene["P"], P)
        check_part(rt, scene["ref"], NX, NY, P, got)
        staged[p * stride * 3:(p * stride + rt.part_pixels(NX, NY, P)) * 3] = got[0]
    full = rt.alloc_fb(NX, NY)
    rt.assemble_split(full, staged, NX, NY, starts, stride)
    torch.cuda.synchronize()
    assert np.array_equal(raw_bits(full.cpu().numpy()).reshape(-1, 3), raw_bits(scene["ref"][1]))


def test_more_parts_than_tiles(rt, cuda, scene):
    """300 parts of 260 tiles: parts 0-4 hold one run each, the others nothing — they return 0 and launch nothing"""
    torch = cuda
    W, O, P = scene["W"], scene["O"], scene["P"]
    L = rt.lib()
    import ctypes as C
    for p in (5, 150, 299):
        assert rt.part_pixels(NX, NY, rt.Partition(p, 300)) == 0
        assert L.rt_render_adaptive_part(None, NX, NY, C.byref(P), W.h, None, O.h, None, rt.Partition(p, 300), None) == 0
    for p in range(5):
        Q = rt.Partition(p, 300)
        check_part(rt, scene["ref"], NX, NY, Q, part_render(rt, torch, W, O, NX, NY, P, Q))


def test_one_part_is_the_whole_frame(rt, cuda, scene):
    """nparts == 1 without a range: the reference layout, exactly rt_render_adaptive"""
    torch = cuda
    st = rt.alloc_rand_state(NX, NY)
    fb = rt.alloc_fb(NX, NY)
    spp = torch.full((NX * NY,), -1, dtype=torch.int32, device="cuda")
    rt.render_init(NX, NY, st)
    rt.render_adaptive_part(fb, NX, NY, scene["P"], scene["W"], st, scene["O"], spp, rt.WHOLE)
    torch.cuda.synchronize()
    r_spp, r_fb, r_st = scene["ref"]
    assert np.array_equal(spp.cpu().numpy(), r_spp)
    assert np.array_equal(raw_bits(fb.cpu().numpy()).reshape(-1, 3), raw_bits(r_fb))
    assert np.array_equal(st.cpu().numpy().view(np.uint32).reshape(-1, 12), r_st)


def test_long_chain_round_0_on_parts(rt, cuda, scene):
    """min_spp >= 16: round 0 of every part runs rt_render(part)'s long-chain pass and sorted tail"""
    W, O = scene["W"], scene["O"]
    P, ref = pick_rel_error(rt, cuda, W, O, NX, NY, 16, 8, 40)
    runs_case(rt, cuda, W, O, NX, NY, P, 3, ref)


def test_context_on_a_side_stream(rt, cuda, scene):
    torch = cuda
    ctx = rt.RenderCtx()
    s = torch.cuda.Stream()
    for p in range(2):
        Q = rt.Partition(p, 2)
        check_part(rt, scene["ref"], NX, NY, Q, part_render(rt, torch, scene["W"], scene["O"], NX, NY, scene["P"], Q, ctx=ctx, stream=s.cuda_stream))
    ctx.close()


# (spheres, SPL or None = no octree, list traversal, nx, ny, kernel that rt_render launches for the scene)
PATHS = {
    "list_reference": (500, None, 0, 131, 71, "k_render<false,0,1>"),
    "octree_dense": (100000, 320, 1, 131, 71, "k_render<true,0,2>"),
}


@pytest.mark.parametrize("name", list(PATHS))
def test_other_paths(rt, cuda, name):
    n, spl, trav, nx, ny, kernel = PATHS[name]
    W = rt.World(n, nx, ny)
    O = rt.Octree(W, spl) if spl else None
    if O is None:
        W.set_list_traversal(trav)
    assert rt.render_kernel_name(W, O) == kernel
    P, ref = pick_rel_error(rt, cuda, W, O, nx, ny, MIN, BATCH, MAX)
    runs_case(rt, cuda, W, O, nx, ny, P, 2, ref)
    if O is not None:
        O.close()
    W.close()
