"""RT_ARITH_CONTRACT on every k_render variant, in both modes (-m gpu): the IEEE scheduling kernels of namespace rt feeding the contracted
render kernel of rt::fmac.

A contract world's pilot, ordering pass, counters and assembly are the kernels every world uses; only k_render is compiled a second time
with contraction allowed.  tests/test_gpu_contract.py holds that mode to its tolerance against the oracle on the sparse-grid variant and
the list; here each variant is reached once, on worlds of 64 x 40, and checked for what needs no tolerance and no measured number:
scheduling never changes a pixel, with or without contraction, so a frame must not depend on whether its pass was computed or kept, on
how it is cut into parts, or on what ran before it.

  k_render<false,*,1>   a list of 22 spheres (below the 64 from which a list gets a grid)
  k_render<true,*,5>    grid_threshold_worlds `switches/solo`    k_render<true,*,4>   `switches/nosolo`
  k_render<true,*,2>    `switches/sparse`                        k_render<true,*,1>   a tree with the reference traversal

Per world: (a) rt_render at 16 spp twice on one context, render_init before each — frames and RNG states byte-identical, and on the tree
variants the second call reused the kept pass (k_restore_counters, then the contracted kernel); (b) the frame rendered as three parts
and put together by rt_assemble is the whole frame (40 tiles in runs of 64: the first part holds them all, in a part's tile-major
layout, behind a part's ordering pass; the other two are empty); (c) four rt_render_progressive passes, run twice from fresh state,
byte-identical pass by pass."""
import numpy as np
import pytest

import grid_threshold_worlds as gw
import material_edge_worlds as mw

pytestmark = pytest.mark.gpu
NX, NY, NS = gw.NX, gw.NY, 16
# (id, last template argument of k_render, TREE)
CASES = [("list22", 1, False), ("solo", 5, True), ("nosolo", 4, True), ("sparse", 2, True), ("reference", 1, True)]


def make(rt, name):
    if name == "list22":
        return rt.World(22, NX, NY).upload(), None
    if name == "reference":
        W = rt.World(500, NX, NY).upload()
        return W, rt.Octree(W, 30).upload().set_traversal(rt.TRAVERSAL_REFERENCE)
    sp, cam = gw.world("switches", name, NX, NY)
    W = mw.gpu_world(rt, sp, cam, NX, NY).upload()
    return W, rt.Octree(W, gw.SPL_OF["switches", name]).upload()


def raw(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("name,variant,tree", CASES, ids=[c[0] for c in CASES])
def test_contracted_variant_behind_the_ieee_scheduling_kernels(rt, cuda, name, variant, tree):
    torch = cuda
    W, O = make(rt, name)
    W.set_arith(rt.ARITH_CONTRACT)
    for mode in (0, 1):
        assert rt.render_kernel_name(W, O, mode) == "k_render<%s,%d,%d>" % ("true" if tree else "false", mode, variant)

    # (a) twice on one context
    ctx = rt.RenderCtx()
    frames = []
    for call in range(2):
        st, fb = rt.alloc_rand_state(NX, NY), rt.alloc_fb(NX, NY)
        rt.render_init(NX, NY, st)
        ctx.render(fb, NX, NY, NS, W, st, O)
        torch.cuda.synchronize()
        frames.append((raw(fb), raw(st)))
    assert frames[0] == frames[1], "%s: the second rt_render on the context differs from the first" % name
    if tree:
        assert ctx.schedule_reuse() == (1, 1), ctx.schedule_reuse()
    ctx.close()
    assert np.frombuffer(frames[0][0], np.uint8).any()                     # (something was rendered)

    # (b) three parts, assembled
    nparts = 3
    per = rt.part_pixels(NX, NY, rt.Partition(0, nparts))
    staged = torch.zeros(per * 3 * nparts, dtype=torch.float32, device="cuda")
    held = 0
    for p in range(nparts):
        P = rt.Partition(p, nparts)
        n = rt.part_pixels(NX, NY, P)
        held += n
        if n == 0:
            continue
        st, fb = rt.alloc_rand_state(NX, NY, P), rt.alloc_fb(NX, NY, P)
        rt.render_init(NX, NY, st, P)
        rt.render(fb, NX, NY, NS, W, st, O, P)
        staged[p * per * 3:(p * per + n) * 3] = fb
    assert held >= NX * NY
    full = rt.alloc_fb(NX, NY)
    rt.assemble(full, staged, NX, NY, nparts)
    torch.cuda.synchronize()
    assert raw(full) == frames[0][0], "%s: the frame assembled from %d parts differs from the whole frame" % (name, nparts)

    # (c) four progressive passes, twice from fresh state
    runs = []
    for run in range(2):
        st, fb = rt.alloc_rand_state(NX, NY), rt.alloc_fb(NX, NY)
        rt.render_init(NX, NY, st)
        passes = []
        for k in range(1, 5):
            rt.render_progressive(fb, NX, NY, k, W, st, O)
            torch.cuda.synchronize()
            passes.append((raw(fb), raw(st)))
        runs.append(passes)
    for k in range(4):
        assert runs[0][k] == runs[1][k], "%s: progressive pass %d differs between two runs from fresh state" % (name, k + 1)
    assert runs[0][0] != runs[0][3]
    if O is not None:
        O.close()
    W.close()
