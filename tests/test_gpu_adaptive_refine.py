"""rt_render_adaptive_begin / rt_render_adaptive_refine (-m gpu): every comparison is bit equality, no tolerances.

begin(P) is rt_render_adaptive_part(P) that also keeps every pixel's sums and count in a state of the caller's; refine(P -> Q)
continues that state and must leave fb, d_spp, the RNG states and the state bytes exactly as begin(Q) leaves them (include/rt_amd.h,
DESIGN.md §5.9 "Refinement").  Buffers start out as a sentinel: the padding of edge tiles in a part must keep it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NX, NY = 203, 77                   # 26 x 10 = 260 tiles: ragged right and top edges
N, SPL = 10000, 32
FLOOR = 0.02
SENTINEL = 0x7FC0DEAD              # a NaN pattern nothing renders
STATE_FILL = 0xA5                  # every byte of a fresh state (padding elements keep it)
RUN = 64

P0 = (4, 64, 4, 0.2, FLOOR)        # (min_spp, max_spp, batch, rel_error, floor)
P1 = (4, 64, 4, 0.1, FLOOR)
P2 = (4, 128, 4, 0.05, FLOOR)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def layout_inside(rt, nx, ny, P):
    """for every element of a part buffer: whether it lies inside the frame (rt_partition's runs or range)"""
    n = rt.part_pixels(nx, ny, P)
    e = np.arange(n, dtype=np.int64)
    lt = e // 64
    if P.tile_end > P.tile_begin:
        tile = P.tile_begin + lt
    elif P.nparts == 1:
        return np.ones(n, bool)
    else:
        tile = ((lt // RUN) * P.nparts + P.part) * RUN + lt % RUN
    tiles_x = (nx + 7) // 8
    i = (tile % tiles_x) * 8 + (e % 64) % 8
    j = (tile // tiles_x) * 8 + (e % 64) // 8
    return (i < nx) & (j < ny)


class Frame:
    """the buffers of one part: fb and d_spp pre-filled with SENTINEL, RNG states from rt_render_init(part), a fresh state"""

    def __init__(self, rt, torch, nx, ny, part):
        self.rt, self.torch, self.nx, self.ny, self.part = rt, torch, nx, ny, part
        n = self.n = rt.part_pixels(nx, ny, part)
        self.fb = torch.full((n * 3,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        self.spp = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
        self.st = rt.alloc_rand_state(nx, ny, part)
        rt.render_init(nx, ny, self.st, part)
        self.state = torch.full((n * rt.ADAPTIVE_STATE_BYTES,), STATE_FILL, dtype=torch.uint8, device="cuda")

    def begin(self, W, O, P):
        self.rt.render_adaptive_begin(self.fb, self.nx, self.ny, ad(self.rt, P), W, self.st, self.state, O, self.spp, self.part)
        return self

    def refine(self, W, O, frm, to):
        self.rt.render_adaptive_refine(self.fb, self.nx, self.ny, ad(self.rt, frm), ad(self.rt, to), W, self.st, self.state, O, self.spp,
                                       self.part)
        return self

    def snap(self):
        self.torch.cuda.synchronize()
        return dict(fb=u32(self.fb.cpu().numpy()).reshape(-1, 3), spp=self.spp.cpu().numpy(),
                    st=self.st.cpu().numpy().view(np.uint32).reshape(-1, 12), state=self.state.cpu().numpy().copy())


def ad(rt, P):
    return rt.Adaptive(*P)


def same(a, b, what=""):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def state_parts(s, n):
    """the state's structure of arrays: S_rgb [n, 3], SL [n], Q [n] (float32), k [n] (int32)"""
    f = s.view(np.float32)
    return f[:3 * n].reshape(n, 3), f[3 * n:4 * n], f[4 * n:5 * n], s.view(np.int32)[5 * n:6 * n]


def chain(rt, torch, W, O, nx, ny, part, steps=(P0, P1, P2)):
    """begin(steps[0]) -> refine -> ... on one set of buffers, against begin(steps[-1]) on fresh ones; returns the snapshots"""
    F = Frame(rt, torch, nx, ny, part).begin(W, O, steps[0])
    seen = [F.snap()]
    for a, b in zip(steps, steps[1:]):
        F.refine(W, O, a, b)
        seen.append(F.snap())
    ref = Frame(rt, torch, nx, ny, part).begin(W, O, steps[-1]).snap()
    same(seen[-1], ref, part)
    inside = layout_inside(rt, nx, ny, part)
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
        rt.render_adaptive_part(R.fb, NX, NY, ad(rt, P1), W, R.st, O, R.spp, part)
        ref = R.snap()
        for k in ("fb", "spp", "st"):
            assert np.array_equal(got[k], ref[k]), (part, k)
        # the state's layout: k is the count, sqrtf(S_rgb * (1/k)) the colour (the reciprocal in double, as rt_render)
        inside = layout_inside(rt, NX, NY, part)
        S, SL, Q, k = state_parts(got["state"], F.n)
        assert np.array_equal(k[inside], got["spp"][inside])
        assert len(np.unique(k[inside])) >= 2
        kk = np.array([np.float32(1.0 / float(np.float32(x))) for x in k[inside]], np.float32)
        assert np.array_equal(u32(np.sqrt(S[inside] * kk[:, None])), got["fb"][inside])
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
            assert (u32(a) == 0xA5A5A5A5).all()


# ---- 3. refine reads only the state ----------------------------------------------------------------------------------------
def test_refine_ignores_fb_and_spp(rt, cuda, scene):
    W, O = scene
    F = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(W, O, P0)
    cuda.cuda.synchronize()
    F.fb.view(cuda.int32).fill_(SENTINEL)
    F.spp.fill_(SENTINEL)
    got = F.refine(W, O, P0, P2).snap()
    same(got, Frame(rt, cuda, NX, NY, rt.WHOLE).begin(W, O, P2).snap())


# ---- 4./5. zero targets: the uniform render --------------------------------------------------------------------------------
def uniform(rt, torch, W, O, nx, ny, ns):
    st = rt.alloc_rand_state(nx, ny)
    fb = rt.alloc_fb(nx, ny)
    rt.render_init(nx, ny, st)
    rt.render(fb, nx, ny, ns, W, st, O)
    torch.cuda.synchronize()
    return u32(fb.cpu().numpy()).reshape(-1, 3), st.cpu().numpy().view(np.uint32).reshape(-1, 12)


def test_zero_target_raising_max_spp_is_the_uniform_render(rt, cuda, scene):
    W, O = scene
    got = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(W, O, (4, 16, 4, 0.0, FLOOR)).refine(W, O, (4, 16, 4, 0.0, FLOOR), (4, 40, 4, 0.0, FLOOR)).snap()
    fb, st = uniform(rt, cuda, W, O, NX, NY, 40)
    assert (got["spp"] == 40).all()
    assert np.array_equal(got["fb"], fb) and np.array_equal(got["st"], st)


def test_refine_to_zero_target_is_the_uniform_render(rt, cuda, scene):
    W, O = scene
    F = Frame(rt, cuda, NX, NY, rt.WHOLE).begin(W, O, (4, 32, 4, 0.2, FLOOR))
    first = F.snap()
    assert (first["spp"] < 32).any()
    got = F.refine(W, O, (4, 32, 4, 0.2, FLOOR), (4, 48, 4, 0.0, FLOOR)).snap()
    fb, st = uniform(rt, cuda, W, O, NX, NY, 48)
    assert (got["spp"] == 48).all()
    assert np.array_equal(got["fb"], fb) and np.array_equal(got["st"], st)


# ---- 6. refining to the same target changes nothing ------------------------------------------------------------------------
def test_refine_to_the_same_target_changes_nothing(rt, cuda, scene):
    W, O = scene
    F = Frame(rt, cuda, NX, NY, rt.Partition(1, 3)).begin(W, O, P1)
    before = F.snap()
    same(F.refine(W, O, P1, P1).snap(), before)


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
    ctx.render_adaptive_begin(F.fb, NX, NY, ad(rt, P0), W, F.st, F.state, O, F.spp, stream=s.cuda_stream)
    ctx.render_adaptive_refine(F.fb, NX, NY, ad(rt, P0), ad(rt, P1), W, F.st, F.state, O, F.spp, stream=s.cuda_stream)
    ctx.render_adaptive_refine(F.fb, NX, NY, ad(rt, P1), ad(rt, P2), W, F.st, F.state, O, F.spp, stream=s.cuda_stream)
    s.synchronize()
    assert len(ctx.times()) == 3
    same(F.snap(), Frame(rt, torch, NX, NY, rt.WHOLE).begin(W, O, P2).snap())
    ctx.close()

