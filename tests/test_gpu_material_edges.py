"""Shading at its branches (-m gpu): scatter(), the 50-bounce loop of color(), the camera and sky() of k_render / k_render_h, and the
accelerator builds, on the worlds of tests/material_edge_worlds.py — several refractive indices in one world (the per-sphere shade
table of world_upload), ref_idx below 1, 0, negative, inf and NaN, negative radii (shells, rooms no path leaves: every pixel a long
chain that ends at the depth limit), albedo 0 and 1e30, fuzz 0 and 1, radius 0 / NaN / inf, lens radius 0, slot 0 a ghost or the room.

Every comparison is bit equality with the CPU oracle; a NaN compares as "NaN where the oracle has NaN" (bitcmp.same_nan_as_ref).
tests/test_material_edge_worlds_host.py shows on the oracle alone that each world reaches the branch it is named for.

Two statements of the issue this file was written for are restated, because the code (rightly) does otherwise:
  * the candidate grids register a sphere by radius * radius, so a negative radius is stored like its positive twin and is NOT sent
    to the large list; the `!(r2 >= 0)` rule of the builds catches a NaN radius.  Asserted here: the grid of a world equals the grid
    of its |radius| twin, and `extremes` (a NaN and an inf radius) has its large spheres.
  * a pixel whose NaN sample comes after the check that stopped it never sees that sample.  Asserted: a pixel with a NaN among the
    samples it TOOK ran to max_spp (rt_amd.h: "a NaN sample makes the comparison false: such a pixel runs to max_spp")."""
import numpy as np
import pytest

import material_edge_worlds as mw
from adaptive_frames import adaptive_frame, pick_rel_error, progressive_samples, stop_rule_model
from bitcmp import f32_bits, same_nan_as_ref
from gpu_frames import render_frame, states_of
from tree_compare import compare
from world_cases import f32_to_half_bits, half_bits

pytestmark = pytest.mark.gpu

NX, NY, NS, SPL = 64, 40, 16, 30
FLOOR = 0.02


def make(rt, name, variant=None, nx=NX, ny=NY, tree=False):
    """(spheres, camera, World, Octree or None): the camera from rt_camera_init, the same floats for the oracle"""
    sp, cam = mw.world(name, nx, ny, variant, rt=rt)
    W = mw.gpu_world(rt, sp, cam, nx, ny)
    return sp, cam, W, (rt.Octree(W, SPL) if tree else None)


_oracle_frames = {}


def oracle_frame(name, variant, tree, nx=NX, ny=NY, ns=NS, sp=None, key=None):
    """the oracle's frame and states of a world, computed once per module and never written to"""
    k = (name, variant, tree, nx, ny, ns, key)
    if k not in _oracle_frames:
        s, cam = mw.world(name, nx, ny, variant)
        fb, st = mw.oracle(s if sp is None else sp, cam, nx, ny, tree=tree, spl=SPL).render(ns, nthreads=8)
        fb.setflags(write=False); st.setflags(write=False)
        _oracle_frames[k] = (fb, st)
    return _oracle_frames[k]


def test_the_closed_form_camera_is_the_librarys(rt):
    for nx, ny, aperture in ((NX, NY, None), (61, 35, None), (NX, NY, 0.0), (131, 99, None)):
        assert np.array_equal(f32_bits(mw.camera_floats(nx, ny, aperture)), f32_bits(mw.library_camera(rt, nx, ny, aperture)))


@pytest.mark.parametrize("name,variant", mw.WORLDS)
def test_list_grid_is_on_and_blind_to_the_sign_of_a_radius(rt, name, variant):
    sp, cam, W, _ = make(rt, name, variant)
    info = W.list_accel_info()
    assert info["enabled"]
    twin = mw.gpu_world(rt, mw.with_positive_radii(sp), cam, NX, NY)
    assert twin.list_accel_info() == info
    if name == "extremes":
        odd = ~(sp["radius"] * sp["radius"] < np.inf) & (sp["material"] != mw.MAT_NONE)
        assert odd[1:].sum() == 2 and info["large_spheres"] >= 2           # radius NaN and inf: never in a column of the grid


# ---------------------------------------------------------------------------------------------------- hit records
@pytest.mark.parametrize("name,variant", [("glass_indices", None), ("shells", None), ("shells", "hollow"), ("tir_room", None), ("extremes", None)])
def test_hit_records(rt, cuda, name, variant):
    """100 000 rays (a quarter from inside negative-radius spheres and the glass of shells, some exactly through the radius-0 sphere's
    centre) through the list and the tree, fast and reference traversal: sphere, t, p and normal equal the oracle's"""
    torch = cuda
    nrays = 100_000
    sp, cam, W, O = make(rt, name, variant, tree=True)
    rays = mw.edge_rays(sp, nrays, 11)
    d_rays = torch.from_numpy(rays).cuda()
    S = mw.oracle(sp, cam, NX, NY, tree=True, spl=SPL)
    ref_list, ref_tree = S.trace(rays, mode=1), S.trace(rays, mode=2)
    neg = mw.negative(sp)
    if neg.size:
        assert np.isin(ref_list["sphere"], neg).mean() >= 0.05
    for label, oct_, mode, ref in (("list", None, rt.TRAVERSAL_FAST, ref_list), ("list_reference", None, rt.TRAVERSAL_REFERENCE, ref_list),
                                  ("tree_reference", O, rt.TRAVERSAL_REFERENCE, ref_tree), ("tree", O, rt.TRAVERSAL_FAST, ref_tree)):
        if oct_ is not None:
            oct_.set_traversal(mode)
        else:
            W.set_list_traversal(mode)
        d_out = torch.zeros(nrays * 32, dtype=torch.uint8, device="cuda")
        rt.trace_rays(W, oct_, d_rays, nrays, d_out)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().view(rt.hit_record_dtype)
        assert np.array_equal(got["sphere"], ref["sphere"]), label
        assert same_nan_as_ref(got["t"], ref["t"]), label
        assert same_nan_as_ref(got["p"], ref["p"]), label
        assert same_nan_as_ref(got["normal"], ref["normal"]), label


# ---------------------------------------------------------------------------------------------------- builds
@pytest.mark.parametrize("name,variant", mw.WORLDS)
def test_device_build_equals_host_build(rt, cuda, name, variant):
    """rt_build_octree_gpu against rt_build_octree, array for array.  A negative radius shrinks a node's box: a shell is stored only
    where its centre lies deeper than |r| inside a leaf cell and matches no child box otherwise (silently: only a rejection at the
    root counts as dropped), so the tree holds fewer entries than that of the |radius| twin, but some of negative radius.  An inf
    radius is stored in every leaf, a NaN radius in none."""
    sp, cam, W, _ = make(rt, name, variant)
    H, G = compare(rt, W.upload(), SPL)
    S = mw.oracle(sp, cam, NX, NY, tree=True, spl=SPL)
    assert H.info()["dropped_outside"] == S.info()["dropped_outside"] and H.info()["leaf_count"] == S.info()["leaf_count"]
    neg = mw.negative(sp)
    if neg.size:
        twin = rt.Octree(mw.gpu_world(rt, mw.with_positive_radii(sp), cam, NX, NY), SPL)
        assert H.info()["flat_entries"] < twin.info()["flat_entries"]
        counts, idx = G.leaves()
        stored = np.unique(idx[np.arange(idx.shape[1])[None, :] < counts[:, None]])
        assert np.intersect1d(stored, neg).size >= (20 if name == "shells" else 1)


@pytest.mark.parametrize("name", ["glass_indices", "shells"])
def test_device_build_equals_host_build_binary16(rt, cuda, name):
    sp, cam = mw.half_world(rt, name, NX, NY)
    W = mw.gpu_world(rt, sp, cam, NX, NY, precision=rt.FP16).upload()
    H = rt.Octree(W, SPL).upload()
    G = rt.Octree(W, SPL, gpu=True)
    assert H.info() == G.info()
    assert np.array_equal(H.nodes().view(np.uint8), G.nodes().view(np.uint8))
    hc, hi = H.leaves(); gc, gi = G.leaves()
    assert np.array_equal(hc, gc) and np.array_equal(hi, gi)
    for k in range(3):                                            # traversal nodes (pair ranges, plane indices), pairs, pair -> sphere
        a, b = H.device_array(k), G.device_array(k)
        assert a.size == b.size and np.array_equal(a, b), k


# ---------------------------------------------------------------------------------------------------- frames
# (the list renders of the two rooms in which every path takes 50 bounces: a smaller frame, to bound the oracle's time)
SLOW_LIST = ("white_room", "mirror_room")
FRAMES = [(n, v, t) + ((48, 32) if n in SLOW_LIST and not t else (NX, NY)) for n, v in mw.WORLDS for t in (False, True)]
FRAMES += [("shells", None, False, 61, 35), ("shells", None, True, 61, 35), ("white_room", None, True, 61, 35), ("white_room", None, False, 45, 27)]   # ragged


@pytest.mark.parametrize("name,variant,tree,nx,ny", FRAMES)
def test_frames_fp32(rt, cuda, name, variant, tree, nx, ny):
    """16 spp (the long-chain pass is on), fast traversal: framebuffer and the first 6 words of every RNG state equal the oracle's"""
    _, _, W, O = make(rt, name, variant, nx, ny, tree)
    fb, st = render_frame(rt, cuda, W, O, nx, ny, NS)
    ref, ref_st = oracle_frame(name, variant, tree, nx, ny)
    assert same_nan_as_ref(fb.cpu().numpy().reshape(ny, nx, 3), ref)
    assert np.array_equal(states_of(st)[:, :6], ref_st[:, :6])
    if name == "white_room":
        assert (f32_bits(ref) == 0).all()                             # a black frame: the states pin every draw of every bounce


@pytest.mark.parametrize("name,nx,ny,ns,tree", [("glass_indices", NX, NY, NS, True), ("shells", NX, NY, NS, True), ("tir_room", NX, NY, NS, True),
                                                ("white_room", 48, 32, 4, True), ("shells", 48, 32, 4, False)])
def test_frames_binary16(rt, cuda, name, nx, ny, ns, tree):
    """k_render_h against the oracle's binary16 render, through the tree and — `shells` once more, where every shell is seen — through
    the list.  The binary16 kernel reads the plain material record, not the fp32 shade table: more than one index (and a
    dielectric's albedo, which nothing may use) tells the two apart."""
    torch = cuda
    sp, cam = mw.half_world(rt, name, nx, ny)
    W = mw.gpu_world(rt, sp, cam, nx, ny, precision=rt.FP16)
    O = rt.Octree(W, SPL) if tree else None
    st = rt.alloc_rand_state(nx, ny)
    fb = rt.alloc_fb(nx, ny, precision=rt.FP16)
    rt.render_init(nx, ny, st)
    rt.render(fb, nx, ny, ns, W, st, O)
    torch.cuda.synchronize()
    ref, ref_st = mw.oracle(sp, cam, nx, ny, tree=tree, spl=SPL, fp16=True).render(ns, nthreads=8)
    got = half_bits(fb).reshape(ny, nx, 3)
    nan = np.isnan(ref)
    assert np.array_equal(got[~nan], f32_to_half_bits(ref)[~nan])
    assert np.isnan(got.view(np.float16)[nan]).all()
    assert np.array_equal(states_of(st)[:, :6], ref_st[:, :6])


# ---------------------------------------------------------------------------------------------------- two worlds, one process
@pytest.mark.parametrize("tree", [False, True])
def test_two_worlds_that_differ_only_in_their_indices(rt, cuda, tree):
    """glass_indices and its twin with every index 1.5, alternating: from fresh handles and through one shared rt_render_ctx every frame
    equals its own oracle — the shade table belongs to the world, and a kept schedule never changes a pixel"""
    torch = cuda
    sp, cam = mw.world("glass_indices", NX, NY, rt=rt)
    twin = mw.with_index(sp, 1.5)
    refs = [oracle_frame("glass_indices", None, tree), oracle_frame("glass_indices", None, tree, sp=twin, key="index 1.5")]
    assert (f32_bits(refs[0][0]) != f32_bits(refs[1][0])).any(axis=2).mean() >= 0.05

    def check(fb, st, which):
        torch.cuda.synchronize()
        assert same_nan_as_ref(fb.cpu().numpy().reshape(NY, NX, 3), refs[which][0]), which
        assert np.array_equal(states_of(st)[:, :6], refs[which][1][:, :6]), which

    A = mw.gpu_world(rt, sp, cam, NX, NY)
    OA = rt.Octree(A, SPL) if tree else None
    check(*render_frame(rt, torch, A, OA, NX, NY, NS), 0)
    B = mw.gpu_world(rt, twin, cam, NX, NY)
    OB = rt.Octree(B, SPL) if tree else None
    for _ in range(2):
        check(*render_frame(rt, torch, B, OB, NX, NY, NS), 1)
        check(*render_frame(rt, torch, A, OA, NX, NY, NS), 0)
    ctx = rt.RenderCtx()
    for which, (W, O) in enumerate([(A, OA), (B, OB)] * 2):
        # fresh handles for every frame of the shared context
        Wf = mw.gpu_world(rt, (sp, twin)[which % 2], cam, NX, NY)
        Of = rt.Octree(Wf, SPL) if tree else None
        for world, octree in ((W, O), (Wf, Of)):
            st = rt.alloc_rand_state(NX, NY); fb = rt.alloc_fb(NX, NY)
            rt.render_init(NX, NY, st)
            ctx.render(fb, NX, NY, NS, world, st, octree)
            check(fb, st, which % 2)
    ctx.close()


# ---------------------------------------------------------------------------------------------------- progressive
@pytest.mark.parametrize("name,tree", [("tir_room", False), ("tir_room", True), ("extremes", False), ("extremes", True)])
def test_progressive_passes(rt, cuda, name, tree):
    """8 passes of rt_render_progressive equal the oracle's render_progressive pass by pass: sums and states"""
    torch = cuda
    sp, cam, W, O = make(rt, name, tree=tree)
    S = mw.oracle(sp, cam, NX, NY, tree=tree, spl=SPL)
    st = rt.alloc_rand_state(NX, NY); fb = rt.alloc_fb(NX, NY)
    rt.render_init(NX, NY, st)
    ref_st = S.render_init()
    ref = np.zeros((NY, NX, 3), np.float32)
    for k in range(1, 9):
        rt.render_progressive(fb, NX, NY, k, W, st, O)
        S.render_progressive(ref, k, ref_st, nthreads=8)
        torch.cuda.synchronize()
        assert same_nan_as_ref(fb.cpu().numpy().reshape(NY, NX, 3), ref), k
        assert np.array_equal(states_of(st)[:, :6], ref_st[:, :6]), k
    if name == "extremes":
        assert np.isnan(ref).any() and np.isinf(ref).any()


# ---------------------------------------------------------------------------------------------------- every pixel a long chain
LX, LY = 131, 99                    # 17 x 13 = 221 tiles: three parts of runs of 64 tiles, ragged right and top edges
ROW_BLOCKS = ((12, 4), (95, 4))     # the 8 rows of the 64 spp frame that the oracle renders (the second block: the ragged tile row)


@pytest.mark.parametrize("name", ["white_room", "tir_room"])
@pytest.mark.parametrize("ns", [16, 64])
def test_frames_made_of_long_chains(rt, cuda, name, ns):
    """A room no path leaves is the extreme input of the long-chain scheduler: every pixel is a long chain.  Whole and as three parts,
    assembled, the bits are the oracle's (at 64 spp for 8 rows of it), and no thin wave is left counted afterwards."""
    torch = cuda
    sp, cam, W, O = make(rt, name, None, LX, LY, tree=True)
    whole, st = render_frame(rt, torch, W, O, LX, LY, ns)
    assert W.render_counters()["thin_waves"] == 0                 # rt_world_render_counters [1]
    nparts = 3
    per = rt.part_pixels(LX, LY, rt.Partition(0, nparts))
    parts = torch.zeros(nparts * per * 3, dtype=torch.float32, device="cuda")
    for p in range(nparts):
        fb, _ = render_frame(rt, torch, W, O, LX, LY, ns, rt.Partition(p, nparts))
        assert W.render_counters()["thin_waves"] == 0
        parts[p * per * 3: p * per * 3 + fb.numel()] = fb
    full = torch.zeros(LX * LY * 3, dtype=torch.float32, device="cuda")
    rt.assemble(full, parts, LX, LY, nparts)
    torch.cuda.synchronize()
    got, got_parts, got_st = whole.cpu().numpy().reshape(LY, LX, 3), full.cpu().numpy().reshape(LY, LX, 3), states_of(st).reshape(LY, LX, 12)
    if ns == 16:
        ref, ref_st = oracle_frame(name, None, True, LX, LY, ns)
        blocks = [(0, LY, ref, ref_st)]
    else:
        S = mw.oracle(sp, cam, LX, LY, tree=True, spl=SPL)
        blocks = [(r0, rows) + S.render(ns, row0=r0, rows=rows, nthreads=rows) for r0, rows in ROW_BLOCKS]
    for r0, rows, ref, ref_st in blocks:
        assert same_nan_as_ref(got[r0:r0 + rows], ref) and same_nan_as_ref(got_parts[r0:r0 + rows], ref), r0
        assert np.array_equal(got_st[r0:r0 + rows].reshape(-1, 12)[:, :6], ref_st[:, :6]), r0


# ---------------------------------------------------------------------------------------------------- adaptive with real NaN samples
@pytest.mark.parametrize("variant,tree", [(None, True), ("ghost0", True), (None, False)])
def test_adaptive_with_nan_samples(rt, cuda, variant, tree):
    """rt_render_adaptive(min 4, batch 4, max 16) on `extremes`: d_spp, the frame and the states equal the model of the rule on the
    per-sample colours; a pixel with a NaN among the samples it took ran to max_spp — also where a finite value in the NaN's place
    would have stopped it earlier"""
    torch = cuda
    lo, step, hi = 4, 4, 16
    _, _, W, O = make(rt, "extremes", variant, tree=tree)
    samples, states = progressive_samples(rt, torch, W, O, NX, NY, hi)
    with np.errstate(all="ignore"):
        rel = pick_rel_error(samples, lo, step, hi, FLOOR)
        m_spp, m_fb = stop_rule_model(samples, rel, FLOOR, lo, step, hi)
    spp, fb, st = adaptive_frame(rt, torch, W, O, NX, NY, rt.Adaptive(lo, hi, step, rel, FLOOR))
    assert np.array_equal(spp, m_spp)
    assert same_nan_as_ref(fb, m_fb)
    assert np.array_equal(st, states[spp - 1, np.arange(spp.size)])
    nan_at = np.isnan(samples).any(axis=2)                                        # [sample, pixel]
    took_nan = (nan_at & (np.arange(1, hi + 1)[:, None] <= spp[None, :])).any(axis=0)
    print("extremes/%s: rel_error %g, %d pixels took a NaN sample, %d have one among their first %d" % (variant, rel, took_nan.sum(), nan_at.any(axis=0).sum(), hi))
    assert took_nan.sum() >= 10 and nan_at[:lo].any(axis=0).sum() >= 10
    # (implied by the equality with the model above; stated because it is the header's sentence)
    assert (spp[took_nan] == hi).all() and (spp[nan_at[:lo].any(axis=0)] == hi).all()
    # the same pixels with the mean of their finite samples in place of every NaN: the rule stops some of them before max_spp
    with np.errstate(all="ignore"):
        ok = np.isfinite(samples)
        mean = np.where(ok, samples, 0.0).sum(axis=0) / np.maximum(ok.sum(axis=0), 1)
        patched = np.where(np.isnan(samples), mean[None], samples).astype(np.float32)
        p_spp, _ = stop_rule_model(patched, rel, FLOOR, lo, step, hi)
    assert (p_spp[took_nan] < hi).sum() >= 1
