"""The candidate grid at the thresholds of its classification rules (-m gpu): the worlds and rays of tests/grid_threshold_worlds.py
through rt_trace_rays (fast and reference traversal), rt_build_octree_gpu, rt_render_guides, rt_render and rt_render_progressive.

Every comparison is bit equality with the CPU oracle's hitable_list::hit / hitTree and render, "NaN where the oracle has NaN"
(bitcmp.same_nan_as_ref); no ray and no pixel is left out.  tests/test_grid_threshold_worlds_host.py shows on the CPU that every world
reaches the threshold it is named for, that the host build files it as the float64 model does, and that the rays fall to both sides
of every precondition of the walk and graze.  Here:
  * hit records: origins on the near zone's boundary aimed at grazing spheres at the centre bound on the far side (|o - c| up to
    41.5, the case K2 is sized for), |d|^2 and |d.y| at 2^-40 / 2^40, subnormal d.x / d.z, rays on the lattice of the world's OWN grid;
  * the device build against the host build, array for array: a one-ulp disagreement of k_classify at R' = Rlim, at dc = 17.5 or at
    a floor() of a column range would file one of the probe spheres differently;
  * guides and frames from inside, outside and the boundary of the near zone;
  * the kernel variant of every world, stated here (not taken from the model), so that a change of a threshold cannot quietly move a
    world off the variant it was built to reach."""
import functools

import numpy as np
import pytest

import denoise_model
import grid_threshold_worlds as gw
import material_edge_worlds as mw
import reference_cases as rc
from bitcmp import same_nan_as_ref
from gpu_frames import render_frame, states_of
from tree_compare import assert_records, compare, compare_empty, traced

pytestmark = pytest.mark.gpu

NX, NY, NS = gw.NX, gw.NY, 4
N_RAYS = 24000
IDS = ["%s%s-%s" % (n, "_" + v if v else "", mode) for n, v, mode, _ in gw.CASES]
TREES = [c for c in gw.CASES if c[2] == "tree"]
# the last template argument of k_render per world and mode: 1 no grid (a list: the scan k_render<false,..>), 2 the dense walk,
# 4 the pooled walk, 5 the pooled walk with chains that start alone
VARIANT = {("rlim", None, "list"): 5, ("rlim", None, "tree"): 5, ("centre_bound", None, "list"): 5,
           ("counts", "h63", "list"): 1, ("counts", "h64", "list"): 5, ("counts", "l64", "list"): 5, ("counts", "l65", "list"): 1,
           ("counts", "t0", "tree"): 5, ("counts", "t8", "tree"): 5, ("counts", "t9", "tree"): 5,
           ("clamps", "tiny", "list"): 5, ("clamps", "tiny", "tree"): 5, ("clamps", "huge", "tree"): 5, ("clamps", "one", "list"): 5,
           ("clamps", "one", "tree"): 5, ("clamps", "none", "tree"): 1,
           ("switches", "coop", "tree"): 4, ("switches", "sparse", "tree"): 2, ("switches", "dense", "tree"): 4,
           ("switches", "solo", "tree"): 5, ("switches", "nosolo", "tree"): 4}


def kernel(name, variant, mode, k=0):
    v = VARIANT[name, variant, mode]
    return "k_render<%s,%d,%d>" % ("false" if (mode == "list" and v == 1) else "true", k, v)


def make(rt, name, variant, mode, spl, cam="own"):
    sp, c = gw.world(name, variant, NX, NY, cam)
    W = mw.gpu_world(rt, sp, c, NX, NY)
    return sp, c, W, (rt.Octree(W, spl) if mode == "tree" else None)


@functools.lru_cache(None)
def oracle_records(name, variant, mode, spl):
    """{family: (rays, the oracle's records)} of a case, computed once and never written to"""
    sp, cam = gw.world(name, variant)
    m = gw.model(sp, mode, gw.stored_by_oracle(sp, cam, spl) if mode == "tree" else None)
    S = gw.oracle(sp, cam, mode == "tree", spl)
    out = {}
    for fam, rays in gw.ray_families(name, variant, sp, m, N_RAYS).items():
        ref = rc.trace(S, rays, 2 if mode == "tree" else 1)
        for a in [rays] + list(ref.values()):
            a.setflags(write=False)
        out[fam] = (rays, ref)
    return out


def test_every_case_has_its_variant_stated_and_all_are_reached():
    assert set(VARIANT) == {(n, v, mode) for n, v, mode, _ in gw.CASES}
    assert set(VARIANT.values()) == {1, 2, 4, 5}


# ---------------------------------------------------------------------------------------------------- hit records
@pytest.mark.parametrize("name,variant,mode,spl", gw.CASES, ids=IDS)
def test_hit_records(rt, cuda, name, variant, mode, spl):
    """zone_rays, precondition_rays, lattice_rays_for and random_rays, 24 000 each, through the fast and the reference traversal:
    sphere, t, p and normal of every ray equal the oracle's"""
    torch = cuda
    sp, cam, W, O = make(rt, name, variant, mode, spl)
    assert rt.render_kernel_name(W, O, 0) == kernel(name, variant, mode)
    for fam, (rays, ref) in oracle_records(name, variant, mode, spl).items():
        assert len(rays) == N_RAYS
        for trav in (rt.TRAVERSAL_FAST, rt.TRAVERSAL_REFERENCE):
            if O is not None:
                O.set_traversal(trav)
            else:
                W.set_list_traversal(trav)
            assert_records(traced(rt, torch, W, O, rays), ref, (fam, "fast" if trav == rt.TRAVERSAL_FAST else "reference"))


# ---------------------------------------------------------------------------------------------------- device build
@pytest.mark.parametrize("name,variant,mode,spl", TREES, ids=[i for i, c in zip(IDS, gw.CASES) if c[2] == "tree"])
def test_device_build_equals_host_build(rt, cuda, name, variant, mode, spl):
    """all 13 device arrays, nodes, leaves and infos of rt_build_octree_gpu equal the host build's, and both are the model's grid"""
    sp, cam, W, _ = make(rt, name, variant, mode, spl)
    if (name, variant) == ("clamps", "none"):
        H, G = compare_empty(rt, W.upload(), spl)
    else:
        H, G = compare(rt, W.upload(), spl)
    m = gw.model(sp, "tree", gw.stored_set(*G.leaves()))
    assert G.accel_info() == gw.info_of(m)
    if m["enabled"]:
        # the model's own statement of where every sphere is filed - columns ix0..ix1 / iz0..iz1, fine bins of the centre - against
        # the entry ranges per column and bin that the host build uploaded (DevAccel::cs; the device build's equal them, above)
        cs = H.device_array(5).view(np.int32)
        want = gw.cell_starts(m)
        assert cs.size == want.size and cs[want.size // 2 - 1] == m["grid_entries"]
        assert np.array_equal(cs, want)
    for k in (0, 1):
        assert rt.render_kernel_name(W, G, k) == kernel(name, variant, mode, k) == gw.kernel_name(m, k)


# ---------------------------------------------------------------------------------------------------- guides and frames
@functools.lru_cache(None)
def oracle_frame(name, variant, mode, spl, cam, ns):
    sp, c = gw.world(name, variant, NX, NY, cam)
    S = gw.oracle(sp, c, mode == "tree", spl)
    fb, st = S.render(ns, nthreads=8)
    fb.setflags(write=False); st.setflags(write=False)
    return fb, st


@pytest.mark.parametrize("cam", ["own", "outside", "edge"])
@pytest.mark.parametrize("name,variant,mode,spl", gw.CASES, ids=IDS)
def test_guides_and_frames(rt, cuda, name, variant, mode, spl, cam):
    """64 x 40: rt_render_guides equals the oracle's records of the pixel-centre rays, rt_render at 4 spp the oracle's frame and states.
    Cameras: the world's own; lookfrom 30 away from (0,1,0) (every primary ray takes the scan, every secondary ray the walk); lookfrom
    exactly 24 away (the lens offsets put the origins to either side of the zone's boundary)."""
    torch = cuda
    sp, c, W, O = make(rt, name, variant, mode, spl, cam)
    d = rt.alloc_guides(NX, NY)
    rt.render_guides(W, O, NX, NY, d)
    torch.cuda.synchronize()
    rays = denoise_model.guide_rays(W.camera[0], NX, NY)
    zone = gw.fast_path(rays)["zone"]
    assert zone.all() if cam != "outside" else not zone.any()
    ref = gw.oracle(sp, c, mode == "tree", spl).trace(rays, mode=2 if mode == "tree" else 1)
    assert_records(d.cpu().numpy().view(rt.hit_record_dtype), ref, "guides")
    assert (ref["sphere"] >= 0).sum() > NX * NY // 4
    fb, st = render_frame(rt, torch, W, O, NX, NY, NS)
    want, want_st = oracle_frame(name, variant, mode, spl, cam, NS)
    assert same_nan_as_ref(fb.cpu().numpy().reshape(NY, NX, 3), want)
    assert np.array_equal(states_of(st)[:, :6], want_st[:, :6])


def test_frame_with_the_long_chain_pass(rt, cuda):
    """16 spp (the pilot pass pre-classifies long chains) on a tree world whose probes sit at Rlim and at the floors of the columns"""
    torch = cuda
    ns = 16
    sp, c, W, O = make(rt, "rlim", None, "tree", 30)
    fb, st = render_frame(rt, torch, W, O, NX, NY, ns)
    want, want_st = oracle_frame("rlim", None, "tree", 30, "own", ns)
    assert same_nan_as_ref(fb.cpu().numpy().reshape(NY, NX, 3), want)
    assert np.array_equal(states_of(st)[:, :6], want_st[:, :6])


@pytest.mark.parametrize("name,variant,mode,spl", [("centre_bound", None, "list", 30), ("clamps", "huge", "tree", 30), ("switches", "sparse", "tree", 64)],
                         ids=["centre_bound", "huge", "sparse"])
def test_parts_and_progressive_passes(rt, cuda, name, variant, mode, spl):
    """a render in three parts, assembled, and two progressive passes equal the oracle: through a grid stretched to the centre bound,
    through an enabled grid without entries, and through the dense walk (k_render<true,1,2>: no other test takes a progressive pass there)"""
    torch = cuda
    sp, c, W, O = make(rt, name, variant, mode, spl)
    assert rt.render_kernel_name(W, O, 1) == kernel(name, variant, mode, 1)
    want, _ = oracle_frame(name, variant, mode, spl, "own", NS)
    nparts = 3
    per = rt.part_pixels(NX, NY, rt.Partition(0, nparts))
    parts = torch.zeros(nparts * per * 3, dtype=torch.float32, device="cuda")
    for p in range(nparts):
        fb, _ = render_frame(rt, torch, W, O, NX, NY, NS, rt.Partition(p, nparts))
        parts[p * per * 3: p * per * 3 + fb.numel()] = fb
    full = torch.zeros(NX * NY * 3, dtype=torch.float32, device="cuda")
    rt.assemble(full, parts, NX, NY, nparts)
    torch.cuda.synchronize()
    assert same_nan_as_ref(full.cpu().numpy().reshape(NY, NX, 3), want)
    S = gw.oracle(sp, c, mode == "tree", spl)
    st = rt.alloc_rand_state(NX, NY); fb = rt.alloc_fb(NX, NY)
    rt.render_init(NX, NY, st)
    ref_st = S.render_init()
    ref = np.zeros((NY, NX, 3), np.float32)
    for k in (1, 2):
        rt.render_progressive(fb, NX, NY, k, W, st, O)
        S.render_progressive(ref, k, ref_st, nthreads=8)
        torch.cuda.synchronize()
        assert same_nan_as_ref(fb.cpu().numpy().reshape(NY, NX, 3), ref), k
        assert np.array_equal(states_of(st)[:, :6], ref_st[:, :6]), k
