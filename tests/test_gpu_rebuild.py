"""rt_octree_rebuild_gpu (-m gpu): the tree of a moved world rebuilt in the handle of an earlier rt_build_octree_gpu equals a FRESH
rt_build_octree_gpu of the same world - every rt_octree_debug_array by size and content, the info calls, nodes and leaves (the
comparison of tests/tree_compare.py, here between two device builds), and frames, guides and hit records rendered through it, byte for
byte, the written-back RNG states included - and rt_octree_rebuild_info reports what the rebuild spared: at most 3 host-blocking waits
(binary16: 2) and nothing regrown while the counts stay within the quarter of slack the handle keeps.  N = 500, SPHERES_PER_LEAF 30,
64 x 40, 4 samples a pixel unless a case says otherwise."""
import numpy as np
import pytest

import build_limit_worlds as bw
import rebuild_growth_world as gw
from tree_compare import ARRAYS
from world_cases import random_rays

pytestmark = pytest.mark.gpu
N, SPL, NX, NY, NS, N_RAYS = 500, 30, 64, 40, 4, 4096
EINVAL = -1


# ---------------------------------------------------------------------------------------------------- helpers
def assert_same_tree(R, G, arrays=range(13), grid_contents=True):
    """tree_compare.compare between a rebuilt handle R and a fresh device build G.  grid_contents=False, a tree that stores no sphere:
    the grid arrays by size alone (no kernel reads them while the grid is off; either build leaves them unset: DESIGN.md 5.7)"""
    assert R.info() == G.info()
    assert R.build_path() == G.build_path()
    if len(arrays) > 3:
        assert R.accel_info() == G.accel_info()
    assert np.array_equal(R.nodes().view(np.uint8), G.nodes().view(np.uint8))
    rc, ri = R.leaves(); gc, gi = G.leaves()
    assert np.array_equal(rc, gc) and np.array_equal(ri, gi)
    for k in arrays:
        a, b = R.device_array(k), G.device_array(k)
        assert a.size == b.size, ARRAYS[k]
        if (ARRAYS[k] == "large_hot" and a.size == 0) or (k >= 3 and not grid_contents):
            continue
        assert np.array_equal(a, b), ARRAYS[k]


def move(torch, W, slots, dx):
    """every sphere of `slots` moved by dx in x, through rt_world_set_geometry"""
    g = W.get_geometry()
    g[torch.from_numpy(np.asarray(slots)).cuda(), 0] += dx
    W.set_geometry(g)
    return g


def seventh_small(W):
    sp = W.spheres
    small = np.where((sp["material"] != -1) & (sp["radius"] < 0.5))[0]
    return small[small > 0][::7]


def frame(rt, torch, W, O, precision=None, nx=NX, ny=NY, ns=NS):
    fb = rt.alloc_fb(nx, ny, precision=rt.FP32 if precision is None else precision)
    st = rt.alloc_rand_state(nx, ny)
    rt.render_init(nx, ny, st)
    rt.render(fb, nx, ny, ns, W, st, O)
    torch.cuda.synchronize()
    return fb.cpu().numpy().view(np.uint8), st.cpu().numpy()


def looks(rt, torch, W, O, d_rays):
    """frame, RNG states, guides and hit records through O, as bytes"""
    fb, st = frame(rt, torch, W, O)
    guides = rt.alloc_guides(NX, NY)
    rt.render_guides(W, O, NX, NY, guides)
    recs = torch.zeros(N_RAYS * 32, dtype=torch.uint8, device="cuda")
    rt.trace_rays(W, O, d_rays, N_RAYS, recs)
    torch.cuda.synchronize()
    return dict(fb=fb, states=st, guides=guides.cpu().numpy(), records=recs.cpu().numpy())


# ---------------------------------------------------------------------------------------------------- 1. a moved world
def test_rebuild_of_a_moved_world_equals_a_fresh_build(rt, cuda):
    W = rt.World(N, NX, NY).upload()
    R = rt.Octree(W, SPL, gpu=True)
    assert R.rebuild_info()["rebuilds"] == 0 and R.rebuild_info()["regrown"] == 0
    slots = seventh_small(W)
    assert len(slots) > 50
    before = R.device_array(1).copy()
    for k in range(3):
        move(cuda, W, slots, 0.02)
        assert R.rebuild() is R
        G = rt.Octree(W, SPL, gpu=True)
        assert_same_tree(R, G)
        G.close()
        info = R.rebuild_info()
        print("rebuild %d: %s" % (k, info))
        assert info["rebuilds"] == k + 1 and info["regrown"] == 0 and info["host_syncs_last"] <= 3, info
    assert not np.array_equal(before, R.device_array(1))              # the moves reached the tree


# ---------------------------------------------------------------------------------------------------- 2. frames
@pytest.mark.parametrize("mode", ["fast", "reference"])
def test_frames_guides_and_rays_through_a_rebuilt_tree(rt, cuda, mode):
    torch = cuda
    trav = rt.TRAVERSAL_FAST if mode == "fast" else rt.TRAVERSAL_REFERENCE
    d_rays = torch.from_numpy(random_rays(N_RAYS, 2200)).cuda()
    W = rt.World(N, NX, NY).upload()
    R = rt.Octree(W, SPL, gpu=True).set_traversal(trav)
    old = looks(rt, torch, W, R, d_rays)
    move(torch, W, seventh_small(W), 0.02)
    R.rebuild()
    G = rt.Octree(W, SPL, gpu=True).set_traversal(trav)
    got, want = looks(rt, torch, W, R, d_rays), looks(rt, torch, W, G, d_rays)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert not np.array_equal(got["fb"], old["fb"])
    # the mode set before the rebuild is still set.  Both modes render the same bytes, so the mode is read through the one call that
    # tells them apart: the kernel rt_render launches for the tree is the mode's
    other = rt.TRAVERSAL_REFERENCE if mode == "fast" else rt.TRAVERSAL_FAST
    assert rt.render_kernel_name(W, R) == rt.render_kernel_name(W, G)
    G.set_traversal(other)
    assert rt.render_kernel_name(W, R) != rt.render_kernel_name(W, G)


# ---------------------------------------------------------------------------------------------------- 3. growth
def test_a_tree_that_outgrows_the_kept_memory(rt, cuda):
    """first -> grown of tests/rebuild_growth_world.py (tests/test_rebuild_growth_host.py: pairs, entries and large spheres exceed the
    quarter of slack): found on the device, enlarged, run again once; a second rebuild of the same geometry fits"""
    torch = cuda
    W = rt.World(gw.N, gw.NX, gw.NY).upload()
    R = rt.Octree(W, gw.SPL, gpu=True)
    W.set_geometry(torch.from_numpy(gw.geometry(gw.grown_spheres(W.spheres))).cuda())
    R.rebuild()
    info = R.rebuild_info()
    print(info)
    assert info["rebuilds"] == 1 and info["regrown"] >= 1, info
    G = rt.Octree(W, gw.SPL, gpu=True)
    assert G.build_path() == rt.BUILD_DEVICE and G.accel_info()["large_spheres"] > 600
    assert_same_tree(R, G)
    a, b = frame(rt, torch, W, R), frame(rt, torch, W, G)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    R.rebuild()
    again = R.rebuild_info()
    print(again)
    assert again["rebuilds"] == 2 and again["regrown"] == info["regrown"] and again["host_syncs_last"] <= 3, again
    assert_same_tree(R, G)


def grid_piece_bytes(O):
    """the bytes gpubuild::build asks of the grid's piece for this tree, from the sizes of the arrays it holds: strip entries and bricks
    (6, 7), bin starts (5), large list (3, 4), bitmaps (12), the two unsorted key arrays (8 bytes a registration) and the alignment
    allowance of 32 x 256"""
    size = {k: O.device_array(k).size for k in (3, 4, 5, 6, 7, 12)}
    registrations = size[6] // 16 - 16
    return sum(size.values()) + 8 * registrations + 32 * 256


def test_a_grid_that_outgrows_its_piece(rt, cuda):
    """the other way to outgrow: the grid's own piece, whose size the host knows at its second stop and enlarges there.  All but
    every 50th small sphere of create_world's N = 4000 start outside the root box; moved home, the grid holds fifty times the
    registrations (and the tree fifty times the pairs: the run is repeated first, then the grid piece is found too small).  N = 4000:
    the bin starts, which depend on the cell size alone, are 0.7 MB of the piece in both, and the registrations have to outweigh them"""
    torch = cuda
    W = rt.World(4000, NX, NY).upload()
    home = W.get_geometry().clone()
    sp = W.spheres
    small = np.where((sp["material"] != -1) & (sp["radius"] < 0.5))[0]
    away = np.setdiff1d(small[small > 0], small[small > 0][::50])
    few = home.clone()
    few[torch.from_numpy(away).cuda(), :3] = 50.0
    W.set_geometry(few)
    R = rt.Octree(W, SPL, gpu=True)
    assert R.info()["dropped_outside"] == len(away) and R.accel_info()["grid_dim"] > 0
    first = grid_piece_bytes(R)
    W.set_geometry(home)
    R.rebuild()
    info = R.rebuild_info()
    G = rt.Octree(W, SPL, gpu=True)
    print(info, first, grid_piece_bytes(G))
    assert grid_piece_bytes(G) > first + first // 4 + 32 * 256       # the precondition: more than the piece and its quarter of slack
    assert info["rebuilds"] == 1 and info["regrown"] == 1, info
    assert_same_tree(R, G)
    a, b = frame(rt, torch, W, R), frame(rt, torch, W, G)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    R.rebuild()
    assert R.rebuild_info() == dict(rebuilds=2, regrown=1, host_syncs_last=3)
    assert_same_tree(R, G)


# ---------------------------------------------------------------------------------------------------- 4. small and empty
@pytest.mark.parametrize("case", ["n1", "n5", "outside"])
def test_small_and_empty_worlds(rt, cuda, case):
    """N = 1 (the ground alone), N = 5, and a world whose only sphere lies outside the root box: no sphere in the tree, the early
    return before the grid"""
    torch = cuda
    W = (rt.World(5, NX, NY) if case == "n5" else bw.gpu_world(rt, "ground" if case == "n1" else "outside", False, NX, NY)).upload()
    R = rt.Octree(W, SPL, gpu=True)
    for k in range(2):
        if case == "n5":
            move(torch, W, [1, 4], 0.02)
        else:
            W.set_geometry(W.get_geometry())
        R.rebuild()
        G = rt.Octree(W, SPL, gpu=True)
        assert_same_tree(R, G, grid_contents=case == "n5")
        assert (G.info()["flat_entries"] == 0) == (case != "n5")
        a, b = frame(rt, torch, W, R), frame(rt, torch, W, G)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        info = R.rebuild_info()
        assert info["rebuilds"] == k + 1 and info["regrown"] == 0 and info["host_syncs_last"] <= 3, info


# ---------------------------------------------------------------------------------------------------- 5. binary16
def test_binary16(rt, cuda):
    torch = cuda
    W = rt.World(N, NX, NY, precision=rt.FP16).upload()
    R = rt.Octree(W, SPL, gpu=True)
    g = W.get_geometry()
    g[torch.from_numpy(seventh_small(W)).cuda(), 0] += 0.03125      # (a binary16 step at these coordinates' magnitudes or above)
    W.set_geometry(g.to(torch.float16).to(torch.float32))             # exact binary16 images, as rt_world_create expects
    R.rebuild()
    G = rt.Octree(W, SPL, gpu=True)
    assert_same_tree(R, G, arrays=range(3))
    a, b = frame(rt, torch, W, R, rt.FP16), frame(rt, torch, W, G, rt.FP16)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    info = R.rebuild_info()
    assert info["rebuilds"] == 1 and info["regrown"] == 0 and info["host_syncs_last"] <= 2, info


# ---------------------------------------------------------------------------------------------------- 6. declined
def test_declined_and_back(rt, cuda):
    """over_cap of tests/build_limit_worlds.py makes the device build decline.  A handle whose last build was the host's is accepted and
    the device tried again; from a device build the decline moves the host build into the handle; back below the limit the next
    rebuild is the device's"""
    torch = cuda
    spl = 17
    d_small, d_over = (torch.from_numpy(bw.geometry(name)).cuda() for name in ("small", "over_cap"))
    W = bw.gpu_world(rt, "over_cap", False, NX, NY).upload()
    R = rt.Octree(W, spl, gpu=True)
    assert R.build_path() == rt.BUILD_HOST_DECLINED
    for k, (d_geom, path) in enumerate([(d_over, rt.BUILD_HOST_DECLINED), (d_small, rt.BUILD_DEVICE), (d_small, rt.BUILD_DEVICE),
                                        (d_over, rt.BUILD_HOST_DECLINED), (d_small, rt.BUILD_DEVICE)]):
        W.set_geometry(d_geom)
        R.rebuild()
        assert R.build_path() == path, k
        G = rt.Octree(W, spl, gpu=True)                              # (a declined fresh build IS the host tree, uploaded on first use)
        assert_same_tree(R, G)
        a, b = frame(rt, torch, W, R), frame(rt, torch, W, G)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k
        G.close()
        assert R.rebuild_info()["rebuilds"] == k + 1


# ---------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_handle_as_it_was(rt, cuda):
    torch = cuda
    lib = rt.lib()
    W = rt.World(N, NX, NY).upload()
    R = rt.Octree(W, SPL, gpu=True)
    old = frame(rt, torch, W, R)
    other_n = rt.World(N + 1, NX, NY).upload()
    other_precision = rt.World(N, NX, NY, precision=rt.FP16).upload()
    H = rt.Octree(W, SPL)
    host_frame = frame(rt, torch, W, H)
    assert lib.rt_octree_rebuild_gpu(None, W.h, None) == EINVAL
    assert lib.rt_octree_rebuild_gpu(R.h, None, None) == EINVAL
    assert lib.rt_octree_rebuild_gpu(R.h, other_n.h, None) == EINVAL
    assert lib.rt_octree_rebuild_gpu(R.h, other_precision.h, None) == EINVAL
    assert lib.rt_octree_rebuild_gpu(H.h, W.h, None) == EINVAL
    assert lib.rt_octree_rebuild_info(None, None, None, None) == EINVAL
    assert R.rebuild_info()["rebuilds"] == 0 and R.build_path() == rt.BUILD_DEVICE and H.build_path() == rt.BUILD_HOST
    again = frame(rt, torch, W, R)
    assert np.array_equal(again[0], old[0]) and np.array_equal(again[1], old[1])
    again = frame(rt, torch, W, H)
    assert np.array_equal(again[0], host_frame[0]) and np.array_equal(host_frame[0], old[0])


# ---------------------------------------------------------------------------------------------------- 8. keyed state
def test_the_kept_schedule_misses_once_after_a_rebuild(rt, cuda):
    torch = cuda
    W = rt.World(N, NX, NY).upload()
    R = rt.Octree(W, SPL, gpu=True)
    f1 = frame(rt, torch, W, R)
    f2 = frame(rt, torch, W, R)
    reused, computed = W.schedule_reuse()
    assert np.array_equal(f1[0], f2[0]) and reused >= 1
    R.rebuild()                                                       # the same geometry: only the handle's serial tells the trees apart
    f3 = frame(rt, torch, W, R)
    assert W.schedule_reuse() == (reused, computed + 1)
    f4 = frame(rt, torch, W, R)
    assert W.schedule_reuse() == (reused + 1, computed + 1)
    assert np.array_equal(f3[0], f1[0]) and np.array_equal(f4[0], f1[0])
