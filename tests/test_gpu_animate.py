"""GPU tests of a resident world over an animation (-m gpu): rt_world_set_geometry, rt_world_get_geometry and rt_world_set_camera.
Every comparison is bit equality: a world whose geometry or camera was replaced against a FRESH world created with the new values —
frames and written-back RNG states through the tree and through the list path (both traversals), hit records of random rays, guides,
every array of the device-built trees, the geometry read back, the list grid's figures — and one case against the oracle.

Frames are 43x21 (edge tiles in both directions) at 4 spp.  The moved geometry is deterministic: sphere 0 and every i % 3 == 0 stay,
i % 3 == 1 is translated by (0.3, 0.15, -0.2), i % 3 == 2 has its radius times 1.25, and the last hittable translated sphere is sent
to (50, 50, 50), outside the tree's box; for USE_FP16 worlds every value is rounded to binary16 first.

The host staging copy (h_geom) has two readers: the world's list grid, which the list-path cases and rt_world_list_accel_info cover
at N = 500, and the host fallback of rt_build_octree_gpu, which the device build's workspace limit leads to: the worlds here stay
below it, tests/test_gpu_build_limits.py::test_fallback_after_a_move moves a resident world of 161 spheres across it.  The wrapper's own host build (Octree(world, gpu=False)) reads the binding's copy of the list, which
World.set_geometry marks stale in the same way: test_host_build_after_a_move."""
import numpy as np
import pytest

import material_edge_worlds as mw
from world_cases import random_rays

pytestmark = pytest.mark.gpu
NX, NY, NS = 43, 21, 4
SPL = 30
F = np.float32


def geometry_of(sp):
    return np.ascontiguousarray(np.concatenate([sp["center"], sp["radius"][:, None]], 1), F)


def moved_geometry(sp, fp16):
    g = geometry_of(sp)
    i = np.arange(len(sp))
    g[i % 3 == 1, :3] += np.array([0.3, 0.15, -0.2], F)
    g[i % 3 == 2, 3] *= F(1.25)
    far = np.flatnonzero((i % 3 == 1) & (sp["material"] != -1))[-1]
    g[far, :3] = F(50.0)
    if fp16:
        g = g.astype(np.float16).astype(F)
    return g


def with_geometry(sp, g):
    out = sp.copy()
    out["center"], out["radius"] = g[:, :3], g[:, 3]
    return out


def base_world(rt, name, fp16):
    """(spheres, camera) of a named world: create_world at N = 22 (20 spheres and 2 ghost slots) and at N = 500 (list grid and octree
    grid both enabled); "22g", the list of 22 with its two ghost slots — which create_world leaves at the end — moved to slots 1 and 5,
    so that list slot != world index for every sphere behind them; or an edge world of tests/material_edge_worlds.py (ghosts
    throughout, and as slot 0)"""
    prec = rt.FP16 if fp16 else rt.FP32
    if isinstance(name, (int, str)):
        W = rt.World(int(str(name).rstrip("g")), NX, NY, precision=prec)
        sp, cam = W.spheres.copy(), W.camera.copy()
        W.close()
        if name in (22, "22g"):
            assert (sp["material"] == -1).sum() == 2
        if name == "22g":
            sp = sp[[0, 20, 1, 2, 3, 21] + list(range(4, 20))]
            assert sp["material"][1] == -1 and sp["material"][5] == -1 and sp["material"][-1] != -1
        return sp, cam
    if fp16:
        sp, cam = mw.half_world(rt, name[0], NX, NY, name[1])
    else:
        sp, cam = mw.world(name[0], NX, NY, name[1], rt=rt)
    return sp, np.asarray(cam, F).ravel().view(rt.camera_dtype)


def make_world(rt, sp, cam, fp16):
    return rt.World(len(sp), NX, NY, precision=rt.FP16 if fp16 else rt.FP32, spheres=sp, camera=cam)


def outputs(rt, torch, W, O, fp16):
    """everything the test compares of a world and its device-built tree, as host arrays"""
    out = {}
    prec = rt.FP16 if fp16 else rt.FP32
    rays = torch.from_numpy(random_rays(4096, 3)).cuda()
    for path, tree, trav in (("tree", O, None), ("list_fast", None, rt.TRAVERSAL_FAST), ("list_reference", None, rt.TRAVERSAL_REFERENCE)):
        if trav is not None:
            W.set_list_traversal(trav)
        fb, st = rt.alloc_fb(NX, NY, precision=prec), rt.alloc_rand_state(NX, NY)
        rt.render_init(NX, NY, st)
        rt.render(fb, NX, NY, NS, W, st, tree)
        hits = torch.zeros(4096 * 32, dtype=torch.uint8, device="cuda")
        rt.trace_rays(W, tree, rays, 4096, hits)
        torch.cuda.synchronize()
        out[path + ".frame"], out[path + ".states"], out[path + ".trace"] = fb.cpu().numpy().view(np.uint8), st.cpu().numpy(), hits.cpu().numpy()
        if not fp16:
            g = rt.alloc_guides(NX, NY)
            rt.render_guides(W, tree, NX, NY, g)
            torch.cuda.synchronize()
            out[path + ".guides"] = g.cpu().numpy().view(np.uint8)
    W.set_list_traversal(rt.TRAVERSAL_FAST)
    for k in range(3 if fp16 else 13):
        out["tree.array%d" % k] = O.device_array(k).copy()
    out["geometry"] = W.get_geometry().cpu().numpy().view(np.uint8)
    info = W.list_accel_info()
    out["list_accel"] = np.array([info["enabled"], info["grid_dim"], info["grid_entries"], info["large_spheres"]], np.int64)
    out["list_accel.cell"] = np.array([info["cell_size"]], F).view(np.uint8)
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)


CASES = [(22, False), (22, True), ("22g", False), ("22g", True), (500, False), (500, True)] + [(w, False) for w in mw.WORLDS] + [(("extremes", None), True)]


def case_id(c):
    name, fp16 = c
    return "%s-%s" % (name if isinstance(name, (int, str)) else "_".join(str(v) for v in name if v), "fp16" if fp16 else "fp32")


# ---- 4 / 5. a moved world is a fresh world; nothing moved changes nothing ---------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_moved_world_is_a_fresh_world(rt, cuda, case):
    torch = cuda
    name, fp16 = case
    sp, cam = base_world(rt, name, fp16)
    g0, g1 = geometry_of(sp), moved_geometry(sp, fp16)
    assert not np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
    A = make_world(rt, sp, cam, fp16).upload()
    O0 = rt.Octree(A, SPL, gpu=True)
    before = outputs(rt, torch, A, O0, fp16)             # schedules, list grid and tree exist, and the old geometry has been looked at
    if name == 500 and not fp16:
        assert before["list_accel"][0] == 1 and O0.accel_info()["grid_entries"] > 0
    # nothing moved: the same values written again
    A.set_geometry(torch.from_numpy(g0).cuda())
    O0.close()
    O0 = rt.Octree(A, SPL, gpu=True)
    assert_same(outputs(rt, torch, A, O0, fp16), before, "nothing moved")
    # moved
    A.set_geometry(torch.from_numpy(g1).cuda())
    O0.close()
    OA = rt.Octree(A, SPL, gpu=True)
    got = outputs(rt, torch, A, OA, fp16)
    B = make_world(rt, with_geometry(sp, g1), cam, fp16)
    OB = rt.Octree(B, SPL, gpu=True)
    want = outputs(rt, torch, B, OB, fp16)
    assert_same(got, want, "moved")
    assert np.array_equal(got["geometry"], g1.view(np.uint8).reshape(got["geometry"].shape))
    assert not np.array_equal(got["tree.trace"], before["tree.trace"])             # the move shows (a closed white room's frame is black either way)
    if name == 500 and not fp16:
        # ... and the frame is the oracle's on the new geometry
        spB = with_geometry(sp, g1)
        for tree in (False, True):
            ref, _ = mw.oracle(spB, cam.view(F), NX, NY, tree=tree, spl=SPL).render(NS, nthreads=4)
            mine = got["tree.frame" if tree else "list_fast.frame"].view(np.uint32).reshape(NY, NX, 3)
            assert np.array_equal(mine, ref.view(np.uint32)), tree
    for h in (OA, OB, A, B):
        h.close()


# ---- 6. the camera -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_camera_of_a_resident_world(rt, cuda, fp16):
    torch = cuda
    prec = rt.FP16 if fp16 else rt.FP32
    sp, cam0 = base_world(rt, 500, fp16)
    th = np.radians(20.0)
    lookfrom = (13 * np.cos(th) + 3 * np.sin(th), 2.0, -13 * np.sin(th) + 3 * np.cos(th))
    cam1 = rt.camera_init(lookfrom, (0, 0, 0), (0, 1, 0), 30.0, float(np.float16(NX) / np.float16(NY)) if fp16 else NX / NY, 0.1, 10.0, precision=prec)
    A, B = make_world(rt, sp, cam0, fp16), make_world(rt, sp, cam1, fp16)
    OA, OB = rt.Octree(A, SPL, gpu=True), rt.Octree(B, SPL, gpu=True)

    def frame(W, O, st=None):
        fb = rt.alloc_fb(NX, NY, precision=prec)
        if st is None:
            st = rt.alloc_rand_state(NX, NY)
            rt.render_init(NX, NY, st)
        rt.render(fb, NX, NY, NS, W, st, O)
        return fb, st

    def host(*ts):
        torch.cuda.synchronize()
        return [t.cpu().numpy().view(np.uint8) for t in ts]

    f1, s1 = host(*frame(A, OA))
    f2, s2 = host(*frame(A, OA))
    assert np.array_equal(f1, f2) and A.schedule_reuse() == (1, 1)
    A.set_camera(cam1)
    assert np.array_equal(A.get_camera().view(np.uint8), cam1.view(np.uint8))
    f3, s3 = host(*frame(A, OA))
    assert A.schedule_reuse() == (1, 2)                                            # a reuse, then a miss
    fB, sB = host(*frame(B, OB))
    assert np.array_equal(f3, fB) and np.array_equal(s3, sB) and not np.array_equal(f3, f1)
    f4, _ = host(*frame(A, OA))
    assert np.array_equal(f4, fB) and A.schedule_reuse() == (2, 2)                 # and as before from then on
    # the list path, and the guides
    fa, sa = host(*frame(A, None))
    fb_, sb = host(*frame(B, None))
    assert np.array_equal(fa, fb_) and np.array_equal(sa, sb)
    if not fp16:
        ga, gb = rt.alloc_guides(NX, NY), rt.alloc_guides(NX, NY)
        rt.render_guides(A, OA, NX, NY, ga)
        rt.render_guides(B, OB, NX, NY, gb)
        a, b = host(ga, gb)
        assert np.array_equal(a, b)
    # a progressive sequence restarted at sample 1 follows the new camera
    A.set_camera(cam0)
    pa, pb = rt.alloc_fb(NX, NY, precision=prec), rt.alloc_fb(NX, NY, precision=prec)
    sta, stb = rt.alloc_rand_state(NX, NY), rt.alloc_rand_state(NX, NY)
    rt.render_init(NX, NY, sta)
    rt.render_init(NX, NY, stb)
    for s in (1, 2):
        rt.render_progressive(pa, NX, NY, s, A, sta, OA)                           # the old camera: its tile order is kept
    A.set_camera(cam1)
    rt.render_init(NX, NY, sta)
    for s in (1, 2, 3):
        rt.render_progressive(pa, NX, NY, s, A, sta, OA)
        rt.render_progressive(pb, NX, NY, s, B, stb, OB)
    a, b, c, d = host(pa, pb, sta, stb)
    assert np.array_equal(a, b) and np.array_equal(c, d)
    # a launch enqueued before the setter keeps the camera it was launched with
    A.set_camera(cam0)
    st = rt.alloc_rand_state(NX, NY)
    rt.render_init(NX, NY, st)
    fb = rt.alloc_fb(NX, NY, precision=prec)
    rt.render(fb, NX, NY, NS, A, st, OA)
    A.set_camera(cam1)
    old, = host(fb)
    assert np.array_equal(old, f1)
    for h in (OA, OB, A, B):
        h.close()


# ---- 7. the host copies after a move -------------------------------------------------------------------------------------------------
def test_host_build_after_a_move(rt, cuda):
    """the wrapper's host build reads the binding's copy of the list, refreshed from the device after set_geometry; the list grid is
    built on the host from the library's refreshed staging copy (rt_world_list_accel_info, with no render before it)"""
    torch = cuda
    sp, cam = base_world(rt, 500, False)
    g1 = moved_geometry(sp, False)
    A = make_world(rt, sp, cam, False)
    assert A.list_accel_info()["enabled"]                                          # the grid of the OLD geometry exists
    A.set_geometry(torch.from_numpy(g1).cuda())
    B = make_world(rt, with_geometry(sp, g1), cam, False)
    assert A.list_accel_info() == B.list_accel_info()
    HA, HB = rt.Octree(A, SPL).upload(), rt.Octree(B, SPL).upload()
    assert np.array_equal(A.spheres.view(np.uint8), B.spheres.view(np.uint8))
    assert HA.info() == HB.info()
    for k in range(13):
        a, b = HA.device_array(k), HB.device_array(k)
        assert a.size == b.size and np.array_equal(a, b), k
    for h in (HA, HB, A, B):
        h.close()
