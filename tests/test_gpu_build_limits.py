"""rt_build_octree_gpu at the limit of its workspace, its host fallback, and the smallest worlds (-m gpu).  The worlds are those of
tests/build_limit_worlds.py; tests/test_build_limit_worlds_host.py shows on the CPU that `at_cap` has exactly cap = 16 n + 65536
(level-3 cell, sphere) pairs and `over_cap` one more.  Every case states the build its tree must have come from
(rt_octree_build_path) and every comparison is bit equality: trees against the host build Octree(W, spl) through
tree_compare.compare (infos, nodes, leaves, the 13 device arrays; binary16: arrays 0-2), frames (43 x 21, 4 spp, create_world's
camera, framebuffer and written-back RNG states) and 4096 hit records against OracleScene(custom=...).

  a. at_cap: the device builds - 4097 leaves at SPHERES_PER_LEAF 17, drops in every cell at 16, a large list of 133 spheres whose
     bricks are whole (stored shells) or absent (dropped shells);
  b. over_cap: the device declines (a designed return: k_pairs writes no pair past the workspace) and rt_build_octree_gpu returns the
     host build; three declines in a row on one world leave it as it was;
  c. a resident world moved across the limit by rt_world_set_geometry: the fallback reads the world's host staging copy, which the
     setter left stale - the tree and frame must be those of a FRESH world with the new geometry - and moved back it builds on the
     device again; once with setter and build on a non-default, non-blocking stream;
  d. n = 1 and the two n = 2 worlds.

The device build's second decline, `nx > cap || nz > cap` (grid registrations per copy), is reached by no world: a grid sphere has
R' <= Rlim = 1.5 h, so its columns floor((x - R' - g0) / h - 1e-4) .. floor((x + R' - g0) / h + 1e-4) (build_accel, csrc/rt_accel.h)
span at most 3.0002 and number at most 5: nx, nz <= 5 n < 16 n + 65536.  No world here is bent towards it."""
import functools

import numpy as np
import pytest

import build_limit_worlds as bw
import reference_cases as rc
from bitcmp import same_nan_as_ref
from tree_compare import compare, compare_empty

pytestmark = pytest.mark.gpu
NX, NY, NS = bw.NX, bw.NY, bw.NS
SPLS = [16, 17, 30]
MATRIX = [(spl, fp16) for spl in SPLS for fp16 in (False, True)]
MATRIX_IDS = ["spl%d-%s" % (spl, "fp16" if fp16 else "fp32") for spl, fp16 in MATRIX]


# ---------------------------------------------------------------------------------------------------- references, computed once
@functools.lru_cache(None)
def oracle_frame(rt, name, fp16, spl):
    fb, st = bw.oracle(rt, name, fp16, spl).render(NS, nthreads=8)
    fb.setflags(write=False); st.setflags(write=False)
    return fb, st


@functools.lru_cache(None)
def oracle_records(rt, name, fp16, spl):
    rays = bw.rays(fp16)
    ref = bw.oracle(rt, name, fp16, spl).trace(rays, mode=2)
    for a in [rays] + list(ref.values()):
        a.setflags(write=False)
    return rays, ref


# ---------------------------------------------------------------------------------------------------- helpers
def compare16(rt, W, spl):
    """tree_compare.compare for a binary16 world (as test_device_build_of_binary16_trees): infos, nodes, leaves, arrays 0-2"""
    H = rt.Octree(W, spl).upload()
    G = rt.Octree(W, spl, gpu=True)
    assert H.info() == G.info()
    assert np.array_equal(H.nodes().view(np.uint8), G.nodes().view(np.uint8))
    hc, hi = H.leaves(); gc, gi = G.leaves()
    assert np.array_equal(hc, gc) and np.array_equal(hi, gi)
    for k in range(3):
        a, b = H.device_array(k), G.device_array(k)
        assert a.size == b.size and np.array_equal(a, b), k
    return H, G


def tree_of(O, fp16):
    """everything rt_octree_* tells of a tree, as host arrays"""
    out = {"nodes": O.nodes().view(np.uint8)}
    out["leaf_counts"], out["leaf_indices"] = O.leaves()
    for k in range(3 if fp16 else 13):
        out["array%d" % k] = O.device_array(k).copy()
    info = dict(O.info(), **({} if fp16 else O.accel_info()))
    out["info"] = np.array([float(info[k]) for k in sorted(info)])
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)


def frame(rt, torch, W, O, fp16, trav=None):
    """(framebuffer, RNG states) of one render through O, on the current stream, as host arrays"""
    if trav is not None:
        O.set_traversal(trav)
    fb, st = rt.alloc_fb(NX, NY, precision=rt.FP16 if fp16 else rt.FP32), rt.alloc_rand_state(NX, NY)
    rt.render_init(NX, NY, st)
    rt.render(fb, NX, NY, NS, W, st, O)
    torch.cuda.current_stream().synchronize()
    return fb.cpu().numpy().reshape(NY, NX, 3), st.cpu().numpy().view(np.uint32).reshape(-1, 12)


def assert_frame(got, want, fp16, what):
    (fb, st), (ref, ref_st) = got, want
    if fp16:                                                        # the oracle returns exact float images of its binary16 values
        nan = np.isnan(ref)
        assert np.array_equal(fb.view(np.uint16)[~nan], ref.astype(np.float16).view(np.uint16)[~nan]), what
        assert np.isnan(fb[nan]).all(), what
    else:
        assert same_nan_as_ref(fb, ref), what
    assert np.array_equal(st[:, :6], ref_st[:, :6]), what


def assert_frames_and_rays(rt, torch, W, O, name, fp16, spl):
    """frames (fp32: both traversals) and the hit records of bw.rays through O equal the oracle's of the world `name`"""
    want = oracle_frame(rt, name, fp16, spl)
    rays, ref = oracle_records(rt, name, fp16, spl)
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    for trav in ((None,) if fp16 else (rt.TRAVERSAL_REFERENCE, rt.TRAVERSAL_FAST)):
        assert_frame(frame(rt, torch, W, O, fp16, trav), want, fp16, ("frame", trav))
        d_out = torch.zeros(len(rays) * 32, dtype=torch.uint8, device="cuda")
        rt.trace_rays(W, O, d_rays, len(rays), d_out)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().view(rt.hit_record_dtype)
        assert np.array_equal(got["sphere"], ref["sphere"]), ("rays", trav)
        for f in ("t", "p", "normal"):
            assert same_nan_as_ref(got[f], ref[f]), ("rays", trav, f)


# ---------------------------------------------------------------------------------------------------- a. at the limit
@pytest.mark.parametrize("spl,fp16", MATRIX, ids=MATRIX_IDS)
def test_at_the_limit_the_device_builds(rt, cuda, spl, fp16):
    W = bw.gpu_world(rt, "at_cap", fp16).upload()
    H, G = (compare16 if fp16 else compare)(rt, W, spl)
    assert H.build_path() == rt.BUILD_HOST and G.build_path() == rt.BUILD_DEVICE
    info = G.info()
    assert info["flat_entries"] == (512 * 128 if spl == 16 else 68112) and info["dropped_outside"] == 11
    assert (info["dropped_full"] > 0) == (spl == 16)
    if spl != 30:
        assert info["leaf_count"] == 4097
    if not fp16:
        assert G.accel_info()["large_spheres"] == (128 if spl == 16 else 133)
    assert_frames_and_rays(rt, cuda, W, G, "at_cap", fp16, spl)


# ---------------------------------------------------------------------------------------------------- b. one past the limit
@pytest.mark.parametrize("spl,fp16", MATRIX, ids=MATRIX_IDS)
def test_one_past_the_limit_the_device_declines(rt, cuda, spl, fp16):
    W = bw.gpu_world(rt, "over_cap", fp16).upload()
    H, G = (compare16 if fp16 else compare)(rt, W, spl)           # (the call returned 0: the binding raises otherwise)
    assert H.build_path() == rt.BUILD_HOST and G.build_path() == rt.BUILD_HOST_DECLINED
    info = G.info()
    assert info["flat_entries"] == (512 * 128 if spl == 16 else 68113) and info["dropped_outside"] == 10
    assert_frames_and_rays(rt, cuda, W, G, "over_cap", fp16, spl)


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
def test_three_declines_in_a_row(rt, cuda, fp16):
    """the half-made handle of a declined build is freed and the world is left as it was (its host copy is current: nothing is
    downloaded): every tree equals the first, the third renders the oracle's frame, and a world below the limit builds on the device
    afterwards"""
    spl = 17
    W = bw.gpu_world(rt, "over_cap", fp16).upload()
    first = None
    for k in range(3):
        G = rt.Octree(W, spl, gpu=True)
        assert G.build_path() == rt.BUILD_HOST_DECLINED, k
        t = tree_of(G, fp16)
        if first is None:
            first = t
        else:
            assert_same(t, first, "decline %d" % k)
        if k < 2:
            G.close()
    assert_frame(frame(rt, cuda, W, G, fp16), oracle_frame(rt, "over_cap", fp16, spl), fp16, "third tree")
    # the same process builds a world below the limit on the device afterwards
    S = bw.gpu_world(rt, "small", fp16).upload()
    assert rt.Octree(S, spl, gpu=True).build_path() == rt.BUILD_DEVICE


# ---------------------------------------------------------------------------------------------------- c. the fallback after a move
@pytest.mark.parametrize("fp16,own_stream", [(False, False), (True, False), (False, True)], ids=["fp32", "fp16", "fp32-own_stream"])
def test_fallback_after_a_move(rt, cuda, fp16, own_stream):
    """small -> over_cap -> small on one resident world.  The setter and the build that follows it are issued on one stream with no
    synchronisation in between (own_stream: a non-default, non-blocking stream - the ordering the header makes the caller's; the
    fallback's device-wide wait must then see the new values); the fallback builds from the refreshed host copy"""
    torch = cuda
    spl = 17
    g_small, g_over = bw.geometry("small"), bw.geometry("over_cap")
    d_small, d_over = torch.from_numpy(g_small).cuda(), torch.from_numpy(g_over).cuda()
    fresh = {}
    for name in ("small", "over_cap"):
        B = bw.gpu_world(rt, name, fp16).upload()
        OB = rt.Octree(B, spl, gpu=True)
        assert OB.build_path() == (rt.BUILD_DEVICE if name == "small" else rt.BUILD_HOST_DECLINED)
        fresh[name] = (tree_of(OB, fp16), frame(rt, torch, B, OB, fp16))
        OB.close(); B.close()
    assert not np.array_equal(fresh["small"][1][0], fresh["over_cap"][1][0])            # the move shows in the frame
    torch.cuda.synchronize()
    stream = torch.cuda.Stream() if own_stream else torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        A = bw.gpu_world(rt, "small", fp16).upload()
        O = rt.Octree(A, spl, gpu=True)
        assert O.build_path() == rt.BUILD_DEVICE
        got = frame(rt, torch, A, O, fp16)                          # the old geometry has been looked at
        assert_same(tree_of(O, fp16), fresh["small"][0], "small")
        assert np.array_equal(got[0], fresh["small"][1][0]) and np.array_equal(got[1], fresh["small"][1][1])
        for name, d_geom, path in (("over_cap", d_over, rt.BUILD_HOST_DECLINED), ("small", d_small, rt.BUILD_DEVICE)):
            O.close()
            A.set_geometry(d_geom)
            O = rt.Octree(A, spl, gpu=True)                         # nothing between the setter and the build
            assert O.build_path() == path, name
            assert_same(tree_of(O, fp16), fresh[name][0], name)
            got = frame(rt, torch, A, O, fp16)
            assert np.array_equal(got[0].view(np.uint8), fresh[name][1][0].view(np.uint8)) and np.array_equal(got[1], fresh[name][1][1]), name
            assert np.array_equal(A.get_geometry().cpu().numpy().view(np.uint32), (g_over if name == "over_cap" else g_small).view(np.uint32))
        assert_frame(got, oracle_frame(rt, "small", fp16, spl), fp16, "moved back")
        stream.synchronize()
    for h in (O, A):
        h.close()


# ---------------------------------------------------------------------------------------------------- d. the smallest worlds
@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", bw.SMALLEST)
def test_smallest_worlds(rt, cuda, name, fp16):
    """n = 1 (the ground alone) and n = 2 with the sphere inside / outside the root box: built on the device, equal to the host build -
    a tree that stores nothing has no grid - and a frame through each equals the oracle's"""
    spl = 30
    W = bw.gpu_world(rt, name, fp16).upload()
    if fp16:
        H, G = compare16(rt, W, spl)
    elif name == "inside":
        H, G = compare(rt, W, spl)
        assert G.accel_info()["grid_dim"] > 0
    else:
        H, G = compare_empty(rt, W, spl)
    assert G.build_path() == rt.BUILD_DEVICE
    assert G.info()["flat_entries"] == (3 if name == "inside" else 0) and G.info()["node_count"] == (7 if name == "inside" else 1)
    want = oracle_frame(rt, name, fp16, spl)
    for trav in ((None,) if fp16 else (rt.TRAVERSAL_REFERENCE, rt.TRAVERSAL_FAST)):
        assert_frame(frame(rt, cuda, W, G, fp16, trav), want, fp16, trav)
