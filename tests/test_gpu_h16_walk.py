"""closest_tree, the binary16 tree walk (csrc/rt_kernels_fp16.hip), at its pool limits, pair edges and ties (-m gpu).  The worlds and ray
sets are those of tests/h16_walk_worlds.py; tests/test_h16_walk_worlds_host.py shows on the CPU, from a numpy model and the oracle alone,
that every input sits at the rule it is named for: the 7 / 8-pair class boundary and the NaN half of an odd node (leaf_sizes), equal-t
ties between different spheres (twins), a candidate queue that fills inside one pass (stack), roots at, below and above t_min (tmin),
0/0 and +-inf slab parameters (on_planes), task and segment pools that overflow with stalled and finished lanes in one wave (flood).

Every comparison is bit for bit against the oracle's binary16 hitTree / render, and no ray is left out:
  * rt_trace_rays for every (world, ray set), through a host-built tree (rt_build_octree) and a device-built one (rt_build_octree_gpu),
    whose pair arrays - k_pairs<half_t> / k_entries<half_t>: two entries per 16 bytes, a NaN half and id -1 closing an odd node - must
    be the layout the model derives from the library's host tree;
  * launches of 1, 63, 64, 65 and 129 rays against the same rays in one large launch;
  * one frame per world (32 x 24, 4 samples; leaf_sizes and stack: progressive passes as well), where dead and retired lanes share
    the walk's rounds with live ones.

NOT covered, because no tree the library builds reaches them: closest_tree's walk for !regular_planes(T) and its
48-byte-node path for h16_np[0] == 0.  The root box is fixed at (-11, 0, -11) - (11, 2, 11), so h16_plane_table always yields 9 / 9 / 9
planes (27 <= 30) and rt_build.hip sets 9 / 9 / 9 outright.  Nobody should assume these tests run those two branches."""
import functools

import numpy as np
import pytest

import h16_walk_worlds as hw
from tree_compare import assert_records, traced

pytestmark = pytest.mark.gpu
BUILDS = ["host", "device"]


@functools.lru_cache(None)
def device_side(rt, world, build):
    """(uploaded world, tree of that build), kept for the module"""
    W, spl = hw.library_world(rt, world)
    W.upload()
    if build == "device":
        O = rt.Octree(W, spl, gpu=True)
        assert O.build_path() == rt.BUILD_DEVICE
    else:
        O = rt.Octree(W, spl).upload()
        assert O.build_path() == rt.BUILD_HOST
    return W, O


def assert_case(rt, torch, world, build, rays, ref, label):
    W, O = device_side(rt, world, build)
    got = traced(rt, torch, W, O, rays)
    assert np.array_equal(got["sphere"] >= 0, ref["hit"] != 0), label
    assert_records(got, ref, label)
    return got


# ---------------------------------------------------------------------------------------------------- the pair layout
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("world", hw.WORLDS)
def test_pair_arrays_are_the_models_layout(rt, cuda, world, build):
    tree, sp, _, info = hw.host_side(rt, world)
    W, O = device_side(rt, world, build)
    assert O.info() == info
    pairs = O.device_array(1).view(np.uint16).reshape(-1, 4, 2)           # per pair (cx, cy, cz, r^2) x (first, second entry)
    ids = O.device_array(2).view(np.int32).reshape(-1, 2)
    assert len(pairs) == len(ids) == tree.n_pairs
    with np.errstate(over="ignore"):
        c, r = sp["center"].astype(np.float16), sp["radius"].astype(np.float16)
        want = np.concatenate([c, (r * r)[:, None]], 1).view(np.uint16)
    for pos in np.flatnonzero(tree.level == 3):
        m = tree.members[pos]
        for k in range(tree.pairs[pos]):
            p = tree.first[pos] + k
            assert ids[p, 0] == m[2 * k] and np.array_equal(pairs[p, :, 0], want[m[2 * k]]), (pos, k)
            if 2 * k + 1 < len(m):
                assert ids[p, 1] == m[2 * k + 1] and np.array_equal(pairs[p, :, 1], want[m[2 * k + 1]]), (pos, k)
            else:
                assert ids[p, 1] == -1 and np.isnan(pairs[p, :, 1].view(np.float16)).all(), (pos, k)


# ---------------------------------------------------------------------------------------------------- hit records
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("world,rayset", hw.CASES, ids=hw.IDS)
def test_hit_records_are_the_oracles(rt, cuda, world, rayset, build):
    rays, m, ref = hw.host_case(rt, world, rayset)
    assert len(rays) <= 20000
    assert_case(rt, cuda, world, build, rays, ref, (world, rayset, build))


@pytest.mark.parametrize("build", BUILDS)
def test_small_launches_equal_one_large_launch(rt, cuda, build):
    """1, 63, 64, 65 and 129 rays - a lone lane, a wave short of one lane, a full wave, a wave and one lane, two waves and one - of
    on_planes, aimed17 (the odd last node) and aimed13 (small segments) rays on leaf_sizes: the records of the same rays in one launch
    of 3201, which are the oracle's"""
    _, _, S, _ = hw.host_side(rt, "leaf_sizes")
    head = np.concatenate([hw.case_rays("leaf_sizes", "on_planes")[:40], hw.case_rays("leaf_sizes", "aimed17")[:64], hw.case_rays("leaf_sizes", "aimed13")[:25]])
    large = np.concatenate([head, hw.case_rays("leaf_sizes", "on_planes")])
    assert len(head) == max(hw.BATCHES)
    ref = S.trace(large, mode=2)
    whole = assert_case(rt, cuda, "leaf_sizes", build, large, ref, "large")
    assert (ref["sphere"][:129] >= 0).sum() >= 64
    W, O = device_side(rt, "leaf_sizes", build)
    for n in hw.BATCHES:
        got = traced(rt, cuda, W, O, large[:n])
        assert got.tobytes() == whole[:n].tobytes(), n


# ---------------------------------------------------------------------------------------------------- frames
@functools.lru_cache(None)
def oracle_frame(rt, world):
    fb, st = hw.oracle(rt, world).render(hw.NS, nthreads=8)
    fb.setflags(write=False); st.setflags(write=False)
    return fb, st


def assert_frame(torch, fb, st, ref, ref_st, what):
    """as test_gpu_build_limits.assert_frame: the oracle returns exact float images of its binary16 values"""
    got = fb.cpu().numpy().reshape(hw.NY, hw.NX, 3)
    nan = np.isnan(ref)
    assert np.array_equal(got.view(np.uint16)[~nan], ref.astype(np.float16).view(np.uint16)[~nan]), what
    assert np.isnan(got[nan]).all(), what
    assert np.array_equal(st.cpu().numpy().view(np.uint32).reshape(-1, 12)[:, :6], ref_st[:, :6]), what


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("world", hw.WORLDS)
def test_frames_are_the_oracles(rt, cuda, world, build):
    torch = cuda
    W, O = device_side(rt, world, build)
    ref, ref_st = oracle_frame(rt, world)
    seen = hw.host_side(rt, world)[2].trace(hw.pixel_rays(hw.camera(rt, world)), mode=2)["sphere"]
    assert (seen > 0).sum() >= 24 and (seen < 0).sum() >= 24                 # the camera sees the special cells, and past them
    fb, st = rt.alloc_fb(hw.NX, hw.NY, precision=rt.FP16), rt.alloc_rand_state(hw.NX, hw.NY)
    rt.render_init(hw.NX, hw.NY, st)
    rt.render(fb, hw.NX, hw.NY, hw.NS, W, st, O)
    torch.cuda.synchronize()
    assert_frame(torch, fb, st, ref, ref_st, (world, build))


@pytest.mark.parametrize("world", ["leaf_sizes", "stack"])
def test_progressive_passes_are_the_oracles(rt, cuda, world):
    torch = cuda
    W, O = device_side(rt, world, "device")
    S = hw.oracle(rt, world)
    ref_st = S.render_init()
    ref = np.zeros((hw.NY, hw.NX, 3), np.float32)
    fb, st = rt.alloc_fb(hw.NX, hw.NY, precision=rt.FP16), rt.alloc_rand_state(hw.NX, hw.NY)
    rt.render_init(hw.NX, hw.NY, st)
    for k in range(1, 4):
        rt.render_progressive(fb, hw.NX, hw.NY, k, W, st, O)
        S.render_progressive(ref, k, ref_st, nthreads=8)
    torch.cuda.synchronize()
    assert_frame(torch, fb, st, ref, ref_st, world)
