"""CPU tests (not gpu) of tests/build_limit_worlds.py: every world sits where its name says - on the numpy model of k_pairs' count, on
the product's host build (rt_build_octree) and on the oracle alone.  tests/test_gpu_build_limits.py then runs the same worlds through
rt_build_octree_gpu, where `at_cap` must be built on the device and `over_cap` must be declined."""
import numpy as np
import pytest

import build_limit_worlds as bw
from grid_threshold_worlds import stored_set

PRECISIONS = [False, True]
IDS = ["fp32", "fp16"]


def test_the_limit_is_the_device_builds():
    # Restates rt_build.hip:464, `cap = (size_t)16 * n + 65536`: the one quantity taken from the code under test.  That the code
    # takes the branch at this value is what tests/test_gpu_build_limits.py checks (the build path of at_cap and of over_cap).
    assert bw.cap(161) == 16 * 161 + 65536 == 68112


@pytest.mark.parametrize("fp16", PRECISIONS, ids=IDS)
def test_model_counts_sit_at_and_one_past_the_limit(fp16):
    at, over, small = (bw.pairs_model(bw.spheres(n), fp16) for n in bw.NAMES)
    assert len(bw.spheres("at_cap")) == len(bw.spheres("over_cap")) == len(bw.spheres("small")) == 161
    assert at["pairs"] == 68112 == bw.cap(161) and at["outside"] == 11
    assert over["pairs"] == 68113 == bw.cap(161) + 1 and over["outside"] == 10
    assert small["pairs"] == 133 * 8 + 16 and small["outside"] == 11
    # a shell touches all 512 cells, a one-cell sphere one, a sphere outside the box none; the two worlds differ in slot MOVED alone
    assert (at["per_sphere"][bw.SHELLS] == 512).all() and (at["per_sphere"][bw.ONE_CELL] == 1).all() and not at["per_sphere"][bw.MOVED:].any()
    assert at["per_sphere"][bw.MOVED] == 0 and over["per_sphere"][bw.MOVED] == 1
    assert np.array_equal(np.delete(at["per_sphere"], bw.MOVED), np.delete(over["per_sphere"], bw.MOVED))
    a, o = bw.spheres("at_cap"), bw.spheres("over_cap")
    assert np.array_equal(np.delete(a, bw.MOVED).view(np.uint8), np.delete(o, bw.MOVED).view(np.uint8))
    # small and over_cap are one list with two geometries: what rt_world_set_geometry can move between
    s = bw.spheres("small")
    for f in ("material", "albedo", "param"):
        assert np.array_equal(s[f], o[f]), f
    assert not np.array_equal(bw.geometry("small"), bw.geometry("over_cap"))
    # the camera lies outside every shell
    assert bw.spheres("at_cap")["radius"][bw.SHELLS].max() == 11.0625 < np.sqrt(13.0 ** 2 + 1.0 + 3.0 ** 2)
    assert sorted(set(a["material"][bw.SHELLS].tolist())) == [bw.LAMBERTIAN, bw.METAL, bw.DIELECTRIC]


@pytest.mark.parametrize("fp16", PRECISIONS, ids=IDS)
@pytest.mark.parametrize("name,outside", [("at_cap", 11), ("over_cap", 10)])
def test_host_builds(rt, name, outside, fp16):
    """rt_build_octree of the worlds: the entries of the traversal copy are the model's pairs (SPL 30 drops nothing), SPL 17 fills all
    4096 buckets and drops nothing, SPL 16 drops the five outermost shells and every one-cell sphere from every cell"""
    W = bw.gpu_world(rt, name, fp16)
    model = bw.pairs_model(bw.spheres(name), fp16)
    i30, i17, O16 = rt.Octree(W, 30).info(), rt.Octree(W, 17).info(), rt.Octree(W, 16)
    i16 = O16.info()
    for info in (i30, i17, i16):
        assert info["dropped_outside"] == outside == model["outside"] and info["node_count"] == 585
    assert i30["flat_entries"] == model["pairs"] and i30["dropped_full"] == 0 and i30["leaf_count"] == 1 + 512 * 5
    assert i17["leaf_count"] == 4097 and i17["dropped_full"] == 0 and i17["flat_entries"] == model["pairs"]
    assert i16["leaf_count"] == 4097 and i16["dropped_full"] == model["pairs"] - 512 * 128 > 0 and i16["flat_entries"] == 512 * 128
    stored = stored_set(*O16.leaves())
    assert np.array_equal(stored, bw.SHELLS[:128])                 # slots 129..133 and every one-cell sphere are in no leaf
    assert np.array_equal(stored_set(*rt.Octree(W, 17).leaves()), np.flatnonzero(model["per_sphere"]))


@pytest.mark.parametrize("fp16", PRECISIONS, ids=IDS)
@pytest.mark.parametrize("name", bw.SMALLEST)
def test_smallest_worlds(rt, name, fp16):
    """n = 1 and n = 2 are accepted by rt_world_create and rt_build_octree; the tree of `ground` and of `outside` is the root alone"""
    sp = bw.spheres(name)
    assert len(sp) == (1 if name == "ground" else 2)
    info = rt.Octree(bw.gpu_world(rt, name, fp16), 30).info()
    model = bw.pairs_model(sp, fp16)
    assert info["flat_entries"] == model["pairs"] == (3 if name == "inside" else 0)
    assert info["dropped_outside"] == model["outside"] == (1 if name == "outside" else 0)
    assert info["node_count"] == (7 if name == "inside" else 1)
    assert bw.oracle(rt, name, fp16, 30).info()["leaf_entries"] == model["pairs"]


@pytest.mark.parametrize("fp16", PRECISIONS, ids=IDS)
@pytest.mark.parametrize("spl", [16, 17, 30])
@pytest.mark.parametrize("name", ["at_cap", "over_cap"])
def test_rays_hit_the_shells_through_the_tree(rt, name, spl, fp16):
    """the rays of the GPU test, on the oracle: at least a quarter of those that hit anything hit a shell, found in the tree's leaves;
    with SPL 16 none hits a dropped sphere; the aimed rays start outside every shell"""
    rays = bw.rays(fp16)
    assert rays.shape == (bw.N_RAYS, 6)
    far = np.linalg.norm(rays[-bw.N_AIMED:, :3].astype(np.float64) - [0.0, 1.0, 0.0], axis=1)
    assert far.min() > 11.0625
    ref = bw.oracle(rt, name, fp16, spl).trace(rays, mode=2)
    hit = ref["sphere"] >= 0
    shell = np.isin(ref["sphere"], bw.SHELLS)
    # floors: a quarter of the rays start inside the innermost shell, and every aimed ray crosses all shells in exact arithmetic (in
    # binary16 the far-away quarter of random_rays overflows and hits nothing, and a grazing aimed ray may miss)
    assert hit.sum() >= bw.N_RAYS // 4 and 4 * shell.sum() >= hit.sum()
    assert shell[-bw.N_AIMED:].sum() >= bw.N_AIMED // 2
    if spl == 16:
        assert ref["sphere"].max() <= bw.SHELLS[127]
    else:
        assert (ref["sphere"] == bw.SHELLS[-1]).any()              # the outermost shell, from outside


@pytest.mark.parametrize("fp16", PRECISIONS, ids=IDS)
def test_build_path_of_a_host_build(rt, fp16):
    assert (rt.BUILD_HOST, rt.BUILD_DEVICE, rt.BUILD_HOST_DECLINED) == (0, 1, 2)
    assert rt.Octree(bw.gpu_world(rt, "over_cap", fp16), 30).build_path() == rt.BUILD_HOST
    assert rt.lib().rt_octree_build_path(None) == -1
