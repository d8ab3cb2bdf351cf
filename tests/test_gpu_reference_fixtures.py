"""The kernels, held DIRECTLY to what the reference's own functions computed (-m gpu): tests/golden/reference_hits.npz and
reference_octrees.npz were recorded from a CPU build of the reference's headers (golden/make_reference_golden.py), not from the oracle.
k_trace (fast and reference traversal, list and tree), k_trace_h (binary16) and k_guides against the hit records; the device-built
octree (rt_build_octree_gpu, nodes and leaves in the reference's numbering) against the octree digests.  All nine worlds of
material_edge_worlds.WORLDS and one random_world world.  Bit equality, "NaN where the reference has NaN" (bitcmp.same_nan_as_ref).
Reads nothing outside tests/golden/.  Frames of the reference's own render loops: tests/test_gpu_reference_frames.py."""
import os

import numpy as np
import pytest

import reference_cases as rc
from bitcmp import f32_bits, same_nan_as_ref
from tree_compare import traced

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = list(rc.EDGE) + ["random_1"]


@pytest.fixture(scope="module")
def gold():
    return {f: np.load(os.path.join(GOLD, "reference_%s.npz" % f)) for f in ("hits", "bounces", "octrees")}


def gpu_world(rt, w, fp16):
    return rt.World(w[2].size, rc.NX, rc.NY, precision=rt.FP16 if fp16 else rt.FP32, spheres=rc.as_spheres(*w[:3]), camera=w[3].view(rt.camera_dtype))


def assert_records(got, g, key, label):
    assert np.array_equal(got["sphere"], g[key + "sphere"]), label
    for f in ("t", "p", "normal"):
        assert same_nan_as_ref(got[f], g[key + f]), (label, f)


@pytest.mark.parametrize("name", NAMES)
def test_trace_and_guides_fp32(rt, cuda, gold, name):
    """k_trace in its four modes on the whole ray set; k_guides, whose GX x GY pixel-centre rays open the ray set, on its head"""
    torch = cuda
    w = rc.world_of(gold, name, False)
    W = gpu_world(rt, w, False)
    O = rt.Octree(W, w[4])
    rays = gold["hits"][name + "_rays"]
    head = rc.GX * rc.GY
    assert np.array_equal(f32_bits(rays[:head]), f32_bits(rc.ray_set(name, w, 0)))          # the fixture's head IS the guides' ray set
    k = rc.tag(name, False)
    for label, oct_, mode, m in (("list", None, rt.TRAVERSAL_FAST, "list"), ("list_reference", None, rt.TRAVERSAL_REFERENCE, "list"),
                                 ("tree_reference", O, rt.TRAVERSAL_REFERENCE, "tree"), ("tree", O, rt.TRAVERSAL_FAST, "tree")):
        if oct_ is not None:
            oct_.set_traversal(mode)
        else:
            W.set_list_traversal(mode)
        assert_records(traced(rt, torch, W, oct_, rays), gold["hits"], "%s_%s_" % (k, m), label)
        d = rt.alloc_guides(rc.GX, rc.GY)
        rt.render_guides(W, oct_, rc.GX, rc.GY, d)
        torch.cuda.synchronize()
        got = d.cpu().numpy().view(rt.hit_record_dtype)
        assert_records(got, {f: gold["hits"]["%s_%s_%s" % (k, m, f)][:head] for f in ("sphere", "t", "p", "normal")}, "", label + " guides")
    assert (gold["hits"][k + "_tree_sphere"] >= 0).sum() >= 16


@pytest.mark.parametrize("name", NAMES)
def test_trace_binary16(rt, cuda, gold, name):
    """k_trace_h through the list and the tree"""
    torch = cuda
    w = rc.world_of(gold, name, True)
    W = gpu_world(rt, w, True)
    O = rt.Octree(W, w[4])
    rays = rc.half(gold["hits"][name + "_rays"])
    k = rc.tag(name, True)
    for oct_, m in ((None, "list"), (O, "tree")):
        assert_records(traced(rt, torch, W, oct_, rays), gold["hits"], "%s_%s_" % (k, m), m)
    assert (gold["hits"][k + "_tree_sphere"] >= 0).sum() >= 8


@pytest.mark.parametrize("fp16", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_device_built_octree(rt, cuda, gold, name, fp16):
    """rt_build_octree_gpu: counts, nodes and leaves are buildOctree's"""
    w = rc.world_of(gold, name, fp16)
    W = gpu_world(rt, w, fp16).upload()
    G = rt.Octree(W, w[4], gpu=True)
    cuda.cuda.synchronize()
    k = "%s_spl%d_" % (rc.tag(name, fp16), w[4])
    info = G.info()
    assert [info[f] for f in ("node_count", "leaf_count", "dropped_full", "dropped_outside")] == gold["octrees"][k + "counts"].tolist()
    nodes = G.nodes()
    counts, idx = G.leaves()
    assert np.array_equal(rc.sha(nodes["level"], nodes["aabb"], nodes["children"], counts, idx), gold["octrees"][k + "sha"])
