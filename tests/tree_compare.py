"""What the tree and grid tests share: the device build of a tree against the host build, array for array, and hit records through
rt_trace_rays against a reference's."""
import numpy as np

from bitcmp import same_nan_as_ref

ARRAYS = ["nodes", "ent_hot", "ent_id", "large_hot", "large_brick", "cs", "hot", "brick", "memb_start", "memb_cell", "cellnode", "bits_index", "cellbits"]


def compare(rt, W, spl):
    H = rt.Octree(W, spl).upload()
    G = rt.Octree(W, spl, gpu=True)
    assert H.info() == G.info()
    assert H.accel_info() == G.accel_info()
    assert np.array_equal(H.nodes().view(np.uint8), G.nodes().view(np.uint8))                  # OctNode[585], reference numbering
    hc, hi = H.leaves(); gc, gi = G.leaves()
    assert np.array_equal(hc, gc) and np.array_equal(hi, gi)                                   # OctLeaf contents, reference numbering
    for k, name in enumerate(ARRAYS):
        a, b = H.device_array(k), G.device_array(k)
        assert a.size == b.size, name
        if name == "large_hot" and a.size == 0:
            continue
        assert np.array_equal(a, b), name
    return H, G


def compare_empty(rt, W, spl):
    """compare for a tree that stores no sphere: there is no grid, and the contents of the grid arrays are unspecified
    (no kernel reads them while enabled == 0; the device build leaves them unset).  The comparison covers the infos, the
    reference-layout nodes and leaves, the traversal nodes and the (empty) entry arrays, and the sizes rt_octree_debug_array states for
    the grid arrays of either build"""
    H = rt.Octree(W, spl).upload()
    G = rt.Octree(W, spl, gpu=True)
    assert H.info() == G.info() and H.info()["flat_entries"] == 0
    assert H.accel_info() == G.accel_info() == dict(grid_dim=0, cell_size=0.0, grid_entries=0, large_spheres=0)
    assert np.array_equal(H.nodes().view(np.uint8), G.nodes().view(np.uint8))
    hc, hi = H.leaves(); gc, gi = G.leaves()
    assert np.array_equal(hc, gc) and np.array_equal(hi, gi) and not hc.any()
    for k in range(3):
        a, b = H.device_array(k), G.device_array(k)
        assert a.size == b.size and np.array_equal(a, b), k
    for k in range(3, 13):
        assert H.device_array(k).size == G.device_array(k).size, k
    return H, G


def traced(rt, torch, W, O, rays):
    """the hit records of rt_trace_rays for an [n, 6] ray array (copied: a cached, read-only array is fine)"""
    d_rays = torch.from_numpy(np.array(rays, np.float32)).cuda()
    d_out = torch.zeros(len(rays) * 32, dtype=torch.uint8, device="cuda")
    rt.trace_rays(W, O, d_rays, len(rays), d_out)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(rt.hit_record_dtype)


def assert_records(got, ref, label):
    assert np.array_equal(got["sphere"], ref["sphere"]), label
    for f in ("t", "p", "normal"):
        assert same_nan_as_ref(got[f], ref[f]), (label, f)
