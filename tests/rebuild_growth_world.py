"""The two layouts of the growth case of rt_octree_rebuild_gpu (tests/test_gpu_rebuild.py): one resident world whose tree outgrows what
the handle kept.

  first   create_world, N = 2000, radius 0.1: the small spheres spread over the whole root box, one or two level-3 cells each.
  grown   the same list with every small sphere drawn into the level-3 cell [0, 2.75) x [0, 0.25) x [0, 2.75) (a 45 x 45 lattice, each
          resting on the ground), every third of them with four times the radius: a sphere of radius 0.4 reaches four cells in y and is
          too large for the grid's columns (R' > 1.5 h with h from the median radius, which stays 0.1), so it goes to the large list.

A rebuild sizes its count-dependent arrays by the previous build's counts plus a quarter; `counts` gives those counts from the HOST build
(rt_build_octree, no device) and from build_limit_worlds.pairs_model, and tests/test_rebuild_growth_host.py holds them to the 1.25:
pairs, bucket entries and large spheres of `grown` exceed it.  The grid registrations do NOT: the enlarged spheres leave the grid for the
large list, and a small sphere registers in as many columns as before - the host test states the figures.  SPHERES_PER_LEAF is 320, so
that the 2000 members of one cell fit its eight buckets and nothing is dropped.

A helper module (no tests, not a conftest)."""
import numpy as np

import build_limit_worlds as bw

F = np.float32
N, SPL, NX, NY = 2000, 320, 64, 40
CELL = 2.75                                                 # a level-3 cell's extent in x and z
SLACK = 1.25


def small_slots(spheres):
    """the slots that hold a small sphere (not the ground, not the three unit spheres, no ghost)"""
    s = np.where((spheres["material"] != -1) & (spheres["radius"] < F(0.5)))[0]
    return s[s > 0]


def grown_spheres(spheres):
    """the list of `grown` from the list of `first`"""
    g = spheres.copy()
    small = small_slots(spheres)
    side = int(np.ceil(np.sqrt(len(small))))
    k = np.arange(len(small))
    g["center"][small, 0] = ((k % side + 0.5) * CELL / side).astype(F)
    g["center"][small, 2] = ((k // side + 0.5) * CELL / side).astype(F)
    g["radius"][small[::3]] *= F(4)
    g["center"][small, 1] = g["radius"][small]
    return g


def geometry(spheres):
    """(cx, cy, cz, radius) per slot: what rt_world_set_geometry takes"""
    return np.ascontiguousarray(np.concatenate([spheres["center"], spheres["radius"][:, None]], 1), F)


def counts(rt, spheres, camera):
    """what the build counts for this list, from the host build and the pairs model: dict(pairs, entries, leaves, registrations, large)"""
    W = rt.World(len(spheres), NX, NY, spheres=spheres, camera=camera)
    O = rt.Octree(W, SPL)
    try:
        info, accel = O.info(), O.accel_info()
        assert info["dropped_full"] == 0
        return dict(pairs=bw.pairs_model(spheres, False)["pairs"], entries=info["flat_entries"], leaves=info["leaf_count"],
                    registrations=accel["grid_entries"], large=accel["large_spheres"])
    finally:
        O.close(); W.close()
