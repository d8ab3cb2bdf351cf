"""CPU test of rt_render_kernel_name over its whole argument space (not gpu): the function builds what it needs on the host and never
starts the HIP runtime.  Worlds of both precisions, IEEE and — binary32 — contracted arithmetic; no tree under both list traversals at
22 and 500 spheres, an octree with the default traversal on a sparse, a solo and a dense world of grid_threshold_worlds, an octree
with traversal 0; modes -1 to 5.  Besides: a tree of the other precision, a NULL world, a buffer one byte short.

The expected values are literals: EXPECTED is what the library returned at the commit before the render launchers and the backend
choice were written once (162f50d) — `python tests/test_render_kernel_name_host.py` prints the table of the library it loads.  The
library has to keep answering exactly this: the name where the call returns 0, else its return code (E, S)."""
import ctypes as C
import functools

import pytest

import grid_threshold_worlds as gw

RT_EINVAL, RT_ENOTSUP = -1, -4
NX, NY = 64, 40
MODES = range(-1, 6)
BACKENDS = ("fp32", "contract", "fp16")
# (label, the world's spheres: a create_world count or a (name, variant) of grid_threshold_worlds, SPL or None = no octree,
#  traversal of the tree / the list or None = the default)
TREES = [("list22_t0", 22, None, 0), ("list22_t1", 22, None, 1), ("list500_t0", 500, None, 0), ("list500_t1", 500, None, 1),
         ("oct_coop", ("switches", "coop"), 64, None), ("oct_sparse", ("switches", "sparse"), 64, None),
         ("oct_solo", ("switches", "solo"), 64, None), ("oct_dense", ("switches", "dense"), 64, None), ("oct500_t0", 500, 30, 0)]
# the other calls on (world, tree of "oct500_t0"): a buffer one byte short of mode 0's name, one that just fits, cap == 0, and a tree of
# the other precision in modes 0 and 3
EXTRA = ("short_by_one", "exact_fit", "cap_zero", "other_precision_tree/0", "other_precision_tree/3")


def make(rt, backend, spheres, spl, trav):
    prec = rt.FP16 if backend == "fp16" else rt.FP32
    if isinstance(spheres, tuple):
        sp, cam = gw.world(*spheres)
        W = rt.World(len(sp), NX, NY, precision=prec, spheres=sp, camera=cam.view(rt.camera_dtype))
    else:
        W = rt.World(spheres, NX, NY, precision=prec)
    if backend == "contract":
        W.set_arith(rt.ARITH_CONTRACT)
    O = rt.Octree(W, spl) if spl else None
    if trav is not None:
        (O.set_traversal if O is not None else W.set_list_traversal)(trav)
    return W, O


def ask(rt, world, octree, mode, cap=64):
    """the name (return code 0) or the return code; a refusal leaves the buffer as it was"""
    buf = C.create_string_buffer(64)
    rc = rt.lib().rt_render_kernel_name(world.h if world is not None else None, octree.h if octree is not None else None, mode, buf, cap)
    assert rc == 0 or buf.value == b""
    return buf.value.decode() if rc == 0 else rc


@functools.lru_cache(None)
def answers(rt):
    """per row of EXPECTED the tuple of answers: a (backend, tree) over MODES, a backend's EXTRA, a NULL world over MODES"""
    out = {}
    for backend in BACKENDS:
        for label, spheres, spl, trav in TREES:
            W, O = make(rt, backend, spheres, spl, trav)
            out["%s/%s" % (backend, label)] = tuple(ask(rt, W, O, mode) for mode in MODES)
            if label == "oct500_t0":
                name = ask(rt, W, O, 0)
                W2, O2 = make(rt, "fp32" if backend == "fp16" else "fp16", 500, 30, None)
                out["%s/extra" % backend] = (ask(rt, W, O, 0, cap=len(name)), ask(rt, W, O, 0, cap=len(name) + 1), ask(rt, W, O, 0, cap=0),
                                             ask(rt, W, O2, 0), ask(rt, W, O2, 3))
                O2.close()
                W2.close()
            if O is not None:
                O.close()
            W.close()
    out["null_world"] = tuple(ask(rt, None, None, mode) for mode in MODES)
    return out


E, S = RT_EINVAL, RT_ENOTSUP
# modes:                -1, 0, 1, 2, 3, 4, 5 — EXTRA for the "extra" rows
EXPECTED = {
    "fp32/list22_t0": (E, "k_render<false,0,1>", "k_render<false,1,1>", E, "k_render<false,3,1>", "k_render<false,4,1>", E),
    "fp32/list22_t1": (E, "k_render<false,0,1>", "k_render<false,1,1>", E, "k_render<false,3,1>", "k_render<false,4,1>", E),
    "fp32/list500_t0": (E, "k_render<false,0,1>", "k_render<false,1,1>", E, "k_render<false,3,1>", "k_render<false,4,1>", E),
    "fp32/list500_t1": (E, "k_render<true,0,5>", "k_render<true,1,5>", E, "k_render<true,3,5>", "k_render<true,4,5>", E),
    "fp32/oct_coop": (E, "k_render<true,0,4>", "k_render<true,1,4>", E, "k_render<true,3,4>", "k_render<true,4,4>", E),
    "fp32/oct_sparse": (E, "k_render<true,0,2>", "k_render<true,1,2>", E, "k_render<true,3,2>", "k_render<true,4,2>", E),
    "fp32/oct_solo": (E, "k_render<true,0,5>", "k_render<true,1,5>", E, "k_render<true,3,5>", "k_render<true,4,5>", E),
    "fp32/oct_dense": (E, "k_render<true,0,4>", "k_render<true,1,4>", E, "k_render<true,3,4>", "k_render<true,4,4>", E),
    "fp32/oct500_t0": (E, "k_render<true,0,1>", "k_render<true,1,1>", E, "k_render<true,3,1>", "k_render<true,4,1>", E),
    "fp32/extra": (E, "k_render<true,0,1>", E, E, E),
    "contract/list22_t0": (E, "k_render<false,0,1>", "k_render<false,1,1>", E, "k_render<false,3,1>", "k_render<false,4,1>", E),
    "contract/list22_t1": (E, "k_render<false,0,1>", "k_render<false,1,1>", E, "k_render<false,3,1>", "k_render<false,4,1>", E),
    "contract/list500_t0": (E, "k_render<false,0,1>", "k_render<false,1,1>", E, "k_render<false,3,1>", "k_render<false,4,1>", E),
    "contract/list500_t1": (E, "k_render<true,0,5>", "k_render<true,1,5>", E, "k_render<true,3,5>", "k_render<true,4,5>", E),
    "contract/oct_coop": (E, "k_render<true,0,4>", "k_render<true,1,4>", E, "k_render<true,3,4>", "k_render<true,4,4>", E),
    "contract/oct_sparse": (E, "k_render<true,0,2>", "k_render<true,1,2>", E, "k_render<true,3,2>", "k_render<true,4,2>", E),
    "contract/oct_solo": (E, "k_render<true,0,5>", "k_render<true,1,5>", E, "k_render<true,3,5>", "k_render<true,4,5>", E),
    "contract/oct_dense": (E, "k_render<true,0,4>", "k_render<true,1,4>", E, "k_render<true,3,4>", "k_render<true,4,4>", E),
    "contract/oct500_t0": (E, "k_render<true,0,1>", "k_render<true,1,1>", E, "k_render<true,3,1>", "k_render<true,4,1>", E),
    "contract/extra": (E, "k_render<true,0,1>", E, E, E),
    "fp16/list22_t0": (E, "k_render_h<false,0>", "k_render_h<false,1>", E, "k_render_h<false,3>", S, E),
    "fp16/list22_t1": (E, "k_render_h<false,0>", "k_render_h<false,1>", E, "k_render_h<false,3>", S, E),
    "fp16/list500_t0": (E, "k_render_h<false,0>", "k_render_h<false,1>", E, "k_render_h<false,3>", S, E),
    "fp16/list500_t1": (E, "k_render_h<false,0>", "k_render_h<false,1>", E, "k_render_h<false,3>", S, E),
    "fp16/oct_coop": (E, "k_render_h<true,0>", "k_render_h<true,1>", E, "k_render_h<true,3>", S, E),
    "fp16/oct_sparse": (E, "k_render_h<true,0>", "k_render_h<true,1>", E, "k_render_h<true,3>", S, E),
    "fp16/oct_solo": (E, "k_render_h<true,0>", "k_render_h<true,1>", E, "k_render_h<true,3>", S, E),
    "fp16/oct_dense": (E, "k_render_h<true,0>", "k_render_h<true,1>", E, "k_render_h<true,3>", S, E),
    "fp16/oct500_t0": (E, "k_render_h<true,0>", "k_render_h<true,1>", E, "k_render_h<true,3>", S, E),
    "fp16/extra": (E, "k_render_h<true,0>", E, E, E),
    "null_world": (E, E, E, E, E, E, E),
}


def test_the_table_is_complete():
    assert set(EXPECTED) == {"%s/%s" % (b, t[0]) for b in BACKENDS for t in TREES} | {b + "/extra" for b in BACKENDS} | {"null_world"}
    assert all(len(v) == (len(EXTRA) if k.endswith("/extra") else len(MODES)) for k, v in EXPECTED.items())
    flat = [x for v in EXPECTED.values() for x in v]
    assert {x for x in flat if isinstance(x, int)} == {RT_EINVAL, RT_ENOTSUP}
    # every (TREE, COOPG) the binary32 ladder can launch is named in every mode that has a call, and both TREE arguments of binary16
    names = {x for x in flat if isinstance(x, str)}
    for mode in (0, 1, 3, 4):
        assert {"k_render<false,%d,1>" % mode} | {"k_render<true,%d,%d>" % (mode, v) for v in (1, 2, 4, 5)} <= names
    for mode in (0, 1, 3):
        assert {"k_render_h<false,%d>" % mode, "k_render_h<true,%d>" % mode} <= names


@pytest.mark.parametrize("row", sorted(EXPECTED))
def test_answers(rt, row):
    assert answers(rt)[row] == EXPECTED[row]


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dd2360-raytracing_amd"))
    import rt_amd
    for k, v in answers(rt_amd).items():
        print('    "%s": (%s),' % (k, ", ".join('"%s"' % x if isinstance(x, str) else {RT_EINVAL: "E", RT_ENOTSUP: "S"}[x] for x in v)))
