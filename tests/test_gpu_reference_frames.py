"""k_render, k_render_h, k_render_init and the progressive pass, held DIRECTLY to frames of the reference's own render loops (-m gpu):
tests/golden/reference_frames.npz was recorded from a CPU build of main.cu's text above `int main(` (golden/make_reference_golden.py,
oracle/ref_main_capi.cpp), not from the oracle.  The cases are those of tests/reference_frames.py: create_world at N = 5 to 10000,
tree and list, overflowing buckets, binary16, rows of the 1200 x 800 frame of the reference as shipped, three progressive passes.

For each case rt.World builds the library's own rt_create_world (its list digest and camera are the fixture's), and the frame is
rendered by rt_render_init + rt_render, or rt_render_progressive passes: through the list and the tree, fast and reference traversal,
the host-built and the device-built tree.  Frame bits are compared with bitcmp.same_nan_as_ref, the RNG states by their digest.
A pixel the fixture marks as ghost (the reference has no result there, see ref_main_capi.cpp) takes no part.
Reads nothing outside tests/golden/."""
import os

import numpy as np
import pytest

import reference_frames as rf
from bitcmp import f32_bits, same_nan_as_ref
from gpu_frames import render_frame, states_of

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "reference_frames.npz"))


def created_world(rt, gold, case):
    W = rt.World(case.n, case.nx, case.ny, precision=rt.FP16 if case.fp16 else rt.FP32)
    assert np.array_equal(rf.list_digest_of_world(W), gold[case.name + "_list_sha"]), "rt_create_world's list is not the reference's"
    assert np.array_equal(f32_bits(W.camera.view(np.float32)), f32_bits(gold[case.name + "_camera"]))
    return W


def variants(rt, W, case):
    """(label, octree or None), each set up for one way through the kernels"""
    if not case.octree:
        for label, mode in (("list", rt.TRAVERSAL_FAST), ("list_reference", rt.TRAVERSAL_REFERENCE)):
            W.set_list_traversal(mode)
            yield label, None
        return
    for built, gpu in (("host_tree", False), ("device_tree", True)):
        O = rt.Octree(W.upload() if gpu else W, case.spl, gpu=gpu)
        for label, mode in (("fast", rt.TRAVERSAL_FAST), ("reference", rt.TRAVERSAL_REFERENCE)):
            O.set_traversal(mode)
            yield "%s_%s" % (built, label), O


@pytest.mark.parametrize("case", rf.RENDER, ids=lambda c: c.name)
def test_render(rt, cuda, gold, case):
    torch = cuda
    W = created_world(rt, gold, case)
    want, g = gold[case.name + "_frame"].astype(np.float32), gold[case.name + "_ghost"]
    rows = rf.rows_of(case)
    assert want.shape == (len(rows), case.nx, 3)
    n = 0
    for label, O in variants(rt, W, case):
        fb, st = render_frame(rt, torch, W, O, case.nx, case.ny, case.ns, precision=rt.FP16 if case.fp16 else None)
        got = fb.cpu().numpy().astype(np.float32).reshape(case.ny, case.nx, 3)[rows]
        assert same_nan_as_ref(got[~g], want[~g]), label
        states = states_of(st).reshape(case.ny, case.nx, 12)[rows]
        assert np.array_equal(rf.state_digest(states, g), gold[case.name + "_states_sha"]), label
        n += 1
    assert n == (4 if case.octree else 2)


@pytest.mark.parametrize("case", rf.PROGRESSIVE, ids=lambda c: c.name)
def test_render_progressive(rt, cuda, gold, case):
    torch = cuda
    W = created_world(rt, gold, case)
    want = gold[case.name + "_frame"]
    assert want.shape == (case.passes, case.ny, case.nx, 3) and not gold[case.name + "_ghost"].any()
    for label, O in variants(rt, W, case):
        st = rt.alloc_rand_state(case.nx, case.ny)
        fb = rt.alloc_fb(case.nx, case.ny)
        fb.fill_(rf.PROGRESSIVE_START)                      # pass 1 must assign over it
        rt.render_init(case.nx, case.ny, st)
        for k in range(1, case.passes + 1):
            rt.render_progressive(fb, case.nx, case.ny, k, W, st, O)
            torch.cuda.synchronize()
            assert same_nan_as_ref(fb.cpu().numpy().reshape(case.ny, case.nx, 3), want[k - 1]), (label, k)
        assert np.array_equal(rf.state_digest(states_of(st)), gold[case.name + "_states_sha"]), label
