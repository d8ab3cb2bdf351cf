"""Edge cases of the REFERENCE that the experiment harness and the build tests discovered, pinned on the GPU (-m gpu):

  * hitTree and hitable_list::hit do not always agree (SURVEY fact 6 says they do; probed there at N = 22 / 500 / 2000).  traverseTree only
    reaches spheres through the level-3 cells whose slab tests pass (acceleration_structure.h:276-304); hitable_list::hit tests every
    sphere (hitable_list.h:21-29).  N = 1000, r = 0.1, 1200x800x10 (the harness's cell): ONE pixel of the frame differs, (671, 450).
    Both paths are reproduced as they are: each frame equals the oracle's, and they differ exactly where the oracle's two frames differ.
  * a tree whose buckets overflow (acceleration_structure.h:135-136: "leaf nodes are full", the sphere is silently dropped; :284-285:
    the bucket scan stops at the first empty slot): N = 2000 with SPHERES_PER_LEAF 3 drops 834 insertions.  The RENDER through that
    tree — fast traversal and reference traversal — equals the oracle's; the dropped spheres are invisible, so the frame is not the list's.
"""
import numpy as np
import pytest

from bitcmp import f32_bits, same_nan_as_ref
from gpu_frames import frame_image, render_frame
from oracle_lib import OracleScene

pytestmark = pytest.mark.gpu


def test_list_and_octree_disagree_in_one_pixel_exactly_as_the_reference_paths_do(rt, cuda):
    torch = cuda
    nx, ny, ns, n, spl = 1200, 800, 10, 1000, 30
    W = rt.World(n, nx, ny)
    O = rt.Octree(W, spl)
    assert O.info()["dropped_full"] == 0 and O.info()["dropped_outside"] == 0          # nothing is missing from the tree: the paths differ by traversal alone
    f_list = frame_image(render_frame(rt, torch, W, None, nx, ny, ns)[0], nx, ny)
    f_tree = frame_image(render_frame(rt, torch, W, O, nx, ny, ns)[0], nx, ny)
    differ = np.argwhere((f32_bits(f_list) != f32_bits(f_tree)).any(axis=2) & ~(np.isnan(f_list).any(axis=2) & np.isnan(f_tree).any(axis=2)))
    assert [tuple(int(v) for v in d) for d in differ] == [(450, 671)], differ             # (row j, column i): pixel (671, 450), j counted from the bottom row
    # the two reference paths on the CPU: the rows around that pixel, and a few others
    rows = (0, 200, 449, 450, 451, 799)
    S_list = OracleScene(n, nx, ny, use_octree=False)
    S_tree = OracleScene(n, nx, ny, use_octree=True, spl=spl)
    o_lists = {}
    for r in rows:
        o_list = o_lists[r] = S_list.render(ns, row0=r, rows=1, nthreads=1)[0][0]
        o_tree = S_tree.render(ns, row0=r, rows=1, nthreads=1)[0][0]
        assert same_nan_as_ref(f_list[r], o_list), "list row %d differs from the oracle's hitable_list path" % r
        assert same_nan_as_ref(f_tree[r], o_tree), "octree row %d differs from the oracle's hitTree path" % r
        d = np.flatnonzero((f32_bits(o_list) != f32_bits(o_tree)).any(axis=1) & ~np.isnan(o_list).any(axis=1))
        assert list(d) == ([671] if r == 450 else []), (r, d)
    # the values the harness recorded: list (0.4648, 0.5031, 0.4974), octree (0.4479, 0.4836, 0.5074)
    assert np.allclose(f_list[450, 671], (0.4648, 0.5031, 0.4974), atol=5e-5) and np.allclose(f_tree[450, 671], (0.4479, 0.4836, 0.5074), atol=5e-5)
    # the plain list-order scan and the literal tree traversal give the same two frames as the default (grid) paths
    W.set_list_traversal(rt.TRAVERSAL_REFERENCE)
    f_list_ref = frame_image(render_frame(rt, torch, W, None, nx, ny, ns)[0], nx, ny)
    assert same_nan_as_ref(f_list_ref, f_list), "the list-order scan differs from the default list path"
    for r in (449, 450, 451):
        assert same_nan_as_ref(f_list_ref[r], o_lists[r]), "list-order scan row %d differs from the oracle's hitable_list path" % r
    O.set_traversal(rt.TRAVERSAL_REFERENCE)
    f_tree_ref = frame_image(render_frame(rt, torch, W, O, nx, ny, ns)[0], nx, ny)
    assert same_nan_as_ref(f_tree_ref, f_tree)


def test_render_through_a_tree_with_full_buckets_equals_the_oracle(rt, cuda):
    torch = cuda
    nx, ny, ns, n, spl = 400, 300, 8, 2000, 3
    W = rt.World(n, nx, ny)
    O = rt.Octree(W, spl)
    info = O.info()
    assert info["dropped_full"] == 834 and info["dropped_outside"] == 0                  # host/rt_scene.hpp == oracle (tests/test_host_sanitizers.py prints the same)
    S = OracleScene(n, nx, ny, use_octree=True, spl=spl)
    assert S.info()["dropped_full"] == 834
    want = S.render(ns, nthreads=8)[0]
    fast = frame_image(render_frame(rt, torch, W, O, nx, ny, ns)[0], nx, ny)
    assert same_nan_as_ref(fast, want), "fast traversal through overflowing buckets differs from the oracle"
    O.set_traversal(rt.TRAVERSAL_REFERENCE)
    assert same_nan_as_ref(frame_image(render_frame(rt, torch, W, O, nx, ny, ns)[0], nx, ny), want), "reference traversal through overflowing buckets differs from the oracle"
    # the device-built tree drops the same insertions and renders the same frame
    Og = rt.Octree(W, spl, gpu=True)
    assert Og.info()["dropped_full"] == 834
    assert same_nan_as_ref(frame_image(render_frame(rt, torch, W, Og, nx, ny, ns)[0], nx, ny), want)
    # the dropped spheres are invisible through the tree and visible in the list: the frames differ in many pixels
    f_list = frame_image(render_frame(rt, torch, W, None, nx, ny, ns)[0], nx, ny)
    assert ((f32_bits(f_list) != f32_bits(fast)).any(axis=2)).sum() > 100
    # binary16 (USE_FP16): same tree shape rules, bit-exact against the fp16 oracle
    Wh = rt.World(n, nx, ny, precision=rt.FP16)
    Oh = rt.Octree(Wh, spl)
    assert Oh.info()["dropped_full"] > 0
    Sh = OracleScene(n, nx, ny, fp16=True, use_octree=True, spl=spl)
    st = rt.alloc_rand_state(nx, ny)
    fb = rt.alloc_fb(nx, ny, precision=rt.FP16)
    rt.render_init(nx, ny, st)
    rt.render(fb, nx, ny, 2, Wh, st, Oh)
    torch.cuda.synchronize()
    got = fb.cpu().numpy().view(np.uint16).reshape(ny, nx, 3)
    wanth = Sh.render(2, nthreads=8)[0].astype(np.float16)
    nan = np.isnan(wanth)
    assert np.array_equal(got[~nan], wanth.view(np.uint16)[~nan]) and np.isnan(got.view(np.float16)[nan]).all()
