"""rt_multi_render_adaptive on the one GPU of the test box (-m gpu): N ranks as N fresh child processes on GPU 0 through the
custom-gather form (tests/multi_worker.py adaptive; RCCL refuses two ranks on one device), one rank over RCCL, and the refusals.
Every comparison is bit equality with the single-process rt_render_adaptive."""
import ctypes as C
import re

import pytest

from rank_runner import run_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world,nx,ny,n,spl,lo,hi,step,rel", [
    (2, 203, 117, 10000, 32, 4, 32, 4, 0.1),     # ragged frame: 26 x 15 tiles, 7 runs — part 0 holds 4, part 1 holds 3 (the last of 6 tiles)
    (3, 203, 77, 500, 0, 16, 40, 8, 0.1),        # three ranks, hitable_list path, round 0 with the long-chain pass
    (8, 640, 200, 500, 30, 4, 24, 4, 0.1),       # 2000 tiles = 31.25 runs: 3 rounds of 8 runs and an incomplete fourth; 8 GPU processes
    (3, 64, 40, 500, 30, 4, 12, 4, 0.1),         # 40 tiles, less than one run: ranks 1 and 2 hold nothing and still make both gather calls
])
def test_multi_adaptive_child_processes_on_one_gpu(rt, cuda, world, nx, ny, n, spl, lo, hi, step, rel):
    out = run_ranks("adaptive", world, nx, ny, n, spl, lo, hi, step, rel, 0.02)
    m = re.search(r"frame and counts EQUAL the single-process frame \(counts \[(.*)\]\)", out)
    assert m, out
    assert len(m.group(1).split(",")) >= 2, m.group(1)          # a mixed frame: the count map says something


def noop_gather(user, d_send, send_bytes, d_parts, stride, root, stream):
    return 0


@pytest.fixture(scope="module")
def scene(rt, cuda):
    W = rt.World(500, 200, 120)
    O = rt.Octree(W, 30)
    yield W, O
    O.close()
    W.close()


def test_refusals(rt, cuda, scene):
    """balanced splits: RT_ENOTSUP; a root without fb_full, bad parameters: RT_EINVAL; a binary16 world: RT_ENOTSUP"""
    torch = cuda
    W, O = scene
    L = rt.lib()
    P = rt.Adaptive(4, 16, 4, 0.1, 0.02)
    M = rt.Multi(0, 1, gather=noop_gather)
    fb = torch.zeros(200 * 120 * 3, dtype=torch.float32, device="cuda")

    def go(fb_ptr, params=P, world=W, precision=rt.FP32):
        return L.rt_multi_render_adaptive(M.h, fb_ptr, 200, 120, C.byref(params), world.h, O.h if world is W else None, precision, 0, None, rt._stream())
    for mode in (rt.SPLIT_BALANCED, rt.SPLIT_BALANCED_CACHED):
        M.set_split(mode)
        assert go(rt._dev(fb)) == -4
    M.set_split(rt.SPLIT_RUNS)
    assert go(None) == -1                                                  # the root needs fb_full
    assert go(rt._dev(fb), params=rt.Adaptive(4, 18, 4, 0.1, 0.02)) == -1   # (max - min) % batch != 0
    w16 = rt.World(500, 200, 120, precision=rt.FP16)
    assert go(rt._dev(fb), world=w16, precision=rt.FP16) == -4
    w16.close()
    M.close()


def test_multi_adaptive_one_rank_over_rccl(rt, cuda, scene):
    """rt_multi_init with one rank (RCCL bound at run time, probed first): the frame and the map go straight into fb_full / d_spp_full"""
    torch = cuda
    W, O = scene
    nx, ny = 200, 120
    assert rt.multi_probe() == 0
    P = rt.Adaptive(4, 32, 4, 0.1, 0.02)
    M = rt.Multi(0, 1, unique_id=rt.multi_unique_id())
    full = torch.zeros(nx * ny * 3, dtype=torch.float32, device="cuda")
    spp = torch.full((nx * ny,), -1, dtype=torch.int32, device="cuda")
    M.render_adaptive(full, nx, ny, P, W, O, d_spp_full=spp)
    torch.cuda.synchronize()
    st = rt.alloc_rand_state(nx, ny)
    fb = rt.alloc_fb(nx, ny)
    want = torch.full((nx * ny,), -1, dtype=torch.int32, device="cuda")
    rt.render_init(nx, ny, st)
    rt.render_adaptive(fb, nx, ny, P, W, st, O, want)
    torch.cuda.synchronize()
    assert torch.equal(full.view(torch.int32), fb.view(torch.int32))
    assert torch.equal(spp, want)
    call_ms, kernel_ms = M.last_render_ms()
    assert 0 < kernel_ms <= call_ms
    M.close()
