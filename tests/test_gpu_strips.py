"""The candidate strips (csrc/rt_accel.h) at their seams (-m gpu): rays built ON the structure's lattice — origins exactly on column
edges and fine-bin edges, directions along a column, at slope exactly +-1 (where the major axis flips), nearly flat and nearly
vertical, origins at sphere centres, on sphere surfaces, on the y-slab's faces — through the fast traversal, the library's own
reference scan and the oracle's hitTree / hitable_list::hit.  A walk that leaves out the column of a hit point, or a bin of a
centre, shows here as a missing or farther hit.  Random rays are the campaign's business (tools/campaign.py)."""
import numpy as np
import pytest

from bitcmp import f32_bits
from oracle_lib import OracleScene
from world_cases import lattice_rays

pytestmark = pytest.mark.gpu


def trace(rt, torch, W, O, rays):
    n = len(rays)
    d_rays = torch.from_numpy(rays).cuda()
    d_out = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    rt.trace_rays(W, O, d_rays, n, d_out)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(rt.hit_record_dtype)


@pytest.mark.parametrize("n,spl,frame", [(10000, 32, (1200, 800)), (500, 0, (1200, 800)), (100000, 320, (3840, 2160))])
def test_rays_on_the_strips_lattice(rt, cuda, n, spl, frame):
    torch = cuda
    nx, ny = frame
    W = rt.World(n, nx, ny)
    O = rt.Octree(W, spl) if spl else None
    info = O.accel_info() if O else W.list_accel_info()
    assert info["grid_dim"] > 0
    S = OracleScene(n, nx, ny, use_octree=bool(spl), spl=spl or 30)
    sp = W.spheres
    nrays = 120_000 if n <= 10000 else 40_000
    rays = lattice_rays(info, sp["center"].astype(np.float64), sp["radius"].astype(np.float64), nrays, 4242 + n)
    ref = S.trace(rays, mode=2 if spl else 1)
    outs = []
    for mode in (rt.TRAVERSAL_FAST, rt.TRAVERSAL_REFERENCE):
        if O: O.set_traversal(mode)
        else: W.set_list_traversal(mode)
        outs.append(trace(rt, torch, W, O, rays))
    assert ref["hit"].sum() > nrays // 10
    for got in outs:
        assert np.array_equal(got["sphere"], ref["sphere"])
        assert np.array_equal(f32_bits(got["t"]), f32_bits(ref["t"]))
        assert np.array_equal(f32_bits(got["p"]), f32_bits(ref["p"]))
        assert np.array_equal(f32_bits(got["normal"]), f32_bits(ref["normal"]))
