"""GPU tests of rt_render_guides and rt_denoise (-m gpu).  Every comparison is bit equality except the quality check:
the guides against rt_trace_rays on the same pixel-centre rays (built in numpy) and against the CPU oracle's trace, on the tree, list and
dense-grid paths; the filter against the numpy float32 model of tests/denoise_model.py."""
import os
import subprocess

import numpy as np
import pytest

import denoise_model
from bitcmp import f32_bits, same_any_nan
from oracle_lib import OracleScene
from tree_compare import traced

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY = 203, 77                   # ragged: neither a multiple of the 16x16 filter tile nor of the 8x8 render tile
N, SPL = 10000, 32


def gpu_guides(rt, torch, W, O, nx, ny):
    d = rt.alloc_guides(nx, ny)
    rt.render_guides(W, O, nx, ny, d)
    torch.cuda.synchronize()
    return d, d.cpu().numpy().view(rt.hit_record_dtype)


def assert_records_equal(got, ref):
    assert np.array_equal(got["sphere"], ref["sphere"])
    for f in ("t", "p", "normal"):
        assert np.array_equal(f32_bits(got[f]), f32_bits(ref[f])), f


def rendered(rt, torch, W, O, nx, ny, ns):
    st = rt.alloc_rand_state(nx, ny)
    fb = rt.alloc_fb(nx, ny)
    rt.render_init(nx, ny, st)
    rt.render(fb, nx, ny, ns, W, st, O)
    torch.cuda.synchronize()
    return fb


# ---- guides --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,path", [(NX, NY, "tree"), (1200, 800, "tree"), (NX, NY, "list_fast"), (NX, NY, "list_reference"),
                                        (NX, NY, "tree_reference")])
def test_guides_are_the_traced_centre_rays(rt, cuda, nx, ny, path):
    torch = cuda
    W = rt.World(N, nx, ny)
    O = rt.Octree(W, SPL) if path.startswith("tree") else None
    if path == "tree_reference":
        O.set_traversal(rt.TRAVERSAL_REFERENCE)
    elif O is None:
        W.set_list_traversal(rt.TRAVERSAL_REFERENCE if path == "list_reference" else rt.TRAVERSAL_FAST)
    if path == "tree":
        assert rt.render_kernel_name(W, O, 0) == "k_render<true,0,4>"             # the sparse grid's pooled walk
    _, got = gpu_guides(rt, torch, W, O, nx, ny)
    rays = denoise_model.guide_rays(W.camera[0], nx, ny)
    assert_records_equal(got, traced(rt, torch, W, O, rays))
    assert (got["sphere"] >= 0).sum() > nx * ny // 2 and (got["sphere"] == -1).sum() > 0
    if nx * ny <= NX * NY:                                                         # the CPU oracle need not trace full frames
        ref = OracleScene(N, nx, ny, use_octree=O is not None, spl=SPL).trace(rays, mode=2 if O is not None else 1)
        assert_records_equal(got, ref)


def test_guides_on_a_dense_grid(rt, cuda):
    """C5's world (100 000 spheres, SPHERES_PER_LEAF 320) takes the dense grid's pooled walk, as rt_render does"""
    torch = cuda
    W = rt.World(100000, 3840, 2160)
    O = rt.Octree(W, 320)
    assert rt.render_kernel_name(W, O, 0) == "k_render<true,0,2>"
    _, got = gpu_guides(rt, torch, W, O, NX, NY)
    rays = denoise_model.guide_rays(W.camera[0], NX, NY)
    assert_records_equal(got, traced(rt, torch, W, O, rays))
    assert_records_equal(got, OracleScene(100000, 3840, 2160, use_octree=True, spl=320).trace(rays, mode=2))
    assert (got["sphere"] >= 0).sum() > NX * NY // 2


@pytest.mark.parametrize("tree", [True, False])
def test_guides_of_a_contract_world_are_the_ieee_guides(rt, cuda, tree):
    torch = cuda
    W = rt.World(N, NX, NY)
    O = rt.Octree(W, SPL) if tree else None
    _, ieee = gpu_guides(rt, torch, W, O, NX, NY)
    W.set_arith(rt.ARITH_CONTRACT)
    _, fmac = gpu_guides(rt, torch, W, O, NX, NY)
    assert_records_equal(fmac, ieee)


# ---- the filter ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(rt, cuda):
    """the tree world at 203x77: rt_render(16), the sum of 8 progressive passes, and the guides"""
    torch = cuda
    denoise_model.self_check()                     # the model follows the rule before the kernels are held to the model
    W = rt.World(N, NX, NY)
    O = rt.Octree(W, SPL)
    fb16 = rendered(rt, torch, W, O, NX, NY, 16)
    st = rt.alloc_rand_state(NX, NY)
    acc = rt.alloc_fb(NX, NY)
    rt.render_init(NX, NY, st)
    for s in range(1, 9):
        rt.render_progressive(acc, NX, NY, s, W, st, O)
    d_hits, hits = gpu_guides(rt, torch, W, O, NX, NY)
    yield dict(W=W, O=O, gamma=fb16, sum=acc, d_hits=d_hits, hits=hits)
    O.close()
    W.close()


def run(rt, torch, fb_in, d_hits, nx, ny, params, out=None):
    out = torch.full_like(fb_in, 7.0) if out is None else out
    work = rt.alloc_denoise_work(nx, ny)
    rt.denoise(out, fb_in, nx, ny, d_hits, params, work)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def model(rt, fb, hits, nx, ny, p):
    return denoise_model.denoise(fb, hits, nx, ny, p.input, p.samples, p.levels, p.normal_pow_log2, p.sigma_position, p.sigma_color)


CASES = [dict(levels=1), dict(levels=2), dict(levels=3), dict(levels=4), dict(levels=5),
         dict(normal_pow_log2=-1), dict(sigma_position=0.0), dict(sigma_color=0.0),
         dict(normal_pow_log2=-1, sigma_position=0.0, sigma_color=0.0), dict(normal_pow_log2=10, levels=8)]


@pytest.mark.parametrize("kw", CASES, ids=[",".join("%s=%s" % kv for kv in c.items()) for c in CASES])
@pytest.mark.parametrize("mode", ["gamma", "sum"])
def test_denoise_matches_the_model(rt, cuda, scene, mode, kw):
    torch = cuda
    p = rt.denoise_params(rt.DENOISE_INPUT_SUM if mode == "sum" else rt.DENOISE_INPUT_GAMMA, 8, **kw)
    fb = scene[mode]
    got = run(rt, torch, fb, scene["d_hits"], NX, NY, p)
    ref = model(rt, fb.cpu().numpy(), scene["hits"], NX, NY, p)
    assert np.array_equal(f32_bits(got), f32_bits(ref))
    assert np.isfinite(got).all()
    if mode == "gamma":
        assert not np.array_equal(got, fb.cpu().numpy())                           # the filter did something


@pytest.mark.parametrize("mode", ["gamma", "sum"])
def test_denoise_in_place(rt, cuda, scene, mode):
    torch = cuda
    p = rt.denoise_params(rt.DENOISE_INPUT_SUM if mode == "sum" else rt.DENOISE_INPUT_GAMMA, 8, levels=4)
    ref = run(rt, torch, scene[mode], scene["d_hits"], NX, NY, p)
    buf = scene[mode].clone()
    got = run(rt, torch, buf, scene["d_hits"], NX, NY, p, out=buf)
    assert np.array_equal(f32_bits(got), f32_bits(ref))


@pytest.mark.parametrize("mode", ["gamma", "sum"])
def test_pass_through_pixels(rt, cuda, scene, mode):
    """injected NaN and Inf pixels and the sky keep their display value, and no other pixel takes them as a tap"""
    torch = cuda
    sky = scene["hits"]["sphere"] == -1
    assert sky.sum() > 100
    fb = scene[mode].clone()
    host = fb.cpu().numpy().reshape(-1, 3)
    rng = np.random.default_rng(3)
    hit_px = np.flatnonzero(~sky)
    bad = rng.choice(hit_px, 40, replace=False)
    host[bad[:10], 0] = np.float32("nan")
    host[bad[10:20], 1] = np.float32("inf")
    host[bad[20:30], 2] = np.float32("-inf")
    host[bad[30:], :] = np.float32(3e38)                      # finite, but GAMMA's c*c overflows: pass-through too
    fb.copy_(torch.from_numpy(host.reshape(-1)))
    p = rt.denoise_params(rt.DENOISE_INPUT_SUM if mode == "sum" else rt.DENOISE_INPUT_GAMMA, 8, levels=5)
    got = run(rt, torch, fb, scene["d_hits"], NX, NY, p)
    ref = model(rt, host.reshape(-1), scene["hits"], NX, NY, p)
    assert same_any_nan(got, ref)
    g3 = got.reshape(-1, 3)
    if mode == "gamma":
        keep = sky.copy()
        keep[bad] = True
        assert np.array_equal(f32_bits(g3[keep]), f32_bits(host[keep]))                    # the exact input bits
        assert np.array_equal(f32_bits(g3), f32_bits(ref.reshape(-1, 3)))
    else:
        assert same_any_nan(g3[sky], np.sqrt(host[sky] / np.float32(8)))
    fine = np.ones(NX * NY, bool)
    fine[bad] = False
    assert np.isfinite(g3[fine]).all()                                              # nothing leaked into a neighbour


@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 37), (41, 1), (17, 2)])
def test_tiny_frames(rt, cuda, nx, ny):
    torch = cuda
    W = rt.World(500, nx, ny)
    O = rt.Octree(W, 30)
    fb = rendered(rt, torch, W, O, nx, ny, 4)
    d_hits, hits = gpu_guides(rt, torch, W, O, nx, ny)
    rays = denoise_model.guide_rays(W.camera[0], nx, ny)
    assert_records_equal(hits, traced(rt, torch, W, O, rays))
    for p in (rt.denoise_params(levels=3), rt.denoise_params(rt.DENOISE_INPUT_SUM, 3, levels=8)):
        got = run(rt, torch, fb, d_hits, nx, ny, p)
        assert same_any_nan(got, model(rt, fb.cpu().numpy(), hits, nx, ny, p))
    O.close()
    W.close()


def test_denoise_captured_in_a_graph(rt, cuda, scene):
    torch = cuda
    p = rt.denoise_params(levels=5)
    ref = run(rt, torch, scene["gamma"], scene["d_hits"], NX, NY, p)
    out = torch.zeros_like(scene["gamma"])
    work = rt.alloc_denoise_work(NX, NY)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rt.denoise(out, scene["gamma"], NX, NY, scene["d_hits"], p, work)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(f32_bits(out.cpu().numpy()), f32_bits(ref))


def test_denoised_16spp_is_closer_to_1024spp(rt, cuda):
    """C3 (1200x800, N = 10 000, SPL 32) at 16 spp, default weights: lower RMSE against rt_render(1024) over the finite pixels, and
    the same number of non-finite pixels as the raw frame"""
    torch = cuda
    nx, ny = 1200, 800
    W = rt.World(N, nx, ny)
    O = rt.Octree(W, SPL)
    ref = rendered(rt, torch, W, O, nx, ny, 1024).cpu().numpy().reshape(-1, 3).astype(np.float64)
    fb = rendered(rt, torch, W, O, nx, ny, 16)
    raw = fb.cpu().numpy().reshape(-1, 3).astype(np.float64)
    d_hits, _ = gpu_guides(rt, torch, W, O, nx, ny)
    den = run(rt, torch, fb, d_hits, nx, ny, rt.denoise_params()).reshape(-1, 3).astype(np.float64)
    assert (~np.isfinite(den)).sum() == (~np.isfinite(raw)).sum()
    fin = np.isfinite(ref).all(1) & np.isfinite(raw).all(1) & np.isfinite(den).all(1)
    e_raw = float(np.sqrt(((raw[fin] - ref[fin]) ** 2).mean()))
    e_den = float(np.sqrt(((den[fin] - ref[fin]) ** 2).mean()))
    assert e_den < e_raw, (e_den, e_raw)
    O.close()
    W.close()


# ---- the host program ----------------------------------------------------------------------------------------------------------
def rt_main(tmp_path, *extra):
    exe = os.path.join(ROOT, "dd2360-raytracing_amd", "rt_main")
    args = ["3", "500", "64", "40", "8", "1", "30", "0.1", "0", "0"] + [str(a) for a in extra]
    for f in tmp_path.glob("output.ppm"):
        f.unlink()
    p = subprocess.run([exe] + args, cwd=tmp_path, capture_output=True, timeout=120)
    return p, (tmp_path / "output.ppm").read_bytes() if p.returncode == 0 else None


def test_rt_main_denoises(rt, cuda, tmp_path):
    torch = cuda
    p, got = rt_main(tmp_path, 0, 4, 4, 0, 5)                      # REL_ERROR 0 (off), MIN_SPP, BATCH, FLOOR, DENOISE = 5
    assert p.returncode == 0, p.stderr.decode()
    assert "Denoising: 5 levels" in p.stderr.decode()
    W = rt.World(500, 64, 40)
    O = rt.Octree(W, 30)
    fb = rendered(rt, torch, W, O, 64, 40, 8)
    d_hits, _ = gpu_guides(rt, torch, W, O, 64, 40)
    den = run(rt, torch, fb, d_hits, 64, 40, rt.denoise_params(levels=5))
    assert got == rt.format_ppm(den, 64, 40)
    assert got != rt.format_ppm(fb.cpu().numpy(), 64, 40)
    O.close()
    W.close()


def test_rt_main_without_denoise_is_unchanged(rt, cuda, tmp_path):
    p0, plain = rt_main(tmp_path)
    assert p0.returncode == 0, p0.stderr.decode()
    p1, off = rt_main(tmp_path, 0, 4, 4, 0, 0)
    assert p1.returncode == 0, p1.stderr.decode()
    assert off == plain
    assert "Denoising" not in p1.stderr.decode()
    exe = os.path.join(ROOT, "dd2360-raytracing_amd", "rt_main")
    p = subprocess.run([exe, "1", "500", "64", "40", "8", "1", "30", "0.1", "1", "0", "0", "4", "4", "0", "5"], cwd=tmp_path,
                       capture_output=True, timeout=120)
    assert p.returncode != 0 and "DENOISE" in p.stderr.decode()
