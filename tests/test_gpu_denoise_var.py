"""GPU tests of rt_denoise_adaptive (-m gpu).  Every comparison is bit equality except the quality check: the kernels — the LDS form
of the steps 1 and 2 and the plain form of the larger steps — against the numpy float32 model of tests/denoise_var_model.py, fed with
the state and the frame read back from the GPU; against rt_denoise where the two rules coincide; along a refinement chain; in place,
on pass-through pixels, on tiny frames, in a captured graph; through the host program; and the RMSE against 1024 spp on C3."""
import os
import subprocess

import numpy as np
import pytest

import denoise_var_model
from bitcmp import f32_bits, same_any_nan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NY = 203, 77                   # ragged: neither a multiple of the 16x16 filter tile nor of the 8x8 render tile
N, SPL = 10000, 32
ADAPT = (4, 64, 4, 0.1, 0.02)      # (min_spp, max_spp, batch, rel_error, floor): pixels stop at many different counts


def gpu_guides(rt, torch, W, O, nx, ny):
    d = rt.alloc_guides(nx, ny)
    rt.render_guides(W, O, nx, ny, d)
    torch.cuda.synchronize()
    return d, d.cpu().numpy().view(rt.hit_record_dtype)


class Frame:
    """an adaptive frame with its state: begin(P), refine(P -> Q)"""

    def __init__(self, rt, torch, W, O, nx, ny, P):
        self.rt, self.torch, self.W, self.O, self.nx, self.ny = rt, torch, W, O, nx, ny
        self.fb = rt.alloc_fb(nx, ny)
        self.st = rt.alloc_rand_state(nx, ny)
        self.state = rt.alloc_adaptive_state(nx, ny)
        rt.render_init(nx, ny, self.st)
        rt.render_adaptive_begin(self.fb, nx, ny, rt.Adaptive(*P), W, self.st, self.state, O)
        torch.cuda.synchronize()

    def refine(self, frm, to):
        self.rt.render_adaptive_refine(self.fb, self.nx, self.ny, self.rt.Adaptive(*frm), self.rt.Adaptive(*to), self.W, self.st, self.state, self.O)
        self.torch.cuda.synchronize()
        return self

    def k(self):
        return denoise_var_model.state_parts(self.state.cpu().numpy(), self.nx * self.ny)[3]


def run(rt, torch, fb_in, d_hits, d_state, nx, ny, params, out=None):
    out = torch.full_like(fb_in, 7.0) if out is None else out
    work = rt.alloc_denoise_work(nx, ny)
    rt.denoise_adaptive(out, fb_in, nx, ny, d_hits, d_state, params, work)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def model(fb, hits, state, nx, ny, p):
    return denoise_var_model.denoise_adaptive(fb, hits, state, nx, ny, p.levels, p.normal_pow_log2, p.prefilter, p.sigma_position,
                                              p.sigma_variance)


def check_against_model(rt, torch, F, d_hits, hits, nx, ny, p):
    got = run(rt, torch, F.fb, d_hits, F.state, nx, ny, p)
    ref = model(F.fb.cpu().numpy(), hits, F.state.cpu().numpy(), nx, ny, p)
    assert np.array_equal(f32_bits(got), f32_bits(ref))
    return got


@pytest.fixture(scope="module")
def scene(rt, cuda):
    """the tree world at 203x77: an adaptive frame whose pixels stopped at many different counts, its state and the guides"""
    torch = cuda
    denoise_var_model.self_check()                 # the model follows the rule before the kernels are held to the model
    W = rt.World(N, NX, NY)
    O = rt.Octree(W, SPL)
    F = Frame(rt, torch, W, O, NX, NY, ADAPT)
    d_hits, hits = gpu_guides(rt, torch, W, O, NX, NY)
    yield dict(W=W, O=O, F=F, d_hits=d_hits, hits=hits)
    O.close()
    W.close()


# ---- 1. kernel == model --------------------------------------------------------------------------------------------------------
CASES = [dict(levels=1), dict(levels=2), dict(levels=3), dict(levels=4), dict(levels=5), dict(levels=8),
         dict(normal_pow_log2=-1, levels=3), dict(sigma_position=0.0, levels=3), dict(sigma_variance=0.0, levels=3),
         dict(normal_pow_log2=-1, sigma_position=0.0, sigma_variance=0.0, levels=3), dict(normal_pow_log2=10, sigma_variance=8.0, levels=4)]


@pytest.mark.parametrize("kw", CASES, ids=[",".join("%s=%s" % kv for kv in c.items()) for c in CASES])
@pytest.mark.parametrize("prefilter", [0, 1])
def test_matches_the_model(rt, cuda, scene, prefilter, kw):
    torch = cuda
    k = scene["F"].k()
    assert len(np.unique(k)) >= 3, np.unique(k)                                    # the frame is not uniform
    p = rt.denoise_var_params(prefilter=prefilter, **kw)
    got = check_against_model(rt, torch, scene["F"], scene["d_hits"], scene["hits"], NX, NY, p)
    assert np.isfinite(got).all()
    assert not np.array_equal(got, scene["F"].fb.cpu().numpy())                    # the filter did something


# ---- 2. the list path and the dense grid ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["list", "dense"])
def test_matches_the_model_on_other_paths(rt, cuda, path):
    torch = cuda
    if path == "list":
        W, O = rt.World(N, NX, NY), None
    else:
        W = rt.World(100000, 3840, 2160)                                           # C5's world: the dense grid's pooled walk
        O = rt.Octree(W, 320)
        assert rt.render_kernel_name(W, O, 0) == "k_render<true,0,2>"
    F = Frame(rt, torch, W, O, NX, NY, ADAPT)
    assert len(np.unique(F.k())) >= 3
    d_hits, hits = gpu_guides(rt, torch, W, O, NX, NY)
    assert (hits["sphere"] >= 0).sum() > NX * NY // 2
    for p in (rt.denoise_var_params(), rt.denoise_var_params(levels=4, prefilter=0, sigma_variance=2.0)):
        got = check_against_model(rt, torch, F, d_hits, hits, NX, NY, p)
        assert np.isfinite(got).all()
    if O is not None:
        O.close()
    W.close()


# ---- 3. where the rules coincide, the new kernels give what the old ones give -----------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2, 3, 5])
def test_equals_rt_denoise_on_a_uniform_state(rt, cuda, scene, levels):
    torch = cuda
    W, O = scene["W"], scene["O"]
    F = Frame(rt, torch, W, O, NX, NY, (8, 8, 4, 0.0, 0.0))                        # rel_error 0: every pixel runs to max_spp
    k = F.k()
    assert (k == 8).all()
    n = NX * NY
    sums = F.state.view(torch.float32)[:3 * n].clone()                             # S_rgb, interleaved like a frame
    old = rt.denoise_params(rt.DENOISE_INPUT_SUM, 8, levels=levels, sigma_color=0.0)
    out = torch.zeros_like(sums)
    rt.denoise(out, sums, NX, NY, scene["d_hits"], old, rt.alloc_denoise_work(NX, NY))
    torch.cuda.synchronize()
    ref = out.cpu().numpy().reshape(-1, 3)
    new = rt.denoise_var_params(levels=levels, prefilter=0, sigma_variance=0.0, sigma_position=old.sigma_position,
                                normal_pow_log2=old.normal_pow_log2)
    got = run(rt, torch, F.fb, scene["d_hits"], F.state, NX, NY, new).reshape(-1, 3)
    filtered = scene["hits"]["sphere"] != -1
    assert np.isfinite(got[filtered]).all() and filtered.sum() > n // 2
    assert np.array_equal(f32_bits(got[filtered]), f32_bits(ref[filtered]))


# ---- 4. a refinement chain leaves the state of begin(to) -------------------------------------------------------------------------
def test_refined_state_filters_like_begin(rt, cuda, scene):
    torch = cuda
    W, O = scene["W"], scene["O"]
    frm, to = (4, 64, 4, 0.2, 0.02), (4, 128, 4, 0.05, 0.02)
    A = Frame(rt, torch, W, O, NX, NY, frm)
    p = rt.denoise_var_params(levels=3)
    first = run(rt, torch, A.fb, scene["d_hits"], A.state, NX, NY, p)
    A.refine(frm, to)
    B = Frame(rt, torch, W, O, NX, NY, to)
    a = run(rt, torch, A.fb, scene["d_hits"], A.state, NX, NY, p)
    b = run(rt, torch, B.fb, scene["d_hits"], B.state, NX, NY, p)
    assert np.array_equal(f32_bits(a), f32_bits(b))
    assert not np.array_equal(f32_bits(a), f32_bits(first))


# ---- 5. in place, pass-through, tiny frames, a graph ---------------------------------------------------------------------------------
def test_in_place(rt, cuda, scene):
    torch = cuda
    F = scene["F"]
    p = rt.denoise_var_params(levels=4)
    ref = run(rt, torch, F.fb, scene["d_hits"], F.state, NX, NY, p)
    buf = F.fb.clone()
    got = run(rt, torch, buf, scene["d_hits"], F.state, NX, NY, p, out=buf)
    assert np.array_equal(f32_bits(got), f32_bits(ref))


def test_pass_through_pixels(rt, cuda, scene):
    """the sky, injected NaN / Inf sums and an injected k = 1 keep the bits of fb_in, and no other pixel takes them as a tap"""
    torch = cuda
    F = scene["F"]
    n = NX * NY
    sky = scene["hits"]["sphere"] == -1
    assert sky.sum() > 100
    state = F.state.cpu().numpy().copy()
    S, SL, Q, k = denoise_var_model.state_parts(state, n)
    rng = np.random.default_rng(3)
    bad = rng.choice(np.flatnonzero(~sky), 50, replace=False)
    S[bad[:10], 0] = np.float32("nan")
    S[bad[10:20], 1] = np.float32("inf")
    S[bad[20:30], 2] = np.float32("-inf")
    Q[bad[30:35]] = np.float32("inf")                         # the variance is not finite
    SL[bad[35:40]] = np.float32(3e38)                         # SL * SL overflows: d = n*Q - inf, clamped to 0 — NOT pass-through
    k[bad[40:]] = 1
    keep = sky.copy()
    keep[bad[:35]] = True
    keep[bad[40:]] = True
    fb = F.fb.clone()
    host = fb.cpu().numpy().reshape(-1, 3)
    host[bad] = np.float32(0.123)                             # marks what must come through untouched
    fb.copy_(torch.from_numpy(host.reshape(-1)))
    d_state = torch.from_numpy(state).cuda()
    p = rt.denoise_var_params(levels=5)
    got = run(rt, torch, fb, scene["d_hits"], d_state, NX, NY, p)
    ref = model(host.reshape(-1), scene["hits"], state, NX, NY, p)
    assert np.array_equal(f32_bits(got), f32_bits(ref))
    g3 = got.reshape(-1, 3)
    assert np.array_equal(f32_bits(g3[keep]), f32_bits(host[keep]))                        # the exact input bits
    assert not np.array_equal(f32_bits(g3[bad[35:40]]), f32_bits(host[bad[35:40]]))        # filtered: its variance is 0, not missing
    assert np.isfinite(g3[~sky]).all()                                            # nothing leaked into a neighbour


@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 37), (41, 1), (17, 2)])
def test_tiny_frames(rt, cuda, nx, ny):
    torch = cuda
    W = rt.World(500, nx, ny)
    O = rt.Octree(W, 30)
    F = Frame(rt, torch, W, O, nx, ny, (4, 32, 4, 0.1, 0.02))
    d_hits, hits = gpu_guides(rt, torch, W, O, nx, ny)
    for p in (rt.denoise_var_params(levels=3), rt.denoise_var_params(levels=8, prefilter=0)):
        got = run(rt, torch, F.fb, d_hits, F.state, nx, ny, p)
        assert same_any_nan(got, model(F.fb.cpu().numpy(), hits, F.state.cpu().numpy(), nx, ny, p))
    O.close()
    W.close()


def test_captured_in_a_graph(rt, cuda, scene):
    torch = cuda
    F = scene["F"]
    p = rt.denoise_var_params(levels=5)
    ref = run(rt, torch, F.fb, scene["d_hits"], F.state, NX, NY, p)
    out = torch.zeros_like(F.fb)
    work = rt.alloc_denoise_work(NX, NY)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rt.denoise_adaptive(out, F.fb, NX, NY, scene["d_hits"], F.state, p, work)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(f32_bits(out.cpu().numpy()), f32_bits(ref))


# ---- 6. the host program -----------------------------------------------------------------------------------------------------------
def rt_main(tmp_path, *extra):
    exe = os.path.join(ROOT, "dd2360-raytracing_amd", "rt_main")
    args = ["3", "500", "64", "40", "32", "1", "30", "0.1", "0", "0"] + [str(a) for a in extra]
    for f in tmp_path.glob("output.ppm"):
        f.unlink()
    p = subprocess.run([exe] + args, cwd=tmp_path, capture_output=True, timeout=120)
    return p, (tmp_path / "output.ppm").read_bytes() if p.returncode == 0 else None


def test_rt_main_filters_with_the_variance(rt, cuda, tmp_path):
    torch = cuda
    p, got = rt_main(tmp_path, 0.1, 4, 4, 0.02, 3, 2.5)          # REL_ERROR, MIN_SPP, BATCH, FLOOR, DENOISE = 3, DENOISE_SIGMA_VARIANCE
    assert p.returncode == 0, p.stderr.decode()
    assert "Denoising: 3 levels" in p.stderr.decode() and "sigma_variance 2.5" in p.stderr.decode()
    W = rt.World(500, 64, 40)
    O = rt.Octree(W, 30)
    F = Frame(rt, torch, W, O, 64, 40, (4, 32, 4, 0.1, 0.02))
    d_hits, _ = gpu_guides(rt, torch, W, O, 64, 40)
    den = run(rt, torch, F.fb, d_hits, F.state, 64, 40, rt.denoise_var_params(levels=3, sigma_variance=2.5))
    assert got == rt.format_ppm(den, 64, 40)
    assert got != rt.format_ppm(F.fb.cpu().numpy(), 64, 40)
    O.close()
    W.close()


def test_rt_main_without_the_argument_is_unchanged(rt, cuda, tmp_path):
    p0, plain = rt_main(tmp_path, 0.1, 4, 4, 0.02, 3)
    assert p0.returncode == 0, p0.stderr.decode()
    p1, off = rt_main(tmp_path, 0.1, 4, 4, 0.02, 3, 0)
    assert p1.returncode == 0, p1.stderr.decode()
    assert off == plain
    lines = [[l for l in p.stderr.decode().splitlines() if not l.startswith("took ")] for p in (p0, p1)]
    assert lines[0] == lines[1]
    assert "sigma_variance" not in p1.stderr.decode()
    # the bytes of today: rt_render_adaptive + rt_denoise through the library
    torch = cuda
    W = rt.World(500, 64, 40)
    O = rt.Octree(W, 30)
    fb, st = rt.alloc_fb(64, 40), rt.alloc_rand_state(64, 40)
    rt.render_init(64, 40, st)
    rt.render_adaptive(fb, 64, 40, rt.Adaptive(4, 32, 4, 0.1, 0.02), W, st, O)
    d_hits, _ = gpu_guides(rt, torch, W, O, 64, 40)
    out = torch.zeros_like(fb)
    rt.denoise(out, fb, 64, 40, d_hits, rt.denoise_params(levels=3), rt.alloc_denoise_work(64, 40))
    torch.cuda.synchronize()
    assert plain == rt.format_ppm(out.cpu().numpy(), 64, 40)
    O.close()
    W.close()
    for tail in ((0, 4, 4, 0, 3, 2.0), (0.1, 4, 4, 0, 0, 2.0)):                   # without REL_ERROR, without DENOISE
        p, _ = rt_main(tmp_path, *tail)
        assert p.returncode != 0 and "DENOISE_SIGMA_VARIANCE" in p.stderr.decode(), tail


# ---- 7. quality ----------------------------------------------------------------------------------------------------------------
def test_filtered_frames_are_closer_to_1024spp(rt, cuda):
    """C3 (1200x800, N = 10 000, SPL 32), library defaults, uniform states of 16 and of 64 spp (rel_error 0, min_spp = max_spp):
    lower RMSE against rt_render(1024) over the finite pixels at both counts, and the same number of non-finite pixels in and out.

    The bound is the plain inequality at both counts; measured on one MI355X: 0.01828 against 0.03125 and 0.01072 against 0.01504."""
    torch = cuda
    nx, ny = 1200, 800
    W = rt.World(N, nx, ny)
    O = rt.Octree(W, SPL)
    st = rt.alloc_rand_state(nx, ny)
    fb = rt.alloc_fb(nx, ny)
    rt.render_init(nx, ny, st)
    rt.render(fb, nx, ny, 1024, W, st, O)
    torch.cuda.synchronize()
    ref = fb.cpu().numpy().reshape(-1, 3).astype(np.float64)
    d_hits, _ = gpu_guides(rt, torch, W, O, nx, ny)
    results = {}
    for spp in (16, 64):
        F = Frame(rt, torch, W, O, nx, ny, (spp, spp, 4, 0.0, 0.0))
        assert (F.k() == spp).all()
        raw = F.fb.cpu().numpy().reshape(-1, 3).astype(np.float64)
        den = run(rt, torch, F.fb, d_hits, F.state, nx, ny, rt.denoise_var_params()).reshape(-1, 3).astype(np.float64)
        assert (~np.isfinite(den)).sum() == (~np.isfinite(raw)).sum()
        fin = np.isfinite(ref).all(1) & np.isfinite(raw).all(1) & np.isfinite(den).all(1)
        e_raw = float(np.sqrt(((raw[fin] - ref[fin]) ** 2).mean()))
        e_den = float(np.sqrt(((den[fin] - ref[fin]) ** 2).mean()))
        print("C3 %d spp: raw %.5f filtered %.5f" % (spp, e_raw, e_den))
        results[spp] = (e_den, e_raw)
    for spp, (e_den, e_raw) in results.items():
        assert e_den < e_raw, (spp, e_den, e_raw)
    O.close()
    W.close()
