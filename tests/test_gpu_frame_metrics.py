"""rt_frame_levels and rt_frame_compare on the GPU against tests/frame_metrics_model.py: tiny frames, so that block
seams and frame edges dominate.  Integer fields and the SSIM map are exact; the two double sums are bounded by their summation order."""
import ctypes as C
import math

import numpy as np
import pytest

import frame_metrics_model as fm

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SENT = 0xA5


def awkward_frame(nx, ny, seed, dtype=np.float32):
    """uniform values with NaN, +-inf, -0.3, 1.7, 8e6, 1e10 and the level boundaries k/255.99 +- 1 ulp sprinkled in"""
    rng = np.random.default_rng(seed)
    fb = rng.uniform(0.0, 1.0, nx * ny * 3).astype(np.float32)
    k = rng.integers(0, 257, 3 * 80).astype(np.float64)
    edge = (k / 255.99).astype(np.float32)
    special = np.concatenate([np.array([np.nan, np.inf, -np.inf, -0.3, 1.7, 8e6, 1e10, -1e10, 0.0, -0.0, 1.0], np.float32),
                              edge[:80], np.nextafter(edge[80:160], np.float32(2)), np.nextafter(edge[160:], np.float32(-2))])
    at = rng.choice(fb.size, special.size, replace=False)
    fb[at] = special
    if dtype == np.float16:
        with np.errstate(over="ignore"):
            return fb.astype(np.float16)              # 8e6 and 1e10 become inf: still the same rule
    return fb


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_levels(rt, torch, d_fb, nx, ny, precision, fmt, top_first, input=0, samples=1, pad=64):
    n = rt.frame_levels_bytes(nx, ny, fmt)
    out = torch.full((n + pad,), SENT, dtype=torch.uint8, device="cuda")
    rt.frame_levels(out, d_fb, nx, ny, rt.LevelsParams(input, samples, fmt, top_first), precision)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n:] == SENT).all(), "wrote past rt_frame_levels_bytes"
    return got[:n]


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_levels_are_the_p6_bytes(rt, cuda, tmp_path, half):
    torch = cuda
    nx, ny = 37, 23
    fb = awkward_frame(nx, ny, 1, np.float16 if half else np.float32)
    prec = rt.FP16 if half else rt.FP32
    path = tmp_path / "f.ppm"
    rt.write_image(path, fb, nx, ny, prec, rt.IMAGE_P6)
    raw = open(path, "rb").read()
    body = np.frombuffer(raw[len(raw) - nx * ny * 3:], np.uint8)
    got = run_levels(rt, torch, dev(torch, fb), nx, ny, prec, rt.LEVELS_RGB8, 1)
    assert np.array_equal(got, body)
    assert np.array_equal(got, fm.frame_levels(fb, nx, ny, fm.RGB8, 1))
    assert {0, 255} <= set(got.tolist()) and len(set(got.tolist())) > 200


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_levels_other_formats(rt, cuda, half):
    torch = cuda
    nx, ny = 37, 23
    fb = awkward_frame(nx, ny, 2, np.float16 if half else np.float32)
    prec = rt.FP16 if half else rt.FP32
    d = dev(torch, fb)
    top = run_levels(rt, torch, d, nx, ny, prec, rt.LEVELS_RGB8, 1).reshape(ny, nx, 3)
    own = run_levels(rt, torch, d, nx, ny, prec, rt.LEVELS_RGB8, 0).reshape(ny, nx, 3)
    assert np.array_equal(own, top[::-1])
    for top_first, rgb in ((1, top), (0, own)):
        rgba = run_levels(rt, torch, d, nx, ny, prec, rt.LEVELS_RGBA8, top_first).reshape(ny, nx, 4)
        assert (rgba[..., 3] == 255).all() and np.array_equal(rgba[..., :3], rgb)
        g = run_levels(rt, torch, d, nx, ny, prec, rt.LEVELS_GRAY8, top_first)
        assert np.array_equal(g, fm.frame_levels(fb, nx, ny, fm.GRAY8, top_first))
        assert np.array_equal(g, fm.gray(rgb.astype(np.int64)).reshape(-1))


def test_levels_rgba_into_an_unaligned_buffer(rt, cuda):
    torch = cuda
    nx, ny = 37, 23
    fb = awkward_frame(nx, ny, 4)
    n = rt.frame_levels_bytes(nx, ny, rt.LEVELS_RGBA8)
    buf = torch.full((n + 9,), SENT, dtype=torch.uint8, device="cuda")
    rt.frame_levels(buf[1:], dev(torch, fb), nx, ny, rt.LevelsParams(0, 1, rt.LEVELS_RGBA8, 1))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert got[0] == SENT and (got[1 + n:] == SENT).all()
    assert np.array_equal(got[1:1 + n], fm.frame_levels(fb, nx, ny, fm.RGBA8, 1))


def test_levels_of_a_sum_frame(rt, cuda):
    torch = cuda
    nx, ny = 37, 23
    fb = awkward_frame(nx, ny, 3) * np.float32(7)
    with np.errstate(invalid="ignore", divide="ignore"):
        shown = np.sqrt(fb / np.float32(7))
    assert shown.dtype == np.float32
    for fmt in (rt.LEVELS_RGB8, rt.LEVELS_RGBA8, rt.LEVELS_GRAY8):
        got = run_levels(rt, torch, dev(torch, fb), nx, ny, rt.FP32, fmt, 1, rt.DENOISE_INPUT_SUM, 7)
        ref = run_levels(rt, torch, dev(torch, shown), nx, ny, rt.FP32, fmt, 1)
        assert np.array_equal(got, ref)
        assert np.array_equal(got, fm.frame_levels(fb, nx, ny, fmt, 1, fm.SUM, 7))


# ---- rt_frame_compare --------------------------------------------------------------------------------------------------------------
def frame_pair(nx, ny, seed, half_a=False):
    """random greys with step edges on block seams (columns / rows that are multiples of 8, 16, 32, 64), NaN and inf pixels; b is a
    noisy copy of a, so that S spreads over its range"""
    rng = np.random.default_rng(seed)
    seams = np.array([8, 16, 32, 64])
    col = 0.1 * (np.arange(nx)[:, None] >= seams).sum(axis=1)              # a vertical step edge at every seam column
    row = 0.07 * (np.arange(ny)[:, None] >= seams).sum(axis=1)             # and a horizontal one at every seam row
    a = (0.25 * rng.uniform(0.0, 1.0, (ny, nx, 3)) + col[None, :, None] + row[:, None, None]).astype(np.float32)
    b = (a + rng.normal(0, 0.05, a.shape).astype(np.float32)).astype(np.float32)
    if nx > 40:
        b[:, 32:40] = a[:, 32:40]                             # a strip of identical windows across a seam
    n = nx * ny
    bad = rng.choice(n, min(n, 6), replace=False) if n > 12 else np.array([], np.int64)
    af, bf = a.reshape(-1, 3), b.reshape(-1, 3)
    for t, p in enumerate(bad):
        (af if t & 1 else bf)[p, t % 3] = [np.nan, np.inf, -np.inf][t % 3]
    if half_a:
        a = a.astype(np.float16)
    return a.reshape(-1), b.reshape(-1)


def run_compare(rt, torch, a, b, nx, ny, want_map=True):
    """one call with sentinel-padded work and map buffers: (FrameMetrics, map or None)"""
    L = rt.lib()
    wb = L.rt_frame_compare_work_bytes(nx, ny)
    assert wb > 0 and wb % 8 == 0
    work = torch.full((wb + 64,), SENT, dtype=torch.uint8, device="cuda")
    wins = max(nx - 6, 0) * max(ny - 6, 0)
    smap = torch.full((wins + 8,), -7.0, dtype=torch.float64, device="cuda") if want_map else None
    pa = rt.FP16 if a.dtype == np.float16 else rt.FP32
    pb = rt.FP16 if b.dtype == np.float16 else rt.FP32
    m = rt.frame_compare(dev(torch, a), dev(torch, b), nx, ny, work, pa, pb, smap)
    assert (work.cpu().numpy()[wb:] == SENT).all(), "wrote past rt_frame_compare_work_bytes"
    if want_map:
        h = smap.cpu().numpy()
        assert (h[wins:] == -7.0).all(), "wrote past the SSIM map"
        return m, h[:wins]
    return m, None


def assert_matches_model(m, smap, ref):
    for f in ("pixels", "gray_sse", "gray_differ", "windows", "finite_pixels", "reserved"):
        assert getattr(m, f) == ref[f], f
    n = ref["windows"]
    if smap is not None:
        assert np.array_equal(smap.view(np.int64), ref["ssim_map"].reshape(-1).view(np.int64))
    print("ssim_sum", m.ssim_sum, ref["ssim_sum"], abs(m.ssim_sum - ref["ssim_sum"]), "bound", 2 * n * n * U)
    assert abs(m.ssim_sum - ref["ssim_sum"]) <= 2 * n * n * U
    nt = 3 * ref["finite_pixels"]
    print("sq_err", m.sq_err, ref["sq_err"], abs(m.sq_err - ref["sq_err"]), "bound", 2 * nt * U * ref["sq_err"])
    assert abs(m.sq_err - ref["sq_err"]) <= 2 * nt * U * ref["sq_err"]
    if n == 0:
        assert m.ssim_sum == 0.0 and math.isnan(m.ssim)


SHAPES = [(131, 67), (70, 45), (7, 7), (6, 20), (20, 6), (1, 1)]


@pytest.mark.parametrize("half_a", [False, True], ids=["fp32-fp32", "fp16-fp32"])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_compare_matches_the_model(rt, cuda, nx, ny, half_a):
    torch = cuda
    a, b = frame_pair(nx, ny, 100 + nx, half_a)
    ref = fm.compare(a, b, nx, ny)
    if nx * ny > 12:
        assert ref["finite_pixels"] < nx * ny and ref["gray_differ"] > 0          # the frame has what the test is about
    m, smap = run_compare(rt, torch, a, b, nx, ny)
    assert_matches_model(m, smap, ref)
    assert m.psnr == fm.psnr(ref) or abs(m.psnr - fm.psnr(ref)) <= 1e-12 * abs(fm.psnr(ref))
    if ref["finite_pixels"]:
        assert abs(m.rmse - fm.rmse(ref)) <= 1e-12 * fm.rmse(ref)
    m2, none = run_compare(rt, torch, a, b, nx, ny, want_map=False)                # without a map: the same record
    assert bytes(m2) == bytes(m) and none is None
    # the arguments swapped: the integer fields and the map's symmetric S are the same
    ms, smap_s = run_compare(rt, torch, b, a, nx, ny)
    assert (ms.gray_sse, ms.gray_differ, ms.finite_pixels) == (m.gray_sse, m.gray_differ, m.finite_pixels)


@pytest.mark.parametrize("nx,ny", [(131, 67), (7, 7), (20, 6)])
def test_identical_frames(rt, cuda, nx, ny):
    torch = cuda
    a, _ = frame_pair(nx, ny, 7)
    m, smap = run_compare(rt, torch, a, a.copy(), nx, ny)
    assert m.gray_sse == 0 and m.gray_differ == 0 and m.sq_err == 0.0
    assert m.ssim_sum == float(m.windows) and (smap == 1.0).all()
    assert m.psnr == math.inf and m.pixels == nx * ny and m.finite_pixels == nx * ny - 3          # the NaN and inf pixels of a, in both frames
    if m.windows:
        assert m.ssim == 1.0


def test_compare_is_deterministic(rt, cuda):
    torch = cuda
    nx, ny = 131, 67
    a, b = frame_pair(nx, ny, 9)
    m1, s1 = run_compare(rt, torch, a, b, nx, ny)
    m2, s2 = run_compare(rt, torch, a, b, nx, ny)
    assert bytes(m1) == bytes(m2) and np.array_equal(s1.view(np.int64), s2.view(np.int64))


def test_levels_and_compare_captured_in_a_graph(rt, cuda):
    torch = cuda
    nx, ny = 131, 67
    a, b = frame_pair(nx, ny, 13)
    da, db = dev(torch, a), dev(torch, b)
    p = rt.LevelsParams(0, 1, rt.LEVELS_RGBA8, 1)
    ref_lv = run_levels(rt, torch, da, nx, ny, rt.FP32, rt.LEVELS_RGBA8, 1)
    ref_m, ref_map = run_compare(rt, torch, a, b, nx, ny)
    lv = torch.zeros(rt.frame_levels_bytes(nx, ny, rt.LEVELS_RGBA8), dtype=torch.uint8, device="cuda")
    work = rt.alloc_compare_work(nx, ny)
    smap = torch.zeros((nx - 6) * (ny - 6), dtype=torch.float64, device="cuda")
    dm = torch.zeros(8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rt.frame_levels(lv, da, nx, ny, p)
        assert rt.frame_compare(da, db, nx, ny, work, d_ssim_map=smap, d_metrics=dm) is None
    lv.zero_(); smap.zero_(); dm.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(lv.cpu().numpy(), ref_lv)
    assert bytes(rt.frame_metrics(dm)) == bytes(ref_m)
    assert np.array_equal(smap.cpu().numpy().view(np.int64), ref_map.view(np.int64))


def test_bad_arguments_launch_nothing(rt, cuda):
    torch = cuda
    L = rt.lib()
    nx, ny = 20, 9
    a, b = frame_pair(nx, ny, 3)
    da, db = dev(torch, a), dev(torch, b)
    work = torch.full((L.rt_frame_compare_work_bytes(nx, ny) + 8,), SENT, dtype=torch.uint8, device="cuda")
    dm = torch.full((64,), SENT, dtype=torch.uint8, device="cuda")
    smap = torch.full(((nx - 6) * (ny - 6) + 1,), -7.0, dtype=torch.float64, device="cuda")
    out = torch.full((nx * ny * 4,), SENT, dtype=torch.uint8, device="cuda")
    A, B, M, W, S, O = (C.c_void_p(t.data_ptr()) for t in (da, db, dm, work, smap, out))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad = [L.rt_frame_compare(None, 0, B, 0, nx, ny, M, S, W, st), L.rt_frame_compare(A, 0, None, 0, nx, ny, M, S, W, st),
           L.rt_frame_compare(A, 0, B, 0, nx, ny, None, S, W, st), L.rt_frame_compare(A, 0, B, 0, nx, ny, M, S, None, st),
           L.rt_frame_compare(A, 0, B, 0, 0, ny, M, S, W, st), L.rt_frame_compare(A, 0, B, 0, nx, -1, M, S, W, st),
           L.rt_frame_compare(A, 2, B, 0, nx, ny, M, S, W, st), L.rt_frame_compare(A, 0, B, 7, nx, ny, M, S, W, st),
           L.rt_frame_compare(A, 0, B, 0, nx, ny, M, S, C.c_void_p(W.value + 4), st),
           L.rt_frame_compare(A, 0, B, 0, nx, ny, M, C.c_void_p(S.value + 4), W, st),
           L.rt_frame_compare(A, 0, B, 0, 1 << 16, 1 << 15, M, S, W, st)]
    assert bad == [-1] * len(bad)
    p = rt.LevelsParams(0, 1, rt.LEVELS_RGB8, 1)
    bad = [L.rt_frame_levels(None, A, nx, ny, 0, C.byref(p), st), L.rt_frame_levels(O, None, nx, ny, 0, C.byref(p), st),
           L.rt_frame_levels(O, A, nx, ny, 0, None, st), L.rt_frame_levels(O, A, nx, 0, 0, C.byref(p), st),
           L.rt_frame_levels(O, A, nx, ny, 3, C.byref(p), st), L.rt_frame_levels(O, A, nx, ny, 0, C.byref(rt.LevelsParams(2, 1, 0, 1)), st),
           L.rt_frame_levels(O, A, nx, ny, 0, C.byref(rt.LevelsParams(1, 0, 0, 1)), st),
           L.rt_frame_levels(O, A, nx, ny, 0, C.byref(rt.LevelsParams(0, 1, 3, 1)), st),
           L.rt_frame_levels(O, A, nx, ny, 0, C.byref(rt.LevelsParams(0, 1, 0, 2)), st)]
    assert bad == [-1] * len(bad)
    assert L.rt_frame_levels(O, A, nx, ny, 1, C.byref(rt.LevelsParams(1, 4, 0, 1)), st) == -4
    torch.cuda.synchronize()
    for t in (dm, work, out):
        assert (t.cpu().numpy() == SENT).all()
    assert (smap.cpu().numpy() == -7.0).all()


def test_a_rendered_pair(rt, cuda):
    """a 500-sphere world at 200x120, 4 spp against 64 spp: the device record rounds to the model's SSIM and PSNR of the downloaded frames"""
    torch = cuda
    nx, ny = 200, 120
    W = rt.World(500, nx, ny)
    O = rt.Octree(W, 30)
    frames = []
    for ns in (4, 64):
        st = rt.alloc_rand_state(nx, ny)
        fb = rt.alloc_fb(nx, ny)
        rt.render_init(nx, ny, st)
        rt.render(fb, nx, ny, ns, W, st, O)
        frames.append(fb)
    torch.cuda.synchronize()
    work = rt.alloc_compare_work(nx, ny)
    m = rt.frame_compare(frames[0], frames[1], nx, ny, work)
    ref = fm.compare(frames[0].cpu().numpy(), frames[1].cpu().numpy(), nx, ny)
    assert_matches_model(m, None, ref)
    print("ssim", m.ssim, fm.ssim(ref), "psnr", m.psnr, fm.psnr(ref), "rmse", m.rmse, fm.rmse(ref))
    assert 0.0 < m.ssim < 1.0 and 10.0 < m.psnr < 60.0
    assert round(m.ssim, 6) == round(fm.ssim(ref), 6)
    assert round(m.psnr, 3) == round(fm.psnr(ref), 3)
    assert abs(m.rmse - fm.rmse(ref)) <= 1e-12 * fm.rmse(ref)
    O.close()
    W.close()
