"""bench.py --dump-outputs: what the timed path computed in its last step, as .npy files in float32 / float64 within 64 MiB, from
inputs fixed by the arguments; and a plain run (no --full) that does only the timed steps and the result line."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def coded(fb, bench):
    """the framebuffer as --dump-outputs writes it: float32, non-finite channels replaced by their negative codes"""
    a = np.asarray(fb).astype(np.float32)
    a[np.isnan(a)] = bench.DUMP_NAN
    a[a == np.inf] = bench.DUMP_POS_INF
    a[a == -np.inf] = bench.DUMP_NEG_INF
    return a


def test_dump_outputs_layout_and_budget(rt, tmp_path):
    """C3's frame is written whole, C5's as a seeded pixel sample; the RNG states always as a seeded sample; the sample is the
    same from call to call; every file is float32 or float64, every value finite (NaN / inf colour channels as negative codes,
    which no colour can be) and all of them together stay within the budget"""
    bench = _bench_module()
    nx, ny = 1200, 800
    fb = np.random.default_rng(3).uniform(0, 1, nx * ny * 3).astype(np.float32)
    fb[[5, 7, 1000]] = [np.nan, np.inf, -np.inf]                  # the reference's dielectric makes NaN pixels (material.h:95)
    st = np.zeros(nx * ny, rt.rand_state_dtype)
    st["d"] = np.arange(nx * ny, dtype=np.uint32) * 362437
    st["v"] = np.arange(nx * ny * 5, dtype=np.uint32).reshape(-1, 5) + 0xfffff000
    names = bench.dump_outputs(str(tmp_path / "c3"), fb, nx, ny, state=st)
    assert names == ["framebuffer", "rand_state", "rand_state_pixels"]
    got = {n: np.load(str(tmp_path / "c3" / (n + ".npy"))) for n in names}
    assert got["framebuffer"].dtype == np.float32 and got["framebuffer"].shape == (ny, nx, 3)
    assert all(np.isfinite(a).all() for a in got.values())
    assert got["framebuffer"].ravel()[[5, 7, 1000]].tolist() == [bench.DUMP_NAN, bench.DUMP_POS_INF, bench.DUMP_NEG_INF]
    assert np.array_equal(got["framebuffer"].ravel().view(np.uint32), coded(fb, bench).view(np.uint32))
    px = got["rand_state_pixels"].astype(np.int64)
    assert got["rand_state_pixels"].dtype == np.float64 and len(px) == bench.DUMP_STATE_PIXELS and np.all(np.diff(px) > 0)
    assert got["rand_state"].dtype == np.float64 and got["rand_state"].shape == (len(px), 6)
    assert np.array_equal(got["rand_state"][:, 0].astype(np.uint32), st["d"][px])
    assert np.array_equal(got["rand_state"][:, 1:].astype(np.uint32), st["v"][px])        # the uint32 words survive exactly
    assert np.array_equal(bench.sample_pixels(nx * ny, bench.DUMP_STATE_PIXELS), px)       # seeded: the same pixels every run
    # binary16 frame at C5's size: widened exactly, sampled
    nx, ny = 3840, 2160
    fb16 = np.random.default_rng(4).uniform(0, 1, nx * ny * 3).astype(np.float16)
    fb16[::997] = np.nan
    names = bench.dump_outputs(str(tmp_path / "c5"), fb16, nx, ny)
    assert names == ["framebuffer", "framebuffer_pixels"]
    img = np.load(str(tmp_path / "c5" / "framebuffer.npy"))
    px = np.load(str(tmp_path / "c5" / "framebuffer_pixels.npy")).astype(np.int64)
    assert img.dtype == np.float32 and img.shape == (bench.DUMP_FB_PIXELS, 3)
    assert np.isfinite(img).all() and (img == bench.DUMP_NAN).any()
    assert np.array_equal(img, coded(fb16.reshape(-1, 3)[px], bench))
    for case in ("c3", "c5"):
        assert sum(os.path.getsize(str(f)) for f in (tmp_path / case).iterdir()) <= bench.DUMP_BYTES_MAX


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_frame_it_timed(rt, cuda, tmp_path):
    """the default workload (C3) without --full: one result line with the headline fields, no counter passes, no CPU baseline;
    the dumped framebuffer (NaN channels coded) and RNG states are bit-equal to the same frame rendered here through the binding"""
    torch = cuda
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    d = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr.decode()[-3000:])
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f32" and line["value"] > 0
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert "cpu_baseline" not in line and "achieved" not in line["roofline_issue"] and line["roofline"]["traffic"] is None
    # the same frame here: C3, the scene of create_world seed 1984
    nx, ny, spp = 1200, 800, 64
    W = rt.World(10000, nx, ny).upload()
    O = rt.Octree(W, 32).upload()
    st = rt.alloc_rand_state(nx, ny)
    fb = rt.alloc_fb(nx, ny)
    rt.render_init(nx, ny, st)
    rt.render(fb, nx, ny, spp, W, st, O)
    torch.cuda.synchronize()
    img = np.load(str(d / "framebuffer.npy"))
    assert img.shape == (ny, nx, 3) and np.isfinite(img).all()
    assert np.array_equal(img.ravel().view(np.uint32), coded(fb.cpu().numpy(), _bench_module()).view(np.uint32))
    px = np.load(str(d / "rand_state_pixels.npy")).astype(np.int64)
    s = st.cpu().numpy().view(rt.rand_state_dtype)[px]
    want = np.concatenate([s["d"][:, None], s["v"]], axis=1).astype(np.float64)
    assert np.array_equal(np.load(str(d / "rand_state.npy")), want)
