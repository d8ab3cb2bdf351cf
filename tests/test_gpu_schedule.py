"""Scheduling never changes a pixel, on every branch of the hand-out (-m gpu).

k_render hands pixels to lanes through the pilot pass, k_tile_order (tile order, thresholds, the tail mark), the sorted tail
(k_tail_hist / k_tail_scatter), the head of that tail handed out first — from its expensive or from its cheap end (RT_HEAD_SUM_*) —,
the pre-classified long and solo chains, the waves that go thin in flight and the slot interleave.  The one rule: every pixel is
rendered exactly once, by whichever lane, with the same bits.  Each knob setting below runs in a fresh child process
(tests/sched_worker.py; the library reads each knob once per process) that renders every scene of the matrix; the parent compares
each whole frame and each whole written-back RNG state with the CPU oracle bit for bit — a pixel skipped keeps its render_init state,
a pixel rendered twice has its state advanced twice — and proves from the launch's schedule words (rt_world_render_schedule) that
the branch the setting aims at actually ran.  The geometry edges run in-process with the default knobs; the last test pins the rule
that protects the tile order a captured progressive pass reads."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gpu_frames import render_frame
from oracle_lib import OracleScene
from sched_worker import SCENES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240


def tuning(name):
    """a default of csrc/rt_tuning.h"""
    src = open(os.path.join(ROOT, "dd2360-raytracing_amd", "csrc", "rt_tuning.h")).read()
    return float(re.search(r"#define %s ([-0-9.]+)f?\b" % name, src).group(1))


LONG_RATE_MIN = tuning("RT_LONG_RATE_MIN")              # the in-flight threshold's floor, per sample
PILOT_LONG_SUM_MIN = tuning("RT_PILOT_LONG_SUM_MIN")     # the pilot threshold's floor
PILOT_LONG_SUM = tuning("RT_PILOT_LONG_SUM")             # ... and the sum k_long_select uses when the threshold is off or above it
SPARSE = ("solo", "pooled", "part")
FP32 = SPARSE + ("dense",)


# ---- the oracle side ------------------------------------------------------------------------------------------------
def part_pixel_map(nx, ny, part, nparts, run=64):
    """local slot -> row-major pixel of the whole frame for runs of `run` tiles dealt round-robin (include/rt_amd.h), -1 outside"""
    tx_n, ty_n = (nx + 7) // 8, (ny + 7) // 8
    tiles = tx_n * ty_n
    glob = np.arange(tiles)
    local = glob[(glob // run) % nparts == part]                 # this part's tiles, in local order
    assert np.array_equal(np.sort(local), local)
    l = np.arange(64)
    i = (local % tx_n)[:, None] * 8 + (l & 7)[None, :]
    j = (local // tx_n)[:, None] * 8 + (l >> 3)[None, :]
    return np.where((i < nx) & (j < ny), j * nx + i, -1).reshape(-1)


def oracle_memo():
    """a getter of each scene's oracle frame (flattened to pixels x 3) and RNG state (pixels x 12, the order the GPU buffers use),
    each computed once"""
    memo = {}

    def get(name):
        if name not in memo:
            n, spl, nx, ny, ns, fp16, part, _ = SCENES[name]
            fb, st = OracleScene(n, nx, ny, fp16=fp16, use_octree=True, spl=spl).render(ns, nthreads=16)
            fb = fb.reshape(-1, 3)
            if fp16:
                fb = fb.astype(np.float16)
            if part is not None:
                m = part_pixel_map(nx, ny, part[0], part[1])
                fb = np.where((m >= 0)[:, None], fb[np.maximum(m, 0)], np.nan).astype(fb.dtype)
                st = np.where((m >= 0)[:, None], st[np.maximum(m, 0)], 0).astype(np.uint32)
            memo[name] = (fb, st, None if part is None else m >= 0)
        return memo[name]
    return get


@pytest.fixture(scope="module")
def oracle():
    return oracle_memo()


def same_bits(got, want, inside=None):
    """bit-equal, NaN pixels (the reference's dielectric produces them) equal to NaN pixels; `inside`: the slots that hold a pixel"""
    ui = np.uint16 if want.dtype == np.float16 else np.uint32
    inside = np.ones(len(want), bool) if inside is None else inside
    nan = np.isnan(want) & inside[:, None]
    keep = inside[:, None] & ~nan
    gotf = got.view(want.dtype)
    return np.array_equal(got[keep], want.view(ui)[keep]) and bool(np.isnan(gotf[nan]).all())


def check_against_oracle(oracle, name, d):
    fb, st, inside = oracle(name)
    got_fb, got_st = d[name + "_fb"], d[name + "_st"]
    assert got_fb.shape == fb.shape and got_st.shape == st.shape
    bad = ~(got_fb == fb.view(got_fb.dtype)).all(axis=1) & ~np.isnan(fb).any(axis=1)
    if inside is not None:
        bad &= inside
    assert same_bits(got_fb, fb, inside), "%s: %d pixel(s) differ from the oracle, first slots %s" % (name, bad.sum(), np.flatnonzero(bad)[:8])
    rows = np.ones(len(st), bool) if inside is None else inside
    # (the kernel writes back the xorwow words d, v[0..4]; a skipped pixel keeps render_init's, a pixel rendered twice is advanced twice)
    st_bad = ~(got_st[rows, :6] == st[rows, :6]).all(axis=1)
    assert not st_bad.any(), "%s: the RNG state of %d pixel(s) differs from the oracle's" % (name, st_bad.sum())


# ---- the settings: knobs, and what the schedule words must show -------------------------------------------------------
def n_tiles(name):
    n, spl, nx, ny, ns, fp16, part, _ = SCENES[name]
    tiles = ((nx + 7) // 8) * ((ny + 7) // 8)
    if part is None:
        return tiles
    runs = -(-tiles // 64)
    return sum(min(64, tiles - r * 64) for r in range(runs) if r % part[1] == part[0])


def tail_tiles(s, name):
    """(first tile of the tail, tiles in it) of a launch with a tail"""
    n = n_tiles(name)
    r0 = (s["tail_mark"] - 1) // 64
    return r0, n - r0


def expect_common(name, s, c):
    """what every launch shows, whatever the knobs"""
    n = n_tiles(name)
    assert n % 64 and n % 16, (name, n)                          # the scenes are chosen so: ragged last blocks
    assert c["thin_waves"] == 0, (name, c)                        # every wave that went thin was counted back
    assert c["long_chains"] == s["long_raw"] + s["solo_raw"], (name, c, s)
    raw = s["long_raw"] + s["solo_raw"]
    if raw == 0 or raw * 64 > n * 64:                             # k_render's use_long gate: chains are honoured while <= 1/64 of the slots
        assert c["long_handles"] == 0, (name, c, s)
    else:
        assert c["long_handles"] >= raw, (name, c, s)             # every listed chain was taken (handles past the end find the list empty)
    if SCENES[name][5]:                                           # binary16: no thresholds, no tail (rt_amd.h)
        assert [s[k] for k in ("inflight_thr", "static_thr", "tail_mark", "head", "head_thr", "from_end", "solo_raw")] == [0] * 7, (name, s)
        return
    if name != "solo":
        assert s["solo_raw"] == 0, (name, s)                      # only k_render<true,*,5> lists solo chains
    if s["tail_mark"]:
        r0, nt = tail_tiles(s, name)
        assert r0 % 64 == 0 and 0 < nt <= n, (name, s)            # the tail starts on a multiple of 64 tiles (the interleave divides it)
        assert s["head"] <= nt * 64 and s["from_end"] in (0, 1), (name, s)
        if s["from_end"]:
            assert s["head_thr"] > 0, (name, s)
    else:
        assert s["head"] == 0 and s["head_thr"] == 0 and s["from_end"] == 0, (name, s)


def head_first(thr, from_end, nonempty=True):
    def check(name, s, c):
        assert s["tail_mark"] > 0 and s["head_thr"] == thr and s["from_end"] == from_end, (name, s)
        if nonempty:
            assert s["head"] > 0, (name, s)
    return check


def tail_at_end(name, s, c):
    assert s["tail_mark"] > 0 and s["head_thr"] == 0 and s["head"] == 0 and s["from_end"] == 0, (name, s)


def defaults(name, s, c):
    assert s["inflight_thr"] > 0 and s["static_thr"] > 0, (name, s)
    if name == "dense":                                           # below RT_HEAD_LOAD_DENSE iterations per lane: the whole tail at the end
        tail_at_end(name, s, c)
    else:                                                         # sparse grids: the sorted tail first (RT_HEAD_SUM_SPARSE 1)
        head_first(1, 0)(name, s, c)


def no_tail(name, s, c):
    assert s["tail_mark"] == 0 and s["head"] == 0, (name, s)


def whole_tail(name, s, c):
    assert s["tail_mark"] == 1, (name, s)                         # the tail starts at tile 0: no tile slots at all
    if name != "dense":
        assert s["head_thr"] == 1 and s["head"] > 0, (name, s)


def smallest_tail(name, s, c):
    r0, nt = tail_tiles(s, name)
    assert s["tail_mark"] > 0 and r0 % 64 == 0 and 0 < nt < 128, (name, s)   # from the last 64-tile boundary to the ragged last tile
    assert nt % 64 == n_tiles(name) % 64, (name, s)


def gate(name, s, c, is_open):
    """k_render's use_long gate, proved from both sides: the raw count against 1/64 of the slots, and the handles taken"""
    raw = s["long_raw"] + s["solo_raw"]
    if is_open:
        assert 0 < raw <= n_tiles(name) and c["long_handles"] >= raw, (name, s, c)
    else:
        assert raw > n_tiles(name) and c["long_handles"] == 0, (name, s, c)


def static_floor(name, s, c):
    assert s["static_thr"] == PILOT_LONG_SUM_MIN, (name, s)
    if name in ("pooled", "part"):                                # at the floor these list more chains than 1/64 of the slots: use_long off
        gate(name, s, c, False)


def thresholds_off(name, s, c):
    assert s["inflight_thr"] == 0 and s["static_thr"] == 0, (name, s)
    if name in SPARSE:                                            # the pilot's fixed RT_PILOT_LONG_SUM: few chains, all honoured
        gate(name, s, c, True)


def thresholds_high(name, s, c):
    assert s["inflight_thr"] > LONG_RATE_MIN * SCENES[name][4] and s["static_thr"] > PILOT_LONG_SUM, (name, s)
    if name in SPARSE:                                            # (k_long_select then uses RT_PILOT_LONG_SUM itself)
        gate(name, s, c, True)


def inflight_floor(name, s, c):
    assert s["inflight_thr"] == LONG_RATE_MIN * SCENES[name][4], (name, s)   # waves go thin for any chain past the floor


def by_grid(sparse, dense):
    return lambda name, s, c: (dense if name == "dense" else sparse)(name, s, c)


# (id, environment, check of every fp32 scene's schedule words)
SETTINGS = [
    ("defaults", {}, defaults),
    ("f_tail_0", {"RT_F_TAIL": "0"}, no_tail),
    ("f_tail_1", {"RT_F_TAIL": "1"}, whole_tail),
    ("f_tail_smallest", {"RT_F_TAIL": "0.000001"}, smallest_tail),
    ("sparse_tail_at_end__dense_sky_first", {"RT_HEAD_SUM_SPARSE": "0", "RT_HEAD_LOAD_DENSE": "0", "RT_HEAD_SUM_DENSE": "-21"},
     by_grid(tail_at_end, head_first(22, 1))),
    ("sparse_sky_first__dense_whole_tail_first", {"RT_HEAD_SUM_SPARSE": "-21", "RT_HEAD_LOAD_DENSE": "0", "RT_HEAD_SUM_DENSE": "1"},
     by_grid(head_first(22, 1), head_first(1, 0))),
    ("sparse_near_empty_head__dense_cheap_end", {"RT_HEAD_SUM_SPARSE": "255", "RT_HEAD_LOAD_DENSE": "0", "RT_HEAD_SUM_DENSE": "-254"},
     by_grid(head_first(255, 0, nonempty=False), head_first(255, 1))),
    ("f_static_floor", {"RT_F_STATIC": "0.000001"}, static_floor),
    ("thresholds_off", {"RT_F_STATIC": "0", "RT_F_INFLIGHT": "0", "RT_F_INFLIGHT_DENSE": "0"}, thresholds_off),
    ("thresholds_high", {"RT_F_STATIC": "1000", "RT_F_INFLIGHT": "1000", "RT_F_INFLIGHT_DENSE": "1000"}, thresholds_high),
    ("f_inflight_floor", {"RT_F_INFLIGHT": "0.000001", "RT_F_INFLIGHT_DENSE": "0.000001"}, inflight_floor),
]
KNOBS = ("RT_F_TAIL", "RT_HEAD_SUM_SPARSE", "RT_HEAD_SUM_DENSE", "RT_HEAD_LOAD_DENSE", "RT_F_INFLIGHT", "RT_F_INFLIGHT_DENSE", "RT_F_STATIC")
_stopped = []          # the first child that ended by a signal or a timeout: the rest are not started


def run_child(tmp_path, env_knobs):
    if _stopped:
        pytest.fail("not started: an earlier child ended abnormally (%s)" % _stopped[0])
    env = dict(os.environ)
    for k in KNOBS:
        env.pop(k, None)
    env.update(env_knobs)
    out = str(tmp_path / "sched.npz")
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "sched_worker.py"), out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    try:
        o, e = p.communicate(timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        p.kill()
        o, e = p.communicate()
        _stopped.append("timeout with %s" % env_knobs)
        pytest.fail("child with %s timed out after %d s: %s" % (env_knobs, CHILD_TIMEOUT, e.decode()[-3000:]))
    if p.returncode < 0:
        _stopped.append("signal %d with %s" % (-p.returncode, env_knobs))
        pytest.fail("child with %s ended by signal %d: %s" % (env_knobs, -p.returncode, e.decode()[-3000:]))
    assert p.returncode == 0, (env_knobs, p.returncode, o.decode()[-2000:], e.decode()[-3000:])
    return dict(np.load(out))


@pytest.mark.parametrize("setting", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_every_knob_setting_renders_the_oracle_frame(rt, cuda, oracle, tmp_path, setting):
    _, knobs, expect = setting
    d = run_child(tmp_path, knobs)
    for name in SCENES:
        assert str(d[name + "_kernel"]) == SCENES[name][7], (name, str(d[name + "_kernel"]))
        s = dict(zip(rt.SCHEDULE_FIELDS, (int(v) for v in d[name + "_sched"])))
        c = dict(zip(("slots", "thin_waves", "long_chains", "long_handles"), (int(v) for v in d[name + "_cnt"])))
        expect_common(name, s, c)
        if name in FP32:
            expect(name, s, c)
        check_against_oracle(oracle, name, d)


# ---- geometry edges, default knobs, in this process -----------------------------------------------------------------
@pytest.mark.parametrize("n,spl", [(500, 30), (10000, 32)])
@pytest.mark.parametrize("nx,ny", [(7, 5), (8, 300), (300, 8)])
def test_frames_of_one_tile_row_or_column_equal_the_oracle(rt, cuda, n, spl, nx, ny):
    """a frame smaller than one tile, one tile column, one tile row — 16 spp: pilot pass, tail and long chains on"""
    torch = cuda
    W = rt.World(n, nx, ny)
    O = rt.Octree(W, spl)
    fb, st = render_frame(rt, torch, W, O, nx, ny, 16)
    s = W.render_schedule()
    assert s["tail_mark"] == 1 and s["head_thr"] == 1, s            # fewer than 64 tiles: the tail (handed out first) is the whole frame
    assert s["inflight_thr"] > 0 and s["static_thr"] > 0, s
    assert W.render_counters()["thin_waves"] == 0
    ref, ref_st = OracleScene(n, nx, ny, use_octree=True, spl=spl).render(16, nthreads=4)
    got = fb.cpu().numpy().reshape(-1, 3)
    assert same_bits(got.view(np.uint32), ref.reshape(-1, 3))
    assert np.array_equal(st.cpu().numpy().view(np.uint32).reshape(-1, 12)[:, :6], ref_st[:, :6])


def test_part_without_tiles_writes_nothing(rt, cuda):
    """more parts than tiles: the calls of a part without tiles return 0 and touch neither the buffers nor the last launch's words"""
    torch = cuda
    nx, ny, n = 7, 5, 500
    W = rt.World(n, nx, ny)
    O = rt.Octree(W, 30)
    render_frame(rt, torch, W, O, nx, ny, 16)
    before = (W.render_schedule(), W.render_counters())
    P = rt.Partition(1, 2)
    assert rt.part_pixels(nx, ny, P) == 0
    fb = torch.full((64 * 3,), 7.25, dtype=torch.float32, device="cuda")
    st = torch.full((64 * 48,), 0xA5, dtype=torch.uint8, device="cuda")
    L, stream = rt.lib(), rt._stream()
    assert L.rt_render_init(nx, ny, rt._dev(st), P, stream) == 0
    assert L.rt_render(rt._dev(fb), nx, ny, 16, W.h, rt._dev(st), O.h, P, stream) == 0
    assert L.rt_render_progressive(rt._dev(fb), nx, ny, 1, W.h, rt._dev(st), O.h, P, stream) == 0
    torch.cuda.synchronize()
    assert bool((fb == 7.25).all()) and bool((st == 0xA5).all())
    assert (W.render_schedule(), W.render_counters()) == before


# ---- the tile order a captured progressive pass reads ---------------------------------------------------------------
def test_captured_progressive_order_is_never_rewritten_for_another_frame(rt, cuda):
    """A progressive pass captured into a hipGraph reads the tile order the world's context keeps.  Uncaptured first passes of
    other frames on that context — another partition, a smaller frame, a larger frame — must not rewrite it: they are refused
    (RT_EINVAL), and the graph's replays still give the direct passes' bits.  A restart of the captured frame itself is accepted
    and keeps the replays bit-exact."""
    torch = cuda
    nx, ny, n, spl, passes = 400, 225, 500, 30, 5
    W = rt.World(n, nx, ny)
    O = rt.Octree(W, spl)
    L = rt.lib()

    st_a = rt.alloc_rand_state(nx, ny); fb_a = rt.alloc_fb(nx, ny)
    rt.render_init(nx, ny, st_a)
    for k in range(1, passes + 1):
        rt.render_progressive(fb_a, nx, ny, k, W, st_a, O)
    torch.cuda.synchronize()

    st = rt.alloc_rand_state(nx, ny); fb = rt.alloc_fb(nx, ny)
    rt.render_init(nx, ny, st)
    rt.render_progressive(fb, nx, ny, 1, W, st, O)
    rt.render_progressive(fb, nx, ny, 2, W, st, O)
    torch.cuda.synchronize()
    fb2, st2 = fb.clone(), st.clone()                               # the state the graph's passes start from
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rt.render_progressive(fb, nx, ny, 3, W, st, O)            # captured, not executed

    def first_pass(mx, my, part):
        s = rt.alloc_rand_state(mx, my, part); f = rt.alloc_fb(mx, my, part)
        rt.render_init(mx, my, s, part)
        return L.rt_render_progressive(rt._dev(f), mx, my, 1, W.h, rt._dev(s), O.h, part, rt._stream())

    rcs = {"part 0 of 2": first_pass(nx, ny, rt.Partition(0, 2)), "smaller frame": first_pass(200, 120, rt.WHOLE),
           "larger frame": first_pass(800, 450, rt.WHOLE)}
    torch.cuda.synchronize()
    for _ in range(3, passes + 1):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(fb.view(torch.int32), fb_a.view(torch.int32)) and torch.equal(st, st_a), "the replayed passes read a rewritten tile order (%s)" % rcs
    assert rcs == {k: -1 for k in rcs}, rcs                         # RT_EINVAL

    # a restart of the captured frame (same world, tree, size and part) recomputes an order of the same tiles
    assert first_pass(nx, ny, rt.WHOLE) == 0
    fb.copy_(fb2); st.copy_(st2)
    torch.cuda.synchronize()
    for _ in range(3, passes + 1):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(fb.view(torch.int32), fb_a.view(torch.int32)) and torch.equal(st, st_a)
