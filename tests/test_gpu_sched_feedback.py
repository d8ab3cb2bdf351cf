"""The measured pass (csrc/rt_sched_keep.h "Feedback") never changes what a launch computes, and rebuilds a kept pass exactly when it
may (-m gpu).

The rt_render that computes a context's kept pass records every pixel's iteration count; the record's first hit rebuilds the pass from
those counts (k_count_cost, k_tile_order, k_count_select, the tail sort) and later hits reuse the rebuilt pass.  The reference of every
comparison is a child process started with RT_SCHED_FEEDBACK=0 (tests/sched_feedback_worker.py, run once for the module): the frames,
written-back RNG states and schedule words of a library that keeps the pilot's pass.  Frames and states are compared byte for byte.
The shapes: 32 spp (the gate RT_FEEDBACK_MIN_NS), frames above 64 tiles and ragged in tiles, a part, a one-tile frame (fewer than 64 tiles: no tile-ordered stretch, the tail is the frame), a
closed room whose long pixels outnumber 1/64 of the frame, and the two paths that never take part (a dense grid, binary16)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sched_feedback_worker as FW

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300
SOLO_FRAC, SOLO_CAP_DEN = np.float32(0.75), 32        # rt_tuning.h RT_FB_SOLO_FRAC, RT_FB_SOLO_CAP_DEN


@pytest.fixture(scope="module")
def pilot(rt, cuda, tmp_path_factory):
    """every case of FW.CASES rendered by a process that never rebuilds a pass"""
    out = str(tmp_path_factory.mktemp("sched_feedback") / "pilot.npz")
    env = dict(os.environ, RT_SCHED_FEEDBACK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sched_feedback_worker.py"), out], capture_output=True, env=env, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0, (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-3000:])
    return dict(np.load(out))


@pytest.fixture(scope="module")
def worlds(rt, cuda):
    made = {}

    def get(name):
        if name not in made:
            made[name] = FW.make_world(rt, name)
        return made[name]
    yield get
    for W, O in made.values():
        O.close()
        W.close()


def check(rt, torch, pilot, ctx, W, O, case, what, words=None):
    """render `case` on ctx: the bits are the child's; returns (schedule words, counters)"""
    fb, st, s, c = FW.render_case(rt, torch, ctx, W, O, case)
    got_fb, got_st = FW.bits(fb, st)
    assert got_fb.tobytes() == pilot[case + "_fb"].tobytes(), "%s (%s): the frame differs from the child's" % (case, what)
    assert got_st.tobytes() == pilot[case + "_st"].tobytes(), "%s (%s): the RNG states differ from the child's" % (case, what)
    if words == "pilot":
        assert s == pilot[case + "_sched"].tolist(), (case, what, s, pilot[case + "_sched"].tolist())
        assert c[2] == int(pilot[case + "_cnt"][2]), (case, what, c)
    return s, c


def elements(rt, case):
    _, nx, ny, _, part = FW.CASES[case]
    return rt.part_pixels(nx, ny, rt.Partition(*part) if part else rt.WHOLE)


def part_tiles(tiles, part, nparts):
    """the frame's tiles that belong to a part, in the order of its buffer (include/rt_amd.h: runs of 64 tiles dealt round-robin)"""
    t = np.arange(tiles)
    return t[(t // 64) % nparts == part]


def in_frame(rt, case):
    """which buffer elements of the case are pixels (a part's buffer pads its edge tiles)"""
    _, nx, ny, _, part = FW.CASES[case]
    if not part:
        return np.ones(nx * ny, bool)
    tiles_x, tiles_y = (nx + 7) // 8, (ny + 7) // 8
    tiles = part_tiles(tiles_x * tiles_y, *part)
    l = np.arange(64)
    i = (tiles % tiles_x)[:, None] * 8 + (l & 7)[None, :]
    j = (tiles // tiles_x)[:, None] * 8 + (l >> 3)[None, :]
    return ((i < nx) & (j < ny)).reshape(-1)


@pytest.mark.parametrize("case", ["pooled", "pooled_wider", "pooled_part1", "solo", "tiny", "room"])
def test_the_first_hit_rebuilds_the_pass_and_renders_the_same_bits(rt, cuda, pilot, worlds, case):
    torch = cuda
    W, O = worlds(FW.CASES[case][0])
    assert rt.render_kernel_name(W, O) in ("k_render<true,0,4>", "k_render<true,0,5>")
    ctx = rt.RenderCtx()
    try:
        assert ctx.schedule_feedback()["refined"] == 0
        s1, _ = check(rt, torch, pilot, ctx, W, O, case, "call 1: a miss, records", words="pilot")
        f = ctx.schedule_feedback()
        assert (f["refined"], f["has_counts"], f["rebuilt"]) == (0, 1, 0), f
        counts = ctx.schedule_counts(elements(rt, case))
        s2, c2 = check(rt, torch, pilot, ctx, W, O, case, "call 2: rebuilds")
        f = ctx.schedule_feedback()
        assert (f["refined"], f["has_counts"], f["rebuilt"]) == (1, 1, 1), f
        s3, c3 = check(rt, torch, pilot, ctx, W, O, case, "call 3: reuses the rebuilt pass")
        assert ctx.schedule_feedback()["refined"] == 1
        assert s3 == s2 and c3[2] == c2[2], (s2, s3, c2, c3)
        assert ctx.schedule_reuse() == (2, 1), ctx.schedule_reuse()
        # the counts are those of call 1, untouched by the launches that followed
        assert np.array_equal(ctx.schedule_counts(elements(rt, case)), counts)
        # the rebuilt selection is what the rule says: long = the count reaches the launch's in-flight threshold; of those, the ones
        # that reach RT_FB_SOLO_FRAC x the largest count start alone, at most (waves / RT_FB_SOLO_CAP_DEN) of them
        words = dict(zip(rt.SCHEDULE_FIELDS, s2))
        inside = in_frame(rt, case)
        assert counts.size == inside.size and not counts[~inside].any()
        assert f["max_count"] == int(counts.max()) and counts[inside].min() >= FW.NS          # every sample ends in at least one event
        thr = words["inflight_thr"]
        assert thr > 0
        long_px = inside & (counts >= thr)
        alone = long_px & (counts.astype(np.float32) >= SOLO_FRAC * np.float32(counts.max()))
        n_alone = min(int(alone.sum()), f["solo_cap"])
        print("%s: threshold %d, largest count %d, long %d, alone %d (cap %d), pilot's words %s" % (case, thr, counts.max(), long_px.sum(), n_alone, f["solo_cap"], s1))
        assert words["solo_raw"] == n_alone and words["long_raw"] == int(long_px.sum()) - n_alone, (words, int(long_px.sum()), n_alone)
        assert c2[2] == int(long_px.sum())                                                   # rt_render_ctx_counters: long_chains
        if case == "room":
            # the pilot lists every pixel (more than 1/64 of the frame: k_render sets such lists aside); measured, no chain exceeds 50
            # bounces a sample and few fall far below: the rule above, checked above, decides what is long among them
            assert (s1[6] + s1[7]) * 64 > inside.sum() and counts.max() <= 50 * FW.NS
        if case == "tiny":                                      # one tile: no tile-ordered stretch — as in the pilot's pass, the tail is the frame
            assert words["tail_mark"] == s1[2] == 1 and long_px.sum() == 0
    finally:
        ctx.close()


def test_the_counts_do_not_depend_on_the_schedule(rt, cuda, pilot, worlds):
    """a pixel's count is a function of the pixel: the whole frame's counts equal those of its three parts (other launches, other tile
    orders, other waves), gathered"""
    torch = cuda
    W, O = worlds("pooled")
    _, nx, ny, _, _ = FW.CASES["pooled"]
    ctx = rt.RenderCtx()
    try:
        check(rt, torch, pilot, ctx, W, O, "pooled", "whole")
        whole = ctx.schedule_counts(nx * ny).reshape(ny, nx)
        tiles_x = (nx + 7) // 8
        gathered = np.zeros((ny, nx), np.uint16)
        for p in range(3):
            case = "pooled_part%d" % p
            check(rt, torch, pilot, ctx, W, O, case, "part %d" % p)
            part = ctx.schedule_counts(elements(rt, case)).reshape(-1, 64)
            for local, tile in enumerate(part_tiles(tiles_x * ((ny + 7) // 8), p, 3)):
                x0, y0 = (tile % tiles_x) * 8, (tile // tiles_x) * 8
                blk = part[local].reshape(8, 8)[:max(0, min(8, ny - y0)), :max(0, min(8, nx - x0))]
                gathered[y0:y0 + blk.shape[0], x0:x0 + blk.shape[1]] = blk
        assert np.array_equal(gathered, whole)
    finally:
        ctx.close()


@pytest.mark.parametrize("case", FW.NEVER)
def test_launches_outside_the_gate_keep_the_pilots_pass(rt, cuda, pilot, worlds, case):
    """a dense grid, binary16, 16 samples per pixel: nothing is recorded, nothing rebuilt, and every call's words are the pilot's"""
    torch = cuda
    W, O = worlds(FW.CASES[case][0])
    ctx = rt.RenderCtx()
    try:
        for call in range(3):
            check(rt, torch, pilot, ctx, W, O, case, "call %d" % (call + 1), words="pilot")
            f = ctx.schedule_feedback()
            assert (f["refined"], f["has_counts"], f["rebuilt"]) == (0, 0, 0), (case, call, f)
            assert ctx.schedule_reuse() == (call, 1)
        assert rt.lib().rt_render_ctx_schedule_counts(ctx.h, np.zeros(4, np.uint16).ctypes.data, 4) == -1
    finally:
        ctx.close()


def test_a_continuing_sequence_renders_the_childs_bits(rt, cuda, pilot, worlds):
    """render_init once, then three rt_render calls on the continuing states (the counts of frame 1 are an estimate of frames 2 and 3)"""
    torch = cuda
    case, steps = FW.SEQUENCE
    W, O = worlds(FW.CASES[case][0])
    ctx = rt.RenderCtx()
    try:
        fb = st = None
        for k in range(steps):
            fb, st, _, _ = FW.render_case(rt, torch, ctx, W, O, case, fb, st, init=(k == 0))
            got_fb, got_st = FW.bits(fb, st)
            assert got_fb.tobytes() == pilot["seq%d_fb" % k].tobytes() and got_st.tobytes() == pilot["seq%d_st" % k].tobytes(), k
            assert ctx.schedule_feedback()["refined"] == min(k, 1)
        assert ctx.schedule_reuse() == (steps - 1, 1)
    finally:
        ctx.close()


@pytest.mark.parametrize("change", ["pooled_ns33", "pooled_part0", "pooled_wider"])
def test_a_changed_key_after_a_rebuild_misses_and_rebuilds_again(rt, cuda, pilot, worlds, change):
    torch = cuda
    W, O = worlds("pooled")
    ctx = rt.RenderCtx()
    try:
        check(rt, torch, pilot, ctx, W, O, "pooled", "first", words="pilot")
        check(rt, torch, pilot, ctx, W, O, "pooled", "rebuilds")
        assert ctx.schedule_feedback()["refined"] == 1 and ctx.schedule_reuse() == (1, 1)
        check(rt, torch, pilot, ctx, W, O, change, "changed: a miss", words="pilot")
        f = ctx.schedule_feedback()
        assert (f["refined"], f["has_counts"], f["rebuilt"]) == (1, 1, 0) and ctx.schedule_reuse() == (1, 2), (f, ctx.schedule_reuse())
        check(rt, torch, pilot, ctx, W, O, change, "changed, again: rebuilds")
        f = ctx.schedule_feedback()
        assert (f["refined"], f["rebuilt"]) == (2, 1) and ctx.schedule_reuse() == (2, 2), (f, ctx.schedule_reuse())
        check(rt, torch, pilot, ctx, W, O, "pooled", "back: a miss", words="pilot")
        assert ctx.schedule_feedback()["refined"] == 2 and ctx.schedule_reuse() == (2, 3)
    finally:
        ctx.close()


def test_a_capture_on_a_rebuilt_context_turns_the_record_off(rt, cuda, pilot, worlds):
    """as test_a_captured_pass_turns_the_reuse_off_for_its_context (tests/test_gpu_sched_cache.py), on a context whose pass was rebuilt:
    the graph holds the whole pilot pass, its replays render the child's bits, and the context neither reuses nor rebuilds again"""
    torch = cuda
    W, O = worlds("pooled")
    _, nx, ny, ns, _ = FW.CASES["pooled"]
    ctx = rt.RenderCtx()
    try:
        for call in range(3):
            check(rt, torch, pilot, ctx, W, O, "pooled", "call %d" % (call + 1))
        assert ctx.schedule_reuse() == (2, 1) and ctx.schedule_feedback()["refined"] == 1
        st, fb = rt.alloc_rand_state(nx, ny), rt.alloc_fb(nx, ny)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ctx.render(fb, nx, ny, ns, W, st, O)             # captured, not executed
        assert ctx.schedule_reuse() == (2, 2)
        f = ctx.schedule_feedback()
        assert (f["refined"], f["has_counts"], f["rebuilt"]) == (1, 0, 0), f
        for replay in range(2):
            rt.render_init(nx, ny, st)
            g.replay()
            torch.cuda.synchronize()
            got_fb, got_st = FW.bits(fb, st)
            assert got_fb.tobytes() == pilot["pooled_fb"].tobytes() and got_st.tobytes() == pilot["pooled_st"].tobytes(), "replay %d" % replay
        for call in range(3):
            check(rt, torch, pilot, ctx, W, O, "pooled", "after the capture, call %d" % call, words="pilot")
            f = ctx.schedule_feedback()
            assert ctx.schedule_reuse() == (2, 3 + call) and (f["refined"], f["has_counts"], f["rebuilt"]) == (1, 0, 0), (ctx.schedule_reuse(), f)
        del g
    finally:
        ctx.close()
