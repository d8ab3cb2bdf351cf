"""The kept schedule (csrc/rt_sched_keep.h) never changes what a launch computes, and is reused exactly when it may be (-m gpu).

A render context keeps the scheduling pass it ran last; a launch with the same key runs k_restore_counters and the render kernel
only.  The reference of every comparison is a child process started with RT_SCHED_CACHE=0 (tests/sched_cache_worker.py, run once
for the module): the frames, written-back RNG states, schedule words and long-chain counts of a library that runs the pass on every
call.  Frames and states are compared byte for byte.  The shapes are those of tests/sched_worker.py: ragged in tiles, above 64 tiles
(a tail exists), 16 spp (chains are classified)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sched_cache_worker as SW

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240


@pytest.fixture(scope="module")
def uncached(rt, cuda, tmp_path_factory):
    """every case of SW.CASES rendered by a process without the kept schedule"""
    out = str(tmp_path_factory.mktemp("sched_cache") / "uncached.npz")
    env = dict(os.environ, RT_SCHED_CACHE="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sched_cache_worker.py"), out], capture_output=True, env=env, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0, (p.returncode, p.stdout.decode()[-2000:], p.stderr.decode()[-3000:])
    return dict(np.load(out))


@pytest.fixture(scope="module")
def worlds(rt, cuda):
    made = {}

    def get(name):
        if name not in made:
            made[name] = SW.make_world(rt, name)
        return made[name]
    yield get
    for W, O in made.values():
        O.close()
        W.close()


def check(rt, torch, uncached, ctx, W, O, case, what):
    """render `case` on ctx and compare everything with the uncached child's"""
    fb, st, s, c = SW.render_case(rt, torch, ctx, W, O, case)
    got_fb, got_st = SW.bits(fb, st)
    assert got_fb.tobytes() == uncached[case + "_fb"].tobytes(), "%s (%s): the frame differs from the uncached render" % (case, what)
    assert got_st.tobytes() == uncached[case + "_st"].tobytes(), "%s (%s): the RNG states differ from the uncached render" % (case, what)
    assert s == uncached[case + "_sched"].tolist(), (case, what, s, uncached[case + "_sched"].tolist())
    assert c[2] == int(uncached[case + "_cnt"][2]) == s[6] + s[7], (case, what, c, uncached[case + "_cnt"].tolist())
    return got_fb, got_st


@pytest.mark.parametrize("name", ["solo", "pooled", "dense", "part", "h16"])
def test_repeated_frames_reuse_the_schedule_and_render_the_same_bits(rt, cuda, uncached, name):
    torch = cuda
    W, O = SW.make_world(rt, SW.CASES[name][0])          # a world of its own: its context starts without a record
    assert W.schedule_reuse() == (0, 0)
    first = None
    for call in range(3):
        got = check(rt, torch, uncached, None, W, O, name, "call %d" % (call + 1))
        assert W.schedule_reuse() == (call, 1), (name, call, W.schedule_reuse())
        if first is None:
            first = got
        else:
            assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes()
    if not SW.WORLDS[SW.CASES[name][0]][4]:              # (the tail's words exist on the fp32 tree paths: the shapes have a tail)
        assert uncached[name + "_sched"][2] > 0, uncached[name + "_sched"]
    O.close()
    W.close()


# the cases of the worker that change one thing about "pooled" ("part" is the pooled frame's part 1 of 3)
CHANGES = ["pooled_ns17", "pooled_part0", "part", "pooled_wider", "pooled_reference", "pooled_other_world", "pooled_larger"]


@pytest.mark.parametrize("change", CHANGES)
def test_a_changed_key_recomputes_the_schedule(rt, cuda, uncached, worlds, change):
    """each change alone makes the next call a miss, renders the uncached bits, and so does the first frame after it (a miss again:
    one record per context); with the key unchanged in between, calls are hits"""
    torch = cuda
    W, O = worlds("pooled")
    W2, O2 = worlds(SW.CASES[change][0])
    O.set_traversal(rt.TRAVERSAL_FAST)
    ctx = rt.RenderCtx()
    try:
        check(rt, torch, uncached, ctx, W, O, "pooled", "first")
        check(rt, torch, uncached, ctx, W, O, "pooled", "again")
        assert ctx.schedule_reuse() == (1, 1)
        if SW.CASES[change][5]:
            O2.set_traversal(rt.TRAVERSAL_REFERENCE)
        check(rt, torch, uncached, ctx, W2, O2, change, "changed")
        assert ctx.schedule_reuse() == (1, 2), (change, ctx.schedule_reuse())
        check(rt, torch, uncached, ctx, W2, O2, change, "changed, again")
        assert ctx.schedule_reuse() == (2, 2), (change, ctx.schedule_reuse())
        O2.set_traversal(rt.TRAVERSAL_FAST)
        check(rt, torch, uncached, ctx, W, O, "pooled", "back")
        assert ctx.schedule_reuse() == (2, 3), (change, ctx.schedule_reuse())
        check(rt, torch, uncached, ctx, W, O, "pooled", "back, again")
        assert ctx.schedule_reuse() == (3, 3), (change, ctx.schedule_reuse())
    finally:
        O.set_traversal(rt.TRAVERSAL_FAST)
        ctx.close()


def test_a_captured_pass_turns_the_reuse_off_for_its_context(rt, cuda, uncached, worlds):
    """rt_render captured on a context that holds a record: the graph holds the whole pass, its replays render the uncached bits, and
    the context never reuses again — the replays rewrite its workspace without the host knowing"""
    torch = cuda
    W, O = worlds("pooled")
    O.set_traversal(rt.TRAVERSAL_FAST)
    _, nx, ny, ns, _, _ = SW.CASES["pooled"]
    ctx = rt.RenderCtx()
    try:
        check(rt, torch, uncached, ctx, W, O, "pooled", "first")
        check(rt, torch, uncached, ctx, W, O, "pooled", "again")
        assert ctx.schedule_reuse() == (1, 1)
        st, fb = rt.alloc_rand_state(nx, ny), rt.alloc_fb(nx, ny)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ctx.render(fb, nx, ny, ns, W, st, O)             # captured, not executed
        assert ctx.schedule_reuse() == (1, 2)                 # the pass went into the graph
        for replay in range(2):
            rt.render_init(nx, ny, st)
            g.replay()
            torch.cuda.synchronize()
            got_fb, got_st = SW.bits(fb, st)
            assert got_fb.tobytes() == uncached["pooled_fb"].tobytes() and got_st.tobytes() == uncached["pooled_st"].tobytes(), "replay %d" % replay
        for call in range(3):                                  # the recorded key, uncaptured: a miss, now and ever after
            check(rt, torch, uncached, ctx, W, O, "pooled", "after the capture, call %d" % call)
            assert ctx.schedule_reuse() == (1, 3 + call), ctx.schedule_reuse()
        del g
    finally:
        ctx.close()


def test_adaptive_after_render_reuses_the_schedule(rt, cuda, worlds):
    """rt_render_adaptive with min_spp 16 after an rt_render of 16 spp of the same frame on one context: its first launch is a hit,
    and the frame, the sample counts and the RNG states equal those of a fresh context"""
    torch = cuda
    W, O = worlds("pooled")
    O.set_traversal(rt.TRAVERSAL_FAST)
    _, nx, ny, ns, _, _ = SW.CASES["pooled"]
    P = rt.Adaptive(**SW.ADAPTIVE)
    assert P.min_spp == ns

    def adaptive(ctx):
        st, fb = rt.alloc_rand_state(nx, ny), rt.alloc_fb(nx, ny)
        spp = torch.zeros(nx * ny, dtype=torch.int32, device="cuda")
        rt.render_init(nx, ny, st)
        ctx.render_adaptive(fb, nx, ny, P, W, st, O, spp)
        torch.cuda.synchronize()
        return SW.bits(fb, st) + (spp.cpu().numpy(),)

    fresh, used = rt.RenderCtx(), rt.RenderCtx()
    try:
        want = adaptive(fresh)
        assert fresh.schedule_reuse() == (0, 1)
        SW.render_case(rt, torch, used, W, O, "pooled")
        assert used.schedule_reuse() == (0, 1)
        got = adaptive(used)
        assert used.schedule_reuse() == (1, 1), used.schedule_reuse()
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and np.array_equal(got[2], want[2])
        assert want[2].min() >= P.min_spp and want[2].max() > P.min_spp          # some pixels did run on
    finally:
        fresh.close()
        used.close()
