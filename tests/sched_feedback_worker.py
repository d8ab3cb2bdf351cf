"""Child process of tests/test_gpu_sched_feedback.py: renders every case of CASES in a process the parent started with
RT_SCHED_FEEDBACK=0 (the library reads the switch once per process) — the frames, written-back RNG states, schedule words and
counters of a library that never records a pixel's iteration count and never rebuilds a kept pass: the pilot's pass on every call.

usage: sched_feedback_worker.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import material_edge_worlds as mw  # noqa: E402
from sched_worker import SCENES  # noqa: E402

NS = 32                     # RT_FEEDBACK_MIN_NS: the fewest samples per pixel at which a launch records and rebuilds
ROOM = ("white_room", 131, 99)      # tests/test_gpu_material_edges.py: 17 x 13 tiles, every pixel a chain of 50 bounces a sample
# a case: (world, nx, ny, ns, partition or None)
CASES = {
    "pooled": ("pooled", 400, 232, NS, None),              # 50 x 29 = 1450 tiles, k_render<true,0,4>
    "pooled_wider": ("pooled", 401, 232, NS, None),        # ragged: a column of tiles one pixel wide
    "pooled_part0": ("pooled", 400, 232, NS, (0, 3)),
    "pooled_part1": ("pooled", 400, 232, NS, (1, 3)),
    "pooled_part2": ("pooled", 400, 232, NS, (2, 3)),
    "pooled_ns33": ("pooled", 400, 232, NS + 1, None),
    "pooled_ns16": ("pooled", 400, 232, 16, None),         # below the gate
    "solo": ("solo", 603, 403, NS, None),                  # k_render<true,0,5>
    "tiny": ("pooled", 7, 5, NS, None),                    # one tile: fewer than 64, the tail is the frame
    "room": ("room", ROOM[1], ROOM[2], NS, None),          # the pilot lists more long pixels than 1/64 of the frame
    "dense": ("dense", 480, 270, NS, None),                # k_render<true,0,2>: never takes part
    "h16": ("h16", 403, 301, NS, None),                    # binary16: never takes part
}
NEVER = ("dense", "h16", "pooled_ns16")
SEQUENCE = ("pooled", 3)                                   # render_init once, then this many rt_render calls on the continuing states


def make_world(rt, name):
    if name == "room":
        sp, cam = mw.world(ROOM[0], ROOM[1], ROOM[2], None, rt=rt)
        W = mw.gpu_world(rt, sp, cam, ROOM[1], ROOM[2])
        return W, rt.Octree(W, 30)
    n, spl, nx, ny, _, fp16, _, _ = SCENES[name]
    W = rt.World(n, nx, ny, precision=rt.FP16 if fp16 else rt.FP32)
    return W, rt.Octree(W, spl)


def buffers(rt, W, case):
    _, nx, ny, ns, part = CASES[case]
    P = rt.Partition(*part) if part else rt.WHOLE
    return P, rt.alloc_rand_state(nx, ny, P), rt.alloc_fb(nx, ny, P, precision=W.precision)


def render_case(rt, torch, ctx, W, O, case, fb=None, st=None, init=True):
    """(render_init +) render of one case on ctx; returns (fb, st, schedule words, counters)"""
    _, nx, ny, ns, part = CASES[case]
    P = rt.Partition(*part) if part else rt.WHOLE
    if fb is None:
        P, st, fb = buffers(rt, W, case)
    if init:
        rt.render_init(nx, ny, st, P)
    ctx.render(fb, nx, ny, ns, W, st, O, P)
    torch.cuda.synchronize()
    s, c = ctx.schedule(), ctx.counters()
    return fb, st, [s[k] for k in rt.SCHEDULE_FIELDS], [c["slots"], c["thin_waves"], c["long_chains"], c["long_handles"]]


def bits(fb, st):
    return (fb.cpu().numpy().view(np.uint16 if fb.element_size() == 2 else np.uint32).reshape(-1, 3), st.cpu().numpy().view(np.uint32).reshape(-1, 12))


def main():
    import torch
    import rt_amd as rt
    assert os.environ.get("RT_SCHED_FEEDBACK") == "0"
    torch.cuda.set_device(0)
    out, worlds = {}, {}
    for case in CASES:
        wname = CASES[case][0]
        if wname not in worlds:
            worlds[wname] = make_world(rt, wname)
        W, O = worlds[wname]
        ctx = rt.RenderCtx()
        for call in range(2):                            # a miss, then a hit on the pilot's pass: the same bits and words
            fb, st, s, c = render_case(rt, torch, ctx, W, O, case)
            f = ctx.schedule_feedback()
            assert f["refined"] == 0 and f["has_counts"] == 0 and f["rebuilt"] == 0, (case, f)
            got = bits(fb, st)
            if call == 0:
                out[case + "_fb"], out[case + "_st"] = got
                out[case + "_sched"], out[case + "_cnt"] = np.array(s, np.int64), np.array(c, np.int64)
            else:
                assert got[0].tobytes() == out[case + "_fb"].tobytes() and got[1].tobytes() == out[case + "_st"].tobytes(), case
                assert s == out[case + "_sched"].tolist(), case
        assert ctx.schedule_reuse() == (1, 1), (case, ctx.schedule_reuse())
        ctx.close()
    case, steps = SEQUENCE
    W, O = worlds[CASES[case][0]]
    ctx = rt.RenderCtx()
    fb = st = None
    for k in range(steps):
        fb, st, s, c = render_case(rt, torch, ctx, W, O, case, fb, st, init=(k == 0))
        out["seq%d_fb" % k], out["seq%d_st" % k] = bits(fb, st)
    ctx.close()
    np.savez(sys.argv[1], **out)
    print("sched_feedback_worker: %d cases" % len(CASES), flush=True)


if __name__ == "__main__":
    main()
