"""Child process of tests/test_gpu_sched_cache.py: renders every case of CASES once, each on a fresh render context, in a process
the parent started with RT_SCHED_CACHE=0 (the library reads the switch once per process) — the frames, written-back RNG states,
schedule words and counters that a library without the kept schedule computes.

usage: sched_cache_worker.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sched_worker import SCENES  # noqa: E402

# a world: (spheres, octree SPL, the frame its camera was made for, binary16)
WORLDS = {name: (n, spl, nx, ny, fp16) for name, (n, spl, nx, ny, ns, fp16, part, kernel) in SCENES.items() if name != "part"}
WORLDS["small"] = (500, 30, 400, 232, False)          # another world for the pooled frame
# a case: (world, nx, ny, ns, partition or None, reference traversal).  The five frames of the scheduling matrix, then the pooled
# frame with one thing changed at a time.
CASES = {name: ("pooled" if name == "part" else name, nx, ny, ns, part, False) for name, (n, spl, nx, ny, ns, fp16, part, kernel) in SCENES.items()}
CASES.update({
    "pooled_ns17": ("pooled", 400, 232, 17, None, False),
    "pooled_part0": ("pooled", 400, 232, 16, (0, 3), False),
    "pooled_wider": ("pooled", 401, 232, 16, None, False),
    "pooled_reference": ("pooled", 400, 232, 16, None, True),
    "pooled_other_world": ("small", 400, 232, 16, None, False),
    "pooled_larger": ("pooled", 603, 403, 16, None, False),           # 3876 tiles against 1450: the workspace regrows
})
ADAPTIVE = dict(min_spp=16, max_spp=32, batch=8, rel_error=0.05, floor=0.01)


def make_world(rt, name):
    n, spl, nx, ny, fp16 = WORLDS[name]
    W = rt.World(n, nx, ny, precision=rt.FP16 if fp16 else rt.FP32)
    return W, rt.Octree(W, spl)


def render_case(rt, torch, ctx, W, O, case, fb=None, st=None):
    """render_init + render of one case on `ctx` (None: the world's own context); returns (fb, st, schedule words, counters)"""
    _, nx, ny, ns, part, _ = CASES[case]
    P = rt.Partition(*part) if part else rt.WHOLE
    st = rt.alloc_rand_state(nx, ny, P) if st is None else st
    fb = rt.alloc_fb(nx, ny, P, precision=W.precision) if fb is None else fb
    rt.render_init(nx, ny, st, P)
    if ctx is None:
        rt.render(fb, nx, ny, ns, W, st, O, P)
    else:
        ctx.render(fb, nx, ny, ns, W, st, O, P)
    torch.cuda.synchronize()
    s = W.render_schedule() if ctx is None else ctx.schedule()
    c = W.render_counters() if ctx is None else ctx.counters()
    return fb, st, [s[k] for k in rt.SCHEDULE_FIELDS], [c["slots"], c["thin_waves"], c["long_chains"], c["long_handles"]]


def bits(fb, st):
    return (fb.cpu().numpy().view(np.uint16 if fb.element_size() == 2 else np.uint32).reshape(-1, 3), st.cpu().numpy().view(np.uint32).reshape(-1, 12))


def main():
    import torch
    import rt_amd as rt
    assert os.environ.get("RT_SCHED_CACHE") == "0"
    torch.cuda.set_device(0)
    out, worlds = {}, {}
    for case, (wname, nx, ny, ns, part, reference) in CASES.items():
        if wname not in worlds:
            worlds[wname] = make_world(rt, wname)
        W, O = worlds[wname]
        O.set_traversal(rt.TRAVERSAL_REFERENCE if reference else rt.TRAVERSAL_FAST)
        ctx = rt.RenderCtx()
        fb, st, s, c = render_case(rt, torch, ctx, W, O, case)
        assert ctx.schedule_reuse() == (0, 1), (case, ctx.schedule_reuse())
        out[case + "_fb"], out[case + "_st"] = bits(fb, st)
        out[case + "_sched"], out[case + "_cnt"] = np.array(s, np.int64), np.array(c, np.int64)
        ctx.close()
    np.savez(sys.argv[1], **out)
    print("sched_cache_worker: %d cases" % len(CASES), flush=True)


if __name__ == "__main__":
    main()
