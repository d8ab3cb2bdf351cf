#!/usr/bin/env python3
"""An accumulation loop on continuing RNG states, frame by frame: render_init once, then FRAMES x rt_render of one config, each frame
timed with events around the call (scheduling kernels included).  GPU box only.

bench.py re-seeds the states every step, so every step renders the same frame and a schedule built from the previous frame's
per-pixel iteration counts (rt_sched_keep.h "Feedback") knows the next frame exactly.  Here frame k + 1 draws new samples: the counts
are an estimate.  Prints one JSON line: the per-frame times, the median of frames 3 .. FRAMES, and — where the library records counts —
the recall of frame 2's true chains of at least 1 500 iterations in the long and solo lists built from frame 1's counts.

    continuing_bench.py [--tree DIR] [--config c3|c2] [--frames 12]      (--tree: another built checkout of the project, e.g. the parent)
"""
import argparse, json, os, statistics, sys
ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--config", default="c3"); ap.add_argument("--frames", type=int, default=12); ap.add_argument("--long", type=int, default=1500)
a = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "dd2360-raytracing_amd"))
import numpy as np
import torch
import rt_amd as rt
n, spl = {"c3": (10000, 32), "c2": (500, 30)}[a.config]
nx, ny, ns = 1200, 800, 64
W = rt.World(n, nx, ny).upload(); O = rt.Octree(W, spl).upload()
st = rt.alloc_rand_state(nx, ny); fb = rt.alloc_fb(nx, ny)
rt.render_init(nx, ny, st); torch.cuda.synchronize()
ms, st2 = [], None
for k in range(a.frames):
    if k == 1: st2 = st.clone()                                   # the states frame 2 starts from
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); rt.render(fb, nx, ny, ns, W, st, O); e1.record(); torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1))
out = {"tree": a.tree, "config": a.config, "frames_ms": [round(x, 3) for x in ms], "median_3_to_last_ms": round(statistics.median(ms[2:]), 3),
       "schedule_reuse": list(W.schedule_reuse())}
if hasattr(W, "schedule_feedback"):
    f, words = W.schedule_feedback(), W.render_schedule()
    out["feedback"] = f; out["schedule"] = words
    if f["has_counts"]:
        c1 = W.schedule_counts(nx * ny)                           # frame 1's counts: what the rebuilt lists were made from
        ctx = rt.RenderCtx(); ctx.render(fb, nx, ny, ns, W, st2, O); torch.cuda.synchronize()      # frame 2 again, on a context that records it
        c2 = ctx.schedule_counts(nx * ny); ctx.close()
        listed = c1 >= words["inflight_thr"]
        alone = listed & (c1.astype(np.float32) >= np.float32(float(os.environ.get("RT_FB_SOLO_FRAC", "0.75"))) * np.float32(c1.max()))
        true_long = c2 >= a.long
        out["recall"] = {"true_chains": int(true_long.sum()), "in_long_or_solo_list": int((true_long & listed).sum()), "listed": int(listed.sum()),
                         "solo_candidates": int(alone.sum()), "frame2_top": int(c2.max()), "frame1_top": int(c1.max()),
                         "frame2_top25_in_solo_candidates": int(alone[np.argsort(c2)[-25:]].sum()),
                         "rel_rms_error_of_chains_ge_1000": round(float(np.sqrt(np.mean(((c1.astype(np.float64) - c2) / np.maximum(c2, 1))[c2 >= 1000] ** 2))), 3)}
print(json.dumps(out))
