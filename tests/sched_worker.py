"""Child process of tests/test_gpu_schedule.py: renders every scene of the scheduling-invariance matrix once, with the scheduling
knobs the parent put into the environment (rt_api.hip tune_value reads each knob once per process, so every setting needs a
fresh process), and writes per scene the frame, the written-back RNG state, the schedule words and the counters of the launch.

usage: sched_worker.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))

# name: (spheres, octree SPL, nx, ny, spp, binary16, partition (part, nparts) or None, the k_render instantiation it must launch).
# Every frame's local tile count is a multiple of neither 64 nor 16: the last interleave block and the last tail block are ragged.
SCENES = {
    "solo": (500, 30, 603, 403, 16, False, None, "k_render<true,0,5>"),          # 76 x 51 = 3876 tiles
    "pooled": (10000, 32, 400, 232, 16, False, None, "k_render<true,0,4>"),      # 50 x 29 = 1450 tiles
    "dense": (100000, 320, 480, 270, 16, False, None, "k_render<true,0,2>"),     # 60 x 34 = 2040 tiles
    "part": (10000, 32, 400, 232, 16, False, (1, 3), "k_render<true,0,4>"),      # 490 local tiles: 7 runs of 64 and a cut one of 42
    "h16": (500, 30, 403, 301, 16, True, None, "k_render_h<true,0>"),            # 51 x 38 = 1938 tiles
}


def main():
    import torch
    import rt_amd as rt
    out_path = sys.argv[1]
    torch.cuda.set_device(0)
    out = {}
    for name, (n, spl, nx, ny, ns, fp16, part, kernel) in SCENES.items():
        prec = rt.FP16 if fp16 else rt.FP32
        W = rt.World(n, nx, ny, precision=prec)
        O = rt.Octree(W, spl)
        P = rt.Partition(*part) if part else rt.WHOLE
        st = rt.alloc_rand_state(nx, ny, P)
        fb = rt.alloc_fb(nx, ny, P, precision=prec)
        rt.render_init(nx, ny, st, P)
        rt.render(fb, nx, ny, ns, W, st, O, P)
        torch.cuda.synchronize()
        out[name + "_kernel"] = np.array(rt.render_kernel_name(W, O))
        out[name + "_fb"] = fb.cpu().numpy().view(np.uint16 if fp16 else np.uint32).reshape(-1, 3)
        out[name + "_st"] = st.cpu().numpy().view(np.uint32).reshape(-1, 12)
        out[name + "_sched"] = np.array([W.render_schedule()[k] for k in rt.SCHEDULE_FIELDS], np.int64)
        c = W.render_counters()
        out[name + "_cnt"] = np.array([c["slots"], c["thin_waves"], c["long_chains"], c["long_handles"]], np.int64)
        O.close()
        W.close()
    np.savez(out_path, **out)
    print("sched_worker: %d scenes" % len(SCENES), flush=True)


if __name__ == "__main__":
    main()
