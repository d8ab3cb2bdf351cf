"""Child process of tests/test_gpu_multi.py and tests/test_gpu_multi_adaptive.py (started by tests/rank_runner.py): one rank of an
N-rank rt_multi_render or rt_multi_render_adaptive job, all ranks on GPU 0.

RCCL refuses two ranks on one device, so the exchange is the custom-gather form of rt_multi (rt_multi_init_custom): the
callback copies this rank's part to the host (hipMemcpy through the HIP runtime already in the process), gathers over gloo
on 127.0.0.1 and, on the root, copies every other rank's part into its staging slot.  Everything else — partition, render
kernels, staging layout, rt_assemble — is the code path the RCCL form runs.  An adaptive frame calls the callback twice, colours
first (12 bytes per element), then the sample counts (4 bytes); the callback checks that order and every size.  Rank 0 compares
the assembled frame (and count map) with a single-process render of the whole frame and exits 0 on equality.

usage: multi_worker.py plain    RANK WORLD PORT NX NY NS SPHERES SPL(0 = no octree) FP16 SPLIT(0 runs | 1 balanced | 2 balanced, cached)
       multi_worker.py adaptive RANK WORLD PORT NX NY SPHERES SPL(0 = no octree) MIN MAX BATCH REL_ERROR FLOOR
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))


def part_elems(rt, M, nx, ny, r, world):
    """buffer elements of rank r's part: its band of the last balanced split (every rank computed the same starts), or its runs"""
    if M.split_mode != rt.SPLIT_RUNS:
        st = M.last_split()
        return (st[r + 1] - st[r]) * 64
    return rt.part_pixels(nx, ny, rt.Partition(r, world))


def make_gloo_gather(rt, torch, dist, rank, world, nx, ny, px):
    """an rt_gather_fn (include/rt_amd.h) that moves the parts through host memory and a gloo gather.  px: the bytes per element of
    the lanes a frame moves, in call order (a number: one lane).  holder['M'] is the rt.Multi the callback serves (set by the caller
    once it exists), holder['calls'] counts the calls."""
    import numpy as np
    lanes = px if isinstance(px, (tuple, list)) else (px,)
    hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    holder = {"calls": 0}

    def gather(user, d_send, send_bytes, d_parts, stride, root, stream):
        try:
            M = holder["M"]
            b = lanes[holder["calls"] % len(lanes)]
            holder["calls"] += 1
            nbytes = [part_elems(rt, M, nx, ny, r, world) * b for r in range(world)]
            assert send_bytes == nbytes[rank] and stride >= max(nbytes), (send_bytes, stride, nbytes, b)
            if M.split_mode == rt.SPLIT_RUNS:
                assert stride == nbytes[0], (stride, nbytes, b)
            assert (d_parts is not None) == (rank == root)
            if hip.hipStreamSynchronize(stream) != 0:
                return 1
            host = np.zeros(stride, np.uint8)
            if send_bytes and hip.hipMemcpy(host.ctypes.data, d_send, send_bytes, 2) != 0:          # device -> host
                return 2
            mine = torch.from_numpy(host)
            got = [torch.empty_like(mine) for _ in range(world)] if rank == root else None
            dist.gather(mine, got, dst=root)
            if rank == root:
                for r in range(world):
                    if r != root and nbytes[r] and hip.hipMemcpy(d_parts + r * stride, got[r].numpy().ctypes.data, nbytes[r], 1) != 0:
                        return 3
            return 0
        except Exception as e:                                   # nothing may propagate through the C frame
            print("gather callback:", repr(e), file=sys.stderr, flush=True)
            return 9

    return gather, holder


def main():
    adaptive = {"plain": False, "adaptive": True}[sys.argv[1]]
    rank, world, port, nx, ny = [int(a) for a in sys.argv[2:7]]
    if adaptive:
        n, spl, lo, hi, step = [int(a) for a in sys.argv[7:12]]
        rel, floor = float(sys.argv[12]), float(sys.argv[13])
        fp16, split = 0, 0                                       # rt.SPLIT_RUNS, the library's default and the only split of adaptive frames
    else:
        ns, n, spl, fp16, split = [int(a) for a in sys.argv[7:12]]   # split: rt.SPLIT_RUNS 0 (the library's default) | SPLIT_BALANCED 1 | SPLIT_BALANCED_CACHED 2, opt-in
    import torch
    import torch.distributed as dist
    import rt_amd as rt
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    precision = rt.FP16 if fp16 else rt.FP32
    gather, holder = make_gloo_gather(rt, torch, dist, rank, world, nx, ny, (12, 4) if adaptive else 6 if fp16 else 12)

    W = rt.World(n, nx, ny, precision=precision)
    O = rt.Octree(W, spl) if spl > 0 else None
    P = rt.Adaptive(lo, hi, step, rel, floor) if adaptive else None
    M = rt.Multi(rank, world, gather=gather).set_split(split)
    holder["M"] = M
    full = torch.zeros(nx * ny * 3, dtype=torch.float16 if fp16 else torch.float32, device="cuda") if rank == 0 else None
    spp = torch.full((nx * ny,), -1, dtype=torch.int32, device="cuda") if adaptive and rank == 0 else None
    for _ in range(2):                                           # twice: buffers are reused, the RNG starts over (render_init)
        if adaptive:
            M.render_adaptive(full, nx, ny, P, W, O, root=0, d_spp_full=spp)
        else:
            M.render(full, nx, ny, ns, W, O, root=0)
        torch.cuda.synchronize()
    assert holder["calls"] == (4 if adaptive else 2), holder
    call_ms, kernel_ms = M.last_render_ms()
    assert call_ms > 0 and (kernel_ms > 0 or part_elems(rt, M, nx, ny, rank, world) == 0)   # (a rank without pixels launches no render kernel)
    rc = 0
    if rank == 0:
        st = rt.alloc_rand_state(nx, ny)
        fb = rt.alloc_fb(nx, ny, precision=precision)
        rt.render_init(nx, ny, st)
        if adaptive:
            want = torch.full((nx * ny,), -1, dtype=torch.int32, device="cuda")
            rt.render_adaptive(fb, nx, ny, P, W, st, O, want)
        else:
            rt.render(fb, nx, ny, ns, W, st, O)
        torch.cuda.synchronize()
        it = torch.int16 if fp16 else torch.int32
        same = torch.equal(full.view(it), fb.view(it))
        if adaptive:
            same = same and torch.equal(spp, want)
            print("multi_worker: %d-rank frame and counts %s the single-process frame (counts %s)"
                  % (world, "EQUAL" if same else "DIFFER FROM", sorted(set(want.cpu().numpy().tolist()))), flush=True)
        else:
            print("multi_worker: %d-rank frame %s the single-process frame" % (world, "EQUALS" if same else "DIFFERS FROM"), flush=True)
        rc = 0 if same else 3
    dist.barrier()
    M.close()
    dist.destroy_process_group()
    sys.exit(rc)


if __name__ == "__main__":
    main()
