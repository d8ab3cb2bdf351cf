"""Child process of tests/test_gpu_multi_adaptive.py: one rank of an N-rank rt_multi_render_adaptive job, all ranks on GPU 0.

As tests/multi_worker.py: RCCL refuses two ranks on one device, so the exchange is rt_multi_init_custom's callback — the part to the
host, a gloo gather on 127.0.0.1, every other rank's part into its staging slot on the root.  The callback runs twice per frame,
colours first (12 bytes per element), then the sample counts (4 bytes); it checks that order and both sizes.  Rank 0 compares the
assembled frame and count map with a single-process rt_render_adaptive and exits 0 on equality.

usage: multi_adaptive_worker.py RANK WORLD PORT NX NY SPHERES SPL(0 = no octree) MIN MAX BATCH REL_ERROR FLOOR
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))


def make_gloo_gather(rt, torch, dist, rank, world, nx, ny):
    """an rt_gather_fn that moves the parts through host memory and a gloo gather; odd calls carry the counts"""
    import numpy as np
    hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    calls = [0]

    def gather(user, d_send, send_bytes, d_parts, stride, root, stream):
        try:
            px = 12 if calls[0] % 2 == 0 else 4                  # colours, then counts
            calls[0] += 1
            elems = [rt.part_pixels(nx, ny, rt.Partition(r, world)) for r in range(world)]
            assert send_bytes == elems[rank] * px, (send_bytes, elems[rank], px)
            assert stride == elems[0] * px, (stride, elems[0], px)
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
                    nbytes = elems[r] * px
                    if r != root and nbytes and hip.hipMemcpy(d_parts + r * stride, got[r].numpy().ctypes.data, nbytes, 1) != 0:
                        return 3
            return 0
        except Exception as e:                                   # nothing may propagate through the C frame
            print("gather callback:", repr(e), file=sys.stderr, flush=True)
            return 9

    return gather, calls


def main():
    rank, world, port, nx, ny, n, spl, lo, hi, step = [int(a) for a in sys.argv[1:11]]
    rel, floor = float(sys.argv[11]), float(sys.argv[12])
    import torch
    import torch.distributed as dist
    import rt_amd as rt
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    gather, calls = make_gloo_gather(rt, torch, dist, rank, world, nx, ny)

    W = rt.World(n, nx, ny)
    O = rt.Octree(W, spl) if spl > 0 else None
    P = rt.Adaptive(lo, hi, step, rel, floor)
    M = rt.Multi(rank, world, gather=gather)
    full = torch.zeros(nx * ny * 3, dtype=torch.float32, device="cuda") if rank == 0 else None
    spp = torch.full((nx * ny,), -1, dtype=torch.int32, device="cuda") if rank == 0 else None
    for _ in range(2):                                           # twice: buffers are reused, the RNG starts over (render_init)
        M.render_adaptive(full, nx, ny, P, W, O, root=0, d_spp_full=spp)
        torch.cuda.synchronize()
    assert calls[0] == 4, calls
    call_ms, kernel_ms = M.last_render_ms()
    assert call_ms > 0 and kernel_ms > 0
    rc = 0
    if rank == 0:
        st = rt.alloc_rand_state(nx, ny)
        fb = rt.alloc_fb(nx, ny)
        want = torch.full((nx * ny,), -1, dtype=torch.int32, device="cuda")
        rt.render_init(nx, ny, st)
        rt.render_adaptive(fb, nx, ny, P, W, st, O, want)
        torch.cuda.synchronize()
        same = torch.equal(full.view(torch.int32), fb.view(torch.int32)) and torch.equal(spp, want)
        counts = sorted(set(want.cpu().numpy().tolist()))
        print("multi_adaptive_worker: %d-rank frame and counts %s the single-process frame (counts %s)"
              % (world, "EQUAL" if same else "DIFFER FROM", counts), flush=True)
        rc = 0 if same else 3
    dist.barrier()
    M.close()
    dist.destroy_process_group()
    sys.exit(rc)


if __name__ == "__main__":
    main()
