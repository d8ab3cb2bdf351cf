"""Child process of tests/test_gpu_multi_fused.py: one rank of an N-rank rt_multi_render_adaptive job after
rt_multi_set_adaptive_fused(1), all ranks on GPU 0.  The exchange is tests/multi_worker.py's gloo gather (make_gloo_gather, lanes of
12 and 4 bytes per element: colours, then counts); rank 0 compares the assembled frame and count map with the single-process
rt_render_adaptive - the rounds - and exits 0 on equality.

usage: multi_fused_worker.py RANK WORLD PORT NX NY SPHERES SPL(0 = no octree) MIN MAX BATCH REL_ERROR FLOOR
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    rank, world, port, nx, ny, n, spl, lo, hi, step = [int(a) for a in sys.argv[1:11]]
    rel, floor = float(sys.argv[11]), float(sys.argv[12])
    import torch
    import torch.distributed as dist
    import rt_amd as rt
    from multi_worker import make_gloo_gather, part_elems
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    gather, holder = make_gloo_gather(rt, torch, dist, rank, world, nx, ny, (12, 4))
    W = rt.World(n, nx, ny)
    O = rt.Octree(W, spl) if spl > 0 else None
    P = rt.Adaptive(lo, hi, step, rel, floor)
    M = rt.Multi(rank, world, gather=gather)
    holder["M"] = M
    L = rt.lib()
    assert L.rt_multi_set_adaptive_fused(M.h, 2) == -1 and L.rt_multi_set_adaptive_fused(M.h, -1) == -1
    assert M.set_adaptive_fused(0) is M and M.set_adaptive_fused(1) is M
    full = torch.zeros(nx * ny * 3, dtype=torch.float32, device="cuda") if rank == 0 else None
    spp = torch.full((nx * ny,), -1, dtype=torch.int32, device="cuda") if rank == 0 else None
    for _ in range(2):                                           # twice: buffers are reused, the RNG starts over (render_init)
        M.render_adaptive(full, nx, ny, P, W, O, root=0, d_spp_full=spp)
        torch.cuda.synchronize()
    assert holder["calls"] == 4, holder                          # a rank that holds nothing still makes both gather calls
    call_ms, kernel_ms = M.last_render_ms()
    assert call_ms > 0 and (kernel_ms > 0 or part_elems(rt, M, nx, ny, rank, world) == 0)
    rc = 0
    if rank == 0:
        st = rt.alloc_rand_state(nx, ny)
        fb = rt.alloc_fb(nx, ny)
        want = torch.full((nx * ny,), -1, dtype=torch.int32, device="cuda")
        rt.render_init(nx, ny, st)
        rt.render_adaptive(fb, nx, ny, P, W, st, O, want)
        torch.cuda.synchronize()
        same = torch.equal(full.view(torch.int32), fb.view(torch.int32)) and torch.equal(spp, want)
        print("multi_fused_worker: %d-rank fused frame and counts %s the single-process frame (counts %s)"
              % (world, "EQUAL" if same else "DIFFER FROM", sorted(set(want.cpu().numpy().tolist()))), flush=True)
        rc = 0 if same else 3
    dist.barrier()
    M.close()
    dist.destroy_process_group()
    sys.exit(rc)


if __name__ == "__main__":
    main()
