#!/usr/bin/env python3
"""The pace of the longest pixel chains over their lives (diagnostic build librt_amd_stats_light.so).  GPU box only.

A pixel's chain is serial, so a frame ends no sooner than (its longest chain) x (the time one iteration takes in the wave that holds
it).  The kernel stamps every pixel when a third and two thirds of its samples are done (rt_stats.h g_chain_dbg): this prints, for the
chains of at least MIN_ITERS iterations, the microseconds per iteration of each third, the share of each third's iterations that ran in
a wave with at most two live lanes, and how many pixels lie above given fractions of the longest.

    chain_pace.py [n nx ny ns spl [min_iters]]      (default: C3 = 10000 1200 800 64 32, 1500)
"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dd2360-raytracing_amd"))
import numpy as np
import torch
import rt_amd as rt
rt.LIB_PATH = os.path.join(ROOT, "dd2360-raytracing_amd", os.environ.get("RT_STATS_LIB", "librt_amd_stats_light.so"))
L = rt.lib()
L.rt_debug_chains.restype = C.c_int; L.rt_debug_chains.argtypes = [C.c_void_p, C.c_int]
a = [int(x) for x in sys.argv[1:]]
n, nx, ny, ns, spl = a[:5] if len(a) >= 5 else (10000, 1200, 800, 64, 32)
min_iters = a[5] if len(a) > 5 else 1500
assert nx * ny <= 1 << 20, "the stamps cover the first 2^20 pixels of a whole frame"
W = rt.World(n, nx, ny).upload(); O = rt.Octree(W, spl).upload() if spl > 0 else None
st = rt.alloc_rand_state(nx, ny); fb = rt.alloc_fb(nx, ny)
for rep in range(int(os.environ.get("CHAIN_PACE_FRAMES", "2"))):       # the second frame runs on the kept schedule, as the benchmark's steps do
    rt.render_init(nx, ny, st); rt.render(fb, nx, ny, ns, W, st, O); torch.cuda.synchronize()
    img = fb.cpu().numpy().reshape(ny * nx, 3)
    cd = np.zeros((nx * ny, 8), dtype=np.uint32)
    assert L.rt_debug_chains(cd.ctypes.data, nx * ny) == 0
    it = img[:, 0].astype(np.int64)
    tend24 = img[:, 1].astype(np.int64)                                       # (ticks >> 4) mod 2^24
    t0 = cd[:, 6].astype(np.int64); t1 = cd[:, 0].astype(np.int64); t2 = cd[:, 3].astype(np.int64)
    tend = t0 + ((((tend24 << 4) - t0) % (1 << 28)))                           # the end stamp unwrapped behind the start (16-tick steps)
    i1, i2 = cd[:, 1].astype(np.int64), cd[:, 4].astype(np.int64)
    a1, a2, a3 = cd[:, 2].astype(np.int64), cd[:, 5].astype(np.int64), cd[:, 7].astype(np.int64)
    us = lambda ticks: ((ticks) % (1 << 32)) / 100.0
    frame0 = t0.min()
    print("frame %d: %d pixels, longest chain %d iterations, frame ends %.2f ms after the first pixel started" % (rep, nx * ny, it.max(), us(tend - frame0).max() / 1e3))
    started = np.sort(us(t0 - frame0))
    print("  the queue is empty (the last pixel starts) at %.2f ms; 99.9 %% of the pixels have started at %.2f ms; the last pixel ends at %.2f ms" % (
        started[-1] / 1e3, started[int(0.999 * started.size)] / 1e3, us(tend - frame0).max() / 1e3))
    top = it.max()
    print("  pixels above 0.6 / 0.7 / 0.8 / 0.9 of the longest: %s; >= 1500: %d, >= 2000: %d" % (
        " / ".join(str(int((it >= f * top).sum())) for f in (0.6, 0.7, 0.8, 0.9)), (it >= 1500).sum(), (it >= 2000).sum()))
    m = it >= min_iters
    d = [(us(t1 - t0)[m], i1[m], a1[m]), (us(t2 - t1)[m], (i2 - i1)[m], (a2 - a1)[m]), (us(tend - t2)[m], (it - i2)[m], (a3 - a2)[m])]
    print("  chains of >= %d iterations (%d): us per iteration, by third of the samples (first / middle / last):" % (min_iters, m.sum()))
    for q in (10, 50, 90):
        print("    p%-2d  %s" % (q, "  ".join("%6.2f" % np.percentile(x[0] / np.maximum(x[1], 1), q) for x in d)))
    print("    share of those iterations in a wave of at most two live lanes: %s" % "  ".join("%.3f" % (x[2].sum() / max(1, x[1].sum())) for x in d))
    # the same pace split by how alone the chain was in that third
    pace = np.concatenate([x[0] / np.maximum(x[1], 1) for x in d]); alone = np.concatenate([x[2] / np.maximum(x[1], 1) for x in d])
    for lo, hi in ((0.0, 0.1), (0.1, 0.5), (0.5, 0.9), (0.9, 1.01)):
        k = (alone >= lo) & (alone < hi)
        if k.any():
            print("    thirds with %3.0f-%3.0f %% of their iterations in a wave of <= 2 live lanes: %5d, us per iteration p50 %.2f" % (lo * 100, min(hi, 1) * 100, k.sum(), np.median(pace[k])))
    order = np.argsort(it)[::-1][:8]
    print("  the eight longest chains (iterations; start / end ms; us per iteration and share alone of each third):")
    for p in order:
        thirds = [(us(t1 - t0)[p], i1[p], a1[p]), (us(t2 - t1)[p], i2[p] - i1[p], a2[p] - a1[p]), (us(tend - t2)[p], it[p] - i2[p], a3[p] - a2[p])]
        print("    %5d  %6.2f %6.2f   %s" % (it[p], us(t0 - frame0)[p] / 1e3, us(tend - frame0)[p] / 1e3,
                                            "   ".join("%5.2f (%.2f)" % (x[0] / max(1, x[1]), x[2] / max(1, x[1])) for x in thirds)))
    if os.environ.get("CHAIN_PACE_DUMP"):
        np.savez_compressed(os.environ["CHAIN_PACE_DUMP"] + ".%d.npz" % rep, it=it.astype(np.uint16), cd=cd, tend=tend)
