// rt_schedule.hip — the kernels of the render path that trace no ray: the integer half of the scheduling pass and the counters of a
// launch's queue slot, for gfx950 (MI355X, CDNA4).
//
// A scheduling pass is a pilot (k_tile_cost in rt_kernels.hip, k_tile_cost_h in rt_kernels_fp16.hip) or the counts the previous launch
// recorded (k_count_cost, here), followed by what this file holds whatever the precision or the arithmetic mode: k_tile_order (the
// hand-out order of the tiles and the launch's thresholds for "long"), k_long_select / k_count_select (the long and solo chains),
// k_tail_hist / k_tail_scatter (the sorted tail), and k_zero_counters / k_keep_counters / k_restore_counters around every launch.
// All of this changes only WHICH lane renders a pixel and WHEN, never the pixel: integers and a few binary64 operations on one
// thread, no contraction (the flags of rt_kernels.o: the Makefile).
#include <hip/hip_runtime.h>
#include "rt_device.h"
#include "rt_launch.h"
#include "rt_tuning.h"
#include "rt_sched_keep.h"

#pragma clang fp contract(off)

namespace rt {

#define RT_DEV static __device__ __forceinline__

// ---------------------------------------------------------------------------------------------------- selection and order
RT_DEV int cost_class(int w) { const int c = (w - 64) / 64; return c < 0 ? 0 : (c > 7 ? 7 : c); }
// the per-block counts of 2x2 block g (at block coordinates bx, by) and its eight neighbours, summed
RT_DEV int block_sum3x3(const RenderArgs& A, const unsigned char* __restrict__ pilot, long long g, int bx, int by) {
    const int own = pilot[g];
    int sum = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int nx_ = bx + dx, ny_ = by + dy;
            int v = own;
            if (nx_ >= 0 && ny_ >= 0 && nx_ < A.tiles_x * 4 && ny_ < A.tiles_y * 4) {
                long long nl;
                if (part_has((long long)(ny_ >> 2) * A.tiles_x + (nx_ >> 2), A.part, A.nparts, A.tile_begin, A.tile_end, nl)) v = pilot[nl * 16 + (ny_ & 3) * 4 + (nx_ & 3)];
            }
            sum += v;
        }
    return sum;
}
// one thread per 2x2 block: the pilot counts of the block and its eight neighbours decide whether its pixels start as long chains.
// A neighbour outside the frame, or in a tile of another part of a partitioned frame, counts as the block itself.
__global__ __launch_bounds__(256) void k_long_select(RenderArgs A, const unsigned char* __restrict__ pilot, unsigned char* __restrict__ long_flag,
                                                    unsigned int* __restrict__ long_list, int long_sum, int solo_sum, unsigned char* __restrict__ sum8) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= A.n_local_tiles * 16) return;
    const long long local_tile = g >> 4;
    const int sub = (int)(g & 15);
    int tx, ty; local_tile_xy(A, local_tile, tx, ty);
    const int bx = tx * 4 + (sub & 3), by = ty * 4 + (sub >> 2);
    const int sum = block_sum3x3(A, pilot, g, bx, by);
    if (sum8) sum8[g] = (unsigned char)(sum < 255 ? sum : 255);                    // for the tail sort (k_tail_hist / k_tail_scatter)
    // (k_tile_order, which runs first, may have lowered the threshold: a chain is long relative to the launch's load per lane)
    const int abs_sum = (int)A.queue[kQueueThr + 1];
    const bool is_long = sum >= (abs_sum > 0 && abs_sum < long_sum ? abs_sum : long_sum);
    const int lx = 2 * (sub & 3), ly = 2 * (sub >> 2);
#pragma unroll
    for (int q = 0; q < 4; ++q) {                          // the 2x2 block this pilot pixel stands for
        const int px = lx + (q & 1), py = ly + (q >> 1);
        const bool in_img = (tile_px(tx, px) < A.max_x) && (tile_px(ty, py) < A.max_y);
        const long long pid = local_tile * 64 + py * 8 + px;
        long_flag[pid] = (is_long && in_img) ? 1 : 0;
        // the longest of them (3x3 sum >= solo_sum) are listed apart, from the end of the array: k_render starts each in a wave of its own
        if (is_long && in_img) {
            if (sum >= solo_sum) { const unsigned int pos = atomicAdd(A.queue + 4, 1u); long_list[A.n_local_tiles * 64 - 1 - pos] = (unsigned int)pid; }
            else { const unsigned int pos = atomicAdd(A.queue + 2, 1u); long_list[pos] = (unsigned int)pid; }
        }
    }
}

// ---- the measured pass (rt_sched_keep.h "Feedback"): the scheduling pass from the iteration counts the previous launch of this very
// frame recorded (RenderArgs::iters_out), in place of the pilot's one-sample paths.  k_count_cost takes the place of k_tile_cost and
// writes what it writes, in its units — cost[tile] = 4 x the bounces of 32 samples = 2 x (the tile's iterations) / ns; the byte of a
// 2x2 block = the bounces of 2 samples = (its four pixels' iterations) / (2 ns), capped at 255 — so k_tile_order and the tail sort run
// behind it unchanged; the largest count goes to queue[kQueueMaxCount].  One wave per tile, one lane per pixel.
constexpr int kQueueMaxCount = 6, kQueueSoloAsked = 7;      // words of the launch's slot that only this pass uses (zeroed with the slot)
__global__ __launch_bounds__(256) void k_count_cost(RenderArgs A, const unsigned short* __restrict__ iters, int* __restrict__ cost, unsigned char* __restrict__ pilot) {
    const int lane = threadIdx.x & 63;
    const long long local_tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (local_tile >= A.n_local_tiles) return;                                      // (wave-uniform)
    int tx, ty; local_tile_xy(A, local_tile, tx, ty);
    const int px = lane & 7, py = lane >> 3;
    const int i = tile_px(tx, px), j = tile_px(ty, py);
    const bool in_img = (i < A.max_x) && (j < A.max_y);
    const long long idx = pixel_elem(A, i, j, local_tile, lane);
    const unsigned int v = in_img ? (unsigned int)iters[idx] : 0u;
    unsigned int b = v;                                                              // the 2x2 block: lanes l, l ^ 1, l ^ 8, l ^ 9
    b += (unsigned int)__shfl_xor((int)b, 1); b += (unsigned int)__shfl_xor((int)b, 8);
    unsigned int t = v, m = v;
    for (int off = 32; off > 0; off >>= 1) { t += (unsigned int)__shfl_xor((int)t, off); const unsigned int o = (unsigned int)__shfl_xor((int)m, off); m = o > m ? o : m; }
    const unsigned int ns = (unsigned int)(A.ns > 0 ? A.ns : 1);
    if (lane == 0) { cost[local_tile] = (int)((2u * t) / ns); if (m != 0u) atomicMax(A.queue + kQueueMaxCount, m); }
    if (((px | py) & 1) == 0) { const unsigned int c = b / (2u * ns); pilot[local_tile * 16 + (py >> 1) * 4 + (px >> 1)] = (unsigned char)(c < 255u ? c : 255u); }
}
// k_long_select's sibling: one thread per 2x2 block, the same 3x3 sums for the tail sort — and the long and solo chains chosen by
// PIXEL, from its own count.  A pixel is long when its count reaches the launch's yardstick queue[kQueueThr] (the threshold k_render
// applies in flight, k_tile_order: f_inflight x load with its floor — now known before the start); a long pixel whose count reaches
// solo_frac x the frame's largest starts alone in a wave (listed from the end of long_list), at most solo_cap of them in the order
// the atomics give; the others stay long.  k_render's 1/64 rule (use_long) stands as it is.  extra: [0] the largest count, [1] solo_cap.
__global__ __launch_bounds__(256) void k_count_select(RenderArgs A, const unsigned char* __restrict__ pilot, const unsigned short* __restrict__ iters, unsigned char* __restrict__ long_flag,
                                                     unsigned int* __restrict__ long_list, unsigned char* __restrict__ sum8, float solo_frac, unsigned int solo_cap, unsigned int* __restrict__ extra) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= A.n_local_tiles * 16) return;
    const long long local_tile = g >> 4;
    const int sub = (int)(g & 15);
    int tx, ty; local_tile_xy(A, local_tile, tx, ty);
    const int sum = block_sum3x3(A, pilot, g, tx * 4 + (sub & 3), ty * 4 + (sub >> 2));
    if (sum8) sum8[g] = (unsigned char)(sum < 255 ? sum : 255);
    const unsigned int thr = A.queue[kQueueThr], top = A.queue[kQueueMaxCount];
    if (g == 0 && extra) { extra[0] = top; extra[1] = solo_cap; }
    const float solo_from = solo_frac * (float)top;
    const bool whole = frame_whole(A);
    const int lx = 2 * (sub & 3), ly = 2 * (sub >> 2);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int px = lx + (q & 1), py = ly + (q >> 1);
        const int i = tile_px(tx, px), j = tile_px(ty, py);
        const bool in_img = (i < A.max_x) && (j < A.max_y);
        const long long pid = local_tile * 64 + py * 8 + px;
        const unsigned int count = in_img ? (unsigned int)iters[pixel_elem(A, whole, i, j, pid)] : 0u;
        const bool is_long = in_img && thr != 0u && count >= thr;
        long_flag[pid] = is_long ? 1 : 0;
        if (is_long) {
            bool alone = false;
            if (solo_frac > 0.f && (float)count >= solo_from) {
                const unsigned int asked = atomicAdd(A.queue + kQueueSoloAsked, 1u);
                if (asked < solo_cap) { alone = true; atomicAdd(A.queue + 4, 1u); long_list[A.n_local_tiles * 64 - 1 - asked] = (unsigned int)pid; }
            }
            if (!alone) { const unsigned int pos = atomicAdd(A.queue + 2, 1u); long_list[pos] = (unsigned int)pid; }
        }
    }
}

// one block of 16 waves: stable counting sort of the tiles by cost class, descending (each wave takes a contiguous chunk)
//
// It also sets the launch's yardstick for "long": the pilot's bounce counts predict the launch's iterations (a tile's cost is 4 x
// the bounces of its 32 pilot samples; 64 pixels x ns samples follow them), and iterations / lanes of the persistent grid is what
// one lane will work through — the LOAD.  A pixel whose chain is a sizeable fraction of the load decides when the launch ends
// unless it runs in a thin wave from early on; whether 3000 bounces are long depends on the launch (C5 whole frame: load 18 000;
// one part of eight: 2 250).  queue[kQueueThr] = in-flight threshold in iterations, queue[kQueueThr + 1] = the same as a 3x3 pilot sum (18 samples).
__global__ __launch_bounds__(1024) void k_tile_order(const int* __restrict__ cost, unsigned int* __restrict__ order, long long n, unsigned int* __restrict__ queue,
                                                    int ns, int n_lanes, float f_inflight, float f_static, float f_tail, long long tail_cap_tiles, unsigned int* __restrict__ tail_ws, int head_sum, float head_min_load) {
    if (tail_ws && threadIdx.x < 512) tail_ws[threadIdx.x] = 0u;   // (the tail sort's counts and cursors: k_tail_hist / k_tail_scatter run after this kernel)
    __shared__ int s_cnt[16][8];
    __shared__ long long s_sum[16];
    __shared__ long long s_ccost[16][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long per = ((n + 15) / 16 + 63) / 64 * 64;          // tiles per wave, a multiple of 64
    const long long lo = wave * per, hi = (lo + per < n) ? lo + per : n;
    int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long csum = 0;
    long long ccost[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // (eight loads in flight per lane: one block sorts the whole frame's tiles, and a pass of dependent round trips per 64 tiles is what it costs)
    for (long long t0 = lo + lane; t0 < hi; t0 += 512) {
        int wv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) wv[u] = (t0 + 64 * u < hi) ? cost[t0 + 64 * u] : -1;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int w = wv[u] < 0 ? 0 : wv[u];
            const int c = wv[u] < 0 ? -1 : cost_class(w);
            csum += w;
#pragma unroll
            for (int k = 0; k < 8; ++k) { cnt[k] += (c == k) ? 1 : 0; ccost[k] += (c == k) ? w : 0; }
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        for (int off = 32; off > 0; off >>= 1) ccost[k] += __shfl_xor(ccost[k], off);
        if (lane == 0) s_ccost[wave][k] = ccost[k];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        for (int off = 32; off > 0; off >>= 1) cnt[k] += __shfl_xor(cnt[k], off);
        if (lane == 0) s_cnt[wave][k] = cnt[k];
    }
    for (int off = 32; off > 0; off >>= 1) csum += __shfl_xor(csum, off);
    if (lane == 0) s_sum[wave] = csum;
    __syncthreads();
    if (threadIdx.x == 0 && queue && n_lanes > 0 && ns > 0) {       // (s_cnt / s_sum / s_ccost are complete: the barrier above)
        long long tot = 0;
        for (int w = 0; w < 16; ++w) tot += s_sum[w];
        const double load = (double)tot * 0.5 * (double)ns / (double)n_lanes;          // predicted iterations per lane
        // (floors: in a launch with a pixel or two per lane every pixel is "long" by this measure — a chain must also be long as chains go)
        double ti = (double)f_inflight * load, tsum = 18.0 * (double)f_static * load / (double)ns;
        if (ti < (double)RT_LONG_RATE_MIN * ns) ti = (double)RT_LONG_RATE_MIN * ns;
        if (tsum < (double)RT_PILOT_LONG_SUM_MIN) tsum = (double)RT_PILOT_LONG_SUM_MIN;
        // the tail of the queue: the last tiles of the order that hold f_tail of the predicted work (tiles of one class taken as alike),
        // from a multiple of 64 on — their pixels are handed out by the tail sort's list (k_tail_hist / k_tail_scatter)
        unsigned int tail_mark = 0u;
        if (f_tail > 0.f && tot > 0) {
            const double want = (1.0 - (double)f_tail) * (double)tot;
            double cum = 0.0; long long r0 = n;
            long long start = 0;
#pragma unroll 1
            for (int k = 7; k >= 0; --k) {
                long long nk = 0, ck = 0;
#pragma unroll 1
                for (int w = 0; w < 16; ++w) { nk += s_cnt[w][k]; ck += s_ccost[w][k]; }
                if (nk > 0 && cum + (double)ck >= want) { r0 = start + (long long)((want - cum) / ((double)ck / (double)nk)); break; }
                cum += (double)ck; start += nk;
            }
            r0 = (r0 / 64) * 64;
            if (r0 < n && (n - r0) <= tail_cap_tiles) tail_mark = (unsigned int)(r0 * 64 + 1);
        }
        queue[kQueueThr + 2] = tail_mark;
        // the tail's pixels whose 3x3 pilot sum reaches head_sum are handed out before the tiles (k_tail_scatter counts them; 0 = none)
        // (head_sum < 0: the pixels whose sum is AT MOST -head_sum — the list's cheap end, the sky — are handed out first instead;
        // launches below head_min_load iterations per lane keep the whole list at the end: they need their cheapest pixels for the drain)
        if (load < (double)head_min_load) head_sum = 0;
        queue[kQueueThr + 4] = (tail_mark != 0u && head_sum > 0) ? (unsigned int)(head_sum > 255 ? 255 : head_sum) : (tail_mark != 0u && head_sum < 0) ? (unsigned int)(-head_sum >= 254 ? 255 : -head_sum + 1) : 0u;
        queue[kQueueThr + 5] = (tail_mark != 0u && head_sum < 0) ? 1u : 0u;
        queue[kQueueThr] = f_inflight > 0.f ? (unsigned int)(ti < 1.0 ? 1.0 : (ti > 4.0e9 ? 4.0e9 : ti)) : 0u;
        queue[kQueueThr + 1] = f_static > 0.f ? (unsigned int)(tsum < 1.0 ? 1.0 : (tsum > 1.0e9 ? 1.0e9 : tsum)) : 0u;
    }
    // class k: after every higher class, behind the earlier waves' share.  (Computed by 128 threads into LDS: with every thread summing
    // the 16 x 8 counts itself the kernel needed 1.1 KB of scratch per lane — for a grid of one block the runtime still sets scratch
    // aside for the whole chip, on a slow path that cost ~80 us a launch.)
    __shared__ int s_tot[8];
    __shared__ int s_base[16][8];
    if (threadIdx.x < 8) {
        int all = 0;
#pragma unroll 1
        for (int w = 0; w < 16; ++w) all += s_cnt[w][threadIdx.x];
        s_tot[threadIdx.x] = all;
    }
    __syncthreads();
    if (threadIdx.x < 128) {
        const int w0 = threadIdx.x >> 3, k0 = threadIdx.x & 7;
        int b = 0;
#pragma unroll 1
        for (int k = k0 + 1; k < 8; ++k) b += s_tot[k];
#pragma unroll 1
        for (int w = 0; w < w0; ++w) b += s_cnt[w][k0];
        s_base[w0][k0] = b;
    }
    __syncthreads();
    int base[8];                                                   // (positions: the frame's tiles fit 31 bits many times over)
#pragma unroll
    for (int k = 0; k < 8; ++k) base[k] = s_base[wave][k];
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (long long t0 = lo; t0 < hi; t0 += 512) {
        int wv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) wv[u] = (t0 + 64 * u + lane < hi) ? cost[t0 + 64 * u + lane] : -1;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (t0 + 64 * u >= hi) break;                           // (wave-uniform)
            const long long t = t0 + 64 * u + lane;
            const int c = wv[u] < 0 ? -1 : cost_class(wv[u]);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const unsigned long long m = __ballot(c == k);
                if (c == k) order[base[k] + __popcll(m & lt)] = (unsigned int)t;
                base[k] += __popcll(m);
            }
        }
    }
}

// The pixels of the queue's tail (tiles of rank >= R0 in the hand-out order), sorted by the pilot's count for their 2x2 block and its
// eight neighbours (k_long_select's sum8), most expensive first: a counting sort over the 256 values in two launches of many blocks
// (k_tail_hist: the histogram; k_tail_scatter: every block ranks its 1024 blocks among themselves in LDS and reserves its stretch of
// each value's range with one atomic) — as one block of 1024 threads it took 158 us of C3's 14.5 ms step, whatever its inner loop did.
// ws: 256 counts + 256 cursors, zeroed by k_tile_order.  Which lane renders a pixel and when never changes the pixel; the order inside
// one value is left to the atomics.
constexpr int kTailChunk = 1024;                                     // 2x2 blocks per thread block (four per thread)
RT_DEV int tail_key(const unsigned int* __restrict__ order, const unsigned char* __restrict__ sum8, long long r0, long long b, long long n_blocks, long long& tile) {
    tile = b < n_blocks ? (long long)order[r0 + (b >> 4)] : -1;
    return tile >= 0 ? 255 - (int)sum8[tile * 16 + (b & 15)] : -1;
}
__global__ __launch_bounds__(256) void k_tail_hist(const unsigned int* __restrict__ order, const unsigned char* __restrict__ sum8, long long n, const unsigned int* __restrict__ queue, unsigned int* __restrict__ ws) {
    __shared__ unsigned int s_bin[256];
    const unsigned int mark = queue[kQueueThr + 2];
    if (mark == 0u) return;
    const long long r0 = (long long)(mark - 1u) / 64, n_blocks = (n - r0) * 16;
    const long long b0 = (long long)blockIdx.x * kTailChunk;
    if (b0 >= n_blocks) return;
    s_bin[threadIdx.x] = 0u;
    __syncthreads();
    int key[4]; long long tile;
#pragma unroll
    for (int u = 0; u < 4; ++u) key[u] = tail_key(order, sum8, r0, b0 + 256 * u + threadIdx.x, n_blocks, tile);
#pragma unroll
    for (int u = 0; u < 4; ++u) if (key[u] >= 0) atomicAdd(&s_bin[key[u]], 4u);
    __syncthreads();
    const unsigned int c = s_bin[threadIdx.x];
    if (c != 0u) atomicAdd(&ws[threadIdx.x], c);
}
__global__ __launch_bounds__(256) void k_tail_scatter(const unsigned int* __restrict__ order, const unsigned char* __restrict__ sum8, unsigned int* __restrict__ tail_list,
                                                     long long n, unsigned int* __restrict__ queue, unsigned int* __restrict__ ws) {
    __shared__ unsigned int s_bin[256], s_base[256], s_wave[4];
    const unsigned int mark = queue[kQueueThr + 2];
    if (mark == 0u) return;
    const long long r0 = (long long)(mark - 1u) / 64, n_blocks = (n - r0) * 16;
    const long long b0 = (long long)blockIdx.x * kTailChunk;
    if (b0 >= n_blocks) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    s_bin[threadIdx.x] = 0u;
    // where value `threadIdx.x` begins in the list: exclusive prefix over the 256 counts (a scan per wave, then the waves' totals)
    const unsigned int cnt = ws[threadIdx.x];
    unsigned int wtot;
    const unsigned int ex = wave_excl_scan(cnt, wtot);
    if (lane == 0) s_wave[wave] = wtot;
    int key[4]; long long tile[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) key[u] = tail_key(order, sum8, r0, b0 + 256 * u + threadIdx.x, n_blocks, tile[u]);
    __syncthreads();
    unsigned int start = ex;
    for (int w = 0; w < wave; ++w) start += s_wave[w];
    // the list's first entries — every pixel whose 3x3 sum reaches the head threshold (values 255 ... thr = bins 0 ... 255 - thr) — are
    // handed out before the tiles: their count is where bin 256 - thr begins
    // (from the cheap end, queue[kQueueThr + 5]: every entry whose sum is below thr — what follows the entries counted above)
    { const unsigned int thr = queue[kQueueThr + 4];
      if (blockIdx.x == 0 && thr != 0u && threadIdx.x == 256u - thr) queue[kQueueThr + 3] = queue[kQueueThr + 5] != 0u ? (unsigned int)(n_blocks * 4) - start : start; }
    unsigned int local[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) local[u] = key[u] >= 0 ? atomicAdd(&s_bin[key[u]], 4u) : 0u;
    __syncthreads();
    const unsigned int mine = s_bin[threadIdx.x];
    s_base[threadIdx.x] = mine != 0u ? start + atomicAdd(&ws[256 + threadIdx.x], mine) : 0u;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (key[u] < 0) continue;
        const int sub = (int)((b0 + 256 * u + threadIdx.x) & 15);
        const unsigned int pos = s_base[key[u]] + local[u];
        const int lx = 2 * (sub & 3), ly = 2 * (sub >> 2);
#pragma unroll
        for (int q = 0; q < 4; ++q) tail_list[pos + q] = (unsigned int)(tile[u] * 64 + (ly + (q >> 1)) * 8 + lx + (q & 1));
    }
}

// after a pilot pass (k_tile_cost in rt_kernels.hip, k_tile_cost_h in rt_kernels_fp16.hip) has written the tile costs and, behind the pixel flags,
// the per-block counts: the long-chain list (if asked for) and the hand-out order of the tiles
// (long_sum: the 3x3 pilot sum from which a block's pixels start as long chains; 0 = RT_PILOT_LONG_SUM)
// (counted != NULL: the measured pass — the selection reads the recorded counts, k_count_select, instead of the pilot's sums)
hipError_t launch_select_and_order(const RenderArgs& A, int* cost, unsigned int* order, unsigned char* flags, unsigned int* long_list, hipStream_t st, int long_sum, int solo_sum,
                                   const CountedSelect* counted) {
    // (the order kernel first: it also derives the launch's thresholds for long chains, which the selection reads)
    // flags: 64 bytes per local tile (one per pixel), 16 (the pilot's count per 2x2 block), 16 (that count summed over the block's 3x3 neighbourhood)
    const bool tail = flags && A.tail_list && A.tail_ws && A.f_tail > 0.f;
    hipLaunchKernelGGL(k_tile_order, dim3(1), dim3(1024), 0, st, (const int*)cost, order, (long long)A.n_local_tiles, A.queue, (int)A.ns, (int)A.n_lanes, A.f_inflight, A.f_static,
                       tail ? A.f_tail : 0.f, (long long)A.n_local_tiles, tail ? A.tail_ws : (unsigned int*)nullptr, tail ? A.head_sum : 0, A.head_min_load);
    if (flags) {
        const unsigned char* pilot = flags + (size_t)A.n_local_tiles * 64;
        unsigned char* sum8 = flags + (size_t)A.n_local_tiles * 80;
        if (counted) hipLaunchKernelGGL(k_count_select, dim3((unsigned)((A.n_local_tiles * 16 + 255) / 256)), dim3(256), 0, st, A, pilot, counted->iters, flags, long_list, sum8, counted->solo_frac, counted->solo_cap, counted->extra);
        else hipLaunchKernelGGL(k_long_select, dim3((unsigned)((A.n_local_tiles * 16 + 255) / 256)), dim3(256), 0, st, A, pilot, flags, long_list, long_sum > 0 ? long_sum : RT_PILOT_LONG_SUM, solo_sum, sum8);
        if (tail) {
            const unsigned nb = (unsigned)((A.n_local_tiles * 16 + kTailChunk - 1) / kTailChunk);      // (the tail's size is known on the device only: blocks beyond it return at once)
            hipLaunchKernelGGL(k_tail_hist, dim3(nb), dim3(256), 0, st, (const unsigned int*)order, (const unsigned char*)sum8, (long long)A.n_local_tiles, (const unsigned int*)A.queue, A.tail_ws);
            hipLaunchKernelGGL(k_tail_scatter, dim3(nb), dim3(256), 0, st, (const unsigned int*)order, (const unsigned char*)sum8, (unsigned int*)A.tail_list, (long long)A.n_local_tiles, A.queue, A.tail_ws);
        }
    }
    return hipGetLastError();
}

// the measured pass's k_tile_cost (launch_count_order, rt_kernels.hip)
hipError_t launch_count_cost(const RenderArgs& A, const unsigned short* iters, int* cost, unsigned char* pilot, hipStream_t st) {
    hipLaunchKernelGGL(k_count_cost, dim3((unsigned)((A.n_local_tiles + 3) / 4)), dim3(256), 0, st, A, iters, cost, pilot);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------- a launch's counters
// Zeroes the work counters of a launch.  A kernel of our own instead of hipMemsetAsync: captured into a hipGraph, the memset
// node took effect on the first replay only (ROCm 7.2) — later replays found the queue exhausted and rendered nothing.
__global__ void k_zero_counters(unsigned int* p, int n) { if ((int)threadIdx.x < n) p[threadIdx.x] = 0u; }
hipError_t launch_zero_counters(unsigned int* p, int n, hipStream_t st) {
    hipLaunchKernelGGL(k_zero_counters, dim3(1), dim3(64), 0, st, p, n);
    return hipGetLastError();
}
// The kept schedule (rt_sched_keep.h): the words of a launch's slot that its scheduling pass wrote and the render kernel only reads —
// queue[2], queue[4] (long and solo counts), queue[kQueueThr .. kQueueThr + 5] — as kSchedKeptWords words of the context.
// k_keep_counters saves them once the pass's last kernel is behind it on the stream; k_restore_counters takes the place of
// k_zero_counters in a launch that reuses the pass: the slot's 64 words zeroed, the kept ones written.
__device__ __forceinline__ int kept_word_slot(int k) { return k == 0 ? 2 : k == 1 ? 4 : kQueueThr + (k - 2); }
__global__ void k_keep_counters(const unsigned int* __restrict__ queue, unsigned int* __restrict__ kept) {
    if (threadIdx.x < (unsigned)rt::kSchedKeptWords) kept[threadIdx.x] = queue[kept_word_slot((int)threadIdx.x)];
}
__global__ void k_restore_counters(unsigned int* __restrict__ queue, const unsigned int* __restrict__ kept) {
    // (one wave, one word per lane: lane t owns queue[t], so no word is written twice)
    const int t = (int)threadIdx.x;
    unsigned int v = 0u;
    if (t == 2) v = kept[0];
    else if (t == 4) v = kept[1];
    else if (t >= kQueueThr && t < kQueueThr + 6) v = kept[2 + t - kQueueThr];
    queue[t] = v;
}
hipError_t launch_keep_counters(const unsigned int* queue, unsigned int* kept, hipStream_t st) {
    hipLaunchKernelGGL(k_keep_counters, dim3(1), dim3(64), 0, st, queue, kept);
    return hipGetLastError();
}
hipError_t launch_restore_counters(unsigned int* queue, const unsigned int* kept, hipStream_t st) {
    static_assert(kQueueThr + 6 <= 64 && rt::kSchedKeptWords == 8, "the restore kernel covers a slot of 64 words with one wave");
    hipLaunchKernelGGL(k_restore_counters, dim3(1), dim3(64), 0, st, queue, kept);
    return hipGetLastError();
}

} // namespace rt
