// rt_budget.hip — adaptive sample budgets (DESIGN.md §5.9 "Budgets"): choose, on the device, the K elements of an adaptive state with
// the largest priority (rt_adaptive_priority, ties by the lower element id), and the two bookkeeping kernels of a spend round.
// The selection is a radix select over the 32 key bits, 8 bits a pass, most significant digit first:
//   k_budget_keys      key bits of every element (0 = can never be picked) and the histogram of the top digit
//   k_budget_hist x 3  the histogram of the next digit over the elements that match the prefix found so far
//   k_budget_ties      per block, how many keys lie above the threshold key T and how many equal it
//   k_budget_scan      one block: T, the number of ties to take (K - G) and the pick count; exclusive scans of the per-block counts
//   k_budget_compact   keys above T, and the ties whose rank among the ties is below K - G, written at the block's offset: the list
//                      comes out in id order, without an atomic
// "Which bin holds the K-th key" is not a launch of its own: every block rescans the histograms of the passes before it (256 bins
// each) in its prologue.  Nothing comes back to the host, and the number of launches is fixed.
// -DRT_BUDGET_SORT (tools/mkvariant.sh): the same set by sorting (~key << 32) | id with rocprim and taking the first K — the
// on-device cross-check and the A/B baseline of tools/adaptive_budget_study.py.
// The filter-aware budget (rt_adaptive_budget_select_filtered, DESIGN.md §5.9 "Filter-aware priority") replaces k_budget_keys by
//   k_budget_keys_filtered   per 16x16 tile: the state's (x, v) of the tile and its apron staged in LDS, level 0 of rt_denoise_adaptive
//                            on them, the key of the filtered pixel (rt_adaptive_priority_filtered) and the histogram of the top digit
// and leaves the other launches as they are.  -DRT_BUDGET_FILTER_UNFUSED (tools/mkvariant.sh): the same keys from the denoiser's own
// kernels (k_denoise_var_prepare, k_denoise_var_level<false,1>) and a third that only forms the key — the on-device cross-check and the
// A/B baseline of tools/filtered_budget_study.py.
// The history-aware budget (rt_adaptive_budget_select_temporal, DESIGN.md §5.9 "History-aware priority") replaces it by
//   k_budget_keys_temporal   per 16x16 tile, one lane per pixel: what rt_temporal_accumulate would write for the pixel (temporal_pixel of
//                            rt_temporal.h: the reprojection, four gathered taps, the merge), the key of the merged pixel and the
//                            histogram of the top digit
// and again leaves the other launches as they are.
#include <hip/hip_runtime.h>
#ifdef RT_BUDGET_SORT
#include <rocprim/device/device_radix_sort.hpp>
#endif
#include "rt_device.h"
#include "rt_launch.h"
#include "rt_temporal.h"

namespace rt {

constexpr int kBudgetMaxBlocks = 1024;                   // a block of 256 threads covers `span` consecutive elements, 256 at a time; at most
                                                         // this many blocks, so that a pass ends in at most 1024 x 256 global adds
constexpr int kBudgetHistWords = 4 * 256;                // workspace: four histograms, T and the tie quota, then per block the ties and the keys above T
constexpr int kBudgetSelWords = 8;
constexpr int kBudgetWsWords = kBudgetHistWords + kBudgetSelWords + 2 * kBudgetMaxBlocks;

static long long budget_span(long long n) {
    const long long per = (n + kBudgetMaxBlocks - 1) / kBudgetMaxBlocks;
    return per <= 1024 ? 1024 : (per + 255) / 256 * 256;
}

// One count per valid lane into the block's LDS histogram.  The keys of a rendered frame share their exponent bits, so most of a
// wave meets in a few bins: up to four times, the lanes that hold the first pending lane's digit are counted with one ballot and
// ONE LDS add; whatever is left after that (a pass over mantissa bits: all digits differ) adds for itself.
__device__ __forceinline__ void budget_hist_add(bool valid, unsigned int digit, unsigned int* sh_hist) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(valid);
    for (int it = 0; it < 4 && todo != 0ull; ++it) {
        const int leader = __ffsll(todo) - 1;
        const unsigned int d = __shfl(digit, leader);
        const bool mine = valid && digit == d;
        const unsigned long long m = __ballot(mine);
        if (lane == leader) atomicAdd(&sh_hist[d], (unsigned int)__popcll(m));
        if (mine) valid = false;
        todo &= ~m;
    }
    if (valid) atomicAdd(&sh_hist[digit], 1u);
}
__device__ __forceinline__ unsigned int budget_lane_rank(unsigned long long m) {          // set bits of m below this lane
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
// for thread t of the block's 256: the sum of v over the threads >= t (sh: 4 words)
__device__ __forceinline__ unsigned int budget_suffix_sum(unsigned int v, unsigned int* sh) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned int o = __shfl_down(v, off);
        if (lane + off < 64) v += o;
    }
    if (lane == 0) sh[w] = v;
    __syncthreads();
    for (int ww = w + 1; ww < 4; ++ww) v += sh[ww];
    __syncthreads();
    return v;
}
// ... and over the threads < t, with the block's total (sh: 4 words)
__device__ __forceinline__ unsigned int budget_prefix_sum(unsigned int v, unsigned int& total, unsigned int* sh) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned int inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned int o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
    }
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    unsigned int before = inc - v;
    for (int ww = 0; ww < w; ++ww) before += sh[ww];
    total = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return before;
}
// The digits of the K-th largest key that the first `passes` histograms fix (prefix), and rem = K minus the keys above that prefix:
// in every pass the bin b with  sum(hist[b..255]) >= rem > sum(hist[b+1..255]).  K >= 1 and K <= the number of keys, so pass 0 has
// such a bin, and pass q + 1 counts exactly the keys of pass q's bin, of which rem are still wanted.  Block-uniform.  (sh: 8 words)
__device__ __forceinline__ void budget_resolve(const unsigned int* __restrict__ hist, int passes, unsigned int K, unsigned int& prefix,
                                               unsigned int& rem, unsigned int* sh) {
    prefix = 0u; rem = K;
    for (int q = 0; q < passes; ++q) {
        if (threadIdx.x == 0) { sh[4] = 0u; sh[5] = 0u; }
        const unsigned int h = hist[q * 256 + threadIdx.x];
        const unsigned int s = budget_suffix_sum(h, sh);
        if (s >= rem && s - h < rem) { sh[4] = threadIdx.x; sh[5] = rem - (s - h); }
        __syncthreads();
        prefix = (prefix << 8) | sh[4]; rem = sh[5];
        __syncthreads();
    }
}

// One thread per element: the key bits of rt_adaptive_priority, 0 for an element that is not eligible (padding of an edge tile,
// k + batch > max_spp, key 0) — key 0 is never picked.  hist != NULL: the histogram of the top digit.
__global__ __launch_bounds__(256) void k_budget_keys(AdaptState s, long long n, long long span, AdaptFrame fr, int batch, int max_spp, float floor_lum,
                                                     unsigned int* __restrict__ keys, unsigned int* __restrict__ hist) {
    __shared__ unsigned int sh_hist[256];
    sh_hist[threadIdx.x] = 0u;
    __syncthreads();
    const bool whole = part_whole(fr.nparts, fr.tile_begin, fr.tile_end);
    const long long begin = (long long)blockIdx.x * span;
    for (long long o = 0; o < span && begin + o < n; o += 256) {
        const long long t = begin + o + threadIdx.x;
        const bool valid = t < n;
        unsigned int key = 0u;
        if (valid) {
            if (whole || adapt_in_frame(t, fr)) {
                const int k = s.k[t];
                if ((long long)k + batch <= (long long)max_spp) key = __float_as_uint(adapt_priority(s.sl[t], s.q[t], k, floor_lum));
            }
            keys[t] = key;
        }
        if (hist) budget_hist_add(valid, key >> 24, sh_hist);
    }
    __syncthreads();
    const unsigned int c = sh_hist[threadIdx.x];
    if (hist && c) atomicAdd(&hist[threadIdx.x], c);
}
// pass 1..3: the histogram of digit `pass` over the keys whose higher digits are the prefix of the K-th key
__global__ __launch_bounds__(256) void k_budget_hist(const unsigned int* __restrict__ keys, long long n, long long span, unsigned int K, unsigned int* hist, int pass) {
    __shared__ unsigned int sh_hist[256];
    __shared__ unsigned int sh[8];
    if (K == 0u) return;
    sh_hist[threadIdx.x] = 0u;
    unsigned int prefix, rem;
    budget_resolve(hist, pass, K, prefix, rem, sh);          // (its barriers also publish sh_hist's zeroes)
    const int shift = 24 - 8 * pass;
    const long long begin = (long long)blockIdx.x * span;
    for (long long o = 0; o < span && begin + o < n; o += 256) {
        const long long t = begin + o + threadIdx.x;
        const unsigned int key = t < n ? keys[t] : 0u;
        budget_hist_add(t < n && (key >> (shift + 8)) == prefix, (key >> shift) & 255u, sh_hist);
    }
    __syncthreads();
    const unsigned int c = sh_hist[threadIdx.x];
    if (c) atomicAdd(&hist[pass * 256 + threadIdx.x], c);
}
// the threshold key T (the K-th largest) and how many keys equal to it are to be taken; K == 0 and T == 0 take none
__device__ __forceinline__ void budget_threshold(const unsigned int* __restrict__ hist, unsigned int K, unsigned int& T, unsigned int& need, unsigned int* sh) {
    if (K == 0u) { T = 0xffffffffu; need = 0u; return; }     // (no key has these bits: a NaN priority is 0)
    budget_resolve(hist, 4, K, T, need, sh);
    if (T == 0u) need = 0u;                                  // fewer eligible elements than K: all of them are above T
}
__global__ __launch_bounds__(256) void k_budget_ties(const unsigned int* __restrict__ keys, long long n, long long span, unsigned int K,
                                                     const unsigned int* __restrict__ hist, unsigned int* __restrict__ blk_tie, unsigned int* __restrict__ blk_above) {
    __shared__ unsigned int sh[8];
    unsigned int T, need;
    budget_threshold(hist, K, T, need, sh);
    const long long begin = (long long)blockIdx.x * span;
    unsigned int ct = 0u, ca = 0u;                           // (per wave)
    for (long long o = 0; o < span && begin + o < n; o += 256) {
        const long long t = begin + o + threadIdx.x;
        const unsigned int key = t < n ? keys[t] : 0u;
        ct += (unsigned int)__popcll(__ballot(t < n && key == T));
        ca += (unsigned int)__popcll(__ballot(t < n && key > T));
    }
    if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = ct; sh[4 + (threadIdx.x >> 6)] = ca; }
    __syncthreads();
    if (threadIdx.x == 0) { blk_tie[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]); blk_above[blockIdx.x] = (sh[4] + sh[5]) + (sh[6] + sh[7]); }
}
// one block: sel = {T, ties to take}, both per-block counts become their exclusive scans (for a block: the ties and the keys above T
// in the blocks before it, that is at lower ids), and *count the number of picks
__global__ __launch_bounds__(256) void k_budget_scan(const unsigned int* __restrict__ hist, unsigned int K, unsigned int* __restrict__ blk_tie,
                                                     unsigned int* __restrict__ blk_above, int nblk, unsigned int* __restrict__ sel, unsigned int* __restrict__ count) {
    __shared__ unsigned int sh[8];
    unsigned int T, need;
    budget_threshold(hist, K, T, need, sh);
    unsigned int ties = 0u, above = 0u;
    for (int b0 = 0; b0 < nblk; b0 += 256) {
        const int i = b0 + threadIdx.x;
        unsigned int tt, ta;
        const unsigned int bt = budget_prefix_sum(i < nblk ? blk_tie[i] : 0u, tt, sh);
        const unsigned int ba = budget_prefix_sum(i < nblk ? blk_above[i] : 0u, ta, sh);
        if (i < nblk) { blk_tie[i] = ties + bt; blk_above[i] = above + ba; }
        ties += tt; above += ta;
    }
    if (threadIdx.x == 0) { sel[0] = T; sel[1] = need; *count = above + (ties < need ? ties : need); }
}
__global__ __launch_bounds__(256) void k_budget_compact(const unsigned int* __restrict__ keys, long long n, long long span, const unsigned int* __restrict__ sel,
                                                        const unsigned int* __restrict__ blk_tie, const unsigned int* __restrict__ blk_above,
                                                        unsigned int* __restrict__ list, unsigned int K) {
    __shared__ unsigned int sh[8];
    const unsigned int T = sel[0], need = sel[1];
    unsigned int run = blk_tie[blockIdx.x];                                   // ties at lower ids
    unsigned int at = blk_above[blockIdx.x] + (run < need ? run : need);     // picks at lower ids: where this block writes
    const int w = threadIdx.x >> 6;
    const long long begin = (long long)blockIdx.x * span;
    for (long long o = 0; o < span && begin + o < n; o += 256) {
        const long long t = begin + o + threadIdx.x;
        const unsigned int key = t < n ? keys[t] : 0u;
        bool pick = t < n && key > T;
        if (run < need) {                                    // (block-uniform) some of this block's ties may still be wanted
            const bool tie = t < n && key == T;
            const unsigned long long m = __ballot(tie);
            if ((threadIdx.x & 63) == 0) sh[w] = (unsigned int)__popcll(m);
            __syncthreads();
            unsigned int rank = run + budget_lane_rank(m);
            for (int ww = 0; ww < w; ++ww) rank += sh[ww];
            run += (sh[0] + sh[1]) + (sh[2] + sh[3]);
            pick = pick || (tie && rank < need);
        }
        const unsigned long long mp = __ballot(pick);
        if ((threadIdx.x & 63) == 0) sh[4 + w] = (unsigned int)__popcll(mp);
        __syncthreads();
        unsigned int pos = at + budget_lane_rank(mp);
        for (int ww = 0; ww < w; ++ww) pos += sh[4 + ww];
        at += (sh[4] + sh[5]) + (sh[6] + sh[7]);
        if (pick && pos < K) list[pos] = (unsigned int)t;     // (the set never exceeds K: the list's capacity is not left to that proof)
        __syncthreads();
    }
}

#ifdef RT_BUDGET_SORT
__global__ __launch_bounds__(256) void k_budget_sort_pack(const unsigned int* __restrict__ keys, long long n, unsigned long long* __restrict__ out,
                                                          unsigned int* __restrict__ count) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t == 0) *count = 0u;
    if (t < n) out[t] = ((unsigned long long)~keys[t] << 32) | (unsigned long long)t;
}
// the first K of the sorted keys, without those of key 0 (the wave's picked lanes append with one atomic, adapt_append of rt_adaptive.hip)
__global__ __launch_bounds__(256) void k_budget_sort_take(const unsigned long long* __restrict__ sorted, unsigned int K, unsigned int* __restrict__ list,
                                                          unsigned int* __restrict__ count) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long v = t < (long long)K ? sorted[t] : 0ull;
    const bool pick = t < (long long)K && (unsigned int)(v >> 32) != 0xffffffffu;
    const unsigned long long mask = __ballot(pick);
    if (mask != 0ull) {
        unsigned int base = 0;
        if ((threadIdx.x & 63) == 0) base = atomicAdd(count, (unsigned int)__popcll(mask));
        base = __shfl(base, 0);
        if (pick) list[base + budget_lane_rank(mask)] = (unsigned int)v;
    }
}
static size_t budget_sort_temp(long long n) {
    size_t need = 0;
    (void)rocprim::radix_sort_keys(nullptr, need, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (size_t)n, 0u, 64u, (hipStream_t)nullptr);
    return need;
}
#endif

// bytes of the selection workspace for a state of n elements (filtered: and of what the unfused variant of the filtered key needs)
static size_t budget_ws_head(long long n) {
    size_t b = sizeof(unsigned int) * (size_t)kBudgetWsWords;
#ifdef RT_BUDGET_SORT
    b = (b + 255) / 256 * 256 + (2 * sizeof(unsigned long long) * (size_t)n + 255) / 256 * 256 + budget_sort_temp(n);
#else
    (void)n;
#endif
    return b;
}
size_t budget_ws_bytes(long long n, bool filtered) {
    size_t b = budget_ws_head(n);
#ifdef RT_BUDGET_FILTER_UNFUSED
    if (filtered) b = (b + 255) / 256 * 256 + (size_t)RT_DENOISE_WORK_BYTES * (size_t)n;
#else
    (void)filtered;
#endif
    return b;
}
// A selection is: budget_select_begin, one launch that writes the n key words and adds the histogram of their top digit to `hist`
// (NULL: the sorting variant needs none), budget_select_finish.
static hipError_t budget_select_begin(unsigned int* ws, unsigned int*& hist, hipStream_t st) {
#ifdef RT_BUDGET_SORT
    (void)ws; (void)st;
    hist = nullptr;
    return hipSuccess;
#else
    hist = ws;
    return hipMemsetAsync(hist, 0, sizeof(unsigned int) * kBudgetHistWords, st);
#endif
}
static hipError_t budget_select_finish(long long n, unsigned int K, unsigned int* keys, unsigned int* ws, unsigned int* list, unsigned int* count, hipStream_t st) {
#ifdef RT_BUDGET_SORT
    const size_t head = (sizeof(unsigned int) * (size_t)kBudgetWsWords + 255) / 256 * 256;
    unsigned long long* in = (unsigned long long*)((char*)ws + head);
    unsigned long long* out = in + n;
    void* temp = (char*)in + (2 * sizeof(unsigned long long) * (size_t)n + 255) / 256 * 256;
    size_t need = budget_sort_temp(n);
    hipLaunchKernelGGL(k_budget_sort_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keys, n, in, count);
    const hipError_t e = rocprim::radix_sort_keys(temp, need, in, out, (size_t)n, 0u, 64u, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_budget_sort_take, dim3(K / 256 + 1), dim3(256), 0, st, out, K, list, count);
#else
    const long long span = budget_span(n);
    const unsigned nblk = (unsigned)((n + span - 1) / span);          // <= kBudgetMaxBlocks
    unsigned int* hist = ws; unsigned int* sel = ws + kBudgetHistWords; unsigned int* blk_tie = sel + kBudgetSelWords; unsigned int* blk_above = blk_tie + kBudgetMaxBlocks;
    for (int pass = 1; pass < 4; ++pass) hipLaunchKernelGGL(k_budget_hist, dim3(nblk), dim3(256), 0, st, keys, n, span, K, hist, pass);
    hipLaunchKernelGGL(k_budget_ties, dim3(nblk), dim3(256), 0, st, keys, n, span, K, hist, blk_tie, blk_above);
    hipLaunchKernelGGL(k_budget_scan, dim3(1), dim3(256), 0, st, hist, K, blk_tie, blk_above, (int)nblk, sel, count);
    hipLaunchKernelGGL(k_budget_compact, dim3(nblk), dim3(256), 0, st, keys, n, span, sel, blk_tie, blk_above, list, K);
#endif
    return hipGetLastError();
}
// The K (<= n) elements of the state with the largest keys into list, their number into *count.  keys: n words, ws: budget_ws_bytes(n).
hipError_t launch_budget_select(const AdaptState& s, long long n, const AdaptFrame& fr, int batch, int max_spp, float floor_lum, unsigned int K,
                                unsigned int* keys, unsigned int* ws, unsigned int* list, unsigned int* count, hipStream_t st) {
    const long long span = budget_span(n);
    const unsigned nblk = (unsigned)((n + span - 1) / span);          // <= kBudgetMaxBlocks
    unsigned int* hist;
    const hipError_t e = budget_select_begin(ws, hist, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_budget_keys, dim3(nblk), dim3(256), 0, st, s, n, span, fr, batch, max_spp, floor_lum, keys, hist);
    return budget_select_finish(n, K, keys, ws, list, count, st);
}

// ---- the filter-aware key (rt_amd.h, rt_adaptive_budget_select_filtered) ---------------------------------------------------------
// Whole row-major frames of at most RT_DENOISE_MAX_PIXELS pixels: a pixel index, 2 * p + 1 and a tile count fit an int, 3 * p does not.
#ifndef RT_BUDGET_FILTER_UNFUSED
// A block owns `per` consecutive 16x16 tiles (at most kBudgetMaxBlocks blocks: one global add per bin and block, as k_budget_keys).
// Per tile: the tile and its apron of 2 in k_denoise_var_level<*, 1>'s LDS layout — colour + variance and both guide halves, 20 rows
// of 32 16-byte slots each, 30 KB, the same slots read by the same lanes, so its bank argument holds here (rt_denoise.hip) — but
// filled straight from the state: every staged pixel computes k_denoise_var_prepare's (x, v) and pass-through mark itself (a pixel
// of the apron is computed by up to four tiles; 144 of 400 per tile, against a float4 written and read back per pixel).  Then one
// lane per pixel: level 0 of the filter as that kernel writes it, the key, the key bits (0 = not eligible) and the top digit's count.
// 30 KB + 1 KB of LDS: four blocks a CU.  The arithmetic is copied, not shared, so that the denoiser's kernels stay as they compile.
__global__ __launch_bounds__(256) void k_budget_keys_filtered(AdaptState s, const float4* __restrict__ g, int max_x, int max_y, int tiles_x, int tiles, int per,
                                                              DenoiseVarLevel L, int batch, int max_spp, float floor_lum, unsigned int* __restrict__ keys,
                                                              float* __restrict__ keys_out, unsigned int* __restrict__ hist) {
    constexpr int S = 20, ST = 32;
    __shared__ float4 sx[S * ST], sg0[S * ST], sg1[S * ST];
    __shared__ unsigned int sh_hist[256];
    sh_hist[threadIdx.x] = 0u;                                       // (published by the first tile's barrier)
    const int li = (int)(threadIdx.x & 15), lj = (int)(threadIdx.x >> 4);
    const int c = (lj + 2) * ST + li + 2;                            // the centre's slot
    const int first = (int)blockIdx.x * per;
    const int last = first + per < tiles ? first + per : tiles;
    for (int tile = first; tile < last; ++tile) {
        const int tx = tile % tiles_x, ty = tile / tiles_x;
        const int i0 = tx * 16 - 2, j0 = ty * 16 - 2;
        for (int e = (int)threadIdx.x; e < S * S; e += 256) {
            const int ej = e / S, ei = e - ej * S;
            const int qi = i0 + ei, qj = j0 + ej;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, -1.0f);         // outside the frame: pass-through
            if (qi >= 0 && qi < max_x && qj >= 0 && qj < max_y) {
                const int q = qj * max_x + qi;
                const long long e3 = 3 * (long long)q;
                const int k = s.k[q];
                const float nf = (float)k;
                v.x = s.rgb[e3] / nf; v.y = s.rgb[e3 + 1] / nf; v.z = s.rgb[e3 + 2] / nf;
                const float sl = s.sl[q];
                float d = nf * s.q[q] - sl * sl;
                d = d > 0.0f ? d : 0.0f;
                v.w = d / ((nf * nf) * (nf - 1.0f));
                const float4 g1 = g[2 * q + 1];
                if (__float_as_int(g1.w) == -1 || k < 2 || !__builtin_isfinite(v.x) || !__builtin_isfinite(v.y) || !__builtin_isfinite(v.z) || !__builtin_isfinite(v.w))
                    v = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
                else { sg0[ej * ST + ei] = g[2 * q]; sg1[ej * ST + ei] = g1; }
            }
            sx[ej * ST + ei] = v;
        }
        __syncthreads();
        const int i = tx * 16 + li, j = ty * 16 + lj;
        const bool inside = i < max_x && j < max_y;
        unsigned int key = 0u;
        if (inside) {
            const int p = j * max_x + i;
            const int k = s.k[p];
            const float4 xp = sx[c];
            float pr;
            if (xp.w < 0.0f) {                                       // pass-through: the raw rule
                pr = adapt_priority(s.sl[p], s.q[p], k, floor_lum);
            } else {
                const float4 gp0 = sg0[c], gp1 = sg1[c];             // (t, P) and (N, sphere)
                const int sp = __float_as_int(gp1.w);
                const float tt = gp0.x * gp0.x;
                float vb = xp.w;
                if (L.prefilter) {
                    const float k3[3] = {0.25f, 0.5f, 0.25f};
                    float sg = 0.0f, sv = 0.0f;
#pragma unroll
                    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                        for (int dx = -1; dx <= 1; ++dx) {
                            const int t = c + dy * ST + dx;
                            const float vq = sx[t].w;
                            if (vq < 0.0f) continue;
                            if (__float_as_int(sg1[t].w) != sp) continue;
                            const float gw = k3[dx + 1] * k3[dy + 1];
                            sg = sg + gw;
                            sv = sv + gw * vq;
                        }
                    }
                    vb = sv / sg;
                }
                const float den = L.sv2 * vb + RT_DENOISE_VAR_EPS;
                const float lp = (xp.x + xp.y) + xp.z;
                const float k5[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
                float sw = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
                for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
                    for (int dx = -2; dx <= 2; ++dx) {
                        const int t = c + dy * ST + dx;
                        const float4 xq = sx[t];
                        if (xq.w < 0.0f) continue;                   // a pass-through pixel (or one outside the frame) is never a tap
                        const float4 gq1 = sg1[t];
                        if (__float_as_int(gq1.w) != sp) continue;   // another sphere
                        float wn = 1.0f;
                        if (L.npow >= 0) {
                            const float d = (gp1.x * gq1.x + gp1.y * gq1.y) + gp1.z * gq1.z;
                            wn = d > 0.0f ? d : 0.0f;
                            for (int e = 0; e < L.npow; ++e) wn = wn * wn;
                        }
                        float apos = 0.0f;
                        if (L.use_pos) {
                            const float4 gq0 = sg0[t];
                            const float ex = gp0.y - gq0.y, ey = gp0.z - gq0.z, ez = gp0.w - gq0.w;
                            apos = (((ex * ex + ey * ey) + ez * ez) / tt) * L.inv_sp2;
                        }
                        float avar = 0.0f;
                        if (L.use_var) {
                            const float dl = lp - ((xq.x + xq.y) + xq.z);
                            avar = (dl * dl) / den;
                        }
                        const float w = (k5[dx + 2] * k5[dy + 2] * wn) / ((1.0f + apos) * (1.0f + avar));
                        sw = sw + w;
                        s0 = s0 + w * xq.x; s1 = s1 + w * xq.y; s2 = s2 + w * xq.z;
                        s3 = s3 + (w * w) * xq.w;
                    }
                }
                const float y0 = s0 / sw, y1 = s1 / sw, y2 = s2 / sw;
                pr = adapt_priority_filtered((y0 + y1) + y2, s3 / (sw * sw), floor_lum);
            }
            if (keys_out) keys_out[p] = pr;
            if ((long long)k + batch <= (long long)max_spp) key = __float_as_uint(pr);
            keys[p] = key;
        }
        if (hist) budget_hist_add(inside, key >> 24, sh_hist);
        __syncthreads();                                             // the tile has been read: the next one may be staged
    }
    __syncthreads();
    const unsigned int cnt = sh_hist[threadIdx.x];
    if (hist && cnt) atomicAdd(&hist[threadIdx.x], cnt);
}
#else
// the third kernel of the unfused variant: y = what level 0 left, (y, v') or .w < 0 for a pass-through pixel; laid out as k_budget_keys
__global__ __launch_bounds__(256) void k_budget_keys_from_level(const float4* __restrict__ y, AdaptState s, long long n, long long span, int batch, int max_spp,
                                                                float floor_lum, unsigned int* __restrict__ keys, float* __restrict__ keys_out,
                                                                unsigned int* __restrict__ hist) {
    __shared__ unsigned int sh_hist[256];
    sh_hist[threadIdx.x] = 0u;
    __syncthreads();
    const long long begin = (long long)blockIdx.x * span;
    for (long long o = 0; o < span && begin + o < n; o += 256) {
        const long long t = begin + o + threadIdx.x;
        const bool valid = t < n;
        unsigned int key = 0u;
        if (valid) {
            const int k = s.k[t];
            const float4 v = y[t];
            const float pr = v.w < 0.0f ? adapt_priority(s.sl[t], s.q[t], k, floor_lum) : adapt_priority_filtered((v.x + v.y) + v.z, v.w, floor_lum);
            if (keys_out) keys_out[t] = pr;
            if ((long long)k + batch <= (long long)max_spp) key = __float_as_uint(pr);
            keys[t] = key;
        }
        if (hist) budget_hist_add(valid, key >> 24, sh_hist);
    }
    __syncthreads();
    const unsigned int c = sh_hist[threadIdx.x];
    if (hist && c) atomicAdd(&hist[threadIdx.x], c);
}
#endif
// launch_budget_select with the filtered key: the state of a whole row-major frame and its guides (both checked by the caller: 16-byte
// aligned hits, max_x * max_y <= RT_DENOISE_MAX_PIXELS).  keys_out (may be NULL): the key of every pixel before the eligibility mask.
// ws: budget_ws_bytes(n, true).
hipError_t launch_budget_select_filtered(const AdaptState& s, const rt_hit_record* hits, int max_x, int max_y, const rt_denoise_var_params& P, int batch,
                                         int max_spp, float floor_lum, unsigned int K, unsigned int* keys, float* keys_out, unsigned int* ws,
                                         unsigned int* list, unsigned int* count, hipStream_t st) {
    const long long n = (long long)max_x * max_y;
    unsigned int* hist;
    hipError_t e = budget_select_begin(ws, hist, st);
    if (e != hipSuccess) return e;
#ifndef RT_BUDGET_FILTER_UNFUSED
    const int tiles_x = (max_x + 15) / 16, tiles_y = (max_y + 15) / 16;
    const int tiles = tiles_x * tiles_y;                              // (<= 2^30 / 256 + two edges: fits)
    const int per = (tiles + kBudgetMaxBlocks - 1) / kBudgetMaxBlocks;
    const unsigned nblk = (unsigned)((tiles + per - 1) / per);        // <= kBudgetMaxBlocks, every block owns at least one tile
    hipLaunchKernelGGL(k_budget_keys_filtered, dim3(nblk), dim3(256), 0, st, s, (const float4*)hits, max_x, max_y, tiles_x, tiles, per,
                       denoise_var_level(P, 0), batch, max_spp, floor_lum, keys, keys_out, hist);
#else
    float4* work = (float4*)((char*)ws + (budget_ws_head(n) + 255) / 256 * 256);
    e = launch_denoise_var_level0(s.rgb, max_x, max_y, hits, s.rgb, P, work, st);      // (fb_in: only copied into pass-through pixels, whose colour nobody reads)
    if (e != hipSuccess) return e;
    const long long span = budget_span(n);
    hipLaunchKernelGGL(k_budget_keys_from_level, dim3((unsigned)((n + span - 1) / span)), dim3(256), 0, st, work + n, s, n, span, batch, max_spp, floor_lum,
                       keys, keys_out, hist);
#endif
    return budget_select_finish(n, K, keys, ws, list, count, st);
}

// ---- the history-aware key (rt_amd.h, rt_adaptive_budget_select_temporal) ---------------------------------------------------------
// Whole row-major frames of at most RT_DENOISE_MAX_PIXELS pixels, as the filtered key.  A block owns `per` consecutive 16x16 tiles (at
// most kBudgetMaxBlocks blocks: one global add per bin and block), one lane per pixel.  The pixel is ranked by what rt_temporal_accumulate
// would leave of it: temporal_pixel (rt_temporal.h) is that kernel's own body — the state, both guide halves, the reprojection through
// the previous camera, the four taps' loads issued before any of them is tested, the merge — so the rule exists once.  The taps go
// straight through the caches: where a tile lands in the last frame depends on the camera, there is no fixed apron to stage.  A pixel
// without anything accumulated (neff == 0: EMPTY) keeps the raw key, as in k_budget_keys_filtered.  LDS: the 256-word histogram alone.
__global__ __launch_bounds__(256) void k_budget_keys_temporal(TemporalArgs T, int tiles, int per, int batch, int max_spp, float floor_lum,
                                                              unsigned int* __restrict__ keys, float* __restrict__ keys_out, unsigned int* __restrict__ hist) {
    __shared__ unsigned int sh_hist[256];
    sh_hist[threadIdx.x] = 0u;
    __syncthreads();
    const int li = (int)(threadIdx.x & 15), lj = (int)(threadIdx.x >> 4);
    const int first = (int)blockIdx.x * per;
    const int last = first + per < tiles ? first + per : tiles;
    for (int tile = first; tile < last; ++tile) {
        const int tx = tile % T.tiles_x, ty = tile / T.tiles_x;
        const int i = tx * 16 + li, j = ty * 16 + lj;
        const bool inside = i < T.max_x && j < T.max_y;
        unsigned int key = 0u;
        if (inside) {
            const int p = j * T.max_x + i;
            const TemporalPixel R = temporal_pixel(T, p);
            const float pr = R.neff == 0.0f ? adapt_priority(R.sl, R.q, R.k, floor_lum)                       // EMPTY: the raw rule
                                            : adapt_priority_filtered((R.out.x + R.out.y) + R.out.z, R.out.w, floor_lum);
            if (keys_out) keys_out[p] = pr;
            if ((long long)R.k + batch <= (long long)max_spp) key = __float_as_uint(pr);
            keys[p] = key;
        }
        if (hist) budget_hist_add(inside, key >> 24, sh_hist);
    }
    __syncthreads();
    const unsigned int cnt = sh_hist[threadIdx.x];
    if (hist && cnt) atomicAdd(&hist[threadIdx.x], cnt);
}
// launch_budget_select with the history-aware key: the state and guides of a whole row-major frame and the last frame's history, guides
// and camera (all checked by the caller, as launch_temporal_accumulate's; hist_in == nullptr: the first frame).  keys_out (may be
// NULL): the key of every pixel before the eligibility mask.  ws: budget_ws_bytes(n, false).
hipError_t launch_budget_select_temporal(const void* state, const void* hist_in, const rt_hit_record* hits, const rt_hit_record* hits_prev,
                                         const rt_camera* cam_prev, const int32_t* kind, int n_kind, int max_x, int max_y, const rt_temporal_params& P,
                                         int batch, int max_spp, float floor_lum, unsigned int K, unsigned int* keys, float* keys_out, unsigned int* ws,
                                         unsigned int* list, unsigned int* count, hipStream_t st) {
    const long long n = (long long)max_x * max_y;
    unsigned int* hist;
    const hipError_t e = budget_select_begin(ws, hist, st);
    if (e != hipSuccess) return e;
    const TemporalArgs T = temporal_args(nullptr, hist_in, hits, hits_prev, cam_prev, state, kind, n_kind, max_x, max_y, P);
    const int tiles = T.tiles_x * ((max_y + 15) / 16);                // (<= 2^30 / 256 + two edges: fits)
    const int per = (tiles + kBudgetMaxBlocks - 1) / kBudgetMaxBlocks;
    const unsigned nblk = (unsigned)((tiles + per - 1) / per);        // <= kBudgetMaxBlocks, every block owns at least one tile
    hipLaunchKernelGGL(k_budget_keys_temporal, dim3(nblk), dim3(256), 0, st, T, tiles, per, batch, max_spp, floor_lum, keys, keys_out, hist);
    return budget_select_finish(n, K, keys, ws, list, count, st);
}

// ---- the bookkeeping of a spend round --------------------------------------------------------------------------------------
// before the round: fb gets S_rgb of the chosen pixels, where the resumed k_render<*, 2, *> reads it (k_adapt_refine_seed's active branch)
__global__ __launch_bounds__(256) void k_budget_seed(float* __restrict__ fb, AdaptState s, const unsigned int* __restrict__ list, const unsigned int* __restrict__ count) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < (long long)*count) {
        const unsigned int pid = list[t];
        const float* S = s.rgb + (size_t)pid * 3;
        float* f = fb + (size_t)pid * 3;
        f[0] = S[0]; f[1] = S[1]; f[2] = S[2];
    }
}
// after the round: every listed pixel has taken `batch` samples more and is finalised — k_adapt_refine_check without the rule
__global__ __launch_bounds__(256) void k_budget_final(float* __restrict__ fb, AdaptState s, const unsigned int* __restrict__ list, const unsigned int* __restrict__ count,
                                                      int32_t* __restrict__ spp, int batch, uint32_t* __restrict__ picked) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t == 0 && picked) *picked = *count;
    if (t < (long long)*count) {
        const unsigned int pid = list[t];
        const int k = s.k[pid] + batch;
        s.k[pid] = k;
        float* f = fb + (size_t)pid * 3;
        float* S = s.rgb + (size_t)pid * 3;
        const float kk = (float)(1.0 / (double)(float)k);                // vec3::operator/=(real_t), as k_render MODE 0
        S[0] = f[0]; S[1] = f[1]; S[2] = f[2];
        f[0] = sqrtf(f[0] * kk); f[1] = sqrtf(f[1] * kk); f[2] = sqrtf(f[2] * kk);
        if (spp) spp[pid] = k;
    }
}
// (cap: the capacity of the list, at least one block so that `picked` is written for an empty round)
hipError_t launch_budget_seed(float* fb, const AdaptState& s, const unsigned int* list, const unsigned int* count, unsigned int cap, hipStream_t st) {
    hipLaunchKernelGGL(k_budget_seed, dim3(cap / 256 + 1), dim3(256), 0, st, fb, s, list, count);
    return hipGetLastError();
}
hipError_t launch_budget_final(float* fb, const AdaptState& s, const unsigned int* list, const unsigned int* count, unsigned int cap, int32_t* spp, int batch,
                               uint32_t* picked, hipStream_t st) {
    hipLaunchKernelGGL(k_budget_final, dim3(cap / 256 + 1), dim3(256), 0, st, fb, s, list, count, spp, batch, picked);
    return hipGetLastError();
}

} // namespace rt
