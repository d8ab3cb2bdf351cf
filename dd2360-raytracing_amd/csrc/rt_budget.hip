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
// Which key ranks the pixels is the caller's BudgetKey (rt_launch.h); launch_budget_select is the one launcher.  The three key kernels
// differ in the priority of a pixel and share their tail (budget_key_store, budget_key_count) and the block histogram (budget_hist_begin, _flush).
// The filter-aware budget (rt_adaptive_budget_select_filtered, DESIGN.md §5.9 "Filter-aware priority") replaces k_budget_keys by
//   k_budget_keys_filtered   per 16x16 tile: the state's (x, v) of the tile and its apron staged in LDS, level 0 of rt_denoise_adaptive
//                            on them, the key of the filtered pixel (rt_adaptive_priority_filtered) and the histogram of the top digit
// and leaves the other launches as they are.  The moments, the staged tile and the level are the denoiser's own functions (rt_filter.h):
// the key is what k_denoise_var_prepare and k_denoise_var_level<false, 1> would leave, by construction.
// The history-aware budget (rt_adaptive_budget_select_temporal, DESIGN.md §5.9 "History-aware priority") replaces it by
//   k_budget_keys_temporal   per 16x16 tile, one lane per pixel: what rt_temporal_accumulate would write for the pixel (temporal_pixel of
//                            rt_temporal.h: the reprojection, four gathered taps, the merge), the key of the merged pixel and the
//                            histogram of the top digit
// and again leaves the other launches as they are.
#include <hip/hip_runtime.h>
#include "rt_device.h"
#include "rt_filter.h"
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

// The block histogram of a key kernel: zeroed and published, and after the block's last element added to the top digit's histogram
// (hist == NULL: none is kept), one global add per bin that is not empty.
__device__ __forceinline__ void budget_hist_begin(unsigned int* sh_hist) {
    sh_hist[threadIdx.x] = 0u;
    __syncthreads();
}
__device__ __forceinline__ void budget_hist_flush(const unsigned int* sh_hist, unsigned int* __restrict__ hist) {
    __syncthreads();
    const unsigned int c = sh_hist[threadIdx.x];
    if (hist && c) atomicAdd(&hist[threadIdx.x], c);
}
// The tail of a key kernel.  For a lane that holds element t: the priority before the mask to keys_out (may be NULL) and the key bits
// to keys — 0 for an element that is not eligible, which is never picked.  Then for every lane of the block (valid: the lane holds
// an element; the others still take part in the wave's ballots): the count of the key's top digit.
__device__ __forceinline__ bool budget_eligible(int k, int batch, int max_spp) { return (long long)k + batch <= (long long)max_spp; }
__device__ __forceinline__ unsigned int budget_key_store(long long t, float pr, bool eligible, unsigned int* __restrict__ keys, float* __restrict__ keys_out) {
    if (keys_out) keys_out[t] = pr;
    const unsigned int key = eligible ? __float_as_uint(pr) : 0u;
    keys[t] = key;
    return key;
}
__device__ __forceinline__ void budget_key_count(bool valid, unsigned int key, unsigned int* __restrict__ hist, unsigned int* sh_hist) {
    if (hist) budget_hist_add(valid, key >> 24, sh_hist);
}

// One thread per element: the key bits of rt_adaptive_priority, 0 for an element that is not eligible (padding of an edge tile,
// k + batch > max_spp, key 0) — key 0 is never picked.  hist != NULL: the histogram of the top digit.
__global__ __launch_bounds__(256) void k_budget_keys(AdaptState s, long long n, long long span, AdaptFrame fr, int batch, int max_spp, float floor_lum,
                                                     unsigned int* __restrict__ keys, unsigned int* __restrict__ hist) {
    __shared__ unsigned int sh_hist[256];
    budget_hist_begin(sh_hist);
    const bool whole = part_whole(fr.nparts, fr.tile_begin, fr.tile_end);
    const long long begin = (long long)blockIdx.x * span;
    for (long long o = 0; o < span && begin + o < n; o += 256) {
        const long long t = begin + o + threadIdx.x;
        const bool valid = t < n;
        unsigned int key = 0u;
        if (valid) {
            float pr = 0.0f;
            bool take = false;
            if (whole || adapt_in_frame(t, fr)) {
                const int k = s.k[t];
                take = budget_eligible(k, batch, max_spp);
                if (take) pr = adapt_priority(s.sl[t], s.q[t], k, floor_lum);
            }
            key = budget_key_store(t, pr, take, keys, nullptr);
        }
        budget_key_count(valid, key, hist, sh_hist);
    }
    budget_hist_flush(sh_hist, hist);
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
            unsigned int rank = run + rank_below(m);
            for (int ww = 0; ww < w; ++ww) rank += sh[ww];
            run += (sh[0] + sh[1]) + (sh[2] + sh[3]);
            pick = pick || (tie && rank < need);
        }
        const unsigned long long mp = __ballot(pick);
        if ((threadIdx.x & 63) == 0) sh[4 + w] = (unsigned int)__popcll(mp);
        __syncthreads();
        unsigned int pos = at + rank_below(mp);
        for (int ww = 0; ww < w; ++ww) pos += sh[4 + ww];
        at += (sh[4] + sh[5]) + (sh[6] + sh[7]);
        if (pick && pos < K) list[pos] = (unsigned int)t;     // (the set never exceeds K: the list's capacity is not left to that proof)
        __syncthreads();
    }
}

// bytes of the selection workspace (for a state of any size)
size_t budget_ws_bytes() { return sizeof(unsigned int) * (size_t)kBudgetWsWords; }
// A selection is: budget_select_begin, one launch that writes the n key words and adds the histogram of their top digit to `hist`,
// budget_select_finish.
static hipError_t budget_select_begin(unsigned int* ws, unsigned int*& hist, hipStream_t st) {
    hist = ws;
    return hipMemsetAsync(hist, 0, sizeof(unsigned int) * kBudgetHistWords, st);
}
static hipError_t budget_select_finish(long long n, unsigned int K, unsigned int* keys, unsigned int* ws, unsigned int* list, unsigned int* count, hipStream_t st) {
    const long long span = budget_span(n);
    const unsigned nblk = (unsigned)((n + span - 1) / span);          // <= kBudgetMaxBlocks
    unsigned int* hist = ws; unsigned int* sel = ws + kBudgetHistWords; unsigned int* blk_tie = sel + kBudgetSelWords; unsigned int* blk_above = blk_tie + kBudgetMaxBlocks;
    for (int pass = 1; pass < 4; ++pass) hipLaunchKernelGGL(k_budget_hist, dim3(nblk), dim3(256), 0, st, keys, n, span, K, hist, pass);
    hipLaunchKernelGGL(k_budget_ties, dim3(nblk), dim3(256), 0, st, keys, n, span, K, hist, blk_tie, blk_above);
    hipLaunchKernelGGL(k_budget_scan, dim3(1), dim3(256), 0, st, hist, K, blk_tie, blk_above, (int)nblk, sel, count);
    hipLaunchKernelGGL(k_budget_compact, dim3(nblk), dim3(256), 0, st, keys, n, span, sel, blk_tie, blk_above, list, K);
    return hipGetLastError();
}

// ---- the keys of whole row-major frames (FILTERED, TEMPORAL) -------------------------------------------------------------------------
// Frames of at most RT_DENOISE_MAX_PIXELS pixels: a pixel index, 2 * p + 1 and a tile count fit an int, 3 * p does not.  A block owns
// `per` consecutive 16x16 tiles (at most kBudgetMaxBlocks blocks: one global add per bin and block, as k_budget_keys), one lane per pixel.
struct BudgetTiles { int tiles_x, tiles, per; unsigned nblk; };
static BudgetTiles budget_tiles(int max_x, int max_y) {
    BudgetTiles G;
    G.tiles_x = (max_x + 15) / 16;
    G.tiles = G.tiles_x * ((max_y + 15) / 16);                        // (<= 2^30 / 256 + two edges: fits)
    G.per = (G.tiles + kBudgetMaxBlocks - 1) / kBudgetMaxBlocks;
    G.nblk = (unsigned)((G.tiles + G.per - 1) / G.per);               // <= kBudgetMaxBlocks, every block owns at least one tile
    return G;
}

// The filter-aware key (rt_amd.h, rt_adaptive_budget_select_filtered).  Per tile: the tile and its apron of 2 in the LDS layout of
// k_denoise_var_level<*, 1> (filter_stage_tile, rt_filter.h: 30 KB, + 1 KB of histogram: four blocks a CU), but filled straight from the
// state: every staged pixel computes k_denoise_var_prepare's (x, v) and pass-through mark itself (a pixel of the apron is computed by up
// to four tiles; 144 of 400 per tile, against a float4 written and read back per pixel).  Then one lane per pixel: level 0 of the
// filter as that kernel writes it (filter_level_pixel<1>), the key of the filtered pixel, and the tail.
__global__ __launch_bounds__(256) void k_budget_keys_filtered(AdaptState s, const float4* __restrict__ g, int max_x, int max_y, int tiles_x, int tiles, int per,
                                                              DenoiseVarLevel L, int batch, int max_spp, float floor_lum, unsigned int* __restrict__ keys,
                                                              float* __restrict__ keys_out, unsigned int* __restrict__ hist) {
    __shared__ float4 sx[filter_tile_slots(1)], sg0[filter_tile_slots(1)], sg1[filter_tile_slots(1)];
    __shared__ unsigned int sh_hist[256];
    budget_hist_begin(sh_hist);
    const int li = (int)(threadIdx.x & 15), lj = (int)(threadIdx.x >> 4);
    const int c = filter_tile_centre<1>(li, lj);
    const int first = (int)blockIdx.x * per;
    const int last = first + per < tiles ? first + per : tiles;
    for (int tile = first; tile < last; ++tile) {
        const int tx = tile % tiles_x, ty = tile / tiles_x;
        filter_stage_tile<1>(sx, sg0, sg1, g, tx, ty, max_x, max_y, [&](int q) {
            const StateMoments m = state_moments(s, q);
            const float4 g1 = g[2 * q + 1];
            return state_pass_through(m, __float_as_int(g1.w)) ? make_float4(0.0f, 0.0f, 0.0f, -1.0f) : m.c;
        });
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
                const float4 y = filter_level_pixel<1>(nullptr, nullptr, sx, sg0, sg1, c, i, j, max_x, max_y, xp, L);
                pr = adapt_priority_filtered((y.x + y.y) + y.z, y.w, floor_lum);
            }
            key = budget_key_store(p, pr, budget_eligible(k, batch, max_spp), keys, keys_out);
        }
        budget_key_count(inside, key, hist, sh_hist);
        __syncthreads();                                             // the tile has been read: the next one may be staged
    }
    budget_hist_flush(sh_hist, hist);
}

// The history-aware key (rt_amd.h, rt_adaptive_budget_select_temporal).  The pixel is ranked by what rt_temporal_accumulate would leave
// of it: temporal_pixel (rt_temporal.h) is that kernel's own body — the state, both guide halves, the reprojection through the previous
// camera, the four taps' loads issued before any of them is tested, the merge — so the rule exists once.  The taps go straight through
// the caches: where a tile lands in the last frame depends on the camera, there is no fixed apron to stage.  A pixel without anything
// accumulated (neff == 0: EMPTY) keeps the raw key, as in k_budget_keys_filtered.  LDS: the 256-word histogram alone.
__global__ __launch_bounds__(256) void k_budget_keys_temporal(TemporalArgs T, int tiles, int per, int batch, int max_spp, float floor_lum,
                                                              unsigned int* __restrict__ keys, float* __restrict__ keys_out, unsigned int* __restrict__ hist) {
    __shared__ unsigned int sh_hist[256];
    budget_hist_begin(sh_hist);
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
            key = budget_key_store(p, pr, budget_eligible(R.k, batch, max_spp), keys, keys_out);
        }
        budget_key_count(inside, key, hist, sh_hist);
    }
    budget_hist_flush(sh_hist, hist);
}

// The K (<= n) elements of the state with the largest keys into list, their number into *count.  key says which key ranks them and
// holds that key's inputs, all checked by the caller (rt_launch.h).  keys: n words, ws: budget_ws_bytes().  fr: the frame and the
// part the n elements belong to (FILTERED and TEMPORAL: the whole row-major frame, n = fr.max_x * fr.max_y).
hipError_t launch_budget_select(const BudgetKey& key, const void* state, long long n, const AdaptFrame& fr, int batch, int max_spp, float floor_lum,
                                unsigned int K, unsigned int* keys, unsigned int* ws, unsigned int* list, unsigned int* count, hipStream_t st) {
    unsigned int* hist;
    const hipError_t e = budget_select_begin(ws, hist, st);
    if (e != hipSuccess) return e;
    const AdaptState s = adapt_state(const_cast<void*>(state), n);
    if (key.rank == BudgetKey::RAW) {
        const long long span = budget_span(n);
        const unsigned nblk = (unsigned)((n + span - 1) / span);      // <= kBudgetMaxBlocks
        hipLaunchKernelGGL(k_budget_keys, dim3(nblk), dim3(256), 0, st, s, n, span, fr, batch, max_spp, floor_lum, keys, hist);
    } else {
        const BudgetTiles G = budget_tiles(fr.max_x, fr.max_y);
        if (key.rank == BudgetKey::FILTERED) {
            hipLaunchKernelGGL(k_budget_keys_filtered, dim3(G.nblk), dim3(256), 0, st, s, (const float4*)key.hits, fr.max_x, fr.max_y, G.tiles_x, G.tiles, G.per,
                               denoise_var_level(*key.filter, 0), batch, max_spp, floor_lum, keys, key.keys_out, hist);
        } else {
            const rt_temporal_inputs& in = *key.in;
            const TemporalArgs T = temporal_args(nullptr, in.d_hist_in, in.d_hits, in.d_hits_prev, in.cam_prev, state, key.kind, key.n_kind, fr.max_x,
                                                 fr.max_y, *key.temporal);
            hipLaunchKernelGGL(k_budget_keys_temporal, dim3(G.nblk), dim3(256), 0, st, T, G.tiles, G.per, batch, max_spp, floor_lum, keys, key.keys_out, hist);
        }
    }
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
