// rt_adaptive.hip — the checks between the rounds of rt_render_adaptive, rt_render_adaptive_begin and rt_render_adaptive_refine
//  for gfx950 (MI355X, CDNA4): the stop rule of include/rt_amd.h applied to the running sums that a round of
// k_render<*, 2, *> (rt_kernels.hip) leaves behind, the finished pixels' colours, and the list of the pixels that run on.
// One thread per pixel, no ray is traced here.  Every floating-point operation is one IEEE binary32 operation (the reciprocal of the
// sample count in binary64, as k_render MODE 0 forms it); no contraction (the flags of rt_kernels.o: the Makefile).
#include <hip/hip_runtime.h>
#include "rt_device.h"
#include "rt_launch.h"
#include "rt_adapt_rule.h"

#pragma clang fp contract(off)

namespace rt {

// (the stop rule every check calls, adapt_rule: rt_adapt_rule.h — k_render<*, 3, *> applies the same function inside the render kernel)
// the wave's active lanes append their pixel to list_out, one atomic per wave — the order never changes a pixel
__device__ __forceinline__ void adapt_append(bool active, unsigned int pid, unsigned int* list_out, unsigned int* count_out) {
    const unsigned long long mask = __ballot(active);
    if (mask != 0ull) {
        unsigned int base = 0;
        if ((threadIdx.x & 63) == 0) base = atomicAdd(count_out, (unsigned int)__popcll(mask));
        base = __shfl(base, 0);
        const unsigned int rank = rank_below(mask);
        if (active) list_out[base + rank] = pid;
    }
}
// rt_render_adaptive's check after a round that left every active pixel at k samples: a pixel stops when the rule
// holds, or when the round is the last one.  A stopped pixel gets rt_render's colour at ns = k (k_render MODE 0's end_pixel: the
// reciprocal in double, then sqrtf) and its count; the others are appended to list_out.
// list_in == NULL: round 0, element t of the buffer for thread t.  In a part (a compact tile-major buffer, rt_partition) the elements
// of edge tiles that fall outside the frame are padding: round 0 never rendered them, and the check leaves them alone — no colour,
// no count, never listed (the lists hold in-frame pixels only, so later rounds need no such test).
// KEEP (rt_render_adaptive_begin): a stopped pixel also leaves its S_rgb and k in the caller's refinement state.
template <bool KEEP>
__device__ __forceinline__ void adapt_check(float* __restrict__ fb, const float* __restrict__ sl, const float* __restrict__ q,
                                            const unsigned int* __restrict__ list_in, const unsigned int* __restrict__ count_in, long long n_all,
                                            unsigned int* __restrict__ list_out, unsigned int* __restrict__ count_out, int32_t* __restrict__ spp,
                                            int k, int last, float rel_error, float floor_lum, const AdaptFrame& fr, const AdaptState& keep) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n = count_in ? (long long)*count_in : n_all;
    bool active = false;
    unsigned int pid = 0;
    bool inside = true;
    if (!list_in && t < n && !frame_whole(fr)) {                                         // (adapt_in_frame of rt_device.h, restated: with the call in its place hipcc emits
        const long long tile = part_tile(t >> 6, fr.part, fr.nparts, fr.tile_begin, fr.tile_end);      // other instruction text for k_adapt_check and k_adapt_check_keep — rounds 19 and 30)
        const int tx = (int)(tile % fr.tiles_x), ty = (int)(tile / fr.tiles_x);
        inside = tile_px(tx, (int)(t & 7)) < fr.max_x && tile_px(ty, (int)((t >> 3) & 7)) < fr.max_y;
    }
    if (t < n && inside) {
        pid = list_in ? list_in[t] : (unsigned int)t;
        bool stop = last != 0;
        if (!stop) stop = adapt_rule(sl[pid], q[pid], k, rel_error, floor_lum);
        if (stop) {
            float* f = fb + (size_t)pid * 3;
            const float kk = (float)(1.0 / (double)(float)k);                // vec3::operator/=(real_t), as k_render MODE 0
            if constexpr (KEEP) {
                float* s = keep.rgb + (size_t)pid * 3;
                s[0] = f[0]; s[1] = f[1]; s[2] = f[2];
                keep.k[pid] = k;
            }
            f[0] = sqrtf(f[0] * kk); f[1] = sqrtf(f[1] * kk); f[2] = sqrtf(f[2] * kk);
            if (spp) spp[pid] = k;
        } else {
            active = true;
        }
    }
    adapt_append(active, pid, list_out, count_out);
}
__global__ __launch_bounds__(256) void k_adapt_check(float* __restrict__ fb, const float* __restrict__ sl, const float* __restrict__ q,
                                                     const unsigned int* __restrict__ list_in, const unsigned int* __restrict__ count_in, long long n_all,
                                                     unsigned int* __restrict__ list_out, unsigned int* __restrict__ count_out, int32_t* __restrict__ spp,
                                                     int k, int last, float rel_error, float floor_lum, AdaptFrame fr) {
    adapt_check<false>(fb, sl, q, list_in, count_in, n_all, list_out, count_out, spp, k, last, rel_error, floor_lum, fr, AdaptState{});
}
__global__ __launch_bounds__(256) void k_adapt_check_keep(float* __restrict__ fb, AdaptState s,
                                                          const unsigned int* __restrict__ list_in, const unsigned int* __restrict__ count_in, long long n_all,
                                                          unsigned int* __restrict__ list_out, unsigned int* __restrict__ count_out, int32_t* __restrict__ spp,
                                                          int k, int last, float rel_error, float floor_lum, AdaptFrame fr) {
    adapt_check<true>(fb, s.sl, s.q, list_in, count_in, n_all, list_out, count_out, spp, k, last, rel_error, floor_lum, fr, s);
}

// rt_render_adaptive_refine, before its first round: one thread per buffer element (padding skipped as in round 0's check).  A pixel
// of the state stopped after k samples under the previous target; under the new one it stops there when k == max_spp or the rule
// holds — fb gets its colour again from S_rgb, d_spp its count — and otherwise goes on: fb gets S_rgb (where the resumed MODE 2 round
// reads it) and the pixel is listed.  The state itself is not written.
__global__ __launch_bounds__(256) void k_adapt_refine_seed(float* __restrict__ fb, AdaptState s, long long n_all, unsigned int* __restrict__ list_out,
                                                           unsigned int* __restrict__ count_out, int32_t* __restrict__ spp,
                                                           int max_spp, float rel_error, float floor_lum, AdaptFrame fr) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    bool active = false;
    const unsigned int pid = (unsigned int)t;
    if (t < n_all && (frame_whole(fr) || adapt_in_frame(t, fr))) {
        const int k = s.k[pid];
        const float* S = s.rgb + (size_t)pid * 3;
        float* f = fb + (size_t)pid * 3;
        if (k >= max_spp || adapt_rule(s.sl[pid], s.q[pid], k, rel_error, floor_lum)) {
            const float kk = (float)(1.0 / (double)(float)k);
            f[0] = sqrtf(S[0] * kk); f[1] = sqrtf(S[1] * kk); f[2] = sqrtf(S[2] * kk);
            if (spp) spp[pid] = k;
        } else {
            f[0] = S[0]; f[1] = S[1]; f[2] = S[2];
            active = true;
        }
    }
    adapt_append(active, pid, list_out, count_out);
}
// the check after a resumed round of rt_render_adaptive_refine: the listed pixels have taken `batch` samples more than the state's k.
// k is written back every round; a pixel stops at max_spp or when the rule holds, and is finalised as k_adapt_check_keep does.
__global__ __launch_bounds__(256) void k_adapt_refine_check(float* __restrict__ fb, AdaptState s,
                                                            const unsigned int* __restrict__ list_in, const unsigned int* __restrict__ count_in,
                                                            unsigned int* __restrict__ list_out, unsigned int* __restrict__ count_out, int32_t* __restrict__ spp,
                                                            int batch, int max_spp, float rel_error, float floor_lum) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    bool active = false;
    unsigned int pid = 0;
    if (t < (long long)*count_in) {
        pid = list_in[t];
        const int k = s.k[pid] + batch;
        s.k[pid] = k;
        if (k >= max_spp || adapt_rule(s.sl[pid], s.q[pid], k, rel_error, floor_lum)) {
            float* f = fb + (size_t)pid * 3;
            float* S = s.rgb + (size_t)pid * 3;
            const float kk = (float)(1.0 / (double)(float)k);
            S[0] = f[0]; S[1] = f[1]; S[2] = f[2];
            f[0] = sqrtf(f[0] * kk); f[1] = sqrtf(f[1] * kk); f[2] = sqrtf(f[2] * kk);
            if (spp) spp[pid] = k;
        } else {
            active = true;
        }
    }
    adapt_append(active, pid, list_out, count_out);
}
__global__ __launch_bounds__(256) void k_adapt_zero(unsigned int* p, int n) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n) p[t] = 0u;
}

hipError_t launch_adapt_check(float* fb, const float* sl, const float* q, const unsigned int* list_in, const unsigned int* count_in, long long n_all,
                              unsigned int* list_out, unsigned int* count_out, int32_t* spp, int k, bool last, float rel_error, float floor_lum,
                              const AdaptFrame& fr, hipStream_t st) {
    if (n_all <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_adapt_check, dim3((unsigned)((n_all + 255) / 256)), dim3(256), 0, st, fb, sl, q, list_in, count_in, n_all, list_out, count_out, spp,
                       k, last ? 1 : 0, rel_error, floor_lum, fr);
    return hipGetLastError();
}
hipError_t launch_adapt_check_keep(float* fb, const AdaptState& s, const unsigned int* list_in, const unsigned int* count_in, long long n_all,
                                   unsigned int* list_out, unsigned int* count_out, int32_t* spp, int k, bool last, float rel_error, float floor_lum,
                                   const AdaptFrame& fr, hipStream_t st) {
    if (n_all <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_adapt_check_keep, dim3((unsigned)((n_all + 255) / 256)), dim3(256), 0, st, fb, s, list_in, count_in, n_all, list_out, count_out, spp,
                       k, last ? 1 : 0, rel_error, floor_lum, fr);
    return hipGetLastError();
}
hipError_t launch_adapt_refine_seed(float* fb, const AdaptState& s, long long n_all, unsigned int* list_out, unsigned int* count_out, int32_t* spp,
                                    int max_spp, float rel_error, float floor_lum, const AdaptFrame& fr, hipStream_t st) {
    if (n_all <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_adapt_refine_seed, dim3((unsigned)((n_all + 255) / 256)), dim3(256), 0, st, fb, s, n_all, list_out, count_out, spp,
                       max_spp, rel_error, floor_lum, fr);
    return hipGetLastError();
}
hipError_t launch_adapt_refine_check(float* fb, const AdaptState& s, const unsigned int* list_in, const unsigned int* count_in, long long n_all,
                                     unsigned int* list_out, unsigned int* count_out, int32_t* spp, int batch, int max_spp, float rel_error, float floor_lum,
                                     hipStream_t st) {
    if (n_all <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_adapt_refine_check, dim3((unsigned)((n_all + 255) / 256)), dim3(256), 0, st, fb, s, list_in, count_in, list_out, count_out, spp,
                       batch, max_spp, rel_error, floor_lum);
    return hipGetLastError();
}
hipError_t launch_adapt_zero(unsigned int* p, int n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_adapt_zero, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, n);
    return hipGetLastError();
}

} // namespace rt
