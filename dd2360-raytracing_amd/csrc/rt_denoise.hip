// rt_denoise.hip — the edge-avoiding à-trous filter of rt_denoise (include/rt_amd.h): no reference counterpart.
//
// One prepare launch turns the input frame into linear colour (float4 per pixel in the caller's workspace, .w = 1 for a pixel that is
// filtered, 0 for a pass-through pixel whose .xyz already hold its display value), then one launch per level.  A level's block is a
// 16x16 pixel tile, one lane per pixel; the 25 taps read colour as one float4 and the guide as the two 16-byte halves of the 32-byte
// rt_hit_record, straight through the caches.  Levels ping-pong between the workspace's two buffers; the last one writes fb_out.
// No atomics, no LDS, no grid-wide synchronisation: levels are ordered by the stream.
//
// rt_denoise_adaptive (the variance-guided filter on the adaptive state) has kernels of its own below, k_denoise_var_prepare and
// k_denoise_var_level: the same launches and workspace, .w = the variance of the pixel's mean luminance (negative = pass-through).
// Its level kernel stages the tile and its apron in LDS for the steps 1 and 2 and reads through the caches for larger steps.
// What these kernels compute per pixel — the moments of a state element, the terms of a tap, one level for one pixel, the staged
// tile — is written once in rt_filter.h, which the filtered budget key (rt_budget.hip) and temporal accumulation (rt_temporal.h)
// share; the kernels here are the launch shapes around those rules.
//
// Numeric contract: one IEEE binary32 rounding per operation in the order the header states, no contraction (also on the command
// line), correctly rounded division and sqrt (hipcc default), sums in tap order — tests/denoise_model.py reproduces it bit for bit.
#include <hip/hip_runtime.h>
#include "../../include/rt_amd.h"
#include "rt_device.h"
#include "rt_filter.h"
#include "rt_launch.h"

#pragma clang fp contract(off)

namespace rt {

struct DenoiseLevel {
    int32_t h;             // tap step 2^L
    int32_t npow;          // normal_pow_log2 (-1 = no normal term)
    int32_t use_pos, use_col;
    float inv_sp2;         // 1 / sigma_position^2
    float col_scale;       // 4^L / sigma_color^2
};

// linear colour and the pass-through mark of every pixel (one lane per pixel, row-major)
__global__ __launch_bounds__(256) void k_denoise_prepare(float4* x, const float* fb_in, const rt_hit_record* hits, int n, int input, float samples) {
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;                  // (n <= 2^30: p + 255 fits an int)
    if (p >= n) return;
    const long long e = 3 * (long long)p;                                     // (3 * p does not: 64-bit colour offsets)
    const float c0 = fb_in[e], c1 = fb_in[e + 1], c2 = fb_in[e + 2];
    float4 v;
    if (input == RT_DENOISE_INPUT_GAMMA) { v.x = c0 * c0; v.y = c1 * c1; v.z = c2 * c2; }
    else { v.x = c0 / samples; v.y = c1 / samples; v.z = c2 / samples; }
    v.w = 1.0f;
    if (hits[p].sphere == -1 || !__builtin_isfinite(v.x) || !__builtin_isfinite(v.y) || !__builtin_isfinite(v.z)) {
        // the display value, as the input has it: GAMMA the bits of fb_in, SUM sqrt(fb / n)
        if (input == RT_DENOISE_INPUT_GAMMA) { v.x = c0; v.y = c1; v.z = c2; }
        else { v.x = sqrtf(v.x); v.y = sqrtf(v.y); v.z = sqrtf(v.z); }
        v.w = 0.0f;
    }
    x[p] = v;
}

// one level: y_p = sum(w * x_q) / sum(w) over the 5x5 taps q = p + h*(dx, dy), dy outer, both from -2 (rt_amd.h states w)
template <bool LAST>
__global__ __launch_bounds__(256) void k_denoise_level(const float4* __restrict__ x, float4* __restrict__ y, float* __restrict__ fb_out,
                                                       const float4* __restrict__ g, int max_x, int max_y, int tiles_x, DenoiseLevel L) {
    const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)(blockIdx.x / (unsigned)tiles_x);
    const int i = tx * 16 + (int)(threadIdx.x & 15), j = ty * 16 + (int)(threadIdx.x >> 4);
    if (i >= max_x || j >= max_y) return;
    const int p = j * max_x + i;
    const float4 xp = x[p];
    float4 out = xp;
    if (xp.w != 0.0f) {
        const float4 gp0 = g[2 * p], gp1 = g[2 * p + 1];          // (t, P) and (N, sphere)
        const int sp = __float_as_int(gp1.w);
        const float tt = gp0.x * gp0.x;
        float sw = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
            const int qj = j + L.h * dy;
            if (qj < 0 || qj >= max_y) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int qi = i + L.h * dx;
                if (qi < 0 || qi >= max_x) continue;
                const int q = qj * max_x + qi;
                const float4 xq = x[q];
                if (xq.w == 0.0f) continue;                         // a pass-through pixel is never a tap
                const float4 gq1 = g[2 * q + 1];
                if (__float_as_int(gq1.w) != sp) continue;          // another sphere (the sky is pass-through already)
                const float wn = tap_normal_weight(gp1, gq1, L.npow);
                const float apos = L.use_pos ? tap_position_term(gp0, &g[2 * q], tt, L.inv_sp2) : 0.0f;
                float acol = 0.0f;
                if (L.use_col) {
                    const float cx = xp.x - xq.x, cy = xp.y - xq.y, cz = xp.z - xq.z;
                    acol = ((cx * cx + cy * cy) + cz * cz) * L.col_scale;
                }
                const float w = (tap_kernel(dx, dy) * wn) / ((1.0f + apos) * (1.0f + acol));
                sw = sw + w;
                s0 = s0 + w * xq.x; s1 = s1 + w * xq.y; s2 = s2 + w * xq.z;
            }
        }
        out.x = s0 / sw; out.y = s1 / sw; out.z = s2 / sw;
    }
    if (LAST) {
        float* o = fb_out + 3 * (long long)p;
        if (xp.w != 0.0f) { o[0] = sqrtf(out.x); o[1] = sqrtf(out.y); o[2] = sqrtf(out.z); }
        else { o[0] = out.x; o[1] = out.y; o[2] = out.z; }
    } else {
        y[p] = out;
    }
}

// the whole filter on `st`; the arguments have been checked by rt_denoise (16-byte aligned hits and work; max_x * max_y <= 2^30, so that
// the pixel index p, the guide index 2 * p + 1 and a tap's i + 2h, j + 2h fit an int — the colour offsets 3 * p + c do not, and are
// computed in 64 bits)
hipError_t launch_denoise(float* fb_out, const float* fb_in, int max_x, int max_y, const rt_hit_record* hits, const rt_denoise_params& P,
                          float4* work, hipStream_t st) {
    const int n = max_x * max_y;
    hipLaunchKernelGGL(k_denoise_prepare, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, work, fb_in, hits, n, (int)P.input, (float)P.samples);
    const int tiles_x = (max_x + 15) / 16, tiles_y = (max_y + 15) / 16;
    const unsigned blocks = (unsigned)tiles_x * (unsigned)tiles_y;
    const float sp2 = P.sigma_position * P.sigma_position, sc2 = P.sigma_color * P.sigma_color;
    for (int l = 0; l < P.levels; ++l) {
        DenoiseLevel L;
        L.h = 1 << l;
        L.npow = P.normal_pow_log2;
        L.use_pos = P.sigma_position > 0.0f;
        L.use_col = P.sigma_color > 0.0f;
        L.inv_sp2 = L.use_pos ? 1.0f / sp2 : 0.0f;
        L.col_scale = L.use_col ? (float)(1 << (2 * l)) / sc2 : 0.0f;
        const float4* src = work + (size_t)(l & 1) * (size_t)n;
        float4* dst = work + (size_t)((l + 1) & 1) * (size_t)n;
        if (l == P.levels - 1) hipLaunchKernelGGL(k_denoise_level<true>, dim3(blocks), dim3(256), 0, st, src, dst, fb_out, (const float4*)hits, max_x, max_y, tiles_x, L);
        else hipLaunchKernelGGL(k_denoise_level<false>, dim3(blocks), dim3(256), 0, st, src, dst, fb_out, (const float4*)hits, max_x, max_y, tiles_x, L);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

// ---- rt_denoise_adaptive: variance-guided weights from the adaptive state (rt_amd.h) ------------------------------------
// Steps up to this one take the LDS form of the level kernel (tools/mkvariant.sh -DRT_DENOISE_VAR_LDS_MAX_STEP=0: the plain form
// everywhere, for the A/B of DESIGN.md §5.10; both forms compute the same bits)
#ifndef RT_DENOISE_VAR_LDS_MAX_STEP
#define RT_DENOISE_VAR_LDS_MAX_STEP 2
#endif

// (DenoiseVarLevel, one level's parameters: rt_device.h)

// mean colour and the variance of the mean luminance of every pixel, from the state (one lane per pixel, row-major); a pass-through
// pixel holds the bits of fb_in and .w = -1 (a kept variance is never negative)
__global__ __launch_bounds__(256) void k_denoise_var_prepare(float4* x, const float* fb_in, const rt_hit_record* hits, AdaptState S, int n) {
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (p >= n) return;
    const StateMoments m = state_moments(S, p);
    float4 v = m.c;
    if (state_pass_through(m, hits[p].sphere)) {
        const long long e = 3 * (long long)p;
        v.x = fb_in[e]; v.y = fb_in[e + 1]; v.z = fb_in[e + 2];
        v.w = -1.0f;
    }
    x[p] = v;
}

// one level (filter_level_pixel of rt_filter.h, where the LDS layout is argued).  H == 0: the plain form, taps through the caches at
// step L.h.  H == 1, 2: step H with the 16x16 tile and its apron of 2H pixels staged in LDS from the level's input.
template <bool LAST, int H>
__global__ __launch_bounds__(256) void k_denoise_var_level(const float4* __restrict__ x, float4* __restrict__ y, float* __restrict__ fb_out,
                                                           const float4* __restrict__ g, int max_x, int max_y, int tiles_x, DenoiseVarLevel L) {
    __shared__ float4 sx[filter_tile_slots(H)], sg0[filter_tile_slots(H)], sg1[filter_tile_slots(H)];
    const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)(blockIdx.x / (unsigned)tiles_x);
    const int li = (int)(threadIdx.x & 15), lj = (int)(threadIdx.x >> 4);
    const int i = tx * 16 + li, j = ty * 16 + lj;
    if constexpr (H != 0) {
        filter_stage_tile<H>(sx, sg0, sg1, g, tx, ty, max_x, max_y, [x](int q) { return x[q]; });
        __syncthreads();
    }
    if (i >= max_x || j >= max_y) return;
    const int p = j * max_x + i;
    const int c = filter_tile_centre<H>(li, lj);                   // (H != 0)
    const float4 xp = H ? sx[c] : x[p];
    float4 out = xp;
    const bool keep = xp.w < 0.0f;                                  // pass-through
    if (!keep) out = filter_level_pixel<H>(x, g, sx, sg0, sg1, c, i, j, max_x, max_y, xp, L);
    if (LAST) {
        float* o = fb_out + 3 * (long long)p;
        if (!keep) { o[0] = sqrtf(out.x); o[1] = sqrtf(out.y); o[2] = sqrtf(out.z); }
        else { o[0] = out.x; o[1] = out.y; o[2] = out.z; }
    } else {
        y[p] = out;
    }
}

template <int H>
static void launch_var_level(bool last, unsigned blocks, hipStream_t st, const float4* src, float4* dst, float* fb_out, const float4* g, int max_x,
                             int max_y, int tiles_x, const DenoiseVarLevel& L) {
    if (last) hipLaunchKernelGGL((k_denoise_var_level<true, H>), dim3(blocks), dim3(256), 0, st, src, dst, fb_out, g, max_x, max_y, tiles_x, L);
    else hipLaunchKernelGGL((k_denoise_var_level<false, H>), dim3(blocks), dim3(256), 0, st, src, dst, fb_out, g, max_x, max_y, tiles_x, L);
}

// the levels of the filter on a prepared workspace (its first float4 buffer: mean colour and variance, .w < 0 = pass-through): shared by
// rt_denoise_adaptive and rt_denoise_history (rt_temporal.hip), whose prepare kernels differ
hipError_t launch_denoise_var_levels(float* fb_out, int max_x, int max_y, const rt_hit_record* hits, const rt_denoise_var_params& P, float4* work,
                                     hipStream_t st) {
    const int n = max_x * max_y;
    const int tiles_x = (max_x + 15) / 16, tiles_y = (max_y + 15) / 16;
    const unsigned blocks = (unsigned)tiles_x * (unsigned)tiles_y;
    for (int l = 0; l < P.levels; ++l) {
        const DenoiseVarLevel L = denoise_var_level(P, l);
        const float4* src = work + (size_t)(l & 1) * (size_t)n;
        float4* dst = work + (size_t)((l + 1) & 1) * (size_t)n;
        const bool last = l == P.levels - 1;
        if (L.h == 1 && RT_DENOISE_VAR_LDS_MAX_STEP >= 1) launch_var_level<1>(last, blocks, st, src, dst, fb_out, (const float4*)hits, max_x, max_y, tiles_x, L);
        else if (L.h == 2 && RT_DENOISE_VAR_LDS_MAX_STEP >= 2) launch_var_level<2>(last, blocks, st, src, dst, fb_out, (const float4*)hits, max_x, max_y, tiles_x, L);
        else launch_var_level<0>(last, blocks, st, src, dst, fb_out, (const float4*)hits, max_x, max_y, tiles_x, L);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

// the whole filter on `st`; the arguments have been checked by rt_denoise_adaptive (as launch_denoise's; `state` is only read)
hipError_t launch_denoise_var(float* fb_out, const float* fb_in, int max_x, int max_y, const rt_hit_record* hits, const void* state,
                              const rt_denoise_var_params& P, float4* work, hipStream_t st) {
    const int n = max_x * max_y;
    hipLaunchKernelGGL(k_denoise_var_prepare, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, work, fb_in, hits,
                       adapt_state(const_cast<void*>(state), (long long)n), n);
    return launch_denoise_var_levels(fb_out, max_x, max_y, hits, P, work, st);
}

} // namespace rt
