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
//
// Numeric contract: one IEEE binary32 rounding per operation in the order the header states, no contraction (also on the command
// line), correctly rounded division and sqrt (hipcc default), sums in tap order — tests/denoise_model.py reproduces it bit for bit.
#include <hip/hip_runtime.h>
#include "../../include/rt_amd.h"
#include "rt_device.h"
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
        const float k[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
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
                float wn = 1.0f;
                if (L.npow >= 0) {
                    const float d = (gp1.x * gq1.x + gp1.y * gq1.y) + gp1.z * gq1.z;
                    wn = d > 0.0f ? d : 0.0f;
                    for (int e = 0; e < L.npow; ++e) wn = wn * wn;
                }
                float apos = 0.0f;
                if (L.use_pos) {
                    const float4 gq0 = g[2 * q];
                    const float ex = gp0.y - gq0.y, ey = gp0.z - gq0.z, ez = gp0.w - gq0.w;
                    apos = (((ex * ex + ey * ey) + ez * ez) / tt) * L.inv_sp2;
                }
                float acol = 0.0f;
                if (L.use_col) {
                    const float cx = xp.x - xq.x, cy = xp.y - xq.y, cz = xp.z - xq.z;
                    acol = ((cx * cx + cy * cy) + cz * cz) * L.col_scale;
                }
                const float w = (k[dx + 2] * k[dy + 2] * wn) / ((1.0f + apos) * (1.0f + acol));
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
    const long long e = 3 * (long long)p;
    const int k = S.k[p];
    const float nf = (float)k;
    float4 v;
    v.x = S.rgb[e] / nf; v.y = S.rgb[e + 1] / nf; v.z = S.rgb[e + 2] / nf;
    const float sl = S.sl[p];
    float d = nf * S.q[p] - sl * sl;
    d = d > 0.0f ? d : 0.0f;
    v.w = d / ((nf * nf) * (nf - 1.0f));
    if (hits[p].sphere == -1 || k < 2 || !__builtin_isfinite(v.x) || !__builtin_isfinite(v.y) || !__builtin_isfinite(v.z) || !__builtin_isfinite(v.w)) {
        v.x = fb_in[e]; v.y = fb_in[e + 1]; v.z = fb_in[e + 2];
        v.w = -1.0f;
    }
    x[p] = v;
}

// one level.  H == 0: the plain form, taps through the caches at step L.h.  H == 1, 2: step H with the 16x16 tile and its apron of 2H
// pixels staged in LDS — colour and both guide halves, 48 bytes a pixel, S = 16 + 4H rows of 32 16-byte slots each: a wave's
// ds_read_b128 is served in groups of 16 lanes that span two tile rows (8 + 8 columns), and a row stride of 32 slots puts those 16
// slots on 16 different bank quads for every tap offset (the natural strides 20 and 24 would collide 2-way).  20 x 32 x 48 B = 30 KB
// (H = 1) and 24 x 32 x 48 B = 36 KB (H = 2) of the CU's 160 KB: four blocks a CU.  Pixels outside the frame are staged as
// pass-through, so a tap needs no bounds test.  The blur of the centre's variance reaches +-1 at step 1: inside the apron.
template <bool LAST, int H>
__global__ __launch_bounds__(256) void k_denoise_var_level(const float4* __restrict__ x, float4* __restrict__ y, float* __restrict__ fb_out,
                                                           const float4* __restrict__ g, int max_x, int max_y, int tiles_x, DenoiseVarLevel L) {
    constexpr int S = 16 + 4 * H, ST = 32;
    __shared__ float4 sx[H ? S * ST : 1], sg0[H ? S * ST : 1], sg1[H ? S * ST : 1];
    const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)(blockIdx.x / (unsigned)tiles_x);
    const int li = (int)(threadIdx.x & 15), lj = (int)(threadIdx.x >> 4);
    const int i = tx * 16 + li, j = ty * 16 + lj;
    if constexpr (H != 0) {
        const int i0 = tx * 16 - 2 * H, j0 = ty * 16 - 2 * H;
        for (int e = (int)threadIdx.x; e < S * S; e += 256) {
            const int ej = e / S, ei = e - ej * S;
            const int qi = i0 + ei, qj = j0 + ej;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
            if (qi >= 0 && qi < max_x && qj >= 0 && qj < max_y) {
                const int q = qj * max_x + qi;
                v = x[q];
                if (!(v.w < 0.0f)) { sg0[ej * ST + ei] = g[2 * q]; sg1[ej * ST + ei] = g[2 * q + 1]; }
            }
            sx[ej * ST + ei] = v;
        }
        __syncthreads();
    }
    if (i >= max_x || j >= max_y) return;
    const int p = j * max_x + i;
    const int c = (lj + 2 * H) * ST + li + 2 * H;                  // the centre's slot (H != 0)
    const float4 xp = H ? sx[c] : x[p];
    float4 out = xp;
    const bool keep = xp.w < 0.0f;                                  // pass-through
    if (!keep) {
        const float4 gp0 = H ? sg0[c] : g[2 * p], gp1 = H ? sg1[c] : g[2 * p + 1];       // (t, P) and (N, sphere)
        const int sp = __float_as_int(gp1.w);
        const float tt = gp0.x * gp0.x;
        // the centre's variance: its own, or the 3x3 blur at step 1 over the pixels that could be its taps
        float vb = xp.w;
        if (L.prefilter) {
            const float k3[3] = {0.25f, 0.5f, 0.25f};
            float sg = 0.0f, sv = 0.0f;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const int qj = j + dy;
                if (!H && (qj < 0 || qj >= max_y)) continue;
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int qi = i + dx;
                    if (!H && (qi < 0 || qi >= max_x)) continue;
                    const int q = qj * max_x + qi, s = c + dy * ST + dx;
                    const float4 xq = H ? sx[s] : x[q];
                    if (xq.w < 0.0f) continue;
                    const float sq = H ? sg1[s].w : g[2 * q + 1].w;
                    if (__float_as_int(sq) != sp) continue;
                    const float gw = k3[dx + 1] * k3[dy + 1];
                    sg = sg + gw;
                    sv = sv + gw * xq.w;
                }
            }
            vb = sv / sg;
        }
        const float den = L.sv2 * vb + RT_DENOISE_VAR_EPS;
        const float lp = (xp.x + xp.y) + xp.z;
        const int h = H ? H : L.h;
        const float k[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
        float sw = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
            const int qj = j + h * dy;
            if (!H && (qj < 0 || qj >= max_y)) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int qi = i + h * dx;
                if (!H && (qi < 0 || qi >= max_x)) continue;
                const int q = qj * max_x + qi, s = c + (dy * H) * ST + dx * H;
                const float4 xq = H ? sx[s] : x[q];
                if (xq.w < 0.0f) continue;                          // a pass-through pixel (or one outside the frame) is never a tap
                const float4 gq1 = H ? sg1[s] : g[2 * q + 1];
                if (__float_as_int(gq1.w) != sp) continue;          // another sphere
                float wn = 1.0f;
                if (L.npow >= 0) {
                    const float d = (gp1.x * gq1.x + gp1.y * gq1.y) + gp1.z * gq1.z;
                    wn = d > 0.0f ? d : 0.0f;
                    for (int e = 0; e < L.npow; ++e) wn = wn * wn;
                }
                float apos = 0.0f;
                if (L.use_pos) {
                    const float4 gq0 = H ? sg0[s] : g[2 * q];
                    const float ex = gp0.y - gq0.y, ey = gp0.z - gq0.z, ez = gp0.w - gq0.w;
                    apos = (((ex * ex + ey * ey) + ez * ez) / tt) * L.inv_sp2;
                }
                float avar = 0.0f;
                if (L.use_var) {
                    const float dl = lp - ((xq.x + xq.y) + xq.z);
                    avar = (dl * dl) / den;
                }
                const float w = (k[dx + 2] * k[dy + 2] * wn) / ((1.0f + apos) * (1.0f + avar));
                sw = sw + w;
                s0 = s0 + w * xq.x; s1 = s1 + w * xq.y; s2 = s2 + w * xq.z;
                s3 = s3 + (w * w) * xq.w;
            }
        }
        out.x = s0 / sw; out.y = s1 / sw; out.z = s2 / sw;
        out.w = s3 / (sw * sw);
    }
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

#ifdef RT_BUDGET_FILTER_UNFUSED
// -DRT_BUDGET_FILTER_UNFUSED (tools/mkvariant.sh): the inputs of the filtered budget key from the kernels above, unchanged — prepare,
// then level 0 into the second half of `work` (RT_DENOISE_WORK_BYTES a pixel): (y, v') of every filtered pixel, .w < 0 for a
// pass-through pixel.  The cross-check and the A/B baseline of k_budget_keys_filtered (rt_budget.hip); fb_in is any 3n readable floats.
hipError_t launch_denoise_var_level0(const float* fb_in, int max_x, int max_y, const rt_hit_record* hits, const void* state,
                                     const rt_denoise_var_params& P, float4* work, hipStream_t st) {
    const int n = max_x * max_y;
    hipLaunchKernelGGL(k_denoise_var_prepare, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, work, fb_in, hits,
                       adapt_state(const_cast<void*>(state), (long long)n), n);
    const int tiles_x = (max_x + 15) / 16, tiles_y = (max_y + 15) / 16;
    launch_var_level<1>(false, (unsigned)tiles_x * (unsigned)tiles_y, st, work, work + (size_t)n, nullptr, (const float4*)hits, max_x, max_y, tiles_x,
                        denoise_var_level(P, 0));
    return hipGetLastError();
}
#endif

} // namespace rt
