// rt_filter.h — the per-pixel rules of the variance-guided filter and of what feeds it (include/rt_amd.h), each ONCE:
//   state_moments, state_pass_through   the "per pixel" line of rt_denoise_adaptive: k_denoise_var_prepare (rt_denoise.hip) writes it,
//                                       k_budget_keys_filtered (rt_budget.hip) stages it, temporal_frame (rt_temporal.h) starts with it
//   tap_kernel, tap_normal_weight, tap_position_term   k[dx]*k[dy], w_n and a_pos of a tap: k_denoise_level (rt_denoise.hip) and filter_level_pixel
//   filter_stage_tile                   the 16x16 tile and its apron in LDS: k_denoise_var_level<*, 1 | 2> stages the level's input,
//                                       k_budget_keys_filtered the moments of the state
//   filter_level_pixel<H>               what one level of rt_denoise_adaptive writes for a filtered pixel: k_denoise_var_level<*, H>,
//                                       and k_budget_keys_filtered (H == 1), which ranks the pixel by it
// Numeric contract: one IEEE binary32 rounding per operation in the order the header states, no contraction (also on the command
// line of the including files), correctly rounded division (hipcc default), sums in tap order — tests/denoise_model.py,
// tests/denoise_var_model.py and tests/filtered_budget_model.py reproduce it bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/rt_amd.h"
#include "rt_device.h"

#pragma clang fp contract(off)

namespace rt {

// ---- the moments of a state element ---------------------------------------------------------------------------------------------
// mean colour (c.xyz) and the variance of the mean luminance (c.w) of element p, with the state values read on the way.
// p < 2^30: 3 * p does not fit an int (64-bit colour offsets).
struct StateMoments { float4 c; float nf, sl, q; int k; };

__device__ __forceinline__ StateMoments state_moments(const AdaptState& S, int p) {
    StateMoments m;
    const long long e = 3 * (long long)p;
    m.k = S.k[p];
    m.nf = (float)m.k;
    m.c.x = S.rgb[e] / m.nf; m.c.y = S.rgb[e + 1] / m.nf; m.c.z = S.rgb[e + 2] / m.nf;
    m.sl = S.sl[p];
    m.q = S.q[p];
    float d = m.nf * m.q - m.sl * m.sl;
    d = d > 0.0f ? d : 0.0f;
    m.c.w = d / ((m.nf * m.nf) * (m.nf - 1.0f));
    return m;
}
// decided once: such a pixel is passed through by the filter (EMPTY for temporal accumulation) and is never a tap of another pixel.
// sphere: the pixel's first hit (rt_hit_record::sphere, -1 = the sky)
__device__ __forceinline__ bool state_pass_through(const StateMoments& m, int sphere) {
    return sphere == -1 || m.k < 2 || !__builtin_isfinite(m.c.x) || !__builtin_isfinite(m.c.y) || !__builtin_isfinite(m.c.z) || !__builtin_isfinite(m.c.w);
}

// ---- the terms of a tap that rt_denoise and rt_denoise_adaptive share ------------------------------------------------------------
// k[dx] * k[dy], dx, dy in -2..2: the 5x5 B3-spline kernel of the à-trous taps
__device__ __forceinline__ float tap_kernel(int dx, int dy) {
    const float k[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    return k[dx + 2] * k[dy + 2];
}
// the guide terms (gp*: the centre's guide halves (t, P) and (N, sphere), gq*: the tap's)
__device__ __forceinline__ float tap_normal_weight(const float4& gp1, const float4& gq1, int npow) {      // npow < 0: no normal term
    float wn = 1.0f;
    if (npow >= 0) {
        const float d = (gp1.x * gq1.x + gp1.y * gq1.y) + gp1.z * gq1.z;
        wn = d > 0.0f ? d : 0.0f;
        for (int e = 0; e < npow; ++e) wn = wn * wn;
    }
    return wn;
}
// tt = t_p^2; gq0 by address: the tap's (t, P) half is loaded here, only where the term is asked
__device__ __forceinline__ float tap_position_term(const float4& gp0, const float4* gq0p, float tt, float inv_sp2) {
    const float4 gq0 = *gq0p;
    const float ex = gp0.y - gq0.y, ey = gp0.z - gq0.z, ez = gp0.w - gq0.w;
    return (((ex * ex + ey * ey) + ez * ez) / tt) * inv_sp2;
}

// ---- the tile in LDS ------------------------------------------------------------------------------------------------------------
// Step H (1 or 2) with the 16x16 tile and its apron of 2H pixels staged in LDS — colour + variance and both guide halves, 48 bytes a
// pixel, three planes of S = 16 + 4H rows of 32 16-byte slots each: a wave's ds_read_b128 is served in groups of 16 lanes that span
// two tile rows (8 + 8 columns), and a row stride of 32 slots puts those 16 slots on 16 different bank quads for every tap offset
// (the natural strides 20 and 24 would collide 2-way).  20 x 32 x 48 B = 30 KB (H = 1) and 24 x 32 x 48 B = 36 KB (H = 2) of the
// CU's 160 KB: four blocks a CU.  Pixels outside the frame are staged as pass-through, so a tap needs no bounds test.
constexpr int kFilterTileStride = 32;
constexpr int filter_tile_rows(int H) { return 16 + 4 * H; }
constexpr int filter_tile_slots(int H) { return H ? filter_tile_rows(H) * kFilterTileStride : 1; }       // (H == 0: nothing is staged)
// the slot of the tile's pixel (li, lj)
template <int H>
__device__ __forceinline__ int filter_tile_centre(int li, int lj) { return (lj + 2 * H) * kFilterTileStride + li + 2 * H; }

// All 256 threads of the block: stage tile (tx, ty).  src(q) is the colour and variance of pixel q of the frame, .w < 0 for a
// pass-through pixel; the guide halves of such a pixel are not staged (nobody reads them).  The caller's barrier publishes the tile.
template <int H, class Src>
__device__ __forceinline__ void filter_stage_tile(float4* sx, float4* sg0, float4* sg1, const float4* __restrict__ g, int tx, int ty, int max_x,
                                                  int max_y, const Src& src) {
    constexpr int S = filter_tile_rows(H), ST = kFilterTileStride;
    const int i0 = tx * 16 - 2 * H, j0 = ty * 16 - 2 * H;
    for (int e = (int)threadIdx.x; e < S * S; e += 256) {
        const int ej = e / S, ei = e - ej * S;
        const int qi = i0 + ei, qj = j0 + ej;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, -1.0f);             // outside the frame: pass-through
        if (qi >= 0 && qi < max_x && qj >= 0 && qj < max_y) {
            const int q = qj * max_x + qi;
            v = src(q);
            if (!(v.w < 0.0f)) { sg0[ej * ST + ei] = g[2 * q]; sg1[ej * ST + ei] = g[2 * q + 1]; }
        }
        sx[ej * ST + ei] = v;
    }
}

// ---- one level for one filtered pixel -------------------------------------------------------------------------------------------
// (y, v') of pixel p = (i, j), whose own (x, v) is xp (not pass-through).  H == 0: the plain form, taps through the caches (x, g) at
// step L.h with bounds tests.  H == 1, 2: step H, taps from the staged tile, c = the pixel's slot.  The blur of the centre's variance
// reaches +-1 at step 1: inside the apron.
template <int H>
__device__ __forceinline__ float4 filter_level_pixel(const float4* __restrict__ x, const float4* __restrict__ g, const float4* sx, const float4* sg0,
                                                     const float4* sg1, int c, int i, int j, int max_x, int max_y, const float4& xp,
                                                     const DenoiseVarLevel& L) {
    constexpr int ST = kFilterTileStride;
    const int p = j * max_x + i;
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
            const float wn = tap_normal_weight(gp1, gq1, L.npow);
            const float apos = L.use_pos ? tap_position_term(gp0, H ? &sg0[s] : &g[2 * q], tt, L.inv_sp2) : 0.0f;
            float avar = 0.0f;
            if (L.use_var) {
                const float dl = lp - ((xq.x + xq.y) + xq.z);
                avar = (dl * dl) / den;
            }
            const float w = (tap_kernel(dx, dy) * wn) / ((1.0f + apos) * (1.0f + avar));
            sw = sw + w;
            s0 = s0 + w * xq.x; s1 = s1 + w * xq.y; s2 = s2 + w * xq.z;
            s3 = s3 + (w * w) * xq.w;
        }
    }
    return make_float4(s0 / sw, s1 / sw, s2 / sw, s3 / (sw * sw));
}

} // namespace rt
