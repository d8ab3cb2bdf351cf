// rt_temporal.h — the per-pixel rule of temporal accumulation (include/rt_amd.h), once: k_temporal_accumulate
// (rt_temporal.hip) writes what temporal_pixel returns as this frame's history, k_budget_keys_temporal (rt_budget.hip) ranks the
// pixel by it, k_temporal_accumulate_moving (rt_animate.hip) writes its MOVING variant: the rule that follows a translated sphere.
// k_temporal_accumulate_rectified (rt_rectify.hip) is either of the two with a functor in the rule's one hook: history rectification.
// Numeric contract: one IEEE binary32 rounding per operation in the order the header states, no contraction (also on the command
// line of the three files), correctly rounded division (hipcc default), sums in tap order — tests/temporal_model.py and
// tests/temporal_moving_model.py reproduce it bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/rt_amd.h"
#include "rt_device.h"
#include "rt_filter.h"

#pragma clang fp contract(off)

namespace rt {

struct TemporalArgs {
    float4* out; float* neff_out;             // this frame's history: float4 [n], then float [n] (the budget key writes neither)
    const float4* in; const float* neff_in;   // the last frame's (in == nullptr: none is asked)
    const float4* g; const float4* g_prev;    // guide records as 16-byte halves: (t, P), (N, sphere)
    AdaptState S;
    const int32_t* kind; int32_t n_kind;      // RT_MAT_* of the world list
    int32_t max_x, max_y, tiles_x;
    int32_t reuse_specular;
    float max_history;                        // (float)params->max_history
    float tol2, min_dot;                      // position_tolerance^2 (rounded once on the host), normal_min_dot
    rt_camera cam;                            // the camera of the frame that wrote `in`
};

// the arguments have been checked by the caller (rt_api.hip): 16-byte aligned histories and guides, max_x * max_y <= 2^30;
// hist_in == nullptr: the first frame (hits_prev and cam_prev are then not looked at)
inline TemporalArgs temporal_args(void* hist_out, const void* hist_in, const rt_hit_record* hits, const rt_hit_record* hits_prev,
                                  const rt_camera* cam_prev, const void* state, const int32_t* kind, int n_kind, int max_x, int max_y,
                                  const rt_temporal_params& P) {
    const long long n = (long long)max_x * max_y;
    TemporalArgs T;
    T.out = (float4*)hist_out; T.neff_out = hist_out ? (float*)(T.out + n) : nullptr;
    T.in = (const float4*)hist_in; T.neff_in = hist_in ? (const float*)(T.in + n) : nullptr;
    T.g = (const float4*)hits; T.g_prev = (const float4*)hits_prev;
    T.S = adapt_state(const_cast<void*>(state), n);
    T.kind = kind; T.n_kind = n_kind;
    T.max_x = max_x; T.max_y = max_y; T.tiles_x = (max_x + 15) / 16;
    T.reuse_specular = P.reuse_specular;
    T.max_history = (float)P.max_history;
    T.tol2 = P.position_tolerance * P.position_tolerance;
    T.min_dot = P.normal_min_dot;
    if (hist_in) T.cam = *cam_prev; else T.cam = rt_camera{};
    return T;
}

// what the MOVING variant takes besides: the world's geometry now and as it was in the frame that wrote `in` ((cx, cy, cz, radius) per
// world-list index, n_kind of them; geom_prev is only read when `in` is there)
struct TemporalMotion { const float4* geom; const float4* geom_prev; };

__device__ inline float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// what rt_temporal_accumulate writes for pixel p — (x.r, x.g, x.b, v) and neff, zeros for an EMPTY pixel — and the state values it
// read on the way (k, SL, Q: the raw budget key of an EMPTY pixel needs them).  p < max_x * max_y <= 2^30: p and the guide index
// 2 * p + 1 fit an int, 3 * p does not (64-bit colour offsets).  Every gathered index is clamped into the frame.
struct TemporalPixel { float4 out; float neff; int k; float sl, q; };

// this frame's values of pixel p, the first lines of the rule: x_c and v_c (c), both halves of its guide record, the state values and
// the EMPTY decision.  temporal_pixel starts with it; k_temporal_accumulate_rectified (rt_rectify.hip) stages its window from it, so
// a window pixel is EMPTY exactly when rt_temporal_accumulate writes zeros for it.
struct TemporalFrame { float4 c, gp0, gp1; float nf, sl, q; int k, sp; bool empty; };

__device__ __forceinline__ TemporalFrame temporal_frame(const TemporalArgs& T, int p) {
    TemporalFrame f;
    const StateMoments m = state_moments(T.S, p);                  // the "per pixel" line of rt_denoise_adaptive
    f.k = m.k; f.nf = m.nf; f.c = m.c; f.sl = m.sl; f.q = m.q;
    f.gp0 = T.g[2 * p]; f.gp1 = T.g[2 * p + 1];
    f.sp = __float_as_int(f.gp1.w);
    f.empty = state_pass_through(m, f.sp);
    return f;
}

// the hook of temporal_pixel: called once for a pixel that has taken history (sg > 0), between m = min(n_h, max_history) and the
// merge, with the history's colour; what it returns is merged as m.  This one changes nothing: the rule of rt_temporal_accumulate.
struct TemporalKeep { __device__ __forceinline__ float operator()(float m, float, float, float, int) const { return m; } };

// MOVING (rt_temporal_accumulate_moving): a sphere whose radius changed its bits is not asked, and the point of a sphere whose centre
// changed its bits is carried back by the translation, P' = (P - c1) + c0 per component, before it is projected and compared.
// temporal_pixel_from takes the pixel's TemporalFrame from the caller, temporal_pixel computes it.
template <bool MOVING = false, class Hook = TemporalKeep>
__device__ __forceinline__ TemporalPixel temporal_pixel_from(const TemporalArgs& T, const TemporalFrame& F, const TemporalMotion* M = nullptr,
                                                             const Hook& hook = Hook()) {
    const int k = F.k;
    const float nf = F.nf;
    const float4 c = F.c;
    const float sl = F.sl;
    const float q = F.q;
    const float4 gp0 = F.gp0, gp1 = F.gp1;
    const int sp = F.sp;
    float Px = gp0.y, Py = gp0.z, Pz = gp0.w;                                      // P', where the point was: P_p unless its sphere moved
    bool resized = false;
    if constexpr (MOVING) {
        if (T.in != nullptr && (unsigned)sp < (unsigned)T.n_kind) {
            const float4 c1 = M->geom[sp], c0 = M->geom_prev[sp];
            resized = __float_as_int(c0.w) != __float_as_int(c1.w);
            if (__float_as_int(c0.x) != __float_as_int(c1.x) || __float_as_int(c0.y) != __float_as_int(c1.y) || __float_as_int(c0.z) != __float_as_int(c1.z)) {
                Px = (Px - c1.x) + c0.x; Py = (Py - c1.y) + c0.y; Pz = (Pz - c1.z) + c0.z;
            }
        }
    }
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float neff = 0.0f;
    const bool empty = F.empty;
    if (!empty) {
        out = c;
        neff = nf;
        bool ask = T.in != nullptr && T.max_history != 0.0f;
        if (ask && !T.reuse_specular) ask = (unsigned)sp < (unsigned)T.n_kind && T.kind[sp] == RT_MAT_LAMBERTIAN;
        if constexpr (MOVING) ask = ask && !resized;
        if (ask) {
            // where the point was seen before: the pinhole inverse of get_ray on the previous camera
            const float* O = T.cam.origin; const float* LL = T.cam.lower_left_corner; const float* H = T.cam.horizontal; const float* V = T.cam.vertical;
            const float Ax = LL[0] - O[0], Ay = LL[1] - O[1], Az = LL[2] - O[2];
            const float Dx = Px - O[0], Dy = Py - O[1], Dz = Pz - O[2];
            const float Wx = H[1] * V[2] - H[2] * V[1], Wy = H[2] * V[0] - H[0] * V[2], Wz = H[0] * V[1] - H[1] * V[0];
            const float lam = dot3(Dx, Dy, Dz, Wx, Wy, Wz) / dot3(Ax, Ay, Az, Wx, Wy, Wz);
            const float s = (dot3(Dx, Dy, Dz, H[0], H[1], H[2]) / lam - dot3(Ax, Ay, Az, H[0], H[1], H[2])) / dot3(H[0], H[1], H[2], H[0], H[1], H[2]);
            const float t = (dot3(Dx, Dy, Dz, V[0], V[1], V[2]) / lam - dot3(Ax, Ay, Az, V[0], V[1], V[2])) / dot3(V[0], V[1], V[2], V[0], V[1], V[2]);
            const float mx = (float)T.max_x, my = (float)T.max_y;
            const float fx = s * mx - 0.5f, fy = t * my - 0.5f;
            if (lam > 0.0f && fx > -1.0f && fx < mx && fy > -1.0f && fy < my) {          // (a NaN rejects)
                const int i0 = (int)floorf(fx), j0 = (int)floorf(fy);                    // -1 .. max - 1
                const float ax = fx - (float)i0, ay = fy - (float)j0;
                const float lim = T.tol2 * (gp0.x * gp0.x);
                // the four taps, b outer: every load first (indices clamped into the frame), then the tests
                float nq[4]; float4 gq0[4], gq1[4], xq[4]; bool in[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int qi = i0 + (u & 1), qj = j0 + (u >> 1);
                    in[u] = qi >= 0 && qi < T.max_x && qj >= 0 && qj < T.max_y;
                    const int ci = qi < 0 ? 0 : (qi >= T.max_x ? T.max_x - 1 : qi), cj = qj < 0 ? 0 : (qj >= T.max_y ? T.max_y - 1 : qj);
                    const int qq = cj * T.max_x + ci;
                    nq[u] = T.neff_in[qq];
                    gq1[u] = T.g_prev[2 * qq + 1];
                    gq0[u] = T.g_prev[2 * qq];
                    xq[u] = T.in[qq];
                }
                float sg = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f, s4 = 0.0f;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (!in[u] || !(nq[u] > 0.0f)) continue;                             // outside the frame; an empty pixel of the last frame
                    if (__float_as_int(gq1[u].w) != sp) continue;                        // another sphere
                    if (!(dot3(gp1.x, gp1.y, gp1.z, gq1[u].x, gq1[u].y, gq1[u].z) >= T.min_dot)) continue;
                    const float ex = Px - gq0[u].y, ey = Py - gq0[u].z, ez = Pz - gq0[u].w;
                    if (!(((ex * ex + ey * ey) + ez * ez) <= lim)) continue;
                    const float g = ((u & 1) ? ax : 1.0f - ax) * ((u >> 1) ? ay : 1.0f - ay);
                    sg = sg + g;
                    s0 = s0 + g * xq[u].x; s1 = s1 + g * xq[u].y; s2 = s2 + g * xq[u].z;
                    s3 = s3 + g * xq[u].w;
                    s4 = s4 + g * nq[u];
                }
                if (sg > 0.0f) {
                    const float hx = s0 / sg, hy = s1 / sg, hz = s2 / sg, hv = s3 / sg, hn = s4 / sg;
                    const float m = hook(hn < T.max_history ? hn : T.max_history, hx, hy, hz, sp);
                    const float a = nf / (m + nf);
                    out.x = hx + a * (c.x - hx); out.y = hy + a * (c.y - hy); out.z = hz + a * (c.z - hz);
                    out.w = ((1.0f - a) * (1.0f - a)) * hv + (a * a) * c.w;
                    neff = m + nf;
                }
            }
        }
    }
    return TemporalPixel{out, neff, k, sl, q};
}

template <bool MOVING = false>
__device__ __forceinline__ TemporalPixel temporal_pixel(const TemporalArgs& T, int p, const TemporalMotion* M = nullptr) {
    return temporal_pixel_from<MOVING>(T, temporal_frame(T, p), M);
}

} // namespace rt
