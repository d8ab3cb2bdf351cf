// rt_adapt_rule.h — the stop rule of adaptive sampling (include/rt_amd.h), written ONCE for the two units that apply
// it: the checks between the rounds (rt_adaptive.hip) and the fused render kernel k_render<*, 3, *> (rt_kernels.hip, its IEEE units).
// Both are compiled without FMA contraction, which the rule needs: one IEEE binary32 rounding per operation.
#pragma once
#include <hip/hip_runtime.h>

namespace rt {

// The stop rule of include/rt_amd.h after k samples, one IEEE binary32 rounding per operation: rel_error > 0 and
// k*Q - S*S <= (rel_error^2 * (k-1)) * max(S, k*floor)^2 (S, Q: sums of the samples' luminance and of its squares).  Every check calls it.
__device__ __forceinline__ bool adapt_rule(float S, float Q, int k, float rel_error, float floor_lum) {
#pragma clang fp contract(off)                                         // (whatever the including unit allows elsewhere)
    const float nk = (float)k;
    const float d = nk * Q - S * S;
    const float nf = nk * floor_lum;
    const float m = S > nf ? S : nf;
    const float tt = rel_error * rel_error;
    return rel_error > 0.f && d <= (tt * (nk - 1.f)) * (m * m);       // NaN anywhere: false, the pixel runs on
}

} // namespace rt
