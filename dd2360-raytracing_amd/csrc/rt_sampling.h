// rt_sampling.h — the two affine maps of the sampling code, in single-rounding form.  ONE definition, compiled into the kernels
// (rt_kernels.hip) and into the exhaustive check (tools/micro/exact_forms.hip, run by tests/test_gpu_exact_forms.py; the premise
// is checked on the host by tests/test_sampling_forms_host.py).
//
// curand_uniform is (float)X * 2^-32 + 2^-33 and the rejection loops form 2.0f * x - 1.0f (material.h:38, camera.h:14), each as two
// rounded operations in the reference.  In both the PRODUCT is exact: 2^-32 and 2 are powers of two, (float)X lies in {0} u [1, 2^32]
// and x in [2^-33, 1], so nothing under- or overflows.  A fused multiply-add rounds the same real number once where the two-step
// form rounds it after an exact step: the same bits, two VALU instructions fewer per draw and one fewer per coordinate
// (v_fma instead of v_mul, v_add).  This is an explicit FMA, not contraction: the translation unit stays -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rt {
// curand_uniform's conversion of a 32-bit draw: x * 2^-32 + 2^-33
static __device__ __forceinline__ float uniform_from_bits(uint32_t X) {
    return __builtin_fmaf((float)X, 2.3283064e-10f, 2.3283064e-10f / 2.0f);
}
// 2x - 1 of a draw
static __device__ __forceinline__ float signed_unit(float x) { return __builtin_fmaf(2.0f, x, -1.0f); }

// The reference's two-rounding forms, for the check only (volatile-free: the check is compiled without contraction, as the kernels are).
static __device__ __forceinline__ float uniform_from_bits_two_step(uint32_t X) {
    const float x = (float)X;
    const float m = x * 2.3283064e-10f;
    return m + (2.3283064e-10f / 2.0f);
}
static __device__ __forceinline__ float signed_unit_two_step(float x) { const float m = 2.0f * x; return m - 1.0f; }
} // namespace rt
