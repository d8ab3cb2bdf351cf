// tools/micro/exact_forms.hip — are the single-rounding forms of the sampling arithmetic (csrc/rt_sampling.h) bit-identical to the
// reference's two-rounding forms?  Checked on the GPU for ALL 2^32 values of the 32-bit draw X:
//   (1) fma((float)X, 2^-32, 2^-33)  against  (float)X * 2^-32 + 2^-33        (curand_uniform)
//   (2) fma(2, u, -1)                against  2 * u - 1                       for u = the value (1) returns — every value a draw can take
// compared as bit patterns.  Also reports the smallest and largest u (the premise of the argument: u in [2^-33, 1]).
// Plain arithmetic, one launch, nothing is written but three counters.
// hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -fno-gpu-flush-denormals-to-zero -o exact_forms exact_forms.hip && ./exact_forms
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include "../../dd2360-raytracing_amd/csrc/rt_sampling.h"       // the kernels' own functions — not a copy
#pragma clang fp contract(off)
struct Out { unsigned long long bad_uniform, bad_signed; uint32_t first_uniform, first_signed, min_bits, max_bits; };
__global__ __launch_bounds__(256) void k(Out* out) {
    // block b, thread t: X = (b << 16) | (j << 8) | t for j in 0..255 — 65536 blocks cover 2^32 values exactly once
    const uint32_t base = ((uint32_t)blockIdx.x << 16) | threadIdx.x;
    unsigned long long nu = 0, ns = 0;
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (uint32_t j = 0; j < 256u; ++j) {
        const uint32_t X = base | (j << 8);
        const float u = rt::uniform_from_bits(X), u2 = rt::uniform_from_bits_two_step(X);
        const uint32_t ub = __float_as_uint(u);
        if (ub != __float_as_uint(u2)) { ++nu; atomicCAS(&out->first_uniform, 0xffffffffu, X); }
        if (__float_as_uint(rt::signed_unit(u)) != __float_as_uint(rt::signed_unit_two_step(u))) { ++ns; atomicCAS(&out->first_signed, 0xffffffffu, X); }
        lo = ub < lo ? ub : lo; hi = ub > hi ? ub : hi;             // u > 0: the bit patterns order as the values do
    }
    if (nu) atomicAdd(&out->bad_uniform, nu);
    if (ns) atomicAdd(&out->bad_signed, ns);
    atomicMin(&out->min_bits, lo); atomicMax(&out->max_bits, hi);
}
int main() {
    Out h = {0, 0, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0u};
    Out* d;
    if (hipMalloc(&d, sizeof(Out)) != hipSuccess || hipMemcpy(d, &h, sizeof(Out), hipMemcpyHostToDevice) != hipSuccess) { printf("no device memory\n"); return 2; }
    hipLaunchKernelGGL(k, dim3(65536), dim3(256), 0, 0, d);
    if (hipMemcpy(&h, d, sizeof(Out), hipMemcpyDeviceToHost) != hipSuccess) { printf("launch failed\n"); return 2; }
    float lo, hi; __builtin_memcpy(&lo, &h.min_bits, 4); __builtin_memcpy(&hi, &h.max_bits, 4);
    printf("all 2^32 draws: %llu uniform values differ from the two-step form, %llu values of 2x-1 differ; u in [%a, %a]\n", h.bad_uniform, h.bad_signed, lo, hi);
    if (h.bad_uniform) printf("first differing uniform: X = 0x%08x\n", h.first_uniform);
    if (h.bad_signed) printf("first differing 2x-1: X = 0x%08x\n", h.first_signed);
    return (h.bad_uniform || h.bad_signed) ? 1 : 0;
}
