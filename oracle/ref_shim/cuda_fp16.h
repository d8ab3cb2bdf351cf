// oracle/ref_shim/cuda_fp16.h — stand-in for CUDA's <cuda_fp16.h>, so that the reference's headers compile unmodified as host
// C++17 (oracle/Makefile, target `ref`).  Test infrastructure only; our own text, nothing of CUDA's.
//
// What it gives:
//   * __host__, __device__, __global__ as nothing and __forceinline__ as `inline`.  __CUDA_ARCH__ stays undefined, so every
//     `#ifdef __CUDA_ARCH__` of the reference takes its host branch: a real_t operator is a float operation rounded once to
//     binary16 (precision_types.h:35-37 and the like).  DESIGN.md §2 names that as the contract for real_t.
//   * struct __half over the compiler's _Float16, with __float2half (round to nearest even) and __half2float (exact).
//   * the two library calls whose result the numeric contract DEFINES instead of leaving to a libm:
//         pow(1 - cos, 5)  = ((x*x)*(x*x))*x in binary64, rounded once to binary32          (material.h:14)
//         tan(theta / 2)   = binary64 tan, rounded once to binary32                          (camera.h:31, :34)
//     Through vec3.h's <math.h> the headers would resolve pow(float, float) to powf, and powf is not that definition: over every
//     third float of [0, 2] (357.9 M values) glibc's powf(x, 5) differs from it on 50 255, binary64 pow(x, 5) on none.  So the two
//     names are taken over here, by those definitions, as function-like macros that are set after every standard header the
//     reference includes has been read.  No other name of libm is touched: sqrt and `/` stay the compiler's (both are correctly
//     rounded IEEE operations).
#pragma once
#include <cassert>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <fstream>
#include <iostream>
#include <math.h>
#include <stdlib.h>
#include <string>
#include <vector>

#ifdef __CUDA_ARCH__
#error "the reference's host branches are the contract: __CUDA_ARCH__ must stay undefined"
#endif

#define __host__
#define __device__
#define __global__
#define __forceinline__ inline

struct __half {
    _Float16 x;
};
static inline __half __float2half(float f) { __half h; h.x = (_Float16)f; return h; }
static inline float __half2float(__half h) { return (float)h.x; }

namespace ref_shim {
// the contract's x^5: exact products in binary64 up to the last, one rounding to binary32
static inline float pow_contract(float x, float e) {
    if (e != 5.0f) { std::fprintf(stderr, "ref_shim: pow(x, %g) is not defined by the contract\n", (double)e); std::abort(); }
    const double d = (double)x;
    const double d2 = d * d;
    return (float)((d2 * d2) * d);
}
// the contract's tan: binary64 tan rounded once (a real_t argument arrives through its operator float)
static inline float tan_contract(float x) { return (float)::tan((double)x); }
}  // namespace ref_shim

// set last: everything above, and every standard header the reference names, is already read
#define pow(x, e) ref_shim::pow_contract((x), (e))
#define tan(x) ref_shim::tan_contract((x))
