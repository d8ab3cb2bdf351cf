// oracle/ref_shim/curand_kernel.h — stand-in for cuRAND's device header, so that the reference's headers compile as host C++17
// (oracle/Makefile, target `ref`).  Test infrastructure only; our own text, written from cuRAND's public documentation of XORWOW
// (Marsaglia's xorshift with five 32-bit words plus a Weyl sequence of step 362437).
//
// The 48-byte state has cuRAND's field order.  Only what the reference uses exists: curand_init with subsequence 0 and offset 0
// (main.cu:80, :93) — any other is refused, because skipping ahead is not written here —, curand and curand_uniform.
// curand_uniform is x * 2^-32 + 2^-33 in binary32, one rounding per operation: (0, 1].
// The seeding constants are NOT pinned by anything the reference ships; they are the ones SURVEY.md App. A.1 recorded.
#pragma once
#include "cuda_fp16.h"
#include <cstdint>

struct curandStateXORWOW {
    unsigned int d, v[5];
    int boxmuller_flag;
    int boxmuller_flag_double;
    float boxmuller_extra;
    double boxmuller_extra_double;
};
typedef struct curandStateXORWOW curandStateXORWOW_t;
typedef struct curandStateXORWOW curandState_t;
typedef struct curandStateXORWOW curandState;
static_assert(sizeof(curandStateXORWOW) == 48, "curandStateXORWOW is 48 bytes");

static inline void curand_init(unsigned long long seed, unsigned long long subsequence, unsigned long long offset, curandStateXORWOW* state) {
    if (subsequence != 0 || offset != 0) {
        std::fprintf(stderr, "ref_shim: curand_init with subsequence %llu, offset %llu: only 0, 0 is written\n", subsequence, offset);
        std::abort();
    }
    const unsigned int s0 = (unsigned int)seed ^ 0xaad26b49u;
    const unsigned int s1 = (unsigned int)(seed >> 32) ^ 0xf7dcefddu;
    const unsigned int t0 = 1099087573u * s0;
    const unsigned int t1 = 2591861531u * s1;
    state->d = 6615241u + t1 + t0;
    state->v[0] = 123456789u + t0;
    state->v[1] = 362436069u ^ t0;
    state->v[2] = 521288629u + t1;
    state->v[3] = 88675123u ^ t1;
    state->v[4] = 5783321u + t0;
    state->boxmuller_flag = 0;
    state->boxmuller_flag_double = 0;
    state->boxmuller_extra = 0.f;
    state->boxmuller_extra_double = 0.;
}

static inline unsigned int curand(curandStateXORWOW* state) {
    const unsigned int t = state->v[0] ^ (state->v[0] >> 2);
    state->v[0] = state->v[1];
    state->v[1] = state->v[2];
    state->v[2] = state->v[3];
    state->v[3] = state->v[4];
    state->v[4] = (state->v[4] ^ (state->v[4] << 4)) ^ (t ^ (t << 1));
    state->d += 362437u;
    return state->v[4] + state->d;
}

static inline float curand_uniform(curandStateXORWOW* state) {
    const float two_pow_minus_32 = 2.3283064e-10f;
    return (float)curand(state) * two_pow_minus_32 + (two_pow_minus_32 / 2.0f);
}
