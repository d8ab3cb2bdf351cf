// upscale_rule_check.cpp — test program (tests/test_upscale_host.py compiles it with g++ -ffp-contract=off and
// -fsanitize=address,undefined and runs it; not part of the product).  Evaluates the upscaling rule of rt_sequence
// (dd2360-raytracing_amd/host/rt_sequence_upscale.hpp) on two hand-made low frames, 5x3 and 1x1, for s = 2, 3 and 4, and prints
// everything as bits: the low frame and its sphere ids, and per high pixel its own sphere id, the number of accepted taps and the
// result.  tests/upscale_model.py computes the same from the printed inputs, and the test compares the bits and counts the branches.
// The frames live in vectors of exactly their size, so a tap read outside the low frame is an AddressSanitizer error.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "rt_sequence_upscale.hpp"

static_assert(sizeof(rt_seq_hit) == 32, "the 32-byte hit record");

static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}

struct Low {
    int nx, ny;
    std::vector<float> c;
    std::vector<rt_seq_hit> g;
};

// The high guides: the id of the low pixel a high pixel lies in, except that
//   (I % s, J % s) == (1, 1) takes the id of the low pixel to the right (for s = 3 these are the pixels with ax == ay == 0: where the two
//   ids differ only taps of weight 0 are accepted; for s = 2 and 4 one to three taps are);
//   (I + 2 * J) % 7 == 3 takes id 77, which no low pixel has: no tap is accepted.
static int high_id(const Low& L, int s, int I, int J) {
    if ((I + 2 * J) % 7 == 3) return 77;
    int i = I / s;
    const int j = J / s;
    if (I % s == 1 && J % s == 1 && i + 1 < L.nx) i++;
    return L.g[(size_t)j * L.nx + i].sphere;
}

static void run(const Low& L, int s) {
    const int NX = s * L.nx, NY = s * L.ny;
    printf("case %d %d %d\n", L.nx, L.ny, s);
    for (int j = 0; j < L.ny; j++)
        for (int i = 0; i < L.nx; i++) {
            const size_t q = (size_t)j * L.nx + i;
            printf("low %d %d %d %08x %08x %08x\n", i, j, L.g[q].sphere, bits(L.c[q * 3]), bits(L.c[q * 3 + 1]), bits(L.c[q * 3 + 2]));
        }
    for (int J = 0; J < NY; J++)
        for (int I = 0; I < NX; I++) {
            const int id = high_id(L, s, I, J);
            float out[3];
            const int taps = rt_seq_upscale_pixel(L.c.data(), L.g.data(), L.nx, L.ny, s, I, J, id, out);
            printf("high %d %d %d %d %08x %08x %08x\n", I, J, id, taps, bits(out[0]), bits(out[1]), bits(out[2]));
        }
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // 5x3, row 0 first: two spheres side by side, sky (-1) on the right, and in the top row sphere 2 and sphere 9, one pixel each
    const int ids[15] = {0, 0, 1, 1, -1,
                         0, 0, 1, -1, -1,
                         2, 9, 1, -1, -1};
    Low A{5, 3, std::vector<float>(45), std::vector<rt_seq_hit>(15)};
    for (int q = 0; q < 15; q++) {
        A.g[q] = rt_seq_hit{};
        A.g[q].sphere = ids[q];
        A.c[q * 3] = 0.05f + 0.061f * (float)q;
        A.c[q * 3 + 1] = 0.93f - 0.047f * (float)q;
        A.c[q * 3 + 2] = 0.2f + 0.013f * (float)(q * q);
    }
    A.c[(1 * 5 + 0) * 3] = -0.f;           // -0 in a channel of a pixel that is blended and copied
    A.c[(0 * 5 + 3) * 3 + 2] = inf;        // +inf: the tap is skipped
    A.c[(2 * 5 + 1) * 3 + 1] = nan;        // NaN in the only pixel of sphere 9: its high pixels accept nothing and copy it,
    A.c[(2 * 5 + 1) * 3 + 2] = -0.f;       // with the -0 beside the NaN
    A.c[(2 * 5 + 4) * 3 + 1] = 1e-30f;     // a square that is subnormal, in the sky
    A.c[(2 * 5 + 2) * 3] = 3e19f;          // a square that overflows: nothing is clamped
    Low B{1, 1, {0.25f, -0.f, 0.7f}, std::vector<rt_seq_hit>(1)};
    B.g[0] = rt_seq_hit{};
    for (int s = RT_SEQ_UPSCALE_MIN; s <= RT_SEQ_UPSCALE_MAX; s++) {
        run(A, s);
        run(B, s);
    }
    printf("upscale_rule_check: ok\n");
    return 0;
}
