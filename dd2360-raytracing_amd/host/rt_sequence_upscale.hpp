// rt_sequence_upscale.hpp — the upscaling rule of rt_sequence (host/sequence.cpp, key `upscale`), written once: the shown frame of
// s*nx x s*ny pixels from the low frame of nx x ny pixels that was sampled, accumulated and filtered, guided by the first-hit records of
// both sizes (rt_render_guides with the same camera; its centre rays make high pixel I lie at ((I + 0.5) / s - 0.5) low pixels).  The
// host program's kernel k_upscale and the stand-alone check tests/host/upscale_rule_check.cpp both evaluate these inlines;
// tests/upscale_model.py is the numpy model, bit for bit.  Nothing is included, so a plain C++ compiler takes the header as it is.
//
// Numeric contract: every value is one IEEE binary32 operation (compile with -ffp-contract=off; under clang the pragma below says it
// again), sums in tap order.  A pixel that accepts no weight is COPIED from the low frame: no arithmetic, so -0 and NaN survive.
//
//   fx = ((float)I + 0.5f) / (float)s - 0.5f;  i0 = (int)floorf(fx);  ax = fx - (float)i0        (fy, j0, ay likewise)
//   taps q = (i0 + a, j0 + b), b outer, both from 0;  w = (a ? ax : 1 - ax) * (b ? ay : 1 - ay)
//   a tap is SKIPPED (not weighted by 0) when it lies outside the low frame, when its guide's sphere is not the high pixel's (sky, -1,
//   matches sky), or when a channel of its colour is not finite
//   accepted taps, in order:  sw = sw + w;  per channel  x = c*c;  y = y + w*x                    (gamma values, blended as light)
//   sw > 0:  out = sqrtf(y / sw) per channel;  otherwise the three floats of low pixel (I / s, J / s), copied
// For s = 2..4 and every width, i0 stays in -1..nx-1 and 0 <= ax < 1, and the low pixel I / s is always one of the two taps of its
// axis; for s = 3 every third column has ax == 0, so a tap can be accepted with weight 0.  Nothing is clamped.
#ifndef RT_SEQUENCE_UPSCALE_HPP
#define RT_SEQUENCE_UPSCALE_HPP

#if defined(__HIPCC__)
#define RT_SEQ_HD __host__ __device__
#else
#define RT_SEQ_HD
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define RT_SEQ_UPSCALE_MIN 2
#define RT_SEQ_UPSCALE_MAX 4

// rt_hit_record of rt_amd.h, restated: 32 bytes, the index of the sphere that was hit last, -1 = sky (sequence.cpp asserts the size
// and the offset against the library's)
struct rt_seq_hit {
    float t, p[3], normal[3];
    int sphere;
};

// where high coordinate I lies on the low axis: the first of its two taps and the weight of the second
RT_SEQ_HD inline void rt_seq_upscale_axis(int I, int s, int* i0, float* a) {
    const float f = ((float)I + 0.5f) / (float)s - 0.5f;
    *i0 = (int)__builtin_floorf(f);
    *a = f - (float)*i0;
}

// neither an infinity nor a NaN: the exponent field is not all ones (a test of bits, no arithmetic)
RT_SEQ_HD inline bool rt_seq_finite(float x) {
    unsigned u;
    __builtin_memcpy(&u, &x, sizeof u);
    return (u & 0x7f800000u) != 0x7f800000u;
}

// High pixel (I, J) of the s-fold frame.  c: the low frame's gamma values, 3 floats a pixel; g: its guides; both nx*ny elements, pixel
// j*nx + i.  sphere: the high guide's own.  Returns the number of accepted taps (0..4); out receives the pixel.
RT_SEQ_HD inline int rt_seq_upscale_pixel(const float* c, const rt_seq_hit* g, int nx, int ny, int s, int I, int J, int sphere, float out[3]) {
    int i0, j0;
    float ax, ay;
    rt_seq_upscale_axis(I, s, &i0, &ax);
    rt_seq_upscale_axis(J, s, &j0, &ay);
    float sw = 0.f, y0 = 0.f, y1 = 0.f, y2 = 0.f;
    int taps = 0;
    for (int b = 0; b < 2; b++)
        for (int a = 0; a < 2; a++) {
            const int i = i0 + a, j = j0 + b;
            if (i < 0 || i >= nx || j < 0 || j >= ny) continue;
            const unsigned long long q = (unsigned long long)j * (unsigned long long)nx + (unsigned long long)i;
            if (g[q].sphere != sphere) continue;
            const float c0 = c[q * 3], c1 = c[q * 3 + 1], c2 = c[q * 3 + 2];
            if (!rt_seq_finite(c0) || !rt_seq_finite(c1) || !rt_seq_finite(c2)) continue;
            const float w = (a ? ax : 1.0f - ax) * (b ? ay : 1.0f - ay);
            const float x0 = c0 * c0, x1 = c1 * c1, x2 = c2 * c2;
            sw = sw + w;
            y0 = y0 + w * x0;
            y1 = y1 + w * x1;
            y2 = y2 + w * x2;
            taps++;
        }
    if (sw > 0.f) {
        out[0] = __builtin_sqrtf(y0 / sw);
        out[1] = __builtin_sqrtf(y1 / sw);
        out[2] = __builtin_sqrtf(y2 / sw);
    } else {
        const unsigned long long q = (unsigned long long)(J / s) * (unsigned long long)nx + (unsigned long long)(I / s);
        out[0] = c[q * 3];
        out[1] = c[q * 3 + 1];
        out[2] = c[q * 3 + 2];
    }
    return taps;
}

#endif // RT_SEQUENCE_UPSCALE_HPP
