// rt_frame.hip — the image end of the pipeline on the device (include/rt_amd.h): rt_frame_levels turns a frame into
// the 8-bit levels rt_write_image's P6 holds, rt_frame_compare gives the notebook's grey SSIM / PSNR (evaluations.ipynb:1021-1027) and
// the studies' float RMSE for two frames without either leaving the device.  No reference counterpart: main.cu quantises on the host.
//
// k_frame_levels: one lane per pixel, one launch.
// k_frame_compare: a block owns a TILE x TILE square of pixels, which are also the window anchors (top-left corners) it evaluates.  It
// stages the grey pairs of that square and of the 6 pixels to its right and above it in LDS — quantised from the two float frames on the
// way in, where the owned pixels' error terms are taken as well —, forms the five sums of every 7x7 window separably in int32 (a row pass
// into LDS, a column pass out of it), evaluates S in binary64, and reduces in a fixed order to ONE 40-byte partial record.
// k_frame_compare_final, a single block, adds the records in block-index order.  No atomics: the 64 result bytes never vary.
//
// Numeric contract: integers until the last three operations of S (two multiplies and a division, IEEE binary64, no contraction,
// correctly rounded division) — tests/frame_metrics_model.py reproduces the map bit for bit and the two double sums up to their order.
#include <hip/hip_runtime.h>
#include <cmath>
#include <limits>
#include "../../include/rt_amd.h"
#include "rt_real.h"

#pragma clang fp contract(off)

namespace rt {

// rt::image_level of host/rt_image.hpp followed by the P6 clamp: NaN, +-inf and values beyond the int range give INT32_MIN, hence 0
__device__ __forceinline__ int frame_level(float c) {
    const double v = 255.99 * (double)c;
    int l = INT32_MIN;
    if (v > -2147483649.0 && v < 2147483648.0) l = (int)v;
    return l < 0 ? 0 : (l > 255 ? 255 : l);
}

// cv2's fixed-point RGB -> gray on three levels
__device__ __forceinline__ int frame_gray(int r, int g, int b) { return (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14; }

template <bool HALF>
__device__ __forceinline__ float frame_channel(const void* fb, long long k) {
    if (HALF) return half_bits_to_float(((const uint16_t*)fb)[k]);
    return ((const float*)fb)[k];
}

// ---- rt_frame_levels ------------------------------------------------------------------------------------------------------------------
// one lane per OUTPUT pixel (row-major in the output's row order); `word`: RGBA8 into a 4-byte aligned d_out, one store a pixel
template <bool HALF>
__global__ __launch_bounds__(256) void k_frame_levels(uint8_t* out, const void* fb, int max_x, int max_y, int sum, float samples, int format,
                                                      int top_first, int word) {
    const int n = max_x * max_y;                                               // <= 2^30
    const int o = (int)blockIdx.x * 256 + (int)threadIdx.x;                    // (o + 255 fits an int)
    if (o >= n) return;
    int p = o;
    if (top_first) { const int r = o / max_x; p = (max_y - 1 - r) * max_x + (o - r * max_x); }
    const long long e = 3 * (long long)p;
    float c0 = frame_channel<HALF>(fb, e), c1 = frame_channel<HALF>(fb, e + 1), c2 = frame_channel<HALF>(fb, e + 2);
    if (sum) { c0 = sqrtf(c0 / samples); c1 = sqrtf(c1 / samples); c2 = sqrtf(c2 / samples); }
    const int r = frame_level(c0), g = frame_level(c1), b = frame_level(c2);
    if (format == RT_LEVELS_GRAY8) {
        out[o] = (uint8_t)frame_gray(r, g, b);
    } else if (format == RT_LEVELS_RGB8) {
        uint8_t* q = out + 3 * (long long)o;
        q[0] = (uint8_t)r; q[1] = (uint8_t)g; q[2] = (uint8_t)b;
    } else if (word) {
        ((uint32_t*)out)[o] = (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16) | 0xff000000u;
    } else {
        uint8_t* q = out + 4 * (long long)o;
        q[0] = (uint8_t)r; q[1] = (uint8_t)g; q[2] = (uint8_t)b; q[3] = 255;
    }
}

// ---- rt_frame_compare -----------------------------------------------------------------------------------------------------------------
constexpr int FC_TILE = 32;                    // owned pixels = window anchors of a block, per side
constexpr int FC_SIDE = FC_TILE + 6;           // staged pixels per side
constexpr int FC_THREADS = 256;

struct FramePartial {                          // one per block, 40 bytes (rt_frame_compare_work_bytes)
    long long gray_sse, gray_differ, finite_pixels;
    double ssim_sum, sq_err;
};
static_assert(sizeof(FramePartial) == 40, "the partial record is 40 bytes");

// LDS layout.  sg: one dword a staged pixel (ga | gb << 8), rows of FC_SIDE dwords with NO padding — the staging loop
// writes consecutive dwords (ds_write_b32, conflict-free whatever the row length), and the row pass reads, per 32-lane half, 32
// consecutive dwords of one row (conflict-free for any stride).  sr: one 16-byte slot a (staged row, anchor column): {Sx | Sy << 16, Sxx,
// Syy, Sxy} of the 7 pixels to the right, rows of 32 slots = 512 bytes, a multiple of the 256-byte bank row: a ds_read_b128 lane group is
// 16 lanes of one row whose columns {0-3, 12-15, 20-27} or {4-11, 16-19, 28-31} are 16 different slots modulo 16, so the column pass is
// conflict-free at every row offset.  38*38*4 + 38*32*16 = 24.7 KB, 28.7 KB with the reduction's 4 KB: five blocks a CU.
template <bool HALF_A, bool HALF_B>
__global__ __launch_bounds__(FC_THREADS) void k_frame_compare(const void* __restrict__ fa, const void* __restrict__ fb, int max_x, int max_y,
                                                              int tiles_x, FramePartial* __restrict__ part, double* __restrict__ map) {
    __shared__ uint32_t sg[FC_SIDE * FC_SIDE];
    __shared__ int4 sr[FC_SIDE * FC_TILE];
    __shared__ long long red_i[3][FC_THREADS / 64];
    __shared__ double red_d[2][FC_THREADS];
    const int tid = (int)threadIdx.x;
    const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)(blockIdx.x / (unsigned)tiles_x);
    const int i0 = tx * FC_TILE, j0 = ty * FC_TILE;

    // stage the grey pairs; a pixel outside the frame is staged as 0 | 0 (no window that is evaluated reads it).  The owned pixels
    // (the first FC_TILE of each side) give the per-pixel terms here: every pixel of the frame is owned by exactly one block.
    int sse = 0, differ = 0, finite = 0;                   // a lane owns at most 4 pixels: 4 * 255^2 fits easily
    double sq = 0.0;
    for (int e = tid; e < FC_SIDE * FC_SIDE; e += FC_THREADS) {
        const int ej = e / FC_SIDE, ei = e - ej * FC_SIDE;
        const int qi = i0 + ei, qj = j0 + ej;
        uint32_t v = 0;
        if (qi < max_x && qj < max_y) {
            const long long k = 3 * (long long)(qj * max_x + qi);               // the pixel index fits an int (<= 2^30 pixels), 3 * p does not
            const float a0 = frame_channel<HALF_A>(fa, k), a1 = frame_channel<HALF_A>(fa, k + 1), a2 = frame_channel<HALF_A>(fa, k + 2);
            const float b0 = frame_channel<HALF_B>(fb, k), b1 = frame_channel<HALF_B>(fb, k + 1), b2 = frame_channel<HALF_B>(fb, k + 2);
            const int ga = frame_gray(frame_level(a0), frame_level(a1), frame_level(a2));
            const int gb = frame_gray(frame_level(b0), frame_level(b1), frame_level(b2));
            v = (uint32_t)ga | ((uint32_t)gb << 8);
            if (ei < FC_TILE && ej < FC_TILE) {
                const int d = ga - gb;
                sse += d * d;
                differ += d != 0;
                if (__builtin_isfinite(a0) && __builtin_isfinite(a1) && __builtin_isfinite(a2) && __builtin_isfinite(b0) &&
                    __builtin_isfinite(b1) && __builtin_isfinite(b2)) {
                    finite += 1;
                    const double d0 = (double)a0 - (double)b0, d1 = (double)a1 - (double)b1, d2 = (double)a2 - (double)b2;
                    sq = sq + d0 * d0; sq = sq + d1 * d1; sq = sq + d2 * d2;
                }
            }
        }
        sg[e] = v;
    }
    __syncthreads();

    // the anchors this block evaluates: those of its square that have a whole window inside the frame
    const int wx = max_x - 6, wy = max_y - 6;              // windows per row / column of the frame (<= 0: none)
    const int ax = min(FC_TILE, wx - i0), ay = min(FC_TILE, wy - j0);
    const bool any = ax > 0 && ay > 0;                     // uniform over the block
    double ss = 0.0;
    if (any) {
        // row pass: the five sums of the 7 pixels from (r, c) to the right, for the rows the column pass reads
        for (int e = tid; e < (ay + 6) * FC_TILE; e += FC_THREADS) {
            const int r = e >> 5, c = e & 31;
            int4 s = make_int4(0, 0, 0, 0);
            if (c < ax) {
                const uint32_t* g = sg + r * FC_SIDE + c;
#pragma unroll
                for (int k = 0; k < 7; ++k) {
                    const int x = (int)(g[k] & 255u), y = (int)(g[k] >> 8);
                    s.x += x | (y << 16); s.y += x * x; s.z += y * y; s.w += x * y;
                }
            }
            sr[e] = s;
        }
        __syncthreads();
        // column pass and S: lane (c, j), rows j, j + 8, ...; the sums of a lane are added in that order
        for (int e = tid; e < ay * FC_TILE; e += FC_THREADS) {
            const int j = e >> 5, c = e & 31;
            if (c >= ax) continue;
            int4 s = make_int4(0, 0, 0, 0);
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const int4 t = sr[(j + k) * FC_TILE + c];
                s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;       // 49 * 255 < 2^16: the packed halves do not carry
            }
            const long long Sx = s.x & 0xffff, Sy = (int)((unsigned)s.x >> 16), Sxx = s.y, Syy = s.z, Sxy = s.w;
            const long long P = Sx * Sy, K = 10000, c1 = 65025, c2 = 585225;
            const long long A1 = K * 2 * P + 2401 * c1, B1 = K * (Sx * Sx + Sy * Sy) + 2401 * c1;
            const long long A2 = K * 2 * (49 * Sxy - P) + 2352 * c2, B2 = K * ((49 * Sxx - Sx * Sx) + (49 * Syy - Sy * Sy)) + 2352 * c2;
            const double num = (double)A1 * (double)A2, den = (double)B1 * (double)B2;
            const double S = num / den;
            ss = ss + S;
            if (map) map[(size_t)(j0 + j) * (size_t)wx + (size_t)(i0 + c)] = S;
        }
    }

    // the block's record, in a fixed order: the integers are exact in any order (wave sums, then the 4 waves); the doubles go through
    // a tree over the 256 lanes whose shape does not depend on the data
    long long r0 = sse, r1 = differ, r2 = finite;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { r0 += __shfl_down(r0, o); r1 += __shfl_down(r1, o); r2 += __shfl_down(r2, o); }
    if ((tid & 63) == 0) { red_i[0][tid >> 6] = r0; red_i[1][tid >> 6] = r1; red_i[2][tid >> 6] = r2; }
    red_d[0][tid] = ss; red_d[1][tid] = sq;
    __syncthreads();
    for (int o = FC_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) { red_d[0][tid] = red_d[0][tid] + red_d[0][tid + o]; red_d[1][tid] = red_d[1][tid] + red_d[1][tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        FramePartial R;
        R.gray_sse = ((red_i[0][0] + red_i[0][1]) + red_i[0][2]) + red_i[0][3];
        R.gray_differ = ((red_i[1][0] + red_i[1][1]) + red_i[1][2]) + red_i[1][3];
        R.finite_pixels = ((red_i[2][0] + red_i[2][1]) + red_i[2][2]) + red_i[2][3];
        R.ssim_sum = red_d[0][0];
        R.sq_err = red_d[1][0];
        part[blockIdx.x] = R;
    }
}

// one block: lane t adds the records of its run of consecutive blocks in block-index order, lane 0 then adds the 256 runs in lane order
__global__ __launch_bounds__(FC_THREADS) void k_frame_compare_final(const FramePartial* __restrict__ part, int nblocks, int max_x, int max_y,
                                                                    rt_frame_metrics* __restrict__ out) {
    __shared__ FramePartial run[FC_THREADS];
    const int tid = (int)threadIdx.x;
    const int per = (nblocks + FC_THREADS - 1) / FC_THREADS;
    const long long b0 = (long long)tid * per;
    const long long b1 = b0 + per < (long long)nblocks ? b0 + per : (long long)nblocks;
    FramePartial a = {0, 0, 0, 0.0, 0.0};
    for (long long b = b0; b < b1; ++b) {
        const FramePartial p = part[b];
        a.gray_sse += p.gray_sse; a.gray_differ += p.gray_differ; a.finite_pixels += p.finite_pixels;
        a.ssim_sum = a.ssim_sum + p.ssim_sum; a.sq_err = a.sq_err + p.sq_err;
    }
    run[tid] = a;
    __syncthreads();
    if (tid != 0) return;
    for (int t = 1; t < FC_THREADS; ++t) {
        const FramePartial p = run[t];
        a.gray_sse += p.gray_sse; a.gray_differ += p.gray_differ; a.finite_pixels += p.finite_pixels;
        a.ssim_sum = a.ssim_sum + p.ssim_sum; a.sq_err = a.sq_err + p.sq_err;
    }
    rt_frame_metrics M;
    M.pixels = (int64_t)max_x * max_y;
    M.gray_sse = a.gray_sse;
    M.gray_differ = a.gray_differ;
    M.windows = (max_x < 7 || max_y < 7) ? 0 : (int64_t)(max_x - 6) * (max_y - 6);
    M.ssim_sum = M.windows ? a.ssim_sum : 0.0;
    M.finite_pixels = a.finite_pixels;
    M.sq_err = a.sq_err;
    M.reserved = 0;
    *out = M;
}

static long long frame_compare_blocks(int max_x, int max_y) {
    return (long long)((max_x + FC_TILE - 1) / FC_TILE) * (long long)((max_y + FC_TILE - 1) / FC_TILE);
}

static bool frame_size_ok(int max_x, int max_y) { return max_x > 0 && max_y > 0 && (long long)max_x * max_y <= RT_DENOISE_MAX_PIXELS; }
static bool frame_precision_ok(int p) { return p == RT_PRECISION_FP32 || p == RT_PRECISION_FP16; }

} // namespace rt

using namespace rt;

extern "C" {

int rt_frame_levels_check(int max_x, int max_y, int precision, const rt_levels_params* params) {
    if (!params || !frame_size_ok(max_x, max_y) || !frame_precision_ok(precision)) return RT_EINVAL;
    const rt_levels_params& P = *params;
    if (P.input != RT_DENOISE_INPUT_GAMMA && P.input != RT_DENOISE_INPUT_SUM) return RT_EINVAL;
    if (P.input == RT_DENOISE_INPUT_SUM && P.samples < 1) return RT_EINVAL;
    if (P.format != RT_LEVELS_RGB8 && P.format != RT_LEVELS_RGBA8 && P.format != RT_LEVELS_GRAY8) return RT_EINVAL;
    if (P.top_first != 0 && P.top_first != 1) return RT_EINVAL;
    if (P.input == RT_DENOISE_INPUT_SUM && precision == RT_PRECISION_FP16) return RT_ENOTSUP;
    return 0;
}

int64_t rt_frame_levels_bytes(int max_x, int max_y, int format) {
    if (!frame_size_ok(max_x, max_y)) return -1;
    const int64_t n = (int64_t)max_x * max_y;
    if (format == RT_LEVELS_RGB8) return 3 * n;
    if (format == RT_LEVELS_RGBA8) return 4 * n;
    if (format == RT_LEVELS_GRAY8) return n;
    return -1;
}

int rt_frame_levels(void* d_out, const void* fb, int max_x, int max_y, int precision, const rt_levels_params* params, void* stream) {
    if (!d_out || !fb) return RT_EINVAL;
    const int rc = rt_frame_levels_check(max_x, max_y, precision, params);
    if (rc) return rc;
    const rt_levels_params& P = *params;
    const int n = max_x * max_y;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const int sum = P.input == RT_DENOISE_INPUT_SUM, word = ((uintptr_t)d_out & 3) == 0;
    const float samples = sum ? (float)P.samples : 1.0f;
    if (precision == RT_PRECISION_FP16)
        hipLaunchKernelGGL(k_frame_levels<true>, grid, block, 0, (hipStream_t)stream, (uint8_t*)d_out, fb, max_x, max_y, sum, samples, (int)P.format, (int)P.top_first, word);
    else
        hipLaunchKernelGGL(k_frame_levels<false>, grid, block, 0, (hipStream_t)stream, (uint8_t*)d_out, fb, max_x, max_y, sum, samples, (int)P.format, (int)P.top_first, word);
    return (int)hipGetLastError();
}

int64_t rt_frame_compare_work_bytes(int max_x, int max_y) {
    if (!frame_size_ok(max_x, max_y)) return -1;
    return (int64_t)sizeof(FramePartial) * frame_compare_blocks(max_x, max_y);
}

int rt_frame_compare(const void* fb_a, int precision_a, const void* fb_b, int precision_b, int max_x, int max_y, rt_frame_metrics* d_metrics,
                     double* d_ssim_map, void* d_work, void* stream) {
    if (!fb_a || !fb_b || !d_metrics || !d_work) return RT_EINVAL;
    if (!frame_size_ok(max_x, max_y) || !frame_precision_ok(precision_a) || !frame_precision_ok(precision_b)) return RT_EINVAL;
    if (((uintptr_t)d_work & 7) || ((uintptr_t)d_ssim_map & 7) || ((uintptr_t)d_metrics & 7)) return RT_EINVAL;
    const int tiles_x = (max_x + FC_TILE - 1) / FC_TILE;
    const int nblocks = (int)frame_compare_blocks(max_x, max_y);               // <= 2^30 / 32 + ...: a 1-pixel-high frame has 2^25 blocks
    const dim3 grid((unsigned)nblocks), block(FC_THREADS);
    FramePartial* part = (FramePartial*)d_work;
    double* map = (max_x < 7 || max_y < 7) ? nullptr : d_ssim_map;
    const hipStream_t st = (hipStream_t)stream;
    const bool ha = precision_a == RT_PRECISION_FP16, hb = precision_b == RT_PRECISION_FP16;
    if (ha && hb) hipLaunchKernelGGL((k_frame_compare<true, true>), grid, block, 0, st, fb_a, fb_b, max_x, max_y, tiles_x, part, map);
    else if (ha) hipLaunchKernelGGL((k_frame_compare<true, false>), grid, block, 0, st, fb_a, fb_b, max_x, max_y, tiles_x, part, map);
    else if (hb) hipLaunchKernelGGL((k_frame_compare<false, true>), grid, block, 0, st, fb_a, fb_b, max_x, max_y, tiles_x, part, map);
    else hipLaunchKernelGGL((k_frame_compare<false, false>), grid, block, 0, st, fb_a, fb_b, max_x, max_y, tiles_x, part, map);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_frame_compare_final, dim3(1), block, 0, st, (const FramePartial*)part, nblocks, max_x, max_y, d_metrics);
    return (int)hipGetLastError();
}

double rt_frame_psnr(const rt_frame_metrics* m) {
    if (!m) return std::numeric_limits<double>::quiet_NaN();
    if (m->gray_sse == 0) return std::numeric_limits<double>::infinity();
    return 10.0 * log10(65025.0 * (double)m->pixels / (double)m->gray_sse);
}

double rt_frame_ssim(const rt_frame_metrics* m) {
    if (!m || m->windows == 0) return std::numeric_limits<double>::quiet_NaN();
    return m->ssim_sum / (double)m->windows;
}

double rt_frame_rmse(const rt_frame_metrics* m) {
    if (!m || m->finite_pixels == 0) return std::numeric_limits<double>::quiet_NaN();
    return sqrt(m->sq_err / (3.0 * (double)m->finite_pixels));
}

} // extern "C"
