// rt_rectify.hip — history rectification (rt_temporal_accumulate_rectified; include/rt_amd.h, DESIGN.md §5.10 "History rectification"):
// no reference counterpart.
//
// k_temporal_accumulate_rectified<MOVING, R> is k_temporal_accumulate (MOVING: k_temporal_accumulate_moving) with one more step for a
// pixel that has taken history: the history's luminance is held against the mean and deviation of THIS frame's luminance over the
// (2R+1)^2 window around the pixel, and a history that lies further out than gamma deviations sheds effective samples before the merge.
// The rule itself is temporal_pixel_from (rt_temporal.h) with RectifyHook in its hook; nothing of it is restated here.
//
// A block is the 16x16 tile of the twin kernels, one lane per pixel.  Before any tap the block stages the tile and an apron of R
// pixels in LDS, two dwords per pixel (l_q and the sphere word): every lane computes its own pixel's frame values (temporal_frame — the
// values the rule needs afterwards anyway) and stores them, and the first (16+2R)^2 - 256 lanes do the same for one apron pixel each
// (68 at R = 1, 144 at R = 2: 24 B of state and one 16-byte guide half a pixel; the unused guide half is never loaded).  A pixel
// outside the frame and an EMPTY pixel are stored with the sphere word -1.  A pixel that reaches the hook is not EMPTY, so its own
// sphere word is not -1, and the one test "sphere word == mine" skips the three kinds of tap the rule skips: no bounds test at a tap.
// Every lane of the block reaches the barrier; lanes outside the frame leave after it.
//
// LDS layout: two planes of dwords, l and sphere, each of 16 + 2R rows of STRIDE = 48 dwords.  A tap is one ds_read_b32 per plane (or
// half of a ds_read2_b32, which is served as two of them): bank (a/4) mod 32, served per 32-lane half.  A half-wave is two tile rows of
// 16 lanes; at a tap (dx, dy) each row reads 16 consecutive dwords and the second row lies STRIDE dwords further on, so the two runs
// use 32 different banks exactly when STRIDE mod 32 = 16.  A row holds 16 + 2R <= 20 dwords, so 48 is the smallest such stride (16 is
// too short); with the natural strides 18 and 20 the runs share 2 and 4 banks, a 2-way conflict at every tap.  Slots of 8 bytes
// (l and sphere side by side) were built first and dropped: the compiler reads them as ds_read2_b32, lanes 2 dwords apart, which
// leaves a half-wave 16 banks for 32 addresses at any stride.  The staging stores of the tile (ds_write_b32, same banking) are the same
// two runs: conflict-free; the apron's runs break at a row end, a 2-way conflict on a few groups once per block.  7680 B a block at
// R = 2, 6912 B at R = 1.
//
// Numeric contract: as rt_temporal.hip's — one IEEE binary32 rounding per operation, no contraction (also on the command line), sums
// in window order; tests/temporal_rectify_model.py reproduces it bit for bit.
#include <hip/hip_runtime.h>
#include "../../include/rt_amd.h"
#include "rt_device.h"
#include "rt_launch.h"
#include "rt_temporal.h"

#pragma clang fp contract(off)

namespace rt {

constexpr int RECTIFY_STRIDE = 48;           // dwords per LDS row: = 16 mod 32, see above

struct RectifyArgs { float gamma, g2, min_count; };      // gamma, gamma * gamma rounded once on the host, (float)min_count

// the window test of one pixel; lc and sc point at the pixel's own dwords in the two staged planes
template <int R>
struct RectifyHook {
    const float* lc; const int* sc;
    RectifyArgs Q;
    __device__ __forceinline__ float operator()(float m, float hx, float hy, float hz, int sp) const {
        if (Q.gamma == 0.0f) return m;
        constexpr int D = 2 * R + 1;
        float l[D * D]; bool in[D * D];
        float cnt = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int u = 0; u < D * D; ++u) {                                        // dy outer, both from -R
            const int o = (u / D - R) * RECTIFY_STRIDE + (u % D - R);
            l[u] = lc[o];
            in[u] = sc[o] == sp;                                                 // outside the frame and EMPTY are staged as -1
            if (in[u]) { cnt = cnt + 1.0f; s1 = s1 + l[u]; }
        }
        const float ml = s1 / cnt;
        float ss = 0.0f;
#pragma unroll
        for (int u = 0; u < D * D; ++u)
            if (in[u]) ss = ss + (l[u] - ml) * (l[u] - ml);
        const float s2 = ss / (cnt - 1.0f);
        if (cnt >= Q.min_count) {
            const float lh = (hx + hy) + hz;
            const float dl = lh - ml;
            const float e2 = dl * dl;
            const float lim = Q.g2 * s2;
            if (e2 > lim) m = m * (lim / e2);                                    // (a NaN keeps m)
        }
        return m;
    }
};

struct RectifySlot { float l; int sphere; };
__device__ __forceinline__ RectifySlot rectify_slot(const TemporalFrame& f) {
    return f.empty ? RectifySlot{0.0f, -1} : RectifySlot{(f.c.x + f.c.y) + f.c.z, f.sp};
}

template <bool MOVING, int R>
__global__ __launch_bounds__(256) void k_temporal_accumulate_rectified(TemporalArgs T, TemporalMotion M, RectifyArgs Q) {
    constexpr int W = 16 + 2 * R, APRON = W * W - 256, BAND = 2 * R * W;         // BAND: the apron's full rows, above and below the tile
    static_assert(APRON <= 256 && W <= RECTIFY_STRIDE, "one apron pixel per lane at the most");
    __shared__ float tile_l[W * RECTIFY_STRIDE];
    __shared__ int tile_s[W * RECTIFY_STRIDE];
    const int tx = (int)(blockIdx.x % (unsigned)T.tiles_x), ty = (int)(blockIdx.x / (unsigned)T.tiles_x);
    const int lx = (int)(threadIdx.x & 15), ly = (int)(threadIdx.x >> 4);
    const int i = tx * 16 + lx, j = ty * 16 + ly;
    const bool inside = i < T.max_x && j < T.max_y;
    const int p = inside ? j * T.max_x + i : 0;                              // (n <= 2^30: p fits an int)
    TemporalFrame F{};
    RectifySlot own{0.0f, -1};
    if (inside) { F = temporal_frame(T, p); own = rectify_slot(F); }
    const int mine = (ly + R) * RECTIFY_STRIDE + (lx + R);
    tile_l[mine] = own.l; tile_s[mine] = own.sphere;
    if ((int)threadIdx.x < APRON) {
        int a = (int)threadIdx.x, sx, sy;
        if (a < BAND) { sy = a / W; sx = a % W; if (sy >= R) sy += 16; }
        else { a -= BAND; sy = R + a / (2 * R); sx = a % (2 * R); if (sx >= R) sx += 16; }
        const int qi = tx * 16 - R + sx, qj = ty * 16 - R + sy;
        RectifySlot v{0.0f, -1};
        if (qi >= 0 && qi < T.max_x && qj >= 0 && qj < T.max_y) v = rectify_slot(temporal_frame(T, qj * T.max_x + qi));
        tile_l[sy * RECTIFY_STRIDE + sx] = v.l; tile_s[sy * RECTIFY_STRIDE + sx] = v.sphere;
    }
    __syncthreads();
    if (!inside) return;
    const RectifyHook<R> hook{&tile_l[mine], &tile_s[mine], Q};
    const TemporalPixel P = temporal_pixel_from<MOVING>(T, F, &M, hook);
    T.out[p] = P.out;
    T.neff_out[p] = P.neff;
}

// the arguments have been checked by rt_temporal_accumulate_rectified (rt_api.hip): as launch_temporal_accumulate_moving's, radius 1 or
// 2; geom_prev == nullptr selects the static rule
hipError_t launch_temporal_accumulate_rectified(void* hist_out, const void* hist_in, const rt_hit_record* hits, const rt_hit_record* hits_prev,
                                                const rt_camera* cam_prev, const float4* geom, const float4* geom_prev, const void* state,
                                                const int32_t* kind, int n_kind, int max_x, int max_y, const rt_temporal_params& P,
                                                const rt_temporal_rectify& Rc, hipStream_t st) {
    const TemporalArgs T = temporal_args(hist_out, hist_in, hits, hits_prev, cam_prev, state, kind, n_kind, max_x, max_y, P);
    const TemporalMotion M{geom, geom_prev};
    const RectifyArgs Q{Rc.gamma, Rc.gamma * Rc.gamma, (float)Rc.min_count};
    const dim3 blocks((unsigned)T.tiles_x * (unsigned)((max_y + 15) / 16));
    const bool moving = geom_prev != nullptr;
    if (Rc.radius == 1) {
        if (moving) hipLaunchKernelGGL((k_temporal_accumulate_rectified<true, 1>), blocks, dim3(256), 0, st, T, M, Q);
        else hipLaunchKernelGGL((k_temporal_accumulate_rectified<false, 1>), blocks, dim3(256), 0, st, T, M, Q);
    } else {
        if (moving) hipLaunchKernelGGL((k_temporal_accumulate_rectified<true, 2>), blocks, dim3(256), 0, st, T, M, Q);
        else hipLaunchKernelGGL((k_temporal_accumulate_rectified<false, 2>), blocks, dim3(256), 0, st, T, M, Q);
    }
    return hipGetLastError();
}

} // namespace rt
