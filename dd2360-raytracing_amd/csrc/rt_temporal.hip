// rt_temporal.hip — temporal accumulation (rt_temporal_accumulate, rt_denoise_history; include/rt_amd.h): no reference
// counterpart.
//
// k_temporal_accumulate turns the adaptive state of this frame and the history of the last one into this frame's history: per pixel the
// mean colour, the variance of the mean luminance and the effective sample count (float4 + float, RT_TEMPORAL_HISTORY_BYTES).  A block is
// a 16x16 pixel tile, one lane per pixel, as in the level kernels of rt_denoise.hip: the first hit of the pixel is projected through the
// previous camera and the four pixels around the landing point are gathered — their effective count, both 16-byte halves of their guide
// record and their float4 history, straight through the caches (a tile lands on a few rows of the previous frame; which ones depends on
// the camera, so there is no fixed apron to stage in LDS).  The four taps' loads are issued before any of them is tested.  One launch,
// no atomics, no LDS.
//
// k_denoise_hist_prepare is the prepare step of rt_denoise_history: the workspace's float4 from a history instead of from the state;
// the levels are k_denoise_var_level, launched by rt_denoise.hip's launch_denoise_var_levels.
//
// Numeric contract: one IEEE binary32 rounding per operation in the order the header states, no contraction (also on the command line),
// correctly rounded division (hipcc default), sums in tap order — tests/temporal_model.py reproduces it bit for bit.
#include <hip/hip_runtime.h>
#include "../../include/rt_amd.h"
#include "rt_device.h"
#include "rt_launch.h"
#include "rt_temporal.h"

#pragma clang fp contract(off)

namespace rt {

// the rule itself is temporal_pixel (rt_temporal.h), shared with the history-aware budget key (k_budget_keys_temporal, rt_budget.hip)
__global__ __launch_bounds__(256) void k_temporal_accumulate(TemporalArgs T) {
    const int tx = (int)(blockIdx.x % (unsigned)T.tiles_x), ty = (int)(blockIdx.x / (unsigned)T.tiles_x);
    const int i = tx * 16 + (int)(threadIdx.x & 15), j = ty * 16 + (int)(threadIdx.x >> 4);
    if (i >= T.max_x || j >= T.max_y) return;
    const int p = j * T.max_x + i;                                           // (n <= 2^30: p fits an int)
    const TemporalPixel R = temporal_pixel(T, p);
    T.out[p] = R.out;
    T.neff_out[p] = R.neff;
}

// the arguments have been checked by rt_temporal_accumulate (rt_api.hip): 16-byte aligned histories and guides, max_x * max_y <= 2^30,
// no overlap of the two histories; hist_in == nullptr: the first frame (hits_prev and cam_prev are then not looked at)
hipError_t launch_temporal_accumulate(void* hist_out, const void* hist_in, const rt_hit_record* hits, const rt_hit_record* hits_prev,
                                      const rt_camera* cam_prev, const void* state, const int32_t* kind, int n_kind, int max_x, int max_y,
                                      const rt_temporal_params& P, hipStream_t st) {
    const TemporalArgs T = temporal_args(hist_out, hist_in, hits, hits_prev, cam_prev, state, kind, n_kind, max_x, max_y, P);
    const unsigned blocks = (unsigned)T.tiles_x * (unsigned)((max_y + 15) / 16);
    hipLaunchKernelGGL(k_temporal_accumulate, dim3(blocks), dim3(256), 0, st, T);
    return hipGetLastError();
}

// rt_denoise_history's prepare: mean colour and variance from the history; a pass-through pixel (nothing accumulated, or a value that is
// not finite — or a negative variance, which accumulate never writes and the level kernels read as the pass-through mark) holds the
// bits of fb_in and .w = -1, as k_denoise_var_prepare leaves it
__global__ __launch_bounds__(256) void k_denoise_hist_prepare(float4* x, const float* fb_in, const float4* hist, const float* neff, int n) {
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (p >= n) return;
    float4 v = hist[p];
    if (neff[p] == 0.0f || !__builtin_isfinite(v.x) || !__builtin_isfinite(v.y) || !__builtin_isfinite(v.z) || !__builtin_isfinite(v.w) || v.w < 0.0f) {
        const long long e = 3 * (long long)p;
        v.x = fb_in[e]; v.y = fb_in[e + 1]; v.z = fb_in[e + 2];
        v.w = -1.0f;
    }
    x[p] = v;
}

// the whole filter on `st`; the arguments have been checked by rt_denoise_history (as launch_denoise_var's; `hist` is only read)
hipError_t launch_denoise_hist(float* fb_out, const float* fb_in, int max_x, int max_y, const rt_hit_record* hits, const void* hist,
                               const rt_denoise_var_params& P, float4* work, hipStream_t st) {
    const int n = max_x * max_y;
    const float4* h = (const float4*)hist;
    hipLaunchKernelGGL(k_denoise_hist_prepare, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, work, fb_in, h, (const float*)(h + n), n);
    return launch_denoise_var_levels(fb_out, max_x, max_y, hits, P, work, st);
}

} // namespace rt
