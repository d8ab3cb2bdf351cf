// rt_animate.hip — one resident world over a sequence of frames (rt_world_set_geometry, rt_temporal_accumulate_moving; include/rt_amd.h,
// DESIGN.md §5.10 "Moving scenes"): no reference counterpart.
//
// k_world_set_geometry rewrites every device array of a world that holds geometry (DevScene, rt_device.h) from the caller's
// (cx, cy, cz, radius) records: geom[i], the geometry half shade[2i] (the material half shade[2i + 1], with a dielectric's precomputed
// values, is left alone) and the hittable list's list_hot[j] = (c, r*r), i = list_id[j] — r*r as rt_world_create computes it: one
// binary32 multiply, or one binary16 multiply for a USE_FP16 world (the host's own half_t, so the bits agree).  One lane per world
// slot and per list slot, plain stores, no atomics, no LDS.
//
// k_temporal_accumulate_moving is the twin of k_temporal_accumulate (rt_temporal.hip): the same tile, the same rule with the MOVING
// lines of rt_temporal.h — the pixel's two geometry records are loaded with its guide halves, before the taps.
//
// Numeric contract: as rt_temporal.hip's — one IEEE binary32 rounding per operation, no contraction (also on the command line);
// tests/temporal_moving_model.py reproduces it bit for bit.
#include <hip/hip_runtime.h>
#include "../../include/rt_amd.h"
#include "rt_device.h"
#include "rt_launch.h"
#include "rt_real.h"
#include "rt_temporal.h"

#pragma clang fp contract(off)

namespace rt {

// list_id[j] < n (rt_world_create wrote it); src holds n records and is none of the world's own arrays
template <bool HALF>
__global__ __launch_bounds__(256) void k_world_set_geometry(float4* geom, float4* shade, float4* list_hot, const int32_t* list_id,
                                                            const float4* src, int n, int n_list) {
    const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;                  // (the grid covers max(n, n_list) <= n < 2^31 - 256)
    if (t < n) {
        const float4 g = src[t];
        geom[t] = g;
        shade[2 * (size_t)t] = g;
    }
    if (t < n_list) {
        const float4 g = src[list_id[t]];
        float r2;
        if constexpr (HALF) { const half_t r(g.w); r2 = (r * r).f(); }       // radius*radius in real_t (sphere.h:21)
        else r2 = g.w * g.w;
        list_hot[t] = make_float4(g.x, g.y, g.z, r2);
    }
}

// the arguments have been checked by rt_world_set_geometry (rt_api.hip): an uploaded world's arrays, n > 0, n_list <= n
hipError_t launch_world_set_geometry(float4* geom, float4* shade, float4* list_hot, const int32_t* list_id, const float4* src, int n, int n_list,
                                     bool half, hipStream_t st) {
    const unsigned blocks = (unsigned)(((long long)n + 255) / 256);
    if (half) hipLaunchKernelGGL(k_world_set_geometry<true>, dim3(blocks), dim3(256), 0, st, geom, shade, list_hot, list_id, src, n, n_list);
    else hipLaunchKernelGGL(k_world_set_geometry<false>, dim3(blocks), dim3(256), 0, st, geom, shade, list_hot, list_id, src, n, n_list);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_temporal_accumulate_moving(TemporalArgs T, TemporalMotion M) {
    const int tx = (int)(blockIdx.x % (unsigned)T.tiles_x), ty = (int)(blockIdx.x / (unsigned)T.tiles_x);
    const int i = tx * 16 + (int)(threadIdx.x & 15), j = ty * 16 + (int)(threadIdx.x >> 4);
    if (i >= T.max_x || j >= T.max_y) return;
    const int p = j * T.max_x + i;                                           // (n <= 2^30: p fits an int)
    const TemporalPixel R = temporal_pixel<true>(T, p, &M);
    T.out[p] = R.out;
    T.neff_out[p] = R.neff;
}

// the arguments have been checked by rt_temporal_accumulate_moving (rt_api.hip): as launch_temporal_accumulate's, and geom / geom_prev
// hold n_kind 16-byte aligned records (geom_prev == nullptr only with hist_in == nullptr)
hipError_t launch_temporal_accumulate_moving(void* hist_out, const void* hist_in, const rt_hit_record* hits, const rt_hit_record* hits_prev,
                                             const rt_camera* cam_prev, const float4* geom, const float4* geom_prev, const void* state,
                                             const int32_t* kind, int n_kind, int max_x, int max_y, const rt_temporal_params& P, hipStream_t st) {
    const TemporalArgs T = temporal_args(hist_out, hist_in, hits, hits_prev, cam_prev, state, kind, n_kind, max_x, max_y, P);
    const TemporalMotion M{geom, geom_prev};
    const unsigned blocks = (unsigned)T.tiles_x * (unsigned)((max_y + 15) / 16);
    hipLaunchKernelGGL(k_temporal_accumulate_moving, dim3(blocks), dim3(256), 0, st, T, M);
    return hipGetLastError();
}

} // namespace rt
