// rt_assemble.hip — part buffers gathered into the row-major frame, for gfx950 (MI355X, CDNA4): rt_assemble and the multi-GPU
// renders after their all-gather (k_assemble, k_assemble_spp for the per-pixel sample counts), and the bands of a balanced split
// (k_assemble_split, both precisions).  Copies only: one lane per pixel of a tile, no arithmetic on the values.  The binary16 twin of
// k_assemble, k_assemble_h, stays with the binary16 kernels (rt_kernels_fp16.hip).
#include <hip/hip_runtime.h>
#include "rt_device.h"
#include "rt_launch.h"

#pragma clang fp contract(off)

namespace rt {

// gather of tile-major part buffers into the row-major frame (after the multi-GPU all-gather)
__global__ __launch_bounds__(256) void k_assemble(float* full, const float* parts, int max_x, int max_y, int tiles_x, int nparts, long long part_stride_px, long long n_tiles) {
    const int lane = threadIdx.x & 63;
    const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const int tx = (int)(tile % tiles_x), ty = (int)(tile / tiles_x);
    const int i = tx * 8 + (lane & 7), j = ty * 8 + (lane >> 3);
    if (i >= max_x || j >= max_y) return;
    int owner; long long local_tile;
    part_owner(tile, nparts, owner, local_tile);
    const long long src = owner * part_stride_px + local_tile * 64 + lane;
    const long long dst = (long long)j * max_x + i;
    full[dst * 3 + 0] = parts[src * 3 + 0]; full[dst * 3 + 1] = parts[src * 3 + 1]; full[dst * 3 + 2] = parts[src * 3 + 2];
}
// its one-channel twin: the per-pixel sample counts of an adaptive multi-GPU frame (rt_multi_render_adaptive), one word per pixel
__global__ __launch_bounds__(256) void k_assemble_spp(int32_t* full, const int32_t* parts, int max_x, int max_y, int tiles_x, int nparts, long long part_stride_px, long long n_tiles) {
    const int lane = threadIdx.x & 63;
    const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;
    const int tx = (int)(tile % tiles_x), ty = (int)(tile / tiles_x);
    const int i = tx * 8 + (lane & 7), j = ty * 8 + (lane >> 3);
    if (i >= max_x || j >= max_y) return;
    int owner; long long local_tile;
    part_owner(tile, nparts, owner, local_tile);
    full[(long long)j * max_x + i] = parts[owner * part_stride_px + local_tile * 64 + lane];
}

// the same for the bands of a balanced split (rt_split_balanced): band p holds the tiles [starts.s[p], starts.s[p + 1]), its buffer begins
// part_stride_px elements behind band p - 1's.  One kernel for both precisions (T = float / uint16_t).
template <class T>
__global__ __launch_bounds__(256) void k_assemble_split(T* full, const T* parts, int max_x, int max_y, int tiles_x, int nparts, long long part_stride_px, SplitStarts starts) {
    const int lane = threadIdx.x & 63;
    const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= starts.s[nparts]) return;
    const int tx = (int)(tile % tiles_x), ty = (int)(tile / tiles_x);
    const int i = tx * 8 + (lane & 7), j = ty * 8 + (lane >> 3);
    if (i >= max_x || j >= max_y) return;
    int owner = 0;
    for (int p = 1; p < nparts; ++p) owner += tile >= starts.s[p] ? 1 : 0;
    const long long src = owner * part_stride_px + (tile - starts.s[owner]) * 64 + lane;
    const long long dst = (long long)j * max_x + i;
    full[dst * 3 + 0] = parts[src * 3 + 0]; full[dst * 3 + 1] = parts[src * 3 + 1]; full[dst * 3 + 2] = parts[src * 3 + 2];
}
hipError_t launch_assemble_split(void* full, const void* parts, int max_x, int max_y, int nparts, const long long* starts, long long part_stride_px, bool half, hipStream_t st) {
    SplitStarts S;
    for (int p = 0; p <= nparts; ++p) S.s[p] = starts[p];
    const int tiles_x = (max_x + 7) / 8;
    const unsigned blocks = (unsigned)((starts[nparts] + 3) / 4);
    if (half) hipLaunchKernelGGL((k_assemble_split<uint16_t>), dim3(blocks), dim3(256), 0, st, (uint16_t*)full, (const uint16_t*)parts, max_x, max_y, tiles_x, nparts, part_stride_px, S);
    else hipLaunchKernelGGL((k_assemble_split<float>), dim3(blocks), dim3(256), 0, st, (float*)full, (const float*)parts, max_x, max_y, tiles_x, nparts, part_stride_px, S);
    return hipGetLastError();
}

hipError_t launch_assemble(float* full, const float* parts, int max_x, int max_y, int nparts, hipStream_t st) {
    const int tiles_x = (max_x + 7) / 8, tiles_y = (max_y + 7) / 8;
    const long long tiles = (long long)tiles_x * tiles_y;
    const long long per_part = part_local_tiles(tiles, 0, nparts) * 64;
    const unsigned blocks = (unsigned)((tiles + 3) / 4);
    hipLaunchKernelGGL(k_assemble, dim3(blocks), dim3(256), 0, st, full, parts, max_x, max_y, tiles_x, nparts, per_part, tiles);
    return hipGetLastError();
}
hipError_t launch_assemble_spp(int32_t* full, const int32_t* parts, int max_x, int max_y, int nparts, hipStream_t st) {
    const int tiles_x = (max_x + 7) / 8, tiles_y = (max_y + 7) / 8;
    const long long tiles = (long long)tiles_x * tiles_y;
    const long long per_part = part_local_tiles(tiles, 0, nparts) * 64;
    const unsigned blocks = (unsigned)((tiles + 3) / 4);
    hipLaunchKernelGGL(k_assemble_spp, dim3(blocks), dim3(256), 0, st, full, parts, max_x, max_y, tiles_x, nparts, per_part, tiles);
    return hipGetLastError();
}

} // namespace rt
