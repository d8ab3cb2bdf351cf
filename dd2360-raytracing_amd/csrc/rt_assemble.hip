// rt_assemble.hip — part buffers gathered into the row-major frame, for gfx950 (MI355X, CDNA4): ONE kernel, k_gather, for rt_assemble,
// rt_assemble_split and the multi-GPU renders after their exchange — colours in both precisions and the per-pixel sample counts of an
// adaptive frame, parts dealt in runs or cut into the bands of a balanced split.  Copies only: one lane per pixel of a tile, no
// arithmetic on the values.
#include <hip/hip_runtime.h>
#include "rt_device.h"
#include "rt_launch.h"

#pragma clang fp contract(off)

namespace rt {

// How a tile finds its owner and its place among the owner's tiles; passed to the kernel by value, so a runs launch carries no SplitStarts.
struct RunsOwner {            // runs of kPartRun tiles dealt round-robin (an rt_partition without a range)
    long long n_tiles;
    __device__ long long tiles(int) const { return n_tiles; }
    __device__ void operator()(long long tile, int nparts, int& owner, long long& local_tile) const { part_owner(tile, nparts, owner, local_tile); }
};
struct BandsOwner {           // bands of a balanced split (rt_split_balanced): band p holds the tiles [starts.s[p], starts.s[p + 1])
    SplitStarts starts;
    __device__ long long tiles(int nparts) const { return starts.s[nparts]; }
    __device__ void operator()(long long tile, int nparts, int& owner, long long& local_tile) const {
        owner = 0;
        for (int p = 1; p < nparts; ++p) owner += tile >= starts.s[p] ? 1 : 0;
        local_tile = tile - starts.s[owner];
    }
};

// Which element of which part is which pixel: part p's buffer begins part_stride_px elements behind part p - 1's and holds its tiles in
// their order, 64 elements a tile; CH values of type T per element.  One lane per pixel of a tile, four tiles a block.
template <class T, int CH, class Owner>
__global__ __launch_bounds__(256) void k_gather(T* full, const T* parts, int max_x, int max_y, int tiles_x, int nparts, long long part_stride_px, Owner own) {
    const int lane = threadIdx.x & 63;
    const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= own.tiles(nparts)) return;
    int tx, ty; tile_xy(tile, tiles_x, tx, ty);
    const int i = tile_px(tx, lane & 7), j = tile_px(ty, lane >> 3);
    if (i >= max_x || j >= max_y) return;
    int owner; long long local_tile;
    own(tile, nparts, owner, local_tile);
    const long long src = owner * part_stride_px + local_tile * 64 + lane;
    const long long dst = (long long)j * max_x + i;
#pragma unroll
    for (int c = 0; c < CH; ++c) full[dst * CH + c] = parts[src * CH + c];
}

template <class T, int CH, class Owner>
static void gather(void* full, const void* parts, int max_x, int max_y, int nparts, long long part_stride_px, long long tiles, const Owner& own, hipStream_t st) {
    hipLaunchKernelGGL((k_gather<T, CH, Owner>), dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, st, (T*)full, (const T*)parts, max_x, max_y, (max_x + 7) / 8, nparts,
                       part_stride_px, own);
}

hipError_t launch_gather(GatherElem elem, void* full, const void* parts, int max_x, int max_y, int nparts, const long long* starts, long long part_stride_px, hipStream_t st) {
    const long long tiles = (long long)((max_x + 7) / 8) * ((max_y + 7) / 8);
    if (starts) {
        BandsOwner own;
        for (int p = 0; p <= nparts; ++p) own.starts.s[p] = starts[p];
        if (elem == kGatherF32x3) gather<float, 3>(full, parts, max_x, max_y, nparts, part_stride_px, tiles, own, st);
        else if (elem == kGatherF16x3) gather<uint16_t, 3>(full, parts, max_x, max_y, nparts, part_stride_px, tiles, own, st);
        else return hipErrorInvalidValue;                     // (no frame moves its sample counts in bands)
    } else {
        const RunsOwner own{tiles};
        const long long stride = part_local_tiles(tiles, 0, nparts) * 64;
        if (elem == kGatherF32x3) gather<float, 3>(full, parts, max_x, max_y, nparts, stride, tiles, own, st);
        else if (elem == kGatherF16x3) gather<uint16_t, 3>(full, parts, max_x, max_y, nparts, stride, tiles, own, st);
        else gather<int32_t, 1>(full, parts, max_x, max_y, nparts, stride, tiles, own, st);
    }
    return hipGetLastError();
}

} // namespace rt
