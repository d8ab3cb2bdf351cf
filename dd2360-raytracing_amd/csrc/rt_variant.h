// rt_variant.h — the walk variants of the binary32 render path, named ONCE.  Plain host C++, no HIP: rt_sched_keep.h includes it.
// A variant is how k_render, k_tile_cost, k_trace and k_guides find a ray's spheres.  Its value is the kernels' COOPG template argument
// (the list scan's kernels are <false, .., 1>) and so part of every kernel symbol that tests, bench.py, tools/regs.sh and rocprofv3 match
// on: the values never change.  render_variant (rt_launch.h) picks one per launch, with_walk (rt_kernels.hip) turns it into the template
// argument; what host code needs to know ABOUT a variant is a predicate below, not a compare of its own.
#pragma once
namespace rt {

enum : int {
    kVariantList = 0,       // k_render<false,MODE,1>: the hitable_list scan
    kVariantTree = 1,       // <true,MODE,1>: per-lane walk — trees without a candidate grid, the reference's traversal
    kVariantDense = 2,      // <true,MODE,2>: dense grids, walk_pool_dense
    kVariantSparse = 4,     // <true,MODE,4>: sparse grids, walk_pool
    kVariantSolo = 5,       // <true,MODE,5>: very sparse grids, walk_pool with the pilot's longest chains in waves of their own
};
// the wave's sphere tests are pooled: a block needs one WalkLds per wave and the hot spheres behind its nodes
constexpr bool variant_pooled(int v) { return v == kVariantDense || v == kVariantSparse || v == kVariantSolo; }
// the ordering pass takes the dense knobs: f_inflight_dense, head_sum_dense, head_min_load
constexpr bool variant_dense(int v) { return v == kVariantDense; }
// the pilot's sums already start solo chains (RT_PILOT_SOLO_SUM)
constexpr bool variant_solo_pilot(int v) { return v == kVariantSolo; }
// k_render records every pixel's iteration count (iters_out): the launches the measured pass can rebuild (rt_sched_keep.h "Feedback")
constexpr bool variant_records_counts(int v) { return v == kVariantSparse || v == kVariantSolo; }

}  // namespace rt
