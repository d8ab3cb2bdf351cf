/* rt_amd_refine_fused.h — the part of the rt_amd.h ABI that refines an adaptive frame in ONE render launch.  rt_amd.h includes it at its
 * end, after rt_amd_fused.h, so a program that includes rt_amd.h has these declarations; including this file alone works too.  The
 * Python binding lists them in rt_amd.SYMBOLS_REFINE_FUSED, and tests/test_refine_fused_abi_host.py holds that table to this file as
 * tests/test_host_and_abi.py holds rt_amd.SYMBOLS to rt_amd.h.  RT_ABI_VERSION stays: these are additions. */
#ifndef RT_AMD_REFINE_FUSED_H
#define RT_AMD_REFINE_FUSED_H
#include "rt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rt_render_adaptive_refine without its rounds (DESIGN.md 5.9 "Fused refinement"): rt_render_adaptive_refine's arguments in its order,
 * and its result.  d_state holds a frame left at target `from`; a seed pass finalises again the pixels that `to` stops where they are
 * and lists the others, and one render kernel runs over that list: every listed pixel resumes from the state — its k samples, its
 * sums, its RNG state — and after k + batch, k + 2 batch, ... samples, the checkpoints of the resumed rounds, the lane that renders
 * it applies the rule of `to` to the running sums; the pixel ends there when the rule holds, and at to->max_spp without being asked.
 * The sums are formed by the same operations in the same order as the rounds form them, so:
 *   - afterwards fb, d_spp, d_rand_state and d_state hold what rt_render_adaptive_refine(from -> to) leaves on the same buffers, byte
 *     for byte — which is what rt_render_adaptive_begin(to) would have left;
 *   - the state may come from rt_render_adaptive_begin, from rt_render_adaptive_fused, or from a chain of refinements of either kind,
 *     and what this call leaves is accepted by everything that accepts begin's state (rt_render_adaptive_refine, this call, every
 *     rt_render_adaptive_spend*, rt_denoise_adaptive, rt_temporal_accumulate*);
 *   - d_spp may be NULL; fb and d_spp are written, never read; part = {0, 1, 0, 0} is the whole row-major frame, any other part
 *     works on its compact tile-major buffers (rt_part_pixels elements; the padding of edge tiles is never touched).
 * Launches: the zeroing of one count word, k_adapt_refine_seed, the zeroing of one counter slot, and ONE render kernel,
 * k_render<*,4,*> — whatever (max_spp - min_spp) / batch is.  No check kernel, no scheduling pass.  The context's adaptive workspace
 * holds the list and its count: no more than rt_render_adaptive_refine reserves for one round.  Asynchronous, no host synchronisation.
 * Refusals, those of rt_render_adaptive_refine in its order: RT_EINVAL for parameters that are invalid or where `to` does not refine
 * `from` (rt_render_adaptive_refine's rule), NULL from / to / world, an invalid partition, a part of more than 2^32 - 1 elements,
 * NULL fb / d_rand_state / d_state, a tree of another precision, a capturing stream; RT_ENOTSUP for RT_PRECISION_FP16 and
 * RT_ARITH_CONTRACT worlds; 0 and nothing launched for a part without tiles.
 * rt_render_ctx_times / rt_world_render_times report the device time of the seed and the render kernel together, as
 * rt_render_adaptive_refine reports its seed and rounds; rt_render_kernel_name(world, d_octree, 4, ...) names the kernel.
 * Not offered: stream capture, a fused spend (a spend selects between its rounds), binary16 worlds (rt_amd_h16_adaptive.h has the
 * adaptive frame for them, and no refinement: DESIGN.md 5.9 "Binary16"). */
int rt_render_adaptive_refine_fused(void* fb, int max_x, int max_y, const rt_adaptive* from, const rt_adaptive* to, const rt_world* world,
                                    rt_rand_state* d_rand_state, const rt_octree* d_octree, int32_t* d_spp, void* d_state,
                                    rt_partition part, void* stream);
int rt_render_adaptive_refine_fused_on(rt_render_ctx* ctx, void* fb, int max_x, int max_y, const rt_adaptive* from, const rt_adaptive* to,
                                       const rt_world* world, rt_rand_state* d_rand_state, const rt_octree* d_octree, int32_t* d_spp,
                                       void* d_state, rt_partition part, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_AMD_REFINE_FUSED_H */
