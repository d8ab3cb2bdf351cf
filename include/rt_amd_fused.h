/* rt_amd_fused.h — the part of the rt_amd.h ABI that renders an adaptive frame in ONE launch.  rt_amd.h includes it at its end, so a
 * program that includes rt_amd.h has these declarations; including this file alone works too.  The Python binding lists them in
 * rt_amd.SYMBOLS_FUSED, and tests/test_fused_abi_host.py holds that table to this file as tests/test_host_and_abi.py holds
 * rt_amd.SYMBOLS to rt_amd.h.  RT_ABI_VERSION stays: these are additions. */
#ifndef RT_AMD_FUSED_H
#define RT_AMD_FUSED_H
#include "rt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rt_render_adaptive_begin's frame without its rounds (DESIGN.md 5.9 "Fused"): the stop rule of rt_adaptive runs inside the render
 * kernel.  Every pixel takes samples from its own RNG stream and, after min_spp, min_spp + batch, ..., max_spp - batch samples — the
 * checkpoints of the rounds —, the lane that renders it applies the rule to the pixel's running sums; the pixel ends there when the
 * rule holds, and at max_spp without being asked.  A pixel is a truncation of its own stream, and the sums are formed in the same
 * order, so the result is the rounds' result, byte for byte:
 *   - d_state != NULL: after the call fb, d_spp, d_rand_state and d_state hold what rt_render_adaptive_begin leaves for the same
 *     arguments on the same initial buffers; rt_render_adaptive_refine, every rt_render_adaptive_spend*, rt_denoise_adaptive and
 *     rt_temporal_accumulate* accept the state as they accept begin's;
 *   - d_state == NULL: fb, d_spp and d_rand_state hold what rt_render_adaptive_part leaves; no sum touches memory;
 *   - d_spp may be NULL; part = {0, 1, 0, 0} is the whole row-major frame, any other part works on its compact tile-major buffers
 *     (rt_part_pixels elements; the padding of edge tiles is never touched).
 * Launches: the scheduling pass of rt_render_adaptive_begin's round 0 (rt_render's pass for ns = min_spp, kept and reused under the
 * same key: begin and the fused call share a context's record) and ONE render kernel, k_render<*,3,*>.  No active lists, no check
 * kernels; the context's adaptive workspace is neither needed nor grown.  Asynchronous, no host synchronisation.
 * Refusals, those of rt_render_adaptive_begin in its order: RT_EINVAL for bad parameters, an invalid partition, a part of more than
 * 2^32 - 1 elements, NULL fb / d_rand_state / params / world, a tree of another precision, a capturing stream; RT_ENOTSUP for
 * RT_PRECISION_FP16 and RT_ARITH_CONTRACT worlds; 0 and nothing launched for a part without tiles.
 * rt_render_ctx_times / rt_world_render_times report the render kernel's device time, rt_render_ctx_counters and
 * rt_render_ctx_schedule its launch; rt_render_kernel_name(world, d_octree, 3, ...) names the kernel.
 * Not offered: stream capture, a fused spend (a spend selects between its rounds).  The fused refine: rt_amd_refine_fused.h.
 * A binary16 world has a call of its own, rt_render_adaptive_h16 (rt_amd_h16_adaptive.h). */
int rt_render_adaptive_fused(void* fb, int max_x, int max_y, const rt_adaptive* params, const rt_world* world,
                             rt_rand_state* d_rand_state, const rt_octree* d_octree, int32_t* d_spp, void* d_state,
                             rt_partition part, void* stream);
int rt_render_adaptive_fused_on(rt_render_ctx* ctx, void* fb, int max_x, int max_y, const rt_adaptive* params, const rt_world* world,
                                rt_rand_state* d_rand_state, const rt_octree* d_octree, int32_t* d_spp, void* d_state,
                                rt_partition part, void* stream);

/* on = 1: rt_multi_render_adaptive renders each rank's part with rt_render_adaptive_fused_on in place of rt_render_adaptive_part_on;
 * lanes, exchange and assembly are untouched, and so are the bits the root receives.  on = 0 (the default): the rounds.
 * RT_EINVAL for a NULL handle or another value. */
int rt_multi_set_adaptive_fused(rt_multi* m, int on);

#ifdef __cplusplus
}
#endif
#endif /* RT_AMD_FUSED_H */
