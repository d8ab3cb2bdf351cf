/* rt_amd_h16_adaptive.h — the part of the rt_amd.h ABI that samples RT_PRECISION_FP16 worlds adaptively.  rt_amd.h includes it at its
 * end, after rt_amd_refine_fused.h, so a program that includes rt_amd.h has these declarations; including this file alone works too.
 * The Python binding lists them in rt_amd.SYMBOLS_H16_ADAPTIVE, and tests/test_h16_adaptive_abi_host.py holds that table to this file
 * as tests/test_host_and_abi.py holds rt_amd.SYMBOLS to rt_amd.h.  RT_ABI_VERSION stays: these are additions.
 *
 * Everything here is for binary16 worlds, and nothing that existed changes: rt_render_adaptive*, _begin, _refine, _fused,
 * _refine_fused and the spends keep answering RT_ENOTSUP for a binary16 world.  The call below is the fused form — the stop rule
 * inside the render kernel — and the only form: binary16 has no rounds, no active lists and no check kernels. */
#ifndef RT_AMD_H16_ADAPTIVE_H
#define RT_AMD_H16_ADAPTIVE_H
#include "rt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rt_render_adaptive_fused for a binary16 world (DESIGN.md 5.9 "Binary16"): its arguments in its order.  fb holds 3 x binary16 per
 * element.  Per sample of a pixel:
 *   - the colour sum is the reference's, in binary16, exactly as rt_render forms it: c = the binary16 value of the sample's colour,
 *     col = col + c per channel with one binary16 rounding; an absorbed path or one cut at depth 50 adds nothing;
 *   - the rule's statistics are binary32, formed from the exact images of c with one IEEE rounding per operation and no contraction:
 *     l = ((float)c.x + (float)c.y) + (float)c.z (0 for an absorbed path), SL = SL + l, Q = Q + l * l, in sample order.  (A binary16
 *     sum has an ulp of 2^-5 to 2^-4 once it passes 32 to 64: a rule fed from it would stall with it.)
 * After k = min_spp, min_spp + batch, ..., max_spp - batch samples the lane that renders the pixel applies rt_adaptive's rule to
 * (SL, Q, k); the pixel ends there when the rule holds, and at max_spp without being asked.  A pixel that ends after k samples is
 * rt_render(ns = k)'s pixel, bit for bit: fb gets real_t(1.0 / (double)float(real_t(k))) times the sum, rounded, then the root,
 * rounded; d_rand_state gets the state after k samples; d_spp (may be NULL) gets k.
 *   - d_state (may be NULL) gets the record in the layout of rt_render_adaptive_begin's state: RT_ADAPTIVE_STATE_BYTES per buffer
 *     element, six arrays of rt_part_pixels words S.r, S.g, S.b, SL, Q, k — S the exact binary32 images of the binary16 colour sums
 *     (the library's convention for binary16 values in float fields).
 *   - part = {0, 1, 0, 0} is the whole row-major frame; any other part works on its compact tile-major buffers (rt_part_pixels
 *     elements; the padding of edge tiles is never touched).
 * Launches: the scheduling pass rt_render runs for this world and part at ns = min_spp (kept and reused under that key) and ONE render
 * kernel, k_render_h<*,3>.  No adaptive workspace.  Asynchronous, no host synchronisation.
 * Refusals, before any device work and in this order: RT_EINVAL for bad parameters or sizes, an invalid partition, a part of more than
 * 2^32 - 1 elements; 0 and nothing launched for a part without tiles; RT_EINVAL for NULL fb / d_rand_state / params / world and for a
 * tree whose precision is not the world's; RT_ENOTSUP for a world that is not RT_PRECISION_FP16 (rt_render_adaptive_fused is the
 * binary32 call); RT_EINVAL on a capturing stream.  The _on forms answer RT_EINVAL without a context.
 * rt_render_ctx_times / rt_world_render_times report the render kernel's device time, rt_*_render_counters and rt_*_render_schedule
 * its launch; rt_render_kernel_name(world, d_octree, 3, ...) names the kernel. */
int rt_render_adaptive_h16(void* fb, int max_x, int max_y, const rt_adaptive* params, const rt_world* world,
                           rt_rand_state* d_rand_state, const rt_octree* d_octree, int32_t* d_spp, void* d_state,
                           rt_partition part, void* stream);
int rt_render_adaptive_h16_on(rt_render_ctx* ctx, void* fb, int max_x, int max_y, const rt_adaptive* params, const rt_world* world,
                              rt_rand_state* d_rand_state, const rt_octree* d_octree, int32_t* d_spp, void* d_state,
                              rt_partition part, void* stream);

/* Not offered for binary16: a refinement of the state (rt_render_adaptive_refine_fused has no binary16 twin: the state is written for
 * callers that read it, nothing in the library resumes from it), calls in rounds (rt_render_adaptive, _part, _begin, _refine), the
 * three spends, rt_multi_render_adaptive, stream capture, guides, denoising, temporal accumulation and rt_sequence; what the existing
 * adaptive entry points answer for a binary16 world (RT_ENOTSUP) is unchanged, and so is rt_render_kernel_name(world, d_octree, 4, ...). */

#ifdef __cplusplus
}
#endif
#endif /* RT_AMD_H16_ADAPTIVE_H */
