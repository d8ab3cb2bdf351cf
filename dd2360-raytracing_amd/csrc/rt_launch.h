// rt_launch.h — the launch surface: every function that one .hip file of the library defines and another one calls, declared ONCE.
// The defining file and every calling file include this header, so a changed parameter or return type is a compile error in the
// file that changed it, not a link error (or nothing at all) somewhere else.  Grouped by the file that holds the definition.
#pragma once
#include <hip/hip_runtime.h>
#include "rt_device.h"
#include "rt_variant.h"

namespace rt {

// ---- rt_kernels.hip: the render path in binary32 (what traces rays, and k_render_init)
hipError_t launch_render_init(rt_rand_state* rs, int max_x, int max_y, int part, int nparts, long long begin, long long end, hipStream_t st);
hipError_t launch_pilot(const RenderArgs& A, bool tree, int* cost, unsigned char* pilot, int* work, hipStream_t st);
hipError_t launch_tile_order(const RenderArgs& A, bool tree, int* cost, unsigned int* order, unsigned char* flags, unsigned int* long_list, hipStream_t st);
hipError_t launch_count_order(const RenderArgs& A, const unsigned short* iters, int* cost, unsigned int* order, unsigned char* flags, unsigned int* long_list,
                              float solo_frac, int solo_cap_den, unsigned int* extra, hipStream_t st);
// (the ONE render launcher of a backend: k_render's MODE 0 to 4, rt_device.h; a mode the backend has no kernel for is hipErrorInvalidValue)
hipError_t launch_render(const RenderArgs& A, bool tree, int mode, hipStream_t st);
hipError_t launch_trace(const DevScene& S, const DevTree& T, bool tree, const float* rays, long long n, rt_hit_record* out, hipStream_t st);
hipError_t launch_guides(const DevScene& S, const DevTree& T, bool tree, int max_x, int max_y, rt_hit_record* out, hipStream_t st);
int render_variant(bool tree, const DevAccel& acc);             // a kVariant* of rt_variant.h
unsigned resident_blocks(const void* kernel, size_t lds);
const char* render_kernel_name(bool tree, int mode, const DevAccel& acc);
#ifdef RT_STATS
hipError_t read_stats(unsigned long long* out, int reset);
hipError_t read_wp_classes(unsigned long long* out, int reset);
hipError_t read_wave_dbg(unsigned long long* out);
hipError_t read_pilot_dbg(int* out, int n);
hipError_t read_chain_dbg(unsigned int* out, int n_pixels);
#endif
// ---- rt_kernels_list.hip: the hitable_list instantiations, called by the launchers above
hipError_t launch_tile_cost_list(const RenderArgs& A, unsigned blocks, int* cost, unsigned char* pilot, hipStream_t st);
hipError_t launch_render_list(const RenderArgs& A, int mode, hipStream_t st);
hipError_t launch_trace_list(const RenderArgs& A, unsigned blocks, const float* rays, long long n, rt_hit_record* out, hipStream_t st);
hipError_t launch_guides_list(const RenderArgs& A, unsigned blocks, long long n, rt_hit_record* out, hipStream_t st);
// ---- rt_kernels_contract.hip: k_render with FMA contraction allowed (rt_world_set_arith(RT_ARITH_CONTRACT)), modes 0 and 1; nothing else is contracted
namespace fmac { hipError_t launch_render(const RenderArgs& A, bool tree, int mode, hipStream_t st); }

// ---- rt_schedule.hip: the integer kernels of the scheduling pass and the counters of a launch's queue slot
hipError_t launch_zero_counters(unsigned int* p, int n, hipStream_t st);
hipError_t launch_keep_counters(const unsigned int* queue, unsigned int* kept, hipStream_t st);
hipError_t launch_restore_counters(unsigned int* queue, const unsigned int* kept, hipStream_t st);
hipError_t launch_count_cost(const RenderArgs& A, const unsigned short* iters, int* cost, unsigned char* pilot, hipStream_t st);
// (counted != NULL: the measured pass — the selection reads the recorded counts, k_count_select, instead of the pilot's sums)
struct CountedSelect { const unsigned short* iters; float solo_frac; unsigned int solo_cap; unsigned int* extra; };
hipError_t launch_select_and_order(const RenderArgs& A, int* cost, unsigned int* order, unsigned char* flags, unsigned int* long_list, hipStream_t st, int long_sum, int solo_sum,
                                   const CountedSelect* counted = nullptr);

// ---- rt_adaptive.hip: the checks between the rounds of rt_render_adaptive and its refinement
hipError_t launch_adapt_check(float* fb, const float* sl, const float* q, const unsigned int* list_in, const unsigned int* count_in, long long n_all,
                              unsigned int* list_out, unsigned int* count_out, int32_t* spp, int k, bool last, float rel_error, float floor_lum,
                              const AdaptFrame& fr, hipStream_t st);
hipError_t launch_adapt_check_keep(float* fb, const AdaptState& s, const unsigned int* list_in, const unsigned int* count_in, long long n_all,
                                   unsigned int* list_out, unsigned int* count_out, int32_t* spp, int k, bool last, float rel_error, float floor_lum,
                                   const AdaptFrame& fr, hipStream_t st);
hipError_t launch_adapt_refine_seed(float* fb, const AdaptState& s, long long n_all, unsigned int* list_out, unsigned int* count_out, int32_t* spp,
                                    int max_spp, float rel_error, float floor_lum, const AdaptFrame& fr, hipStream_t st);
hipError_t launch_adapt_refine_check(float* fb, const AdaptState& s, const unsigned int* list_in, const unsigned int* count_in, long long n_all,
                                     unsigned int* list_out, unsigned int* count_out, int32_t* spp, int batch, int max_spp, float rel_error, float floor_lum,
                                     hipStream_t st);
hipError_t launch_adapt_zero(unsigned int* p, int n, hipStream_t st);

// ---- rt_assemble.hip: part buffers gathered into the row-major frame
// (what an element is: 3 floats, 3 halves, one int32; starts == nullptr: parts in runs, each padded to part 0's size — else the
// starts[nparts + 1] of a balanced split's bands, band p's buffer part_stride_px elements behind band p - 1's)
enum GatherElem { kGatherF32x3, kGatherF16x3, kGatherI32x1 };
hipError_t launch_gather(GatherElem elem, void* full, const void* parts, int max_x, int max_y, int nparts, const long long* starts, long long part_stride_px, hipStream_t st);

// ---- rt_kernels_fp16.hip: the render path in binary16 (launch_render_h: modes 0, 1 and 3)
hipError_t launch_pilot_h(const RenderArgs& A, bool tree, int* cost, unsigned char* pilot, hipStream_t st);
hipError_t launch_tile_order_h(const RenderArgs& A, bool tree, int* cost, unsigned int* order, unsigned char* flags, unsigned int* long_list, hipStream_t st);
hipError_t launch_render_h(const RenderArgs& A, bool tree, int mode, hipStream_t st);
hipError_t launch_trace_h(const DevScene& S, const DevTree& T, bool tree, const float* rays, long long n, rt_hit_record* out, hipStream_t st);
const char* render_kernel_name_h(bool tree, int mode);
#ifdef RT_H16_STATS
hipError_t read_h16_stats(unsigned long long* out, int reset);
#endif

// ---- rt_build.hip
namespace gpubuild {
int build(rt_octree* O, const float4* d_geom, const int32_t* d_kind, int n, int spl, hipStream_t st, bool counted, bool* grid_enlarged);
int rebuild(rt_octree* O, const float4* d_geom, const int32_t* d_kind, int n, int spl, hipStream_t st, bool* regrown);
}

// ---- rt_denoise.hip
hipError_t launch_denoise(float* fb_out, const float* fb_in, int max_x, int max_y, const rt_hit_record* hits, const rt_denoise_params& P,
                          float4* work, hipStream_t st);
hipError_t launch_denoise_var(float* fb_out, const float* fb_in, int max_x, int max_y, const rt_hit_record* hits, const void* state,
                              const rt_denoise_var_params& P, float4* work, hipStream_t st);
hipError_t launch_denoise_var_levels(float* fb_out, int max_x, int max_y, const rt_hit_record* hits, const rt_denoise_var_params& P, float4* work,
                                     hipStream_t st);

// ---- rt_temporal.hip
hipError_t launch_temporal_accumulate(void* hist_out, const void* hist_in, const rt_hit_record* hits, const rt_hit_record* hits_prev,
                                      const rt_camera* cam_prev, const void* state, const int32_t* kind, int n_kind, int max_x, int max_y,
                                      const rt_temporal_params& P, hipStream_t st);
hipError_t launch_denoise_hist(float* fb_out, const float* fb_in, int max_x, int max_y, const rt_hit_record* hits, const void* hist,
                               const rt_denoise_var_params& P, float4* work, hipStream_t st);

// ---- rt_animate.hip
hipError_t launch_world_set_geometry(float4* geom, float4* shade, float4* list_hot, const int32_t* list_id, const float4* src, int n, int n_list,
                                     bool half, hipStream_t st);
hipError_t launch_temporal_accumulate_moving(void* hist_out, const void* hist_in, const rt_hit_record* hits, const rt_hit_record* hits_prev,
                                             const rt_camera* cam_prev, const float4* geom, const float4* geom_prev, const void* state,
                                             const int32_t* kind, int n_kind, int max_x, int max_y, const rt_temporal_params& P,
                                             hipStream_t st);

// ---- rt_rectify.hip (geom_prev == nullptr: the static rule)
hipError_t launch_temporal_accumulate_rectified(void* hist_out, const void* hist_in, const rt_hit_record* hits, const rt_hit_record* hits_prev,
                                                const rt_camera* cam_prev, const float4* geom, const float4* geom_prev, const void* state,
                                                const int32_t* kind, int n_kind, int max_x, int max_y, const rt_temporal_params& P,
                                                const rt_temporal_rectify& Rc, hipStream_t st);

// ---- rt_budget.hip
size_t budget_ws_bytes();
// Which key ranks the pixels of a selection, with that key's inputs (checked by the caller, rt_api.hip):
//   RAW       rt_adaptive_priority of the state's own (SL, Q, k); any part of a frame
//   FILTERED  rt_adaptive_priority_filtered of level 0 of rt_denoise_adaptive(filter) on the state; whole row-major frames of at most
//             RT_DENOISE_MAX_PIXELS pixels, hits: the frame's guides, 16-byte aligned
//   TEMPORAL  rt_adaptive_priority_filtered of what rt_temporal_accumulate(in, temporal) would write; whole frames as FILTERED, the
//             histories and guides of `in` 16-byte aligned (d_hist_in == nullptr: the first frame), kind[n_kind]: RT_MAT_* of the world list
// keys_out (FILTERED, TEMPORAL; may be NULL): the key of every pixel before the eligibility mask.
struct BudgetKey {
    enum Rank { RAW, FILTERED, TEMPORAL } rank = RAW;
    const rt_hit_record* hits = nullptr; const rt_denoise_var_params* filter = nullptr;
    const rt_temporal_inputs* in = nullptr; const rt_temporal_params* temporal = nullptr; const int32_t* kind = nullptr; int n_kind = 0;
    float* keys_out = nullptr;
};
hipError_t launch_budget_select(const BudgetKey& key, const void* state, long long n, const AdaptFrame& fr, int batch, int max_spp, float floor_lum,
                                unsigned int K, unsigned int* keys, unsigned int* ws, unsigned int* list, unsigned int* count, hipStream_t st);
hipError_t launch_budget_seed(float* fb, const AdaptState& s, const unsigned int* list, const unsigned int* count, unsigned int cap, hipStream_t st);
hipError_t launch_budget_final(float* fb, const AdaptState& s, const unsigned int* list, const unsigned int* count, unsigned int cap, int32_t* spp, int batch,
                               uint32_t* picked, hipStream_t st);

} // namespace rt
