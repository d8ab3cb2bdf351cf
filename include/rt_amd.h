/* rt_amd.h — C-ABI of the MI355X-native render path (librt_amd.so).
 *
 * Drop-in boundary for the render path of MuellerNico/DD2360-RayTracing.  The reference has no FFI layer: its
 * boundary is the kernel-launch surface of main.cu plus two host functions.  Every entry point
 * below names the reference interface it replaces (file:line under the reference tree).  POD only, plain
 * pointers and sizes, `int` return (0 = ok, otherwise the hipError_t value, or a negative RT_E* code for argument
 * errors); no exceptions cross the boundary; the caller owns every buffer it passes in; opaque handles are
 * created/destroyed by the matching rt_* calls.  All device work is enqueued on the caller-supplied stream
 * (a hipStream_t passed as void*, NULL = default stream) and is asynchronous unless stated otherwise.
 * Thread-compatible, not thread-safe per handle.
 *
 * There is NO CPU fallback: every compute entry point fails (hipError) when no gfx950 device / code object is
 * available.
 */
#ifndef RT_AMD_H
#define RT_AMD_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 6

/* argument errors (negative so they never collide with hipError_t) */
#define RT_EINVAL (-1)
#define RT_ENOMEM (-2)
#define RT_EIO (-3)
#define RT_ENOTSUP (-4)
#define RT_ECOMM (-5)   /* the multi-GPU exchange failed (RCCL error, or the custom gather returned non-zero) */

/* real_t selection — precision_types.h:8 (USE_FP16) */
#define RT_PRECISION_FP32 0
#define RT_PRECISION_FP16 1

/* material tags — lambertian / metal / dielectric of material.h:52,62,76; NONE marks a never-initialised
 * ("ghost") slot of the world list (main.cu:160-190 fills only 4+k*k of NUM_SPHERES slots): never hittable. */
#define RT_MAT_NONE (-1)
#define RT_MAT_LAMBERTIAN 0
#define RT_MAT_METAL 1
#define RT_MAT_DIELECTRIC 2

/* curandState (48 bytes) — the per-pixel RNG state buffer of main.cu:383 keeps this layout. */
typedef struct rt_rand_state {
    uint32_t d, v[5];
    int32_t boxmuller_flag, boxmuller_flag_double;
    float boxmuller_extra;
    uint32_t pad_;
    double boxmuller_extra_double;
} rt_rand_state;

/* sphere (sphere.h:7-15) together with the material its mat_ptr points to (material.h:52-116).
 * In FP16 mode every float holds the exact image of the binary16 value. */
typedef struct rt_sphere {
    float center[3];
    float radius;
    int32_t material;   /* RT_MAT_* */
    float albedo[3];    /* lambertian / metal */
    float param;        /* metal: fuzz (already clamped to <=1, material.h:66); dielectric: ref_idx */
} rt_sphere;

/* camera (camera.h:51-56), same field order. */
typedef struct rt_camera {
    float origin[3], lower_left_corner[3], horizontal[3], vertical[3], u[3], v[3], w[3];
    float lens_radius;
} rt_camera;

/* OctNode (acceleration_structure.h:35-39), reference layout, for inspection of the built tree. */
typedef struct rt_octnode {
    int32_t level;
    float aabb[6];      /* x_low,y_low,z_low,x_high,y_high,z_high */
    int32_t children[8];
} rt_octnode;

#define RT_OCTREE_MAX_NODES 585 /* NUMBER_NODES, acceleration_structure.h:13 */

/* hit_record (hitable.h:9-15); mat_ptr becomes the index of the sphere that was hit (-1 = miss). */
typedef struct rt_hit_record {
    float t;
    float p[3];
    float normal[3];
    int32_t sphere;
} rt_hit_record;

typedef struct rt_render_ctx rt_render_ctx; /* per-launch state of rt_render: work counters, scheduling workspace, timing events */
typedef struct rt_multi rt_multi;   /* one frame over the GPUs of a node (one process per GPU) */
typedef struct rt_world rt_world;   /* device-resident scene: what d_list / d_world / d_camera reach (main.cu:393-398) */
typedef struct rt_octree rt_octree; /* Octree (acceleration_structure.h:57-62): host reference layout + device traversal copy */

/* Which pixel tiles of the frame this call covers.  The frame is cut into 8x8-pixel tiles (the reference's
 * block shape, main.cu:351-352), numbered row-major from the bottom-left.  Two forms of a part:
 *  - a RANGE (tile_end > tile_begin): the consecutive tiles [tile_begin, tile_end) — a horizontal band of the image.
 *    rt_split_balanced cuts a frame into nparts such bands of equal predicted cost (what rt_multi_render renders by default);
 *    local tile = tile - tile_begin.
 *  - RUNS (tile_begin == tile_end == 0): tiles dealt to the parts in runs of RT_PART_RUN consecutive tiles: tile t lies in run
 *    r = t / RT_PART_RUN, run r belongs to part (r % nparts) and is that part's (r / nparts)-th run;
 *    local tile = (r / nparts) * RT_PART_RUN + t % RT_PART_RUN.  Part 0 never has fewer tiles than another part.
 *    (C5, the slowest of 8 parts on one MI355X: single tiles 106-110 ms, runs of 64: 100-102; whole frame / 8 = 83.)
 * nparts == 1 without a range: the whole frame, buffers in the reference's row-major layout (pixel_index = j*max_x + i).
 * Otherwise buffers are tile-major and compact: element (local_tile*64 + ly*8 + lx).
 * rt_part_pixels() gives the element count of such a buffer. */
#define RT_PART_RUN 64
typedef struct rt_partition {
    int32_t part, nparts;
    int64_t tile_begin, tile_end;
} rt_partition;

/* ---- library ---------------------------------------------------------------------------------------------- */
int rt_abi_version(void);
/* device_count may be NULL. Returns 0 when at least one gfx950 device is usable. */
int rt_device_check(int* device_count);
const char* rt_error_string(int code);

/* ---- host side: scene definition ------------------------------------------------------------------------- */
/* rand_init<<<1,1>>> — main.cu:78-82: curand_init(1984,0,0). Host-side (the world is generated on the host). */
int rt_rand_init(rt_rand_state* rand_state);

/* create_world<<<1,1>>> — main.cu:146-204.  Fills list[num_spheres] (unfilled slots get RT_MAT_NONE) and *cam,
 * advances *rand_state exactly as the reference's single device thread does; *num_created = 4 + k*k filled slots. */
int rt_create_world(rt_sphere* list, int num_spheres, float sphere_radius, rt_camera* cam, int nx, int ny,
                    rt_rand_state* rand_state, int precision, int* num_created);

/* camera::camera — camera.h:22-44 (vfov in degrees). */
int rt_camera_init(rt_camera* cam, const float lookfrom[3], const float lookat[3], const float vup[3], float vfov,
                   float aspect, float aperture, float focus_dist, int precision);

#define RT_TRAVERSAL_REFERENCE 0
#define RT_TRAVERSAL_FAST 1

/* Describes list + camera for the device: replaces the cudaMalloc'ed d_list/d_world/d_camera (main.cu:393-401).
 * Host-only; the device copy is made by rt_world_upload. */
int rt_world_create(const rt_sphere* list, int num_spheres, const rt_camera* cam, int precision, rt_world** out);
/* Creates the device buffers now (otherwise the first render/trace using the handle does it; call this before
 * capturing launches into a hipGraph, since it allocates). */
int rt_world_upload(rt_world* world);
/* How hitable_list::hit (hitable_list.h:16-31, the path taken when no octree is passed) runs on the device.  Both give the
 * reference's hit records bit for bit (fp32): REFERENCE tests every sphere in list order; FAST (default) tests only the
 * spheres the conservative (x,z) grid of the octree path says the ray can touch (the list seen as one unbounded node:
 * lowest index wins among equal t, exactly like the sequential scan) and falls back to the scan for rays it cannot prove.
 * FP16 worlds, lists of fewer than 64 spheres and lists with more than 64 spheres outside the grid's range always use
 * REFERENCE.  The grid is built by the first call that needs it (a render/trace without an octree, or the info call). */
int rt_world_set_list_traversal(rt_world* world, int mode);   /* RT_TRAVERSAL_REFERENCE | RT_TRAVERSAL_FAST */
/* Arithmetic of the fp32 render kernels on this world.  RT_ARITH_IEEE (default): one IEEE binary32 rounding per operation of the
 * reference source, no FMA contraction — the parity contract.  RT_ARITH_CONTRACT: the same kernels compiled with
 * contraction allowed, as nvcc does by default to the reference (Makefile:9 passes no -fmad=false): a*b+c may become one fma with a
 * single rounding (3 instead of 5 operations a dot product).  Pixels then differ from the parity mode in the last bits, and where a
 * last bit flips a decision (a rejection-loop test, a grazing hit) in whole samples: a TOLERANCE mode — tests/test_gpu_contract.py
 * states the measured bounds — reported separately by bench.py --arith contract, never the default.  rt_render / rt_render_progressive
 * only (rt_trace_rays stays IEEE); RT_ENOTSUP for USE_FP16 worlds (binary16 operations are single instructions either way). */
#define RT_ARITH_IEEE 0
#define RT_ARITH_CONTRACT 1
int rt_world_set_arith(rt_world* world, int mode);
int rt_world_list_accel_info(const rt_world* world, int* enabled, int* grid_dim, float* cell_size, int* grid_entries, int* large_spheres);
/* One resident world over a sequence of frames (no reference counterpart, whose scene and camera are fixed; DESIGN.md §5.10 "Moving
 * scenes").  The camera and the sphere geometry of a world can be replaced between frames; materials, kinds and the list order stay.
 *
 * rt_world_set_camera: host only.  Every launch passes the camera by value in its kernel arguments, so the call does no device work
 * and synchronises with nothing: launches already enqueued keep the camera they were launched with, and a captured hipGraph keeps the
 * camera it was captured with.  From the next call on, every entry point that takes the world renders what a fresh
 * rt_world_create(list, n, cam, precision) renders, bit for bit (frames, written-back RNG states, guides, trace records); USE_FP16
 * worlds expect exact binary16 images in the fields, as rt_world_create does.  What is keyed on the world misses once: the kept
 * schedule of every context (rt_world_render_schedule_reuse: `computed` one higher for the first rt_render after the call), the tile
 * order of a progressive sequence, the cached split of RT_SPLIT_BALANCED_CACHED.  A progressive pass with current_sample > 1 after the
 * call adds a sample seen through the NEW camera to the caller's sums of the old one, in the plain tile order: start the sequence
 * again at current_sample == 1, as the reference's viewer does when its camera moves.  To a context that a captured progressive pass
 * has bound to a graph (see "Render contexts"), the moved world is another frame: give the restarted sequence a context of its own.
 * rt_world_camera returns the camera the next launch will use.  RT_EINVAL for NULL.
 *
 * rt_world_set_geometry: d_geom is a device array of world->n x 4 floats (cx, cy, cz, radius) in world-list order, 16-byte aligned,
 * none of the world's own arrays.  It uploads the world if need be and enqueues ONE kernel on `stream` that rewrites every device
 * array holding geometry; after it the world is indistinguishable on the device from a fresh world created from the same list with the
 * new geometry (radius * radius in the world's precision included; values are taken without looking, as rt_world_create takes them:
 * NaN, negative radii).  Launches on other streams that read the world are the caller's to order against `stream`.  What goes stale:
 *   - the host staging copy: whatever needs it (the list grid, the host fallback of rt_build_octree_gpu) first downloads the device
 *     copy — one synchronising copy, only then;
 *   - the world's list grid (rt_world_set_list_traversal): freed; the next launch without an octree builds another ON THE HOST.  The
 *     list path of a moved world pays that build per move: the animated path is the octree path, rt_build_octree_gpu per frame;
 *   - octrees built from the world before the call: they describe the old geometry, and rendering through one is undefined, as through
 *     the tree of another world.  Free them and call rt_build_octree_gpu(world, ...) again, or rebuild one in place with
 *     rt_octree_rebuild_gpu, see rt_amd_rebuild.h;
 *   - kept schedules, progressive tile orders and cached splits miss once, as after rt_world_set_camera.
 * rt_world_get_geometry copies the same layout out, device to device, asynchronously on `stream` (uploads the world if need be): a
 * viewer keeps last frame's geometry with it for rt_temporal_accumulate_moving.  RT_EINVAL for NULL or a misaligned d_geom. */
int rt_world_set_camera(rt_world* world, const rt_camera* cam);
int rt_world_camera(const rt_world* world, rt_camera* out);
int rt_world_set_geometry(rt_world* world, const float* d_geom, void* stream);
int rt_world_get_geometry(const rt_world* world, float* d_out, void* stream);
/* free_world<<<1,1>>> + cudaFree — main.cu:206-219, :464-466. */
int rt_free_world(rt_world* world);

/* buildOctree — acceleration_structure.h:195-217 (host, serial); the upload of main.cu:413-417 is rt_octree_upload.
 * spheres_per_leaf is SPHERES_PER_LEAF (acceleration_structure.h:15, reference value 30). */
int rt_build_octree(const rt_sphere* list, int num_hitables, int spheres_per_leaf, int precision, rt_octree** out);
int rt_octree_upload(rt_octree* octree);   /* the cudaMalloc + cudaMemcpy of main.cu:413-417; implicit on first use */
/* buildOctree + upload in one, ON THE DEVICE: the same tree as rt_build_octree — reference layout (rt_octree_nodes / _leaves),
 * traversal copy and candidate grid, array for array and bit for bit — built from the world's device-resident sphere list
 * (uploads the world if need be) by per-sphere / per-cell kernels and radix sorts; ready to render when the call returns
 * (it synchronises with `stream` a few times: array sizes come back from the device).  N = 100 000, SPHERES_PER_LEAF 320:
 * 1.9 ms instead of 25.6 ms of host build + 3 ms of upload (MI355X box).  USE_FP16 worlds: the tree in binary16 arithmetic, the pair
 * layout and plane table of the binary16 kernels, no candidate grid — again what rt_build_octree + rt_octree_upload give. */
int rt_build_octree_gpu(const rt_world* world, int spheres_per_leaf, rt_octree** out, void* stream);
/* Which build a tree came from (read-only; RT_EINVAL for NULL).  rt_build_octree_gpu declines an input whose (level-3 cell, sphere)
 * pairs outnumber its workspace of 16 * num_spheres + 65536 — many spheres that each span many cells — and then builds the same tree
 * on the host from the world's list (after rt_world_set_geometry: one synchronising download first): RT_BUILD_HOST_DECLINED, a
 * rebuild of tens of milliseconds where the device takes one. */
#define RT_BUILD_HOST 0            /* rt_build_octree */
#define RT_BUILD_DEVICE 1          /* rt_build_octree_gpu, on the device */
#define RT_BUILD_HOST_DECLINED 2   /* rt_build_octree_gpu, on the host after the device build declined */
int rt_octree_build_path(const rt_octree* octree);
/* Rebuilding such a tree in place for a moved world, frame after frame (rt_octree_rebuild_gpu and rt_octree_rebuild_info), is declared
 * in rt_amd_rebuild.h, which this header includes at its end. */
/* one device-resident array of a tree, copied to the host (parity checks of the two builds; binary16 trees: 0-2 only): 0 traversal nodes, 1 bucket
 * entries (c, r^2), 2 entry -> sphere, 3/4 large spheres + bricks, 5 strip bin starts (columns x fine bins; the x copy, then the z copy), 6/7 strip entries + bricks, 8/9 membership
 * lists, 10 cell -> node, 11/12 membership bitmaps.  *bytes = size of the array; copied when cap suffices. */
int rt_octree_debug_array(const rt_octree* octree, int which, void* out, size_t cap, size_t* bytes);
int rt_free_octree(rt_octree* octree);
int rt_octree_flat_info(const rt_octree* octree, int* n_nodes, int* n_entries);   /* traversal copy: nodes used, bucket entries kept */
/* How hitTree walks the tree on the device.  Both produce the reference's hit records bit for bit (fp32):
 * REFERENCE scans every bucket of every visited level-3 node like traverseTree (acceleration_structure.h:276-304);
 * FAST (default) tests only the spheres a conservative (x,z) grid says the ray can touch — sorted strips: a sphere once
 * per column it overlaps, keyed by the fine bin of its centre; grid_dim = columns per axis, cell_size = column width,
 * grid_entries = registrations of the x copy — and falls back to the scan for rays it cannot prove (DESIGN.md 5.2,
 * App. A).  FP16 trees always use REFERENCE. */
int rt_octree_set_traversal(rt_octree* octree, int mode);
int rt_octree_accel_info(const rt_octree* octree, int* grid_dim, float* cell_size, int* grid_entries, int* large_spheres);
/* reference-layout view of the built tree (for parity checks): counts[0..leafCount), indices[leafCount*spl] */
int rt_octree_info(const rt_octree* octree, int* node_count, int* leaf_count, int* spheres_per_leaf,
                   int* dropped_full, int* dropped_outside);
int rt_octree_nodes(const rt_octree* octree, rt_octnode* out_nodes /* [RT_OCTREE_MAX_NODES] */);
int rt_octree_leaves(const rt_octree* octree, int32_t* counts, int32_t* indices);

/* ---- device side: the hot path ----------------------------------------------------------------------------- */
/* number of elements (pixels) of a buffer for this partition of a max_x x max_y frame */
int64_t rt_part_pixels(int max_x, int max_y, rt_partition part);

/* render_init<<<blocks,threads>>> — main.cu:84-94: curand_init(1984 + pixel_index, 0, 0) per pixel. */
int rt_render_init(int max_x, int max_y, rt_rand_state* d_rand_state, rt_partition part, void* stream);

/* render<<<blocks,threads>>> — main.cu:96-117.  fb: device buffer of vec3 (3 x float, or 3 x binary16 in FP16 mode).
 * d_octree == NULL selects the hitable_list path (USE_OCTREE undefined, main.cu:54). */
int rt_render(void* fb, int max_x, int max_y, int ns, const rt_world* world, rt_rand_state* d_rand_state,
              const rt_octree* d_octree, rt_partition part, void* stream);

/* render_progressive<<<blocks,threads>>> — main.cu:119-142: one sample per call, fb = col (current_sample == 1) or fb += col. */
int rt_render_progressive(void* fb, int max_x, int max_y, int current_sample, const rt_world* world,
                          rt_rand_state* d_rand_state, const rt_octree* d_octree, rt_partition part, void* stream);

/* Render contexts.  rt_render / rt_render_progressive keep their per-launch state (work counters, the scheduling workspace of
 * the pilot pass, timing events) in a context owned by the world handle.  Launches that share a context are ordered by the
 * library (the next call's stream waits for the previous render kernel), so calls on one world from several streams are safe
 * but run one after the other; frames that should overlap on one GPU — two partitions of a frame on two streams — take a
 * context each and go through the *_on entry points.  A context first used inside a hipGraph capture must have been
 * prepared before (rt_render_ctx_reserve, or one uncaptured call of the same frame size — in either precision: the binary16
 * render has a pilot pass and a workspace too); timing events are not recorded during a capture.  A captured rt_render_progressive pass
 * bakes the context's tile-order buffer into the graph: from then on the context refuses (RT_EINVAL) the uncaptured first pass
 * (current_sample == 1) of a progressive sequence of any other frame — another world or tree, size or partition — which would
 * rewrite that order under the graph (or, for a larger frame, move it); a restart of the captured frame itself recomputes an
 * order of the same tiles and is accepted.  Give another sequence a context of its own for the graph's lifetime. */
int rt_render_ctx_create(rt_render_ctx** out);
int rt_render_ctx_reserve(rt_render_ctx* ctx, int max_x, int max_y, rt_partition part);   /* workspace for frames of this size, now */
int rt_render_ctx_destroy(rt_render_ctx* ctx);
int rt_render_on(rt_render_ctx* ctx, void* fb, int max_x, int max_y, int ns, const rt_world* world, rt_rand_state* d_rand_state,
                 const rt_octree* d_octree, rt_partition part, void* stream);
int rt_render_progressive_on(rt_render_ctx* ctx, void* fb, int max_x, int max_y, int current_sample, const rt_world* world,
                             rt_rand_state* d_rand_state, const rt_octree* d_octree, rt_partition part, void* stream);
int rt_render_ctx_times(rt_render_ctx* ctx, float* ms_out, int max, int* count);           /* as rt_world_render_times */

/* Adaptive sampling: every pixel takes min_spp samples, then, every `batch` samples, only the pixels whose estimated error is
 * still above the target take more, up to max_spp (no reference counterpart; extends rt_render, main.cu:96-117).
 * The stop rule, after k samples of a pixel (k = min_spp, min_spp + batch, ...), in IEEE binary32, one rounding per operation:
 *   S_rgb = the sum of the sample colours (rt_render's col), SL = sum of l, Q = sum of l * l, where l = (c.x + c.y) + c.z is the
 *   sample's colour c (0 for an absorbed path), all summed in sample order;
 *   n = (float)k;  d = n * Q - SL * SL;  m = SL > n * floor ? SL : n * floor;  t = rel_error * rel_error;
 *   the pixel stops when  rel_error > 0 && d <= (t * (n - 1)) * (m * m)
 * (relative standard error of the mean luminance <= rel_error, the mean floored at `floor`, both sides multiplied out), or at
 * k == max_spp.  A NaN sample makes the comparison false: such a pixel runs to max_spp.  rel_error == 0: every pixel runs to max_spp.
 * Every pixel has its own RNG stream, so the frame is a per-pixel truncation of the uniform render, bit for bit: a pixel that stopped
 * after k samples holds exactly the colour and the written-back RNG state that rt_render with ns = k gives it. */
typedef struct rt_adaptive {
    int32_t min_spp;    /* samples every pixel takes before the first check (>= 2) */
    int32_t max_spp;    /* cap; (max_spp - min_spp) % batch == 0 */
    int32_t batch;      /* samples between two checks (>= 1) */
    float rel_error;    /* target relative standard error of the pixel's mean luminance; 0 = never stop early */
    float floor;        /* luminance level below which the error is measured against this level instead (>= 0) */
} rt_adaptive;
/* The whole frame (no partition), reference layout.  d_rand_state has been through rt_render_init, as for rt_render; d_octree == NULL
 * selects the hitable_list path.  fb receives the gamma-corrected colour (3 x float per pixel), d_spp (optional, may be NULL; one
 * int32 per pixel) each pixel's sample count, d_rand_state the written-back states.  Asynchronous on `stream`, no host
 * synchronisation: 1 + (max_spp - min_spp) / batch rounds of a render and a check kernel, each round reading its active-pixel count
 * from device memory.  Until that work has finished, fb holds running sums for some pixels.
 * RT_EINVAL for bad parameters and frames of more than 2^32 - 1 pixels; RT_ENOTSUP for USE_FP16 worlds and RT_ARITH_CONTRACT worlds.
 * Graph capture is not supported: RT_EINVAL while `stream` is capturing.  The workspace (two floats and two list entries per pixel,
 * one word per round) lives in the render context, grown on demand; the _on form takes a context of the caller's, as
 * rt_render_on does. */
int rt_render_adaptive(void* fb, int max_x, int max_y, const rt_adaptive* params, const rt_world* world, rt_rand_state* d_rand_state,
                       const rt_octree* d_octree, int32_t* d_spp, void* stream);
int rt_render_adaptive_on(rt_render_ctx* ctx, void* fb, int max_x, int max_y, const rt_adaptive* params, const rt_world* world,
                          rt_rand_state* d_rand_state, const rt_octree* d_octree, int32_t* d_spp, void* stream);
/* The same for a part of the frame (rt_partition: runs or a range), placed as rt_render places it.  nparts == 1 without a range is the
 * whole frame: exactly rt_render_adaptive.  Otherwise fb, d_rand_state and d_spp are the part's compact tile-major buffers, element
 * (local_tile*64 + ly*8 + lx) as for rt_render, rt_part_pixels() elements each (d_spp: one int32 per element).  The elements of edge
 * tiles that fall outside the frame are padding: the call never writes them (fb, d_spp and d_rand_state keep what they held — the
 * states what rt_render_init(part) wrote).  Every pixel is bit for bit what rt_render_adaptive gives it in the whole frame (colour,
 * count, state): its RNG stream is keyed by its absolute pixel_index.  A part without tiles: 0, nothing launched.  RT_EINVAL for an
 * invalid partition and for parts of more than 2^32 - 1 elements (the active lists hold 32-bit local ids), otherwise the errors of
 * rt_render_adaptive (RT_ENOTSUP for USE_FP16 and RT_ARITH_CONTRACT worlds, RT_EINVAL during a capture).  Round 0 runs rt_render(part)'s
 * scheduling pass; the workspace is sized by the part's tiles and elements. */
int rt_render_adaptive_part(void* fb, int max_x, int max_y, const rt_adaptive* params, const rt_world* world, rt_rand_state* d_rand_state,
                            const rt_octree* d_octree, int32_t* d_spp, rt_partition part, void* stream);
int rt_render_adaptive_part_on(rt_render_ctx* ctx, void* fb, int max_x, int max_y, const rt_adaptive* params, const rt_world* world,
                               rt_rand_state* d_rand_state, const rt_octree* d_octree, int32_t* d_spp, rt_partition part, void* stream);

/* Refinement: an adaptive frame that can be tightened afterwards without starting over (no reference counterpart; the adaptive
 * counterpart of main.cu:222-345's pass-by-pass refinement).  rt_render_adaptive_begin is rt_render_adaptive_part (same launches, the
 * same fb, d_spp and d_rand_state, bit for bit; part = {0, 1, 0, 0} is the whole row-major frame) that also fills d_state, a device
 * buffer of the caller's of RT_ADAPTIVE_STATE_BYTES x rt_part_pixels(max_x, max_y, part) bytes: every pixel's sums and sample count.
 * rt_render_adaptive_refine continues a frame that begin(from), or a chain of refines ending in `from`, left behind — same world, tree,
 * frame, part, d_rand_state and d_state — to the target `to`: afterwards fb, d_spp, d_rand_state and d_state hold exactly what
 * begin(to) would have left, bit for bit.  Only the pixels that `to` does not stop where they are take more samples.  The earlier
 * contents of fb and d_spp do not matter: every in-frame element is written again (the padding of edge tiles never is).
 * `to` refines `from` when both are valid rt_adaptive parameters with equal min_spp and batch, to.max_spp >= from.max_spp,
 * to.floor <= from.floor, to.rel_error == 0 or 0 < to.rel_error <= from.rel_error, from.rel_error^2 * (from.max_spp - 1) is finite in
 * binary32, and — when from.rel_error^2 underflows to 0 and to.rel_error > 0 — to.floor == from.floor; otherwise RT_EINVAL
 * (DESIGN.md §5.9 "Refinement": the rule of `to` then stops no pixel earlier than the rule of `from`).  Other errors as for
 * rt_render_adaptive_part, and RT_EINVAL for a NULL d_state.  Asynchronous on `stream`, no host synchronisation, never captured; the
 * _on forms take a context of the caller's.  A state from another frame, world, tree or part is undefined behaviour, as a progressive
 * pass on a foreign fb is.  (rt_render_adaptive_refine_fused, rt_amd_refine_fused.h: the same refinement in one render launch.) */
#define RT_ADAPTIVE_STATE_BYTES 24   /* per buffer element of the caller's refinement state */
int rt_render_adaptive_begin(void* fb, int max_x, int max_y, const rt_adaptive* params, const rt_world* world, rt_rand_state* d_rand_state,
                             const rt_octree* d_octree, int32_t* d_spp, void* d_state, rt_partition part, void* stream);
int rt_render_adaptive_begin_on(rt_render_ctx* ctx, void* fb, int max_x, int max_y, const rt_adaptive* params, const rt_world* world,
                                rt_rand_state* d_rand_state, const rt_octree* d_octree, int32_t* d_spp, void* d_state, rt_partition part, void* stream);
int rt_render_adaptive_refine(void* fb, int max_x, int max_y, const rt_adaptive* from, const rt_adaptive* to, const rt_world* world,
                              rt_rand_state* d_rand_state, const rt_octree* d_octree, int32_t* d_spp, void* d_state, rt_partition part, void* stream);
int rt_render_adaptive_refine_on(rt_render_ctx* ctx, void* fb, int max_x, int max_y, const rt_adaptive* from, const rt_adaptive* to,
                                 const rt_world* world, rt_rand_state* d_rand_state, const rt_octree* d_octree, int32_t* d_spp, void* d_state,
                                 rt_partition part, void* stream);

/* Budgets: the opposite contract to a noise target — "this many samples, put them where the frame is noisiest" (no reference
 * counterpart).  A spend continues the state of rt_render_adaptive_begin: it ranks the pixels by their priority and gives the first K
 * of them `batch` samples more, `rounds` times.
 * The priority of a pixel with sums SL, Q after k samples, IEEE binary32, one rounding per operation, no contraction:
 *   n = (float)k;  d = n * Q - SL * SL;  d = d > 0 ? d : 0              (a NaN d becomes 0)
 *   nf = n * floor;  m = SL > nf ? SL : nf
 *   e = d / ((n - 1) * (m * m));  key = e > 0 ? e : 0                    (NaN, e.g. 0 / 0, becomes 0; +inf stays)
 * — the squared relative standard error of the mean luminance, the mean floored at `floor`: the quantity the stop rule of rt_adaptive
 * compares with rel_error^2, divided out.  key is never negative, so its bits read as uint32 order it.  A pixel with a NaN sample has
 * key 0 and is never picked: a budget does not pour samples into a pixel whose error it cannot estimate.  (This differs from the
 * threshold rule of rt_render_adaptive, which runs such a pixel to max_spp.) */
float rt_adaptive_priority(float SL, float Q, int k, float floor);
typedef struct rt_budget {
    int64_t samples;   /* what this call may spend in total, >= 0 */
    int32_t rounds;    /* >= 1: the selection is repeated this many times */
    int32_t batch;     /* samples a chosen pixel takes in one round, >= 1 */
    int32_t max_spp;   /* a pixel with k + batch > max_spp is not eligible */
    float floor;       /* as rt_adaptive.floor: >= 0, finite */
} rt_budget;
/* q = samples / batch picks in total; round r = 0 .. rounds-1 gets K_r = q*(r+1)/rounds - q*r/rounds of them (integer divisions in
 * int64).  rt_adaptive_budget_check: 0, or RT_EINVAL for parameters outside the ranges above, for an overflowing q * rounds and for a
 * K_r above 2^32 - 1.  rt_adaptive_budget_picks: K_r for `round` into *picks (RT_EINVAL also for a round outside 0 .. rounds-1).
 * Host only, no device work. */
int rt_adaptive_budget_check(const rt_budget* params);
int rt_adaptive_budget_picks(const rt_budget* params, int round, int64_t* picks);
/* The selection of one round, alone.  An element of the part's buffer is eligible when it lies inside the frame (not the padding of an
 * edge tile), its k + batch <= max_spp, and its key is greater than 0.  The eligible elements are ordered by key descending and, among
 * equal keys, by element id ascending; the first min(picks, eligible) are chosen.  A budget is an upper bound: what cannot be placed
 * is not carried over.  Only the SET is defined: d_list (device, capacity min(picks, rt_part_pixels)) receives the chosen element
 * ids in no particular order, *d_count (device) their number.  d_state is the state of that frame and part, read only.  Asynchronous
 * on `stream`, a fixed number of launches, nothing comes back to the host.  `ctx` owns the workspace (key bits, histograms, per-block
 * tie counts; grown on demand) and must not be NULL.  RT_EINVAL for that, for bad parameters, picks outside 0 .. 2^32 - 1, NULL
 * buffers, an invalid partition and during a capture; 0 for a part without tiles. */
int rt_adaptive_budget_select(rt_render_ctx* ctx, const void* d_state, int max_x, int max_y, rt_partition part, const rt_budget* params,
                              int64_t picks, uint32_t* d_list, uint32_t* d_count, void* stream);
/* Spend a budget on a frame that rt_render_adaptive_begin, a chain of rt_render_adaptive_refine, or an earlier spend left — same world,
 * tree, frame, part, d_rand_state and d_state.  For every round r: the selection above with K_r; `batch` more samples for every chosen
 * pixel, continued from its sums and its RNG state; then k += batch, the new S_rgb in the state, fb = sqrtf(S * (float)(1.0 /
 * (double)(float)k)) and d_spp = k for each of them.  Every round ends with every pixel finalised, so rounds = R is, bit for bit, R
 * calls with rounds = 1 and samples = K_r * batch; a pixel at k samples holds what rt_render with ns = k gives it.  d_picked (device,
 * `rounds` words, may be NULL) receives every round's pick count.  The parameters alone fix the number of launches.
 * RT_EINVAL for bad parameters, a NULL state, an invalid partition and during a capture; RT_ENOTSUP for USE_FP16 and RT_ARITH_CONTRACT
 * worlds, after the parameter checks; 0 for a part without tiles.
 * A part selects among its own elements: a frame spent part by part is not the frame spent whole, and multi-GPU budgets (which need
 * a histogram exchange) are not provided.  rt_render_adaptive_refine after a spend is not supported: the state is no longer the state
 * of a threshold.  rt_denoise_adaptive accepts the state as it is.  rt_render_adaptive_spend_filtered (below, after rt_denoise_adaptive)
 * ranks by the error that is left after that filter. */
int rt_render_adaptive_spend(void* fb, int max_x, int max_y, const rt_budget* params, const rt_world* world, rt_rand_state* d_rand_state,
                             const rt_octree* d_octree, int32_t* d_spp, void* d_state, rt_partition part, uint32_t* d_picked, void* stream);
int rt_render_adaptive_spend_on(rt_render_ctx* ctx, void* fb, int max_x, int max_y, const rt_budget* params, const rt_world* world,
                                rt_rand_state* d_rand_state, const rt_octree* d_octree, int32_t* d_spp, void* d_state, rt_partition part,
                                uint32_t* d_picked, void* stream);

/* Name of the kernel rt_render (mode 0) / rt_render_progressive (mode 1) launches for this world and tree (d_octree NULL =
 * the hitable_list path), as rocprofv3 shows it without the namespace: "k_render<true,0,4>", "k_render_h<true,0>", ... */
int rt_render_kernel_name(const rt_world* world, const rt_octree* d_octree, int mode, char* out, int cap);

/* Device time of the dominant kernel (k_render / k_render_h) of the most recent rt_render / rt_render_progressive calls on
 * this world: HIP events recorded on the launch stream directly around that kernel (the scheduling pre-pass of rt_render
 * is outside).  Copies up to `max` durations (milliseconds, oldest first, at most the last 64 launches) into ms_out,
 * stores how many in *count, and forgets them.  Synchronises with the recorded events. */
int rt_world_render_times(rt_world* world, float* ms_out, int max, int* count);

/* Scheduling counters of the most recent rt_render on this world / context, read once that launch has finished (waits for it):
 * out4[0] = pixel slots handed out by the work queue, [1] = waves still counted thin (0 after a complete frame), [2] = pixels the
 * pilot pass pre-classified as long chains (0 below 16 samples per pixel; both precisions run the pilot pass), [3] = long-chain
 * handles taken.  Diagnostics only — no counterpart in the reference; which lane renders a pixel never changes the pixel.
 * A render captured into a hipGraph pins ONE slot of the context's counter ring and carries no ordering event: while such a graph
 * replays, its context must not be used by any other launch or replay (they would share the counters, the tile order and the flags) —
 * give every captured render a context of its own (rt_render_ctx_create). */
int rt_world_render_counters(rt_world* world, uint32_t* out4);
int rt_render_ctx_counters(rt_render_ctx* ctx, uint32_t* out4);

/* The words that decided the hand-out of the most recent rt_render on this world / context, read once that launch has finished
 * (waits for it).  Copies the first min(n, RT_SCHEDULE_WORDS) of them into out (0 before any launch):
 * out[0] = in-flight chain threshold (iterations; 0 = off), [1] = the pilot's long-chain threshold (3x3 pilot sum; 0 = off),
 * [2] = first slot of the sorted tail + 1 (0 = no tail; the tail starts on a multiple of 64 tiles), [3] = tail pixels handed out
 * before the tiles, [4] = the 3x3 pilot sum that decided them (0 = none), [5] = 1 when they come from the tail's cheap end,
 * [6] / [7] = long chains / chains started alone in a wave that the pilot listed, before the render kernel's rule that honours
 * them only while they are at most 1/64 of the slots.  [0]..[5] are written by the scheduling pass of the fp32 tree paths (from 4
 * samples per pixel; the tail from 16): the binary16 and list paths leave them at 0.  Diagnostics only, like the counters —
 * which lane renders a pixel never changes the pixel. */
#define RT_SCHEDULE_WORDS 8
int rt_world_render_schedule(rt_world* world, uint32_t* out, int n);
int rt_render_ctx_schedule(rt_render_ctx* ctx, uint32_t* out, int n);

/* The kept schedule.  The scheduling pass of rt_render reads the world, the tree and its traversal mode, the frame size, the partition,
 * the sample count, the precision and the device — never fb or d_rand_state — so a context keeps the pass it ran last, and an rt_render
 * (or the first launch of rt_render_adaptive*) with all of these equal launches no scheduling kernel: it reuses the tile order, the
 * long-chain set and the sorted tail, and rt_*_render_counters / rt_*_render_schedule return what the recomputed pass would.  Which lane
 * renders a pixel never changes the pixel: the frame and the RNG states are the same bits either way.  One record per context; any
 * other key, a regrown or released workspace, or a failed pass drops it.  Inside a stream capture rt_render captures the whole pass as
 * before and the record is not used — and since the graph's replays rewrite the workspace unseen, a context whose scheduling pass has
 * been captured never reuses again.  RT_SCHED_CACHE=0 in the environment turns the reuse off for the process.
 * *reused = launches that reused the record, *computed = scheduling passes issued (or captured), both since the context was created.
 * Host counters: no device work, no synchronisation. */
int rt_render_ctx_schedule_reuse(rt_render_ctx* ctx, uint64_t* reused, uint64_t* computed);
int rt_world_render_schedule_reuse(rt_world* world, uint64_t* reused, uint64_t* computed);

/* The measured pass.  A launch that reuses a kept schedule has just been preceded by a launch of the very same frame with the very same
 * sample count — which knew, when it ended a pixel, how many iterations (scatter or sky events) the pixel took.  On binary32 launches of
 * the sparse-grid kernels (k_render<true,*,4> and <true,*,5>) with at least RT_FEEDBACK_MIN_NS samples per pixel (32), the rt_render that
 * computes a record therefore also records those counts, 16 bits a pixel, saturating; the FIRST launch that reuses the record rebuilds
 * the scheduling pass from them (tile order, sorted tail, the long chains chosen pixel by pixel against the launch's own in-flight
 * threshold, the longest of them started alone in a wave), once per record; later launches reuse the rebuilt pass.  The counts are an
 * estimate where the RNG states continue from call to call and exact where they are re-seeded.  Scheduling only: the frame and the RNG
 * states are the same bits.  The counts end with their record.  RT_SCHED_FEEDBACK=0 in the environment turns recording and rebuilding
 * off for the process.
 * *refined = passes rebuilt since the context was created; out receives the first min(n, RT_FEEDBACK_WORDS) of: [0] 1 when the record
 * holds counts, [1] 1 when its pass is a rebuilt one, and then (waits for the latest launch) [2] the largest count of the frame, [3] the
 * most chains the rebuild would start alone (waves of the render grid / RT_FB_SOLO_CAP_DEN).
 * rt_*_render_schedule_counts copies the record's counts into out: n must be the element count of the launch that recorded them
 * (rt_part_pixels of its frame and partition; indexed like its fb); RT_EINVAL when the record holds none.  Waits for the latest launch. */
#define RT_FEEDBACK_WORDS 4
int rt_render_ctx_schedule_feedback(rt_render_ctx* ctx, uint64_t* refined, uint32_t* out, int n);
int rt_world_render_schedule_feedback(rt_world* world, uint64_t* refined, uint32_t* out, int n);
int rt_render_ctx_schedule_counts(rt_render_ctx* ctx, uint16_t* out, int64_t n);
int rt_world_render_schedule_counts(rt_world* world, uint16_t* out, int64_t n);

/* Reassemble a full row-major frame from nparts tile-major part buffers laid out back to back, each padded to
 * rt_part_pixels(max_x,max_y,{0,nparts}) elements (the layout an all-gather of the parts produces). */
int rt_assemble(void* fb_full, const void* fb_parts, int max_x, int max_y, int nparts, int precision, void* stream);

/* A frame cut into nparts horizontal bands of equal PREDICTED COST (no reference counterpart; extends the launch surface main.cu:422-427).
 * A pilot pass over the whole frame — two one-sample paths per 2x2 pixel block on a private RNG stream, the scheduling pre-pass of
 * rt_render — counts per tile the bounces, the grid entries its paths' walks had to test and the grid columns they stepped through; a tile's
 * cost is a fixed linear form of the three (rt_tuning.h, calibrated on measured band times), and the cuts fall where the running cost passes k/nparts of the total.
 * Integer arithmetic on counts that every GPU of the same kind reproduces bit for bit: every rank of a job computes the same
 * starts[] without talking to the others.  starts[0] = 0 <= ... <= starts[nparts] = number of tiles; part p is
 * rt_partition{p, nparts, starts[p], starts[p+1]} (never empty: RT_EINVAL when the frame has fewer tiles than parts).
 * Why bands: a GPU's rays meet the same part of the scene, as in the undivided frame (runs dealt round-robin keep the whole scene's
 * working set on every GPU for an eighth of the rays).  tile_bounces / tile_tests / tile_columns (host, [tiles], may be NULL) receive the pilot's counts.
 * Synchronises with `stream`.  ctx NULL = the world's own context. */
int rt_split_balanced(rt_render_ctx* ctx, const rt_world* world, const rt_octree* d_octree, int max_x, int max_y, int nparts,
                      int64_t* starts /* [nparts + 1] */, int32_t* tile_bounces, int32_t* tile_tests, int32_t* tile_columns, void* stream);
/* rt_assemble for such a split: band p's buffer begins part_stride_px elements behind band p-1's (>= the largest band). */
int rt_assemble_split(void* fb_full, const void* fb_parts, int max_x, int max_y, int nparts, const int64_t* starts, int64_t part_stride_px,
                      int precision, void* stream);

/* ---- multi-GPU: one frame over the GPUs of one node, one process per GPU -------------------------------------------------
 * No reference counterpart (the reference is single-GPU, launch surface main.cu:422-427).  Every rank computes the same split of
 * the frame's tiles (RT_SPLIT_BALANCED: rt_split_balanced's bands, recomputed for every frame; RT_SPLIT_RUNS, the default: runs of
 * RT_PART_RUN tiles dealt round-robin, no pilot pass over the whole frame), renders its part into a compact tile-major buffer, and
 * ONE exchange brings the parts to the root (RCCL over xGMI: one ncclGroupStart / ncclRecv x (nranks-1) | ncclSend / ncclGroupEnd,
 * straight from the render buffer into the root's staging slots, on the caller's stream), where rt_assemble / rt_assemble_split
 * writes the row-major frame into fb_full.
 * rt_multi_unique_id: rank 0 creates the 128-byte RCCL id and hands it to the other ranks by any means (a file, MPI,
 * torch.distributed over gloo); rt_multi_init: ncclCommInitRank on the calling process's current device.  RCCL is bound at
 * run time (dlopen): RT_ENOTSUP when it is absent. */
#define RT_MULTI_ID_BYTES 128
int rt_multi_unique_id(void* id_out /* [RT_MULTI_ID_BYTES] */);
int rt_multi_init(rt_multi** out, int rank, int nranks, const void* unique_id);
/* Non-collective check of everything rt_multi_init needs before it enters ncclCommInitRank (RCCL bound with all entry points,
 * a render context and events on the current device): 0, RT_ENOTSUP, or the HIP error.  ncclCommInitRank is collective — a
 * rank that fails early in rt_multi_init leaves its peers blocked inside it — so a job probes on every rank, agrees on the
 * result over its own control plane, and then calls rt_multi_init on all ranks or on none (bench.py does). */
int rt_multi_probe(void);
/* The same with a caller-supplied exchange (MPI, gloo, a test harness) instead of RCCL.  Called on every rank after its part
 * is rendered (enqueued on `stream`): rank r's send_bytes at d_send must arrive at d_parts + r * part_stride_bytes on the
 * root before work enqueued on the root's stream afterwards runs.  The root's own part is in place already (its d_send IS its
 * slot); d_parts is NULL on the other ranks.  Device pointers.  Return 0 on success. */
typedef int (*rt_gather_fn)(void* user, const void* d_send, size_t send_bytes, void* d_parts, size_t part_stride_bytes, int root, void* stream);
int rt_multi_init_custom(rt_multi** out, int rank, int nranks, rt_gather_fn gather, void* user);
int rt_multi_destroy(rt_multi* m);
/* how rt_multi_render divides the frame (the same on every rank): */
#define RT_SPLIT_RUNS 0             /* runs of RT_PART_RUN tiles, round-robin (default) */
#define RT_SPLIT_BALANCED 1         /* bands of equal predicted cost, from a pilot pass over the whole frame on every rank, every frame */
#define RT_SPLIT_BALANCED_CACHED 2  /* ... kept while world, tree, frame size stay the same (a static scene rendered again and again) */
int rt_multi_set_split(rt_multi* m, int mode);
/* the split of the last rt_multi_render: starts[nranks + 1] (RT_SPLIT_RUNS: RT_EINVAL) */
int rt_multi_last_split(rt_multi* m, int64_t* starts);
/* buffers for frames of this size now (otherwise the first rt_multi_render of a larger frame allocates) */
int rt_multi_reserve(rt_multi* m, int max_x, int max_y, int precision, int root);
/* render_init + render of this rank's tiles, the exchange, and on the root the assembled frame in fb_full (device buffer of
 * max_x*max_y vec3, reference layout; ignored on the other ranks).  precision must be the world's (RT_EINVAL otherwise: it sizes
 * the part buffers and the exchange).  Asynchronous on `stream`. */
int rt_multi_render(rt_multi* m, void* fb_full, int max_x, int max_y, int ns, const rt_world* world, const rt_octree* d_octree,
                    int precision, int root, void* stream);
/* device time of this rank's own share of the last rt_multi_render: render_init + render (call_ms) and the render kernel
 * alone (kernel_ms) — the ranks' values side by side show the load balance of the tile split.  Synchronises. */
/* rt_multi_render with adaptive sampling (rt_adaptive, the rule of rt_render_adaptive): every rank runs rt_render_init +
 * rt_render_adaptive_part_on on its runs, and the root receives the assembled frame in fb_full and — d_spp_full != NULL — the row-major
 * map of every pixel's sample count (max_x*max_y int32; ignored on the other ranks).  Both equal the whole-frame rt_render_adaptive bit
 * for bit.  RT_SPLIT_RUNS only: the balanced modes return RT_ENOTSUP (their bands are cut on a pilot pass of uniform sampling, which
 * says nothing about where adaptive sampling spends its samples).  RT_ENOTSUP for USE_FP16 and RT_ARITH_CONTRACT worlds, RT_EINVAL for
 * bad parameters, before any rank renders.  Two exchanges: the colour parts, then the count parts (every rank sends its counts,
 * whatever the root asked for).  RCCL: all of them in one ncclGroupStart / ncclGroupEnd, the counts as 4-byte words.  A custom gather
 * (rt_gather_fn) is called twice per frame: first for the colours as in rt_multi_render, then for the counts with send_bytes =
 * 4 x the rank's rt_part_pixels and part_stride_bytes = 4 x the elements of part 0.  A single rank renders straight into fb_full and
 * d_spp_full.  Buffers (a count part per rank, count staging on the root) grow on demand.  rt_multi_last_render_ms covers the
 * rank's adaptive share (render_init to the last check; kernel_ms: round 0 to the last check).  Asynchronous on `stream`. */
int rt_multi_render_adaptive(rt_multi* m, void* fb_full, int max_x, int max_y, const rt_adaptive* params, const rt_world* world,
                             const rt_octree* d_octree, int precision, int root, int32_t* d_spp_full, void* stream);
int rt_multi_last_render_ms(rt_multi* m, float* call_ms, float* kernel_ms);
/* RCCL contexts only: one ncclSend + ncclRecv of `bytes` bytes from this rank to itself inside one group on `stream` */
int rt_multi_selftest(rt_multi* m, const void* d_src, void* d_dst, size_t bytes, void* stream);

/* hitTree (acceleration_structure.h:319-342) / hitable_list::hit (hitable_list.h:16-31) for a batch of rays:
 * d_rays = n x 6 floats (origin, direction) on the device, d_out = n records on the device. t in (0.001, FLT_MAX). */
int rt_trace_rays(const rt_world* world, const rt_octree* d_octree, const float* d_rays, int64_t n,
                  rt_hit_record* d_out, void* stream);

/* ---- denoising (no reference counterpart; filters what render / render_progressive leave, main.cu:96-142) ----------------
 * Frames of at most RT_DENOISE_MAX_PIXELS pixels: the filter kernels index pixels and the halves of their guide records in int. */
#define RT_DENOISE_MAX_PIXELS 1073741824   /* 2^30 */
/* Guide buffers: the first hit of every pixel's centre ray.  d_hits = max_x*max_y records on the device, the reference's row-major
 * layout (pixel_index = j*max_x + i, row 0 at the bottom).  The ray, in binary32 with one rounding per operation:
 *   u = ((float)i + 0.5f) / (float)max_x;  v = ((float)j + 0.5f) / (float)max_y;  o = cam.origin;
 *   d[c] = ((lower_left_corner[c] + u*horizontal[c]) + v*vertical[c]) - origin[c]
 * — camera::get_ray with both pixel-jitter draws 0.5 and no lens offset: a pinhole, so the guides are sharp where a camera with an
 * aperture (C3's is 0.1) renders the frame slightly defocused.  Each record is bit for bit what rt_trace_rays returns for that ray
 * (sphere = -1 and zeros on a miss), through the walk rt_render uses for this world and tree, always in the IEEE arithmetic (also for
 * RT_ARITH_CONTRACT worlds).  RT_EINVAL for NULL pointers, non-positive sizes, frames of more than RT_DENOISE_MAX_PIXELS pixels and a
 * tree whose precision is not the world's; then RT_ENOTSUP for USE_FP16 worlds.  Uploads the world and tree if need be, as
 * rt_trace_rays does. */
int rt_render_guides(const rt_world* world, const rt_octree* d_octree, int max_x, int max_y, rt_hit_record* d_hits, void* stream);

/* An edge-avoiding a-trous filter guided by those records (fp32 frames only).  Everything in IEEE binary32, one rounding per operation,
 * no contraction, no transcendental function, sums in tap order (tests/denoise_model.py is the model, bit for bit):
 *   linear input x:  GAMMA x = c*c per channel;  SUM x = c / (float)samples (the reference viewer's fb / n).
 *   pass-through:    a pixel whose d_hits[p].sphere == -1 (the sky) or whose x has a channel that is not finite keeps its display value —
 *                    GAMMA the bits of fb_in, SUM sqrtf(x) — and is never a tap of another pixel (skipped, not weighted by 0).
 *   level L = 0 .. levels-1, h = 2^L: the taps of pixel p are q = p + h*(dx, dy), dx, dy in -2..2, dy outer, both from -2; a tap is
 *                    skipped when it lies outside the frame, on another sphere (sphere_q != sphere_p) or is a pass-through pixel.
 *   tap weight:      w = (k[dx]*k[dy] * w_n) / ((1 + a_pos) * (1 + a_col)),   k = {1/16, 1/4, 3/8, 1/4, 1/16}
 *                    d = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z;  w_n = d > 0 ? d : 0, then w_n = w_n*w_n normal_pow_log2 times
 *                    a_pos = (((P_p - P_q).x^2 + (P_p - P_q).y^2) + (P_p - P_q).z^2) / (t_p*t_p) * (1 / sigma_position^2)
 *                    a_col = (((x_p - x_q).r^2 + (x_p - x_q).g^2) + (x_p - x_q).b^2) * (4^L / sigma_color^2), x = this level's input
 *                    (the factors in brackets are rounded once on the host; a term that is off is w_n = 1, a_pos = 0 or a_col = 0).
 *   level result:    y_p = sum(w * x_q) / sum(w) per channel, the centre tap included; the next level's input.
 *   output:          fb_out = sqrtf(y) after the last level, the gamma of rt_render.
 * Pass-through is decided once, on the input.  fb_out may equal fb_in (no other overlap).  d_work: caller-owned workspace of
 * RT_DENOISE_WORK_BYTES per pixel (two float4 colour buffers); d_hits and d_work 16-byte aligned.  One prepare launch and one launch per
 * level, no allocation, no synchronisation: the call can be captured into a hipGraph.  RT_EINVAL for NULL pointers, misaligned d_hits /
 * d_work, and whatever rt_denoise_check refuses: non-positive sizes, frames of more than RT_DENOISE_MAX_PIXELS pixels, a NULL params,
 * an unknown input mode, samples < 1 with SUM, levels outside 1..RT_DENOISE_MAX_LEVELS, normal_pow_log2 outside -1..10, negative or
 * non-finite sigmas, and a sigma > 0 whose scale factor above is not finite (0 * inf at the centre tap).  Defaults
 * (RT_DENOISE_DEFAULT_*): chosen on C3 at 16 spp for the lowest RMSE against rt_render at 1024 spp. */
#define RT_DENOISE_INPUT_GAMMA 0   /* fb_in holds sqrt(mean), as rt_render / rt_render_adaptive write it */
#define RT_DENOISE_INPUT_SUM 1     /* fb_in holds the sum of `samples` sample colours, as rt_render_progressive leaves it */
#define RT_DENOISE_MAX_LEVELS 8
#define RT_DENOISE_WORK_BYTES 32   /* per pixel */
#define RT_DENOISE_DEFAULT_LEVELS 2
#define RT_DENOISE_DEFAULT_NORMAL_POW_LOG2 4
#define RT_DENOISE_DEFAULT_SIGMA_POSITION 0.01f
#define RT_DENOISE_DEFAULT_SIGMA_COLOR 0.3f
typedef struct rt_denoise_params {
    int32_t input;            /* RT_DENOISE_INPUT_* */
    int32_t samples;          /* SUM: the current_sample of the progressive sequence (>= 1); GAMMA: ignored */
    int32_t levels;           /* 1 .. RT_DENOISE_MAX_LEVELS; level L uses step 2^L */
    int32_t normal_pow_log2;  /* normal weight = max(dot, 0)^(2^k); -1 = no normal term */
    float sigma_position;     /* relative to the centre's distance t; 0 = no position term */
    float sigma_color;        /* in linear colour, halved every level; 0 = no colour term */
} rt_denoise_params;
int rt_denoise(void* fb_out, const void* fb_in, int max_x, int max_y, const rt_hit_record* d_hits, const rt_denoise_params* params,
               void* d_work, void* stream);
/* The frame-size and parameter checks of rt_denoise alone, on the host, no device work: 0 when rt_denoise accepts a frame of this size
 * with these parameters (given valid buffers), RT_EINVAL otherwise — before the workspace is allocated, for instance. */
int rt_denoise_check(int max_x, int max_y, const rt_denoise_params* params);

/* The same filter with variance-guided weights, on the state an adaptive render left (fp32 frames only): a tap is down-weighted by how
 * many standard errors its luminance lies from the centre's, so the filter blurs where the frame is noisy and fades out where it has
 * converged, pixel by pixel, whatever sample count each pixel stopped at.  d_state is the state of a WHOLE frame — what
 * rt_render_adaptive_begin or a chain of rt_render_adaptive_refine left for part = {0, 1, 0, 0}: row-major, RT_ADAPTIVE_STATE_BYTES per
 * pixel (parts are not offered: a tile-major part has no neighbours to filter with) — and fb_in the frame the same call left (gamma).
 * Everything in IEEE binary32, one rounding per operation, no contraction, no transcendental function, sums in tap order
 * (tests/denoise_var_model.py is the model, bit for bit):
 *   per pixel:       n = (float)k;  x_c = S_c / n per channel;  d = n*Q - SL*SL;  d = d > 0 ? d : 0 (a NaN d becomes 0);
 *                    v = d / ((n*n) * (n - 1)) — the variance of the pixel's mean luminance.
 *   pass-through:    decided once: d_hits[p].sphere == -1, k < 2, or a channel of x or v not finite (an overflowing n*Q or SL*SL included).
 *                    Such a pixel keeps the bits of fb_in and is never a tap of another pixel (skipped, not weighted by 0).
 *   level L = 0 .. levels-1, h = 2^L, this level's input x, v:  l = (x.r + x.g) + x.b.  Taps and skip rules are those of rt_denoise:
 *                    q = p + h*(dx, dy), dx, dy in -2..2, dy outer, both from -2; skipped outside the frame, on another sphere, pass-through.
 *   centre variance: prefilter == 1:  vb_p = sum(g * v_q) / sum(g) over q = p + (dx, dy), dx, dy in -1..1 at step 1 whatever h is, dy
 *                    outer, both from -1, g = k3[dx]*k3[dy], k3 = {1/4, 1/2, 1/4}, the same skip rules;  prefilter == 0:  vb_p = v_p.
 *   tap weight:      w = (k[dx]*k[dy] * w_n) / ((1 + a_pos) * (1 + a_var)),  k, w_n and a_pos exactly as in rt_denoise;
 *                    a_var = ((l_p - l_q)*(l_p - l_q)) / (sv2 * vb_p + RT_DENOISE_VAR_EPS),  sv2 = sigma_variance^2 rounded once on the
 *                    host; a_var = 0 when sigma_variance == 0.  Only the centre's variance enters: a converged pixel refuses a noisy
 *                    neighbour.  sv2 * vb_p may overflow to +inf in a later level (then a_var = 0, or NaN for an infinite l difference):
 *                    nothing is clamped, the operations are performed as written.
 *   level result:    y_p = sum(w * x_q) / sum(w) per channel;  v'_p = sum((w*w) * v_q) / (sum(w) * sum(w));  both the next level's input.
 *   output:          fb_out = sqrtf(y) after the last level.
 * fb_out may equal fb_in (no other overlap).  d_hits from rt_render_guides, d_work of RT_DENOISE_WORK_BYTES per pixel, both 16-byte
 * aligned, as for rt_denoise.  One prepare launch and one launch per level, no allocation, no synchronisation, no atomics: the call can
 * be captured into a hipGraph.  RT_EINVAL for NULL pointers, misaligned d_hits / d_work, and whatever rt_denoise_adaptive_check (host
 * only) refuses: non-positive sizes, frames of more than RT_DENOISE_MAX_PIXELS pixels, a NULL params, levels outside
 * 1..RT_DENOISE_MAX_LEVELS, normal_pow_log2 outside -1..10, prefilter outside 0..1, negative or non-finite sigmas, a sigma_position > 0
 * whose 1 / sigma^2 is not finite and a sigma_variance whose square is not finite.  With sigma_variance == 0, prefilter == 0 and one k
 * for all pixels, every filtered pixel is what rt_denoise gives for RT_DENOISE_INPUT_SUM, samples = k, sigma_color = 0 on S_rgb.
 * Defaults (RT_DENOISE_VAR_DEFAULT_*): one setting for C3 at 16, 64 and 128 spp. */
#define RT_DENOISE_VAR_EPS 1e-8f   /* keeps the centre tap's a_var from 0 / 0 where the variance is 0 */
#define RT_DENOISE_VAR_DEFAULT_LEVELS 1
#define RT_DENOISE_VAR_DEFAULT_NORMAL_POW_LOG2 4
#define RT_DENOISE_VAR_DEFAULT_PREFILTER 1
#define RT_DENOISE_VAR_DEFAULT_SIGMA_POSITION 0.01f
#define RT_DENOISE_VAR_DEFAULT_SIGMA_VARIANCE 4.0f
typedef struct rt_denoise_var_params {
    int32_t levels;           /* 1 .. RT_DENOISE_MAX_LEVELS; level L uses step 2^L */
    int32_t normal_pow_log2;  /* as rt_denoise_params */
    int32_t prefilter;        /* 1: the centre's variance is the 3x3 blur above; 0: its own */
    float sigma_position;     /* as rt_denoise_params; 0 = off */
    float sigma_variance;     /* luminance distance in standard errors of the centre's mean; 0 = no variance term */
} rt_denoise_var_params;
int rt_denoise_adaptive(void* fb_out, const void* fb_in, int max_x, int max_y, const rt_hit_record* d_hits, const void* d_state,
                        const rt_denoise_var_params* params, void* d_work, void* stream);
int rt_denoise_adaptive_check(int max_x, int max_y, const rt_denoise_var_params* params);

/* Temporal accumulation: the history of one frame from the history of the last one, across a camera move (DESIGN.md §5.10 "Temporal
 * accumulation"; fp32 worlds, whole row-major frames, a static scene: both frames use the same sphere list).  A history is
 * RT_TEMPORAL_HISTORY_BYTES per pixel: float4 (x.r, x.g, x.b, v) [n] — the accumulated mean colour and the variance of its luminance —
 * then float neff [n], the effective sample count behind it (0 = nothing); the base 16-byte aligned.  d_state is the state of this
 * frame (as rt_denoise_adaptive takes it), d_hits its guides; d_hits_prev and cam_prev (a host POD, passed to the kernel by value)
 * belong to the frame that wrote d_hist_in.  d_hist_in == NULL marks the first frame (d_hits_prev and cam_prev may then be NULL too).
 * The world supplies kind[sphere] only.  IEEE binary32, one rounding per operation, no contraction; a dot product is
 * (a.x*b.x + a.y*b.y) + a.z*b.z (tests/temporal_model.py is the model, bit for bit):
 *   this frame:      n, x_c = S_c / n, d and v_c exactly as rt_denoise_adaptive's "per pixel" line.  The pixel is EMPTY when it is sky
 *                    (sphere == -1), when k < 2, or when a channel of x_c or v_c is not finite: it writes (0, 0, 0, 0) and neff = 0.
 *   asked at all:    not when d_hist_in == NULL, when max_history == 0, or when reuse_specular == 0 and kind[sphere_p] is not
 *                    RT_MAT_LAMBERTIAN (a sphere index outside the world's list counts as not lambertian).
 *   where it was:    the pinhole inverse of get_ray on cam_prev = (O, LL, H, V):  A = LL - O;  D = P_p - O;  W = H x V, each component
 *                    two products and one subtraction (W.x = H.y*V.z - H.z*V.y, W.y = H.z*V.x - H.x*V.z, W.z = H.x*V.y - H.y*V.x);
 *                    lam = (D.W) / (A.W), rejected unless lam > 0;  s = ((D.H) / lam - A.H) / (H.H);  t likewise with V;
 *                    fx = s * (float)max_x - 0.5f;  fy = t * (float)max_y - 0.5f;  rejected unless fx > -1 && fx < (float)max_x and the
 *                    same for fy (a NaN rejects);  i0 = (int)floorf(fx), ax = fx - (float)i0;  j0, ay likewise.  The mapping is exact for
 *                    cameras of rt_camera_init / rt_create_world, whose horizontal is perpendicular to their vertical; for another
 *                    camera it is the stated arithmetic, not the inverse.
 *   the four taps:   q = (i0 + a, j0 + b), b outer, both from 0;  g = (a ? ax : 1 - ax) * (b ? ay : 1 - ay).  A tap is skipped, not
 *                    weighted by 0, when it lies outside the frame, when neff_in[q] is not > 0, when sphere_q != sphere_p, when
 *                    N_p.N_q is not >= normal_min_dot, or when ((e.x*e.x + e.y*e.y) + e.z*e.z) <= tol2 * (t_p*t_p) does not hold,
 *                    e = P_p - P_q, tol2 = position_tolerance^2 rounded once on the host.  Over the accepted taps, in tap order:
 *                    sg = sum(g);  x_h = sum(g * x_q) / sg per channel;  v_h = sum(g * v_q) / sg;  n_h = sum(g * neff_q) / sg.
 *                    The variance is interpolated, not combined with squared weights: resampled neighbours are correlated, the
 *                    linear form is the conservative one.  No history unless sg > 0.
 *   merging:         m = n_h < (float)max_history ? n_h : (float)max_history;  a = n / (m + n);  x = x_h + a*(x_c - x_h) per channel;
 *                    v = ((1 - a)*(1 - a))*v_h + (a*a)*v_c;  neff = m + n.  Without history x = x_c, v = v_c, neff = n.  Nothing is clamped.
 * d_hist_in and d_hist_out must not overlap.  One launch, no allocation, no synchronisation, no atomics: the call can be captured into a
 * hipGraph once rt_world_upload has run.  RT_EINVAL for NULL or 16-byte-misaligned buffers (histories and guides), a d_hist_in without
 * d_hits_prev or cam_prev, overlapping histories, and whatever rt_temporal_check (host only) refuses: sizes as for rt_denoise, a NULL
 * params, max_history < 0, reuse_specular outside 0..1, a position_tolerance that is not finite and > 0 or whose square is not finite,
 * a normal_min_dot outside [-1, 1]; after those checks RT_ENOTSUP for USE_FP16 worlds.
 * Defaults (RT_TEMPORAL_DEFAULT_*): the setting that loses least on C3 over a static camera and an orbit of 3.5 pixels a frame
 * (tools/temporal_study.py). */
#define RT_TEMPORAL_HISTORY_BYTES 20   /* per pixel: float4 (x.r, x.g, x.b, v) [n], then float neff [n]; base 16-byte aligned */
#define RT_TEMPORAL_DEFAULT_MAX_HISTORY 32
#define RT_TEMPORAL_DEFAULT_REUSE_SPECULAR 0
#define RT_TEMPORAL_DEFAULT_POSITION_TOLERANCE 0.03f
#define RT_TEMPORAL_DEFAULT_NORMAL_MIN_DOT 0.9f
typedef struct rt_temporal_params {
    int32_t max_history;       /* cap on the effective sample count taken over from the history, >= 0; 0 = take nothing */
    int32_t reuse_specular;    /* 0: a first hit on RT_MAT_METAL / RT_MAT_DIELECTRIC starts again; 1: reprojected like any other */
    float position_tolerance;  /* a history tap is accepted when |P_p - P_q|^2 <= tol^2 * t_p^2; finite, > 0, tol^2 finite */
    float normal_min_dot;      /* ... and N_p . N_q >= this; in [-1, 1] */
} rt_temporal_params;
int rt_temporal_check(int max_x, int max_y, const rt_temporal_params* params);             /* host only */
int rt_temporal_accumulate(void* d_hist_out, const void* d_hist_in, const rt_hit_record* d_hits, const rt_hit_record* d_hits_prev,
                           const rt_camera* cam_prev, const void* d_state, const rt_world* world, int max_x, int max_y,
                           const rt_temporal_params* params, void* stream);
/* rt_temporal_accumulate for a world whose spheres moved since the frame that wrote d_hist_in (rt_world_set_geometry; DESIGN.md §5.10
 * "Moving scenes").  d_geom_prev is what rt_world_get_geometry returned for that frame: world->n records (cx, cy, cz, radius), 16-byte
 * aligned; NULL exactly when d_hist_in is NULL.  This frame's geometry is the world's own.  Every other argument, the refusals (plus
 * RT_EINVAL for a d_hist_in without d_geom_prev or with a misaligned one), fp32 worlds only, one launch, no allocation and capture are
 * those of rt_temporal_accumulate, and so is the per-pixel rule, with two changes — each operation rounded once to binary32, no
 * contraction.  With s = sphere_p, c1 = geom[s].xyz, r1 = geom[s].w and c0, r0 the same fields of d_geom_prev[s]:
 *   asked at all:    also not when 0 <= s < n and the bits of r0 differ from the bits of r1: a sphere that changed size starts again.
 *   where it was:    when 0 <= s < n and a component of c0 differs in its bits from c1:
 *                    P' = ((P.x - c1.x) + c0.x, (P.y - c1.y) + c0.y, (P.z - c1.z) + c0.z); otherwise P' = P_p bit for bit (also for an
 *                    s outside the list, which reads no geometry).  P' replaces P_p in D = P' - O and in the tap test e = P' - P_q.
 *                    lim = tol2 * (t_p*t_p), the normal test (a translation keeps normals), the taps and the merge are unchanged.
 * So with nothing moved the call writes the bytes of rt_temporal_accumulate, and on every pixel whose sphere kept its radius it writes
 * what rt_temporal_accumulate writes for a copy of d_hits whose p fields hold P' (tests/temporal_moving_model.py).
 * Out of scope: LIGHTING — the history of a static surface goes on showing the old shadows and reflections of a sphere that moved;
 * max_history bounds that lag.  HISTORY-AWARE BUDGETS keep the static rule (rt_temporal_inputs is a fixed POD): it refuses the taps of
 * a moved sphere, which then ranks as thin history and is given samples — the wanted direction.  Rotation and radius-aware
 * reprojection, multi-GPU frames and parts, binary16 histories. */
int rt_temporal_accumulate_moving(void* d_hist_out, const void* d_hist_in, const rt_hit_record* d_hits, const rt_hit_record* d_hits_prev,
                                  const rt_camera* cam_prev, const float* d_geom_prev, const void* d_state, const rt_world* world,
                                  int max_x, int max_y, const rt_temporal_params* params, void* stream);
/* History rectification: rt_temporal_accumulate (d_geom_prev == NULL) or rt_temporal_accumulate_moving (d_geom_prev given: that
 * call's rule; 16-byte aligned, ignored when d_hist_in is NULL) with one more step — a history that THIS frame's neighbourhood
 * contradicts sheds effective samples before it is merged (DESIGN.md §5.10 "History rectification").  Every argument, buffer, the
 * single launch without allocation, synchronisation or atomics, and capture once the world is uploaded are those of the two calls.  The
 * rule is theirs up to the point where a pixel has taken history (sg > 0): it has x_h = (hx, hy, hz), v_h, n_h and
 * m = n_h < (float)max_history ? n_h : (float)max_history.  Then, each operation rounded once to binary32, no contraction, sums in the
 * stated order (tests/temporal_rectify_model.py is the model, bit for bit):
 *   the window:      q = p + (dx, dy), dx and dy in -radius .. radius, dy outer, both from -radius.  q is skipped, not weighted by 0,
 *                    when it lies outside the frame, when it is EMPTY in this frame (rt_temporal_accumulate's "this frame" line), or when
 *                    the bits of its guide's sphere differ from sphere_p.  The centre is always in the window.
 *                    l_q = (x.r + x.g) + x.b of q's x_c = S_c / n.
 *   first pass:      in window order cnt = cnt + 1.0f;  s1 = s1 + l_q;  then ml = s1 / cnt.
 *   second pass:     in the same order ss = ss + (l_q - ml) * (l_q - ml);  then s2 = ss / (cnt - 1.0f).
 *   the test:        only when gamma != 0 and cnt >= (float)min_count:  lh = (hx + hy) + hz;  dl = lh - ml;  e2 = dl * dl;
 *                    lim = g2 * s2, g2 = gamma * gamma rounded once on the host;  if (e2 > lim) m = m * (lim / e2).  A NaN compares
 *                    false and keeps m.  Nothing is clamped.
 *   merging:         unchanged with this m:  a = n / (m + n);  x = x_h + a*(x_c - x_h);  v = ((1 - a)*(1 - a))*v_h + (a*a)*v_c;  neff = m + n.
 * So: with gamma == 0 the call writes the bytes of rt_temporal_accumulate (d_geom_prev NULL) or of rt_temporal_accumulate_moving
 * (given); a pixel that took no history is untouched by the rule; neff is never above what the unrectified call writes for the pixel
 * (lim / e2 < 1 where it is applied); and x and v are a convex step from the unrectified values towards this frame's (a only grows).
 * The history sheds weight and is not clamped, so the variance rt_denoise_history trusts stays the variance of what was averaged.
 * RT_EINVAL for everything rt_temporal_accumulate refuses, a NULL rectify, whatever rt_temporal_rectify_check (host only) refuses —
 * radius outside 1..2, min_count outside 2..(2*radius+1)^2, a gamma that is negative or not finite or whose square is not finite — and
 * a misaligned non-NULL d_geom_prev; after all of those RT_ENOTSUP for USE_FP16 worlds.
 * Defaults (RT_TEMPORAL_RECTIFY_DEFAULT_*): the setting with the smallest worst-case loss against each scenario's own optimum over
 * static, orbiting and moving scenes (tools/temporal_study.py, tools/animate_study.py, profiles/r19/rectify.txt).
 * Out of scope: HISTORY-AWARE BUDGETS keep the unrectified key (rt_temporal_inputs is a fixed POD); per-channel tests (one luminance
 * test decides for the three channels); multi-GPU frames and parts; binary16 histories. */
#define RT_TEMPORAL_RECTIFY_DEFAULT_RADIUS 1
#define RT_TEMPORAL_RECTIFY_DEFAULT_MIN_COUNT 4
#define RT_TEMPORAL_RECTIFY_DEFAULT_GAMMA 1.5f
typedef struct rt_temporal_rectify {
    int32_t radius;     /* 1..2: the window is the (2r+1)^2 pixels of THIS frame around the pixel */
    int32_t min_count;  /* 2..(2r+1)^2: with fewer accepted window pixels the history is taken as it is */
    float gamma;        /* allowed distance of the history from the window mean, in standard deviations of the window;
                           finite, >= 0, gamma*gamma finite; 0 = off */
} rt_temporal_rectify;
int rt_temporal_rectify_check(const rt_temporal_rectify* r);                               /* host only: 0 or RT_EINVAL */
int rt_temporal_accumulate_rectified(void* d_hist_out, const void* d_hist_in, const rt_hit_record* d_hits, const rt_hit_record* d_hits_prev,
                                     const rt_camera* cam_prev, const float* d_geom_prev, const void* d_state, const rt_world* world,
                                     int max_x, int max_y, const rt_temporal_params* params, const rt_temporal_rectify* rectify,
                                     void* stream);
/* rt_denoise_adaptive with its "per pixel" values taken from a history: x = hist.xyz, v = hist.w; a pixel is pass-through, and keeps
 * the bits of fb_in, when neff == 0 or a channel of x or v is not finite (or v < 0, which rt_temporal_accumulate never writes).  The
 * levels, fb_out == fb_in, buffers, alignment (d_hist 16-byte aligned too), capture and errors are those of rt_denoise_adaptive; d_hits
 * are the guides of the frame the history belongs to.  After rt_temporal_accumulate(NULL history) it is rt_denoise_adaptive bit for bit. */
int rt_denoise_history(void* fb_out, const void* fb_in, int max_x, int max_y, const rt_hit_record* d_hits, const void* d_hist,
                       const rt_denoise_var_params* params, void* d_work, void* stream);

/* Filter-aware budgets: the same selection and the same rounds with a second priority — the relative variance of the pixel AFTER one
 * level of rt_denoise_adaptive's filter, for frames that go through that filter anyway: samples go where the filtered frame is still
 * noisy (DESIGN.md §5.9 "Filter-aware priority").  Whole frames only, row-major, fp32 worlds, at most RT_DENOISE_MAX_PIXELS pixels; the
 * state is that of part = {0, 1, 0, 0}, d_hits what rt_render_guides left (16-byte aligned), `filter` the parameters the frame will be
 * filtered with.  IEEE binary32, one rounding per operation, no contraction, no transcendental function, sums in tap order
 * (tests/filtered_budget_model.py is the model, bit for bit):
 *   per pixel:       x_c = S_c / n, d, v and the pass-through decision exactly as rt_denoise_adaptive's "per pixel" and "pass-through"
 *                    lines state them (sky, k < 2, a channel of x or v not finite); fb_in is not needed.
 *   filtered values: (y_p, v'_p) = what level L = 0 (step 1) of rt_denoise_adaptive computes with `filter`: the same taps, skip rules,
 *                    vb_p (prefilter), w_n, a_pos, a_var and w;  y_p = sum(w * x_q) / sum(w) per channel;
 *                    v'_p = sum((w*w) * v_q) / (sum(w) * sum(w)).  Only this first level is evaluated, whatever filter->levels says
 *                    (rt_denoise_adaptive_check validates levels as usual).
 *   filtered pixel:  l = (y.r + y.g) + y.b;  m = l > floor ? l : floor;  e = v' / (m * m);  key = e > 0 ? e : 0
 *                    (a NaN e becomes 0, +inf stays; nothing is clamped, the operations are performed as written) —
 *                    rt_adaptive_priority_filtered(l, v', floor) on the host.
 *   pass-through:    key = rt_adaptive_priority(SL, Q, k, floor), the raw rule: the filter leaves such a pixel as it is.
 * Both keys estimate one quantity — the variance of a mean over the squared floored mean (the raw key is v / max(SL / n, floor)^2 up
 * to rounding) — so one ordering holds both.  Eligibility (k + batch <= max_spp, key > 0), the ordering, ties by the lower pixel id,
 * K_r and "only the set is defined" are those of rt_adaptive_budget_select. */
float rt_adaptive_priority_filtered(float l, float v, float floor);
/* rt_adaptive_budget_select with that key.  d_keys (device, may be NULL) receives one float per pixel: the key above, before the
 * eligibility mask — the map of where the filtered frame is still noisy.  Errors as for rt_adaptive_budget_select, and RT_EINVAL for
 * whatever rt_denoise_adaptive_check(max_x, max_y, filter) refuses and for a NULL or misaligned d_hits. */
int rt_adaptive_budget_select_filtered(rt_render_ctx* ctx, const void* d_state, const rt_hit_record* d_hits, int max_x, int max_y,
                                       const rt_budget* params, const rt_denoise_var_params* filter, int64_t picks, uint32_t* d_list,
                                       uint32_t* d_count, float* d_keys, void* stream);
/* rt_render_adaptive_spend with that key: the same round, the selection's key kernel exchanged, nothing else.  A state may be continued
 * by either spend in any order; every statement of rt_render_adaptive_spend holds (rounds compose, a pixel at k samples holds what
 * rt_render with ns = k gives it).  fb stays unfiltered: the caller runs rt_denoise_adaptive when it wants the picture.  Errors as for
 * rt_render_adaptive_spend, and RT_EINVAL for the filter checks and a NULL or misaligned d_hits (with the parameter checks, before
 * RT_ENOTSUP). */
int rt_render_adaptive_spend_filtered(void* fb, int max_x, int max_y, const rt_budget* params, const rt_denoise_var_params* filter,
                                      const rt_hit_record* d_hits, const rt_world* world, rt_rand_state* d_rand_state, const rt_octree* d_octree,
                                      int32_t* d_spp, void* d_state, uint32_t* d_picked, void* stream);
int rt_render_adaptive_spend_filtered_on(rt_render_ctx* ctx, void* fb, int max_x, int max_y, const rt_budget* params,
                                         const rt_denoise_var_params* filter, const rt_hit_record* d_hits, const rt_world* world,
                                         rt_rand_state* d_rand_state, const rt_octree* d_octree, int32_t* d_spp, void* d_state, uint32_t* d_picked,
                                         void* stream);

/* History-aware budgets: the same selection and the same rounds with a third priority — the relative variance of the pixel AFTER
 * rt_temporal_accumulate's merge with the last frame's history, for viewers that accumulate over frames: samples go where the history
 * is thin (a disoccluded pixel, a pixel whose taps were refused, a specular first hit with reuse_specular = 0) and not where it
 * already holds max_history samples (DESIGN.md §5.9 "History-aware priority").  Whole frames only, row-major, fp32 worlds, at most
 * RT_DENOISE_MAX_PIXELS pixels; the state is that of part = {0, 1, 0, 0}.  rt_temporal_inputs is what rt_temporal_accumulate takes
 * besides the state and the world: this frame's guides, and the history, guides and camera of the last frame; `temporal` its
 * parameters; the world supplies kind[sphere] only.  IEEE binary32, one rounding per operation, no contraction
 * (tests/temporal_budget_model.py is the model, bit for bit):
 *   merged pixel:    (x.r, x.g, x.b, v) and neff are exactly what rt_temporal_accumulate would write for the pixel with these inputs,
 *                    bit for bit — its EMPTY rule, "asked at all", the reprojection, the four taps and the merge, none restated here.
 *   neff == 0:       (EMPTY) key = rt_adaptive_priority(SL, Q, k, floor), the raw rule: rt_temporal_accumulate and rt_denoise_history
 *                    leave such a pixel as it is.
 *   otherwise:       l = (x.r + x.g) + x.b;  key = rt_adaptive_priority_filtered(l, v, floor).
 * Eligibility (k + batch <= max_spp, key > 0), the ordering, ties by the lower pixel id, K_r and "only the set is defined" are those
 * of rt_adaptive_budget_select.  What follows: with d_hist_in == NULL or max_history == 0 the key of a non-empty pixel is
 * rt_adaptive_priority_filtered on this frame's own (x_c, v_c) — the same quantity as the raw key, but not its bits (other operations,
 * other roundings), so the set may differ from rt_adaptive_budget_select's at the cut; with reuse_specular = 0 a specular first hit is
 * ranked by this frame alone.  A pixel that took history at weight a = n / (m + n) has v = (1 - a)^2 v_h + a^2 v_c. */
typedef struct rt_temporal_inputs {      /* what rt_temporal_accumulate takes besides the state and the world; POD */
    const void* d_hist_in;               /* NULL = first frame (d_hits_prev, cam_prev may then be NULL) */
    const rt_hit_record* d_hits;         /* this frame's guides */
    const rt_hit_record* d_hits_prev;
    const rt_camera* cam_prev;           /* host, passed by value to the kernel */
} rt_temporal_inputs;
/* rt_adaptive_budget_select with that key.  d_keys (device, may be NULL) receives one float per pixel: the key above, before the
 * eligibility mask — the map of where the accumulated frame is still noisy.  Errors in the order of rt_adaptive_budget_select:
 * RT_EINVAL for its own refusals, a NULL world, in or temporal, whatever rt_temporal_check(max_x, max_y, temporal) refuses, NULL or
 * 16-byte-misaligned guides or history and a d_hist_in without d_hits_prev or cam_prev; then RT_ENOTSUP for a USE_FP16 world (a
 * contracted world is accepted: nothing is rendered); RT_EINVAL on a capturing stream.  The world is uploaded if need be. */
int rt_adaptive_budget_select_temporal(rt_render_ctx* ctx, const void* d_state, const rt_world* world, int max_x, int max_y,
                                       const rt_budget* params, const rt_temporal_inputs* in, const rt_temporal_params* temporal,
                                       int64_t picks, uint32_t* d_list, uint32_t* d_count, float* d_keys, void* stream);
/* rt_render_adaptive_spend with that key: the same round, the selection's key kernel exchanged, nothing else.  The key is formed anew
 * every round from the current state and the unchanged history of the last frame.  A state may be continued by any of the three
 * spends in any order; every statement of rt_render_adaptive_spend holds (rounds compose, every round ends finalised, a pixel at k
 * samples holds what rt_render with ns = k gives it).  fb stays unfiltered and d_hist_in is only read: the caller runs
 * rt_temporal_accumulate after the spend for the history it keeps.  Errors as for rt_render_adaptive_spend, and RT_EINVAL for the
 * checks named above (with the parameter checks, before RT_ENOTSUP for USE_FP16 and RT_ARITH_CONTRACT worlds). */
int rt_render_adaptive_spend_temporal(void* fb, int max_x, int max_y, const rt_budget* params, const rt_temporal_inputs* in,
                                      const rt_temporal_params* temporal, const rt_world* world, rt_rand_state* d_rand_state,
                                      const rt_octree* d_octree, int32_t* d_spp, void* d_state, uint32_t* d_picked, void* stream);
int rt_render_adaptive_spend_temporal_on(rt_render_ctx* ctx, void* fb, int max_x, int max_y, const rt_budget* params,
                                         const rt_temporal_inputs* in, const rt_temporal_params* temporal, const rt_world* world,
                                         rt_rand_state* d_rand_state, const rt_octree* d_octree, int32_t* d_spp, void* d_state,
                                         uint32_t* d_picked, void* stream);

/* ---- the image end on the device: 8-bit levels and frame comparison (no reference counterpart) ------------
 * What main.cu:321-333 and evaluations.ipynb:1021-1027 do on the host — quantise a frame, grey it, SSIM / PSNR — for frames that stay
 * on the device.  Frames are in the reference's row-major layout (pixel_index = j*max_x + i, row 0 at the bottom), at most
 * RT_DENOISE_MAX_PIXELS pixels.  tests/frame_metrics_model.py is the model.
 *
 * rt_frame_levels: d_out receives rt_frame_levels_bytes bytes, one pixel after the other in rows of max_x pixels; top_first = 1 puts
 * the frame's row max_y-1 first (the order of a PPM's pixel bytes), 0 keeps the framebuffer's own row order.  Per channel:
 *   value c:  GAMMA the framebuffer's value (RT_PRECISION_FP16: the exact binary32 image of the binary16 value);
 *             SUM (fp32 only) sqrtf(fb / (float)samples), what rt_denoise's pass-through rule and the reference's viewer show.
 *   level:    v = 255.99 * (double)c, one binary64 multiply; the level is INT32_MIN unless v > -2147483649.0 && v < 2147483648.0, else
 *             (int)v, truncated; then clamped to 0..255.  This is the library's P6 rule (rt_write_image), stated on every input: NaN,
 *             +inf, -inf and finite values whose v lies beyond the int range — large positive ones too — all give level 0.
 *   GRAY8:    (r*4899 + g*9617 + b*1868 + 8192) >> 14 on the three levels (cv2's fixed-point RGB to gray).
 * One launch, no allocation, no synchronisation: the call can be captured into a hipGraph.  RT_EINVAL for NULL pointers and whatever
 * rt_frame_levels_check (host only) refuses — a NULL params, non-positive sizes, more than RT_DENOISE_MAX_PIXELS pixels, an unknown
 * precision, input or format, samples < 1 with SUM, top_first outside 0..1 —, then RT_ENOTSUP for SUM with RT_PRECISION_FP16. */
#define RT_LEVELS_RGB8  0   /* 3 bytes a pixel */
#define RT_LEVELS_RGBA8 1   /* 4 bytes, A = 255 */
#define RT_LEVELS_GRAY8 2   /* 1 byte */
typedef struct rt_levels_params {
    int32_t input;      /* RT_DENOISE_INPUT_GAMMA or RT_DENOISE_INPUT_SUM */
    int32_t samples;    /* SUM: the current_sample of the progressive sequence (>= 1); GAMMA: ignored */
    int32_t format;     /* RT_LEVELS_* */
    int32_t top_first;  /* 1: top row first (PPM order); 0: the framebuffer's own row order */
} rt_levels_params;
int rt_frame_levels(void* d_out, const void* fb, int max_x, int max_y, int precision, const rt_levels_params* params, void* stream);
int rt_frame_levels_check(int max_x, int max_y, int precision, const rt_levels_params* params);
/* host only: the size of d_out, -1 for non-positive sizes, more than RT_DENOISE_MAX_PIXELS pixels or an unknown format */
int64_t rt_frame_levels_bytes(int max_x, int max_y, int format);

/* rt_frame_compare: two GAMMA frames of one size, each with its own precision (an fp16 frame against an fp32 one is one call), compared
 * three ways into one 64-byte record in DEVICE memory.  ga, gb are the GRAY8 levels above, computed in the kernel from the float frames.
 *   grey error:  gray_sse = sum (ga - gb)^2 and gray_differ = the pixels with ga != gb; PSNR is cv2.PSNR's 10 log10(255^2 / MSE).
 *   SSIM:        skimage's default (uniform 7x7 window, sample covariance, K1 = 0.01, K2 = 0.03, data range 255, borders cropped), exact
 *                in integers until the last three operations.  For the window whose lowest-index pixel is (i, j), i <= max_x-7,
 *                j <= max_y-7, with the sums over its 49 pixels Sx, Sy, Sxx, Syy, Sxy, P = Sx*Sy in int64, K = 10000, c1 = 65025,
 *                c2 = 585225:
 *                  A1 = K*2*P + 2401*c1                 B1 = K*(Sx*Sx + Sy*Sy) + 2401*c1
 *                  A2 = K*2*(49*Sxy - P) + 2352*c2      B2 = K*((49*Sxx - Sx*Sx) + (49*Syy - Sy*Sy)) + 2352*c2
 *                  S  = ((double)A1 * (double)A2) / ((double)B1 * (double)B2)     three binary64 roundings, no contraction
 *                Every term is below 2^53 (the conversions are exact), B1 and B2 are positive, identical windows give S == 1.0.
 *                d_ssim_map, when not NULL, receives S of every window: (max_y-6) rows of (max_x-6) doubles, framebuffer row order.
 *   float error: over the pixels whose six channels are all finite, sq_err = sum over their 3 channels of ((double)a - (double)b)^2.
 * The integer fields are exact; the two double sums are taken in a fixed order (per block, then over the blocks in index order) without
 * atomics, so the 64 bytes are the same on every run.  A frame with a side below 7 is valid: windows = 0, ssim_sum = 0, the map is not
 * written.  d_work: caller-owned, rt_frame_compare_work_bytes bytes (host only; -1 for non-positive sizes and more than
 * RT_DENOISE_MAX_PIXELS pixels).  Two launches, no allocation, no synchronisation: the call can be captured into a hipGraph.  RT_EINVAL
 * for a NULL fb_a, fb_b, d_metrics or d_work, non-positive sizes, more than RT_DENOISE_MAX_PIXELS pixels, an unknown precision, and a
 * d_metrics, d_work or d_ssim_map that is not 8-byte aligned. */
typedef struct rt_frame_metrics {
    int64_t pixels;          /* max_x * max_y */
    int64_t gray_sse;        /* sum over pixels of (ga - gb)^2 */
    int64_t gray_differ;     /* pixels with ga != gb */
    int64_t windows;         /* (max_x - 6) * (max_y - 6), or 0 when either side is < 7 */
    double  ssim_sum;        /* sum of S over all windows */
    int64_t finite_pixels;   /* pixels whose six channels (a and b) are all finite */
    double  sq_err;          /* over those pixels and their 3 channels: sum of ((double)a - (double)b)^2 */
    int64_t reserved;        /* 0 */
} rt_frame_metrics;
int64_t rt_frame_compare_work_bytes(int max_x, int max_y);
int rt_frame_compare(const void* fb_a, int precision_a, const void* fb_b, int precision_b, int max_x, int max_y,
                     rt_frame_metrics* d_metrics, double* d_ssim_map, void* d_work, void* stream);
/* host only, on a record copied from the device: gray_sse == 0 ? +inf : 10*log10(65025.0 * pixels / gray_sse);  ssim_sum / windows (NaN
 * when windows == 0);  sqrt(sq_err / (3.0 * finite_pixels)) (NaN when finite_pixels == 0).  NaN for a NULL record. */
double rt_frame_psnr(const rt_frame_metrics* m);
double rt_frame_ssim(const rt_frame_metrics* m);
double rt_frame_rmse(const rt_frame_metrics* m);

/* ---- host side: output --------------------------------------------------------------------------------------- */
/* output_to_stream — main.cu:321-333: ASCII P3, top row first, int(255.99*c).  fb is a HOST buffer.
 * path == NULL writes to stdout (output mode 0), otherwise to the file (output mode 3 uses "output.ppm"). */
int rt_write_ppm(const char* path, int nx, int ny, const void* fb, int precision);
/* same bytes into memory; returns the length, or the required length when cap is too small / out is NULL */
int64_t rt_format_ppm(int nx, int ny, const void* fb, int precision, char* out, int64_t cap);

/* Binary companions of the ASCII P3 writer (at 4K the P3 text is ~100 MB and dominates end-to-end time).
 * RT_IMAGE_P6: "P6" binary PPM, same quantisation as main.cu:327-329 (int(255.99*c), clamped to 0..255), top row first.
 * RT_IMAGE_PFM: "PF" float image, little-endian (-1.0 scale), bottom row first (the framebuffer's own row order), the
 * gamma-corrected channel values unquantised.  fb is a HOST buffer in the framebuffer layout of rt_render. */
#define RT_IMAGE_P3 0
#define RT_IMAGE_P6 1
#define RT_IMAGE_PFM 2
int rt_write_image(const char* path, int nx, int ny, const void* fb, int precision, int format);

#ifdef __cplusplus
}
#endif
#include "rt_amd_rebuild.h"   /* part of this ABI: the declarations that follow the ones above, in a file of their own */
#include "rt_amd_fused.h"     /* ... and the adaptive frame in one launch */
#include "rt_amd_refine_fused.h"   /* ... and its refinement in one launch */
#include "rt_amd_h16_adaptive.h"   /* ... and the adaptive frame of binary16 worlds */
#endif /* RT_AMD_H */
