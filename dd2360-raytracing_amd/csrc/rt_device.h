// rt_device.h — device-side data layout shared by the kernels (rt_kernels.hip and its neighbours) and the uploader (rt_api.hip),
// and the few device helpers that more than one kernel file uses (the partition's tile mapping, the pixel hand-out, rank_below, wave_excl_scan).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include "../../include/rt_amd.h"

namespace rt {

// The reference's root box is fixed: (-11, 0, -11)-(11, 2, 11) (acceleration_structure.h:203).  Halved three times it gives 8 x 8 x 8
// level-3 cells of kCellXZ x kCellY x kCellXZ; everything that depends on that geometry — the cell of a hit point, the bricks' cell
// coordinates, the grid's reach — is written in terms of these constants, here, in the kernels and in the device build.
constexpr double kRootHalfXZ = 11.0;            // the box spans [-kRootHalfXZ, kRootHalfXZ] in x and z, [0, 8 kCellY] in y
constexpr double kCellXZ = 2.0 * kRootHalfXZ / 8.0, kCellY = 0.25;
constexpr float kRootHalfXZf = (float)kRootHalfXZ, kInvCellXZf = 1.0f / 2.75f, kInvCellYf = 4.0f;
static_assert(kCellXZ == 2.75 && 1.0 / kCellY == 4.0, "level-3 cells of the reference's root box");

// The tile split of a frame over parts (rt_amd.h, rt_partition).  Two forms: a contiguous range [begin, end) of the row-major tile
// numbering (end > begin: rt_split_balanced cuts the frame into such bands of equal predicted cost), or — begin == end == 0 — runs of
// RT_PART_RUN consecutive tiles dealt round-robin.  Every kernel and the host go through these functions: nothing else knows the mapping.
#ifndef RT_PART_RUN_BUILD
#define RT_PART_RUN_BUILD RT_PART_RUN           // (tools/mkvariant.sh -DRT_PART_RUN_BUILD=n: A/B of the run length)
#endif
constexpr long long kPartRun = RT_PART_RUN_BUILD;
__host__ __device__ inline bool part_whole(int nparts, long long begin, long long end) { return nparts == 1 && end <= begin; }   // the undivided frame: row-major buffers
__host__ __device__ inline long long part_tile(long long local_tile, int part, int nparts, long long begin = 0, long long end = 0) {          // global tile of a part's local tile
    if (end > begin) return begin + local_tile;
    if (nparts == 1) return local_tile;
    return ((local_tile / kPartRun) * nparts + part) * kPartRun + local_tile % kPartRun;
}
__host__ __device__ inline long long part_local_tiles(long long tiles, int part, int nparts, long long begin = 0, long long end = 0) {        // tiles of the frame that belong to `part`
    if (end > begin) return end - begin;
    const long long round = (long long)nparts * kPartRun;
    long long extra = tiles % round - (long long)part * kPartRun;
    extra = extra < 0 ? 0 : (extra > kPartRun ? kPartRun : extra);
    return tiles / round * kPartRun + extra;
}
__host__ __device__ inline void part_owner(long long tile, int nparts, int& part, long long& local_tile) {   // inverse of part_tile (runs)
    const long long run = tile / kPartRun;
    part = (int)(run % nparts);
    local_tile = (run / nparts) * kPartRun + tile % kPartRun;
}
// is `tile` one of this part's, and which of its local tiles
__host__ __device__ inline bool part_has(long long tile, int part, int nparts, long long begin, long long end, long long& local_tile) {
    if (end > begin) { local_tile = tile - begin; return tile >= begin && tile < end; }
    int owner; part_owner(tile, nparts, owner, local_tile);
    return owner == part;
}
// the frame and the part an adaptive check runs over (k_adapt_check: which elements of a compact part buffer are padding)
struct AdaptFrame { int max_x, max_y, tiles_x, part, nparts; long long tile_begin, tile_end; };
// ---- The pixel hand-out: which pixel (i, j) and which buffer element a part's (local tile, position in the tile) or a list entry is,
// and in which order the render kernels' slots go through them.  Written here once; every kernel that decodes goes through it.
// `P` names the frame and the part by its fields max_x, max_y, tiles_x, part, nparts, tile_begin, tile_end: a RenderArgs or an AdaptFrame.
// Buffers: row-major (j * max_x + i) for the undivided frame, compact tile-major (local_tile * 64 + ly * 8 + lx) in a part.  (The statements' order in these helpers is the kernels' instruction text: HISTORY.md, round 30.)
template <class P> __device__ __forceinline__ bool frame_whole(const P& p) { return part_whole(p.nparts, p.tile_begin, p.tile_end); }
// tile -> its column and row of tiles; a tile column (row) and a position 0..7 in it -> pixel column (row)
__device__ __forceinline__ void tile_xy(long long tile, int tiles_x, int& tx, int& ty) { tx = (int)(tile % tiles_x); ty = (int)(tile / tiles_x); }
template <class P> __device__ __forceinline__ void local_tile_xy(const P& p, long long local_tile, int& tx, int& ty) { const long long tile = part_tile(local_tile, p.part, p.nparts, p.tile_begin, p.tile_end); tile_xy(tile, p.tiles_x, tx, ty); }
__device__ __forceinline__ int tile_px(int t, int l) { return t * 8 + l; }
template <class P> __device__ __forceinline__ void local_pixel(const P& p, long long local_tile, int l, int& i, int& j) { int tx, ty; local_tile_xy(p, local_tile, tx, ty); i = tile_px(tx, l & 7); j = tile_px(ty, l >> 3); }   // the tile decode: (local tile, position l = ly * 8 + lx in it) -> pixel
// the list-entry decode: entries are buffer elements (the adaptive lists, rt_adaptive.hip) -> pixel
// (the part's branch is local_pixel of (pid >> 6, pid & 63), spelt out: through the call k_render<*,2,*> and <*,4,*> come out as other text)
template <class P> __device__ __forceinline__ void listed_pixel(const P& p, unsigned int pid, int& i, int& j) {
    if (frame_whole(p)) { i = (int)(pid % (unsigned int)p.max_x); j = (int)(pid / (unsigned int)p.max_x); return; }
    const long long tile = part_tile((long long)(pid >> 6), p.part, p.nparts, p.tile_begin, p.tile_end);
    const int tx = (int)(tile % p.tiles_x), ty = (int)(tile / p.tiles_x);
    i = tile_px(tx, (int)(pid & 7u)); j = tile_px(ty, (int)((pid >> 3) & 7u));
}
// the buffer element of pixel (i, j), which is position l of the part's local tile — or element `compact` of its buffer, `whole` held by the caller
template <class P> __device__ __forceinline__ long long pixel_elem(const P& p, int i, int j, long long local_tile, int l) { return frame_whole(p) ? (long long)j * p.max_x + i : local_tile * 64 + l; }
template <class P> __device__ __forceinline__ long long pixel_elem(const P& p, bool whole, int i, int j, long long compact) { return whole ? (long long)j * p.max_x + i : compact; }
template <class P> __device__ __forceinline__ long long part_elems(const P& p) { return frame_whole(p) ? (long long)p.max_x * p.max_y : p.n_local_tiles * 64; }   // elements of this part's buffers (rt_part_pixels on the host)
// element t of a part's compact tile-major buffer lies inside the frame (the elements of edge tiles outside it are padding)
__device__ __forceinline__ bool adapt_in_frame(long long t, const AdaptFrame& fr) {
    const long long tile = part_tile(t >> 6, fr.part, fr.nparts, fr.tile_begin, fr.tile_end);
    const int tx = (int)(tile % fr.tiles_x), ty = (int)(tile / fr.tiles_x);       // (tile_xy, spelt out: as a call it changes the text of k_budget_keys and k_adapt_refine_seed)
    return tile_px(tx, (int)(t & 7)) < fr.max_x && tile_px(ty, (int)((t >> 3) & 7)) < fr.max_y;
}
// The interleaved slots: consecutive slots are the same pixel position of kIl different tiles (in hand-out order), so the 64 pixels of a
// tile go to 64 different lanes; the last block holds the tiles that are left.  Slot ms -> position in the hand-out order, and l.
// (k_render<true,3,1> takes two other registers with this call in any of twelve forms — HISTORY.md, round 30 — so k_render restates it.)
template <int kIl> __device__ __forceinline__ long long slot_rank(long long ms, long long n_local_tiles, int& l) {
    const long long blk = ms / (64 * kIl);
    const long long tiles_in_blk = (n_local_tiles - blk * kIl) < kIl ? (n_local_tiles - blk * kIl) : kIl;
    const long long within = ms % (64 * kIl);
    const long long rank = blk * kIl + within % tiles_in_blk;
    l = (int)(within / tiles_in_blk); return rank;
}
// The long list is in the pilot's order, the pixels of a 2x2 block and the blocks of a tile next to each other, and neighbours are chains of like length: a stride
// (a prime that does not divide the count, so a permutation) puts them into different waves, each left alone once the shorter ones ended.  Entry of the h-th chain handed out:
__device__ __forceinline__ unsigned int long_list_at(unsigned int h, unsigned int n_long) { const unsigned int stride = n_long % 257u ? 257u : (n_long % 263u ? 263u : 269u); return (unsigned int)(((unsigned long long)h * stride) % n_long); }
// a pixel's generator (XORWOW's six words; rt_rand_state's Box-Muller fields are never used): the register copy every render unit keeps, loaded and stored
struct Rng { uint32_t d, v0, v1, v2, v3, v4; };
template <class RNG> __device__ __forceinline__ void rng_load(RNG& s, const rt_rand_state* st) { s.d = st->d; s.v0 = st->v[0]; s.v1 = st->v[1]; s.v2 = st->v[2]; s.v3 = st->v[3]; s.v4 = st->v[4]; }
template <class RNG> __device__ __forceinline__ void rng_store(rt_rand_state* st, const RNG& s) { st->d = s.d; st->v[0] = s.v0; st->v[1] = s.v1; st->v[2] = s.v2; st->v[3] = s.v3; st->v[4] = s.v4; }

// the caller's refinement state of rt_render_adaptive_begin / _refine, structure of arrays over the n buffer elements:
// S_rgb[3n] (interleaved like fb), SL[n], Q[n], k[n] (int32) — RT_ADAPTIVE_STATE_BYTES = 24 per element
struct AdaptState { float* rgb; float* sl; float* q; int32_t* k; };
__host__ __device__ inline AdaptState adapt_state(void* base, long long n) {
    float* f = (float*)base;
    return AdaptState{f, f + 3 * n, f + 4 * n, (int32_t*)(f + 5 * n)};
}
// rt_adaptive_priority (rt_amd.h): the squared relative standard error of a pixel's mean luminance, the mean floored at floor_lum —
// what adapt_rule compares with rel_error^2, divided out.  IEEE binary32, one rounding per operation (its callers, rt_budget.hip and rt_api.hip,
// are compiled with -ffp-contract=off).  Never negative and never NaN, so its bits read as uint32 order it.
__host__ __device__ inline float adapt_priority(float SL, float Q, int k, float floor_lum) {
    const float n = (float)k;
    float d = n * Q - SL * SL;
    d = d > 0.f ? d : 0.f;                                  // (a NaN d becomes 0)
    const float nf = n * floor_lum;
    const float m = SL > nf ? SL : nf;
    const float e = d / ((n - 1.f) * (m * m));
    return e > 0.f ? e : 0.f;                               // NaN (0/0, a NaN sum) becomes 0; +inf stays
}
// rt_adaptive_priority_filtered (rt_amd.h): the same quantity for a pixel after one level of rt_denoise_adaptive's filter — l the
// luminance of the filtered mean, v the variance of that mean (v' of the level).  Same compilation rule, same properties.
__host__ __device__ inline float adapt_priority_filtered(float l, float v, float floor_lum) {
    const float m = l > floor_lum ? l : floor_lum;          // (a NaN l takes the floor)
    const float e = v / (m * m);
    return e > 0.f ? e : 0.f;                               // NaN becomes 0; +inf stays
}
// one level of rt_denoise_adaptive, as its level kernel and the filtered budget key take it (rt_denoise.hip, rt_budget.hip)
struct DenoiseVarLevel {
    int32_t h;             // tap step 2^L
    int32_t npow;          // normal_pow_log2 (-1 = no normal term)
    int32_t use_pos, use_var, prefilter;
    float inv_sp2;         // 1 / sigma_position^2
    float sv2;             // sigma_variance^2
};
inline DenoiseVarLevel denoise_var_level(const rt_denoise_var_params& P, int l) {
    DenoiseVarLevel L;
    L.h = 1 << l;
    L.npow = P.normal_pow_log2;
    L.use_pos = P.sigma_position > 0.0f;
    L.use_var = P.sigma_variance > 0.0f;
    L.prefilter = P.prefilter;
    L.inv_sp2 = L.use_pos ? 1.0f / (P.sigma_position * P.sigma_position) : 0.0f;
    L.sv2 = L.use_var ? P.sigma_variance * P.sigma_variance : 0.0f;
    return L;
}
constexpr int kMaxSplitParts = 64;
struct SplitStarts { long long s[kMaxSplitParts + 1]; };      // first tile of every band of a balanced split, and the tile count (k_gather by bands, rt_assemble.hip)

// One node of the traversal copy of the Octree, in depth-first pre-order (children in index order, the visit
// order of traverseTree, acceleration_structure.h:276-304).  48 bytes = 3 x 16 B so a lane fetches it with
// three ds_read_b128 from LDS.
struct DevNode {
    float lo[3];      // x_low, y_low, z_low
    float hix;        // x_high
    float hiy, hiz;   // y_high, z_high
    int32_t skip;     // pre-order index of the next node when this one is culled (= end of its subtree)
    int32_t first;    // level-3 node: first entry of its concatenated buckets in ent_hot / ent_id
    int32_t count;    // level-3 node: number of entries (ghost entries removed); 0 for inner nodes
    int32_t ref_index;// index of this node in the reference-layout nodes[] (diagnostics)
    int32_t pad[2];
};
static_assert(sizeof(DevNode) == 48, "DevNode is 3 x float4");

struct DevScene {
    const float4* list_hot;   // [n_list] (cx, cy, cz, radius*radius) of the hittable spheres, list order
    const int32_t* list_id;   // [n_list] index into the world list
    const float4* geom;       // [n] (cx, cy, cz, radius)
    const float4* mat;        // [n] (albedo r,g,b, param)
    const int32_t* kind;      // [n] RT_MAT_*
    const float4* shade;      // [2n] what a hit needs, side by side: geom[i], mat[i] — one 32-byte record, one cache line per hit
                              // (binary32 worlds: a dielectric's mat half is (1/ri, r0^2, ri^2, ri) — its albedo is never read; world_upload, rt_api.hip)
    const uint8_t* kind8;     // [n] RT_MAT_* as bytes (10 KB at C3: stays in the vector L1)
    int32_t n, n_list;
    int32_t ground_valid;     // world list slot 0 is hittable (it is tested first by hitTree)
    rt_camera cam;
};

// Candidate-culling structure for the fast closest-hit path.  It never decides a hit: it only
// enumerates a superset of the spheres whose float sphere::hit can succeed; membership of a sphere in a level-3 cell
// that the reference's traversal visits is then checked with the reference's own slab test.
struct DevAccel {
    const float4* large_hot;   // [n_large] (cx,cy,cz,r^2): tree spheres too big (or too far out) for the grid, always tested
    const float4* large_brick; // [2*n_large] as `brick`
    // The grid: columns of width h along a ray's major axis, each sphere registered ONCE in every column its inflated extent
    // overlaps, a column's entries sorted by the sphere's CENTRE along the minor axis into Gf = G * F fine bins (bin width h / F).
    // A ray asks a column for the bins its line crosses grown by the largest inflated radius (rq_c, in cell units) — the
    // inflation sits in the query, not in the registration, so no sphere appears twice in a column's range.
    // Two copies: columns along x (bin (ix, fz) at ix*Gf + fz) in cs[0 .. G*Gf], columns along z (bin (iz, fx) at iz*Gf + fx) in
    // cs[zoff .. zoff + G*Gf]; cs values index hot[] / brick[] directly (the z copy's entries follow the x copy's).
    const int32_t* cs;
    const float4* hot;         // (cx,cy,cz,r^2)
    // per entry two float4: (lo.x, lo.y, lo.z, bits of the world-list index), (hi.x, hi.y, hi.z, bits of node1) —
    // lo/hi = the sphere's brick in level-3 cell coordinates, margins included (rt_accel.h), lo = +inf when it has none;
    // node1 = the single level-3 node (pre-order index) that stores the sphere, or -1 if several do
    const float4* brick;
    int32_t zoff;
    const int32_t* memb_start; // [n+1] per world-list index: range in memb_cell
    const int32_t* memb_cell;  // pre-order node index (DevNode) of each level-3 node whose buckets hold the sphere
    const int32_t* bits_index; // [n] per world-list index: row of cellbits for spheres stored in several nodes, else -1
    const uint32_t* cellbits;  // rows of 16 words: bit (ix*64 + iy*8 + iz) set = the sphere is stored in that level-3 cell
    const int32_t* cellnode;   // [512] level-3 cell (ix*64 + iy*8 + iz of the root box's 8x8x8 grid) -> pre-order node index, or -1
    int32_t n_large, G;
    int32_t F, Gf;             // fine bins per cell along a column's minor axis, G * F
    float rq_c;                // query growth in cell units: (largest inflated radius + walk slack) / h
    float g0, h, inv_h;        // grid origin (same for x and z), cell size
    float ylo, yhi;            // y-slab covering every grid sphere's inflated ball
    float rmax;                // largest inflated radius R' of a grid sphere
    float zone2;               // fast path only for ray origins with |o - (0,1,0)|^2 <= zone2
    int32_t enabled;
    int32_t coop_groups;       // cooperative walk: up to this many rays side by side (4 on sparse grids, 1 on dense ones)
    int32_t solo_chains;       // very sparse grids (at most one entry per cell on average: lists of a few hundred spheres): the pre-classified
                               // long chains start alone in their waves (k_render<true,*,5>)
};

struct DevTree {
    const float4* nodes4;     // [n_nodes*3] DevNode as float4 triples
    const float4* ent_hot;    // [n_entries] (cx, cy, cz, radius*radius) in traversal order
    const int32_t* ent_id;    // [n_entries] index into the world list
    int32_t n_nodes, n_entries;
    // binary16 trees only (rt_kernels_fp16.hip): the distinct box planes of the tree per axis — the reference's boxes are the
    // root box halved three times, 9 planes an axis — so a ray divides once per plane, not six times per visited node.
    // h16_planes = [x planes | y planes | z planes] (h16_np of each; h16_np[0] == 0: no table, the generic slab test);
    // DevNode::pad[0] holds the node's six plane indices, 5 bits each: x_low, x_high, y_low, y_high, z_low, z_high.
    const float* h16_planes;
    int32_t h16_np[3];
    DevAccel acc;
};

// how many of a ballot's lanes lie below this one: a voting lane's rank among the voters, the slot it takes when they append to a list
static __device__ __forceinline__ unsigned rank_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// exclusive prefix sum over the 64 lanes of a wave (the grid walk's pool, the tail sort's bins): row_shr 1/2/4/8 (a row of 16), then
// row_bcast 15 and 31 — six DPP adds, no LDS
static __device__ __forceinline__ unsigned wave_excl_scan(unsigned v, unsigned& total) {
    int x = (int)v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);     // row_bcast:15 into rows 1 and 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);     // row_bcast:31 into rows 2 and 3
    total = (unsigned)__builtin_amdgcn_readlane(x, 63);
    return (unsigned)x - v;
}

constexpr int kQueueThr = 32;
struct RenderArgs {
    void* fb;
    rt_rand_state* rand_state;
    int32_t max_x, max_y, ns;             // ns = current_sample for the progressive kernel
    int32_t tiles_x, tiles_y;
    int32_t part, nparts;
    int64_t tile_begin, tile_end;         // end > begin: this part is the contiguous tile range [begin, end) (local tile = tile - begin)
    int64_t n_local_tiles;
    unsigned int* queue;                  // counters of this launch, zeroed on the stream: [0] work counter [1] thin waves [2] long chains [3] long head
                                          // [4] solo chains [5] solo head; in the slot's second 128-byte line, written by k_tile_order before the render kernel starts and
                                          // only read by it (the first line is hammered by every wave's atomics: a load from it waits behind them):
                                          // [kQueueThr] in-flight chain threshold (iterations; 0 = the rate rule only) [kQueueThr + 1] pilot-sum threshold
                                          // [kQueueThr + 2] first slot of the queue's tail + 1 (0 = no tail): those slots go through tail_list
    int32_t n_lanes;                      // lanes of the persistent render grid this launch will run on (64 x waves): the per-lane load is the yardstick of a "long" pixel
    const unsigned int* tail_list;        // the pixels of the last tiles of the hand-out order, most expensive 2x2 block first (k_tail_hist / k_tail_scatter); NULL = none
    unsigned int* tail_ws;                // 512 words behind the lists: the tail sort's 256 counts and 256 cursors
    float head_min_load;                  // dense grids: launches of fewer predicted iterations per lane keep the whole tail at the end
    int32_t head_sum, head_sum_dense;     // tail pixels whose 3x3 pilot sum reaches this — or, negative, is at most its magnitude — are handed out FIRST (0 = none; sparse grids / dense grids); queue[kQueueThr + 3] = how many, [kQueueThr + 4] = the sum in force, [kQueueThr + 5] = taken from the list's cheap end
    float f_tail;                         // share of the launch's predicted work handed out per pixel instead of per tile, at the end of the queue
    float f_inflight_dense;               // f_inflight of launches on dense grids (k_render<true,*,2>)
    float f_inflight, f_static;           // a pixel is long when its predicted chain exceeds f x (predicted iterations of the launch / n_lanes): found in flight / by the pilot
    const unsigned int* order;            // hand-out order of the local tiles (most expensive first), or NULL = identity
    const unsigned char* long_flag;       // per local pixel (local_tile*64 + l): pre-classified long chain, or NULL
    const unsigned int* long_list;        // the pre-classified long chains (queue[2] = count, queue[3] = next to hand out)
    DevScene scene;
    DevTree tree;
    // adaptive rounds (k_render<*, 2, *>, rt_render_adaptive): the lane leaves the running sums behind — fb = S_rgb, ad_sl = sum of the
    // samples' luminance, ad_q = sum of its squares — instead of the final colour.  ad_list == NULL: round 0, the whole frame through
    // the scheduled hand-out, from zero; otherwise the pixels (row-major indices) still active, *ad_count of them, resumed from the sums.
    // (a fused frame, k_render<*, 3, *>, has no rounds: these four words carry its FusedArgs instead, below)
    const unsigned int* ad_list;
    const unsigned int* ad_count;
    float* ad_sl;
    float* ad_q;
    // the measured pass (rt_sched_keep.h "Feedback"): per buffer element (indexed like fb) the iterations the pixel took, saturating at
    // 65535, stored by MODE 0 of k_render<true,*,4> and <true,*,5> where it ends a pixel; NULL = not recorded (every other launch)
    unsigned short* iters_out;
};
// The fused adaptive frame (k_render<*, 3, *>, rt_render_adaptive_fused; RenderArgs::ns = max_spp): the stop rule's parameters, which
// the lane itself applies after min_spp, min_spp + batch, ... samples, and where a pixel's end goes — its colour to fb, its count to
// spp (NULL: not wanted) and, state != NULL, S_rgb, SL, Q and k to the caller's refinement state, adapt_state(state, elements of the
// part).  A fused launch has no rounds and reads none of ad_list, ad_count, ad_sl, ad_q: its arguments travel in those 32 bytes, so
// RenderArgs keeps its size and its declaration.  (Appended fields move whatever lies behind the struct in the argument segment of
// every kernel that takes one, the hidden arguments included, and with them a scalar load's offset in those kernels' text; a union
// over the four words changed the order of MODE 2's loads and stores: HISTORY.md, round 28.)
struct FusedArgs { int32_t min_spp, batch; float rel_error, floor; void* state; int32_t* spp; };
static_assert(sizeof(FusedArgs) == 32 && offsetof(RenderArgs, ad_q) + sizeof(float*) - offsetof(RenderArgs, ad_list) == sizeof(FusedArgs),
              "FusedArgs fills the four words of the rounds");
static_assert(sizeof(RenderArgs) == 568, "RenderArgs keeps its size: what lies behind it in a kernel's argument segment keeps its offset");
inline void fused_args_set(RenderArgs& A, const FusedArgs& F) { memcpy((void*)&A.ad_list, &F, sizeof F); }
__device__ __forceinline__ FusedArgs fused_args(const RenderArgs& A) { FusedArgs F; __builtin_memcpy(&F, (const void*)&A.ad_list, sizeof F); return F; }
// The fused refinement (k_render<*, 4, *>, rt_render_adaptive_refine_fused; RenderArgs::ns = to.max_spp): a launch over the list that
// k_adapt_refine_seed leaves, every listed pixel resumed from the caller's state (never NULL here) and run on under the same rule.  Its
// FusedArgs travel where MODE 3's do (min_spp is carried and not read: a resumed pixel's checkpoints count from its own k); the list
// needs one pointer more.  It travels in iters_out, which only MODE 0 reads (a list launch has no measured pass), and its count is the
// word `elements of the part` behind the list's start — the first word of the second of the two lists the adaptive workspace holds,
// which a fused refinement never fills.  The kernel forms that offset from its own arguments, as it does for adapt_state.
static_assert(sizeof(unsigned short*) == sizeof(const unsigned int*) &&
              (offsetof(RenderArgs, iters_out) >= offsetof(RenderArgs, ad_list) + sizeof(FusedArgs) || offsetof(RenderArgs, iters_out) + sizeof(unsigned short*) <= offsetof(RenderArgs, ad_list)),
              "the refinement's list travels in iters_out, outside the words of FusedArgs");
inline void refine_fused_list_set(RenderArgs& A, const unsigned int* list) { memcpy((void*)&A.iters_out, &list, sizeof list); }
__device__ __forceinline__ const unsigned int* refine_fused_list(const RenderArgs& A) { const unsigned int* l; __builtin_memcpy(&l, (const void*)&A.iters_out, sizeof l); return l; }

} // namespace rt
