// rt_multi.hip — one frame over the GPUs of a node: rt_multi_render (include/rt_amd.h).
//
// No reference counterpart (the reference is single-GPU); the launch surface it extends is main.cu:422-427.  One process per
// GPU.  The frame's 8x8 tiles (the reference's block shape, main.cu:351-352) are split over the ranks — by default dealt round-robin
// in runs of RT_PART_RUN consecutive tiles (RT_SPLIT_RUNS), or, opt-in (rt_multi_set_split), cut into horizontal bands of equal
// predicted cost (rt_split_balanced: every rank runs the same pilot pass over the whole frame and cuts it the same way, no
// communication; a GPU's rays then meet the same part of the scene, as in the undivided frame); pixels are independent (the per-pixel
// RNG is keyed by the absolute pixel_index, main.cu:93), so every split gives the bits of the single-GPU frame.  Each rank renders its tiles
// into a compact tile-major buffer (rt_partition) and ONE exchange brings the buffers to the root: with RCCL a single
// ncclGroupStart / ncclRecv x (nranks-1) | ncclSend / ncclGroupEnd straight out of the render buffer and straight into the
// root's staging slots (the root renders into its own slot: no copy anywhere), on the caller's stream; then rt_assemble
// restores the row-major frame.  Payload at 3840x2160: 99.5 MB in all, 12.4 MB per peer, each on its own xGMI link.
//
// RCCL is bound at run time (dlopen "librccl.so.1": a process that already carries an RCCL — PyTorch — shares it; a
// single-GPU user of librt_amd.so needs none).  rt_multi_init_custom takes the exchange as a callback instead (MPI, gloo, a
// test harness): same partition, same buffers, same assemble.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <new>
#include <cstring>
#include <mutex>
#include <algorithm>
#include "../../include/rt_amd.h"
#include "rt_handles.h"
#include "rt_launch.h"

namespace {

// the few RCCL entry points used, with the types of /opt/rocm/include/rccl/rccl.h (ncclResult_t and the enums are ints)
struct NcclId { char internal[128]; };
typedef void* NcclComm;
enum { kNcclInt32 = 2, kNcclFloat16 = 6, kNcclFloat32 = 7 };        // ncclInt32 / ncclFloat16 / ncclFloat32 of rccl.h
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(NcclId*) = nullptr;
    int (*CommInitRank)(NcclComm*, int, NcclId, int) = nullptr;
    int (*CommDestroy)(NcclComm) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, NcclComm, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, NcclComm, hipStream_t) = nullptr;
    bool ok = false;
};
void rccl_bind(Rccl& R) {
    R.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!R.lib) R.lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!R.lib) return;
    R.GetUniqueId = (int (*)(NcclId*))dlsym(R.lib, "ncclGetUniqueId");
    R.CommInitRank = (int (*)(NcclComm*, int, NcclId, int))dlsym(R.lib, "ncclCommInitRank");
    R.CommDestroy = (int (*)(NcclComm))dlsym(R.lib, "ncclCommDestroy");
    R.GroupStart = (int (*)())dlsym(R.lib, "ncclGroupStart");
    R.GroupEnd = (int (*)())dlsym(R.lib, "ncclGroupEnd");
    R.Send = (int (*)(const void*, size_t, int, int, NcclComm, hipStream_t))dlsym(R.lib, "ncclSend");
    R.Recv = (int (*)(void*, size_t, int, int, NcclComm, hipStream_t))dlsym(R.lib, "ncclRecv");
    R.ok = R.GetUniqueId && R.CommInitRank && R.CommDestroy && R.GroupStart && R.GroupEnd && R.Send && R.Recv;
}
Rccl& rccl() {                                        // bound once per process, whichever thread asks first
    static Rccl R;
    static std::once_flag once;
    std::call_once(once, rccl_bind, R);
    return R;
}
#define RT_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (int)e_; } while (0)
#define RT_NCCL(expr) do { if ((expr) != 0) return RT_ECOMM; } while (0)

// A frame moves one or two lanes of data to the root: the colours (3 floats or halves per element) and, for an adaptive frame, the
// sample counts (one int32 per element).  In every order — buffers, gather callbacks, RCCL calls — colours come first.
enum { kColour = 0, kCounts = 1, kLanes = 2 };
struct Lane { void* d_local = nullptr; int64_t local_bytes = 0; void* d_parts = nullptr; int64_t parts_bytes = 0; };
struct LaneFormat { size_t bytes; int dtype; size_t words; };      // bytes per element; RCCL datatype and how many of it an element is
LaneFormat lane_format(int k, int precision) {
    if (k == kCounts) return {sizeof(int32_t), kNcclInt32, 1};
    return precision == RT_PRECISION_FP16 ? LaneFormat{6, kNcclFloat16, 3} : LaneFormat{12, kNcclFloat32, 3};
}

}  // namespace


struct rt_multi {
    int rank = 0, nranks = 1;
    NcclComm comm = nullptr;
    rt_gather_fn gather = nullptr; void* user = nullptr;
    rt_render_ctx* ctx = nullptr;
    // this rank's RNG states (compact, tile-major); per lane its part when it is not the root, the root's staging slots
    void* d_rand = nullptr; int64_t rand_bytes = 0;
    Lane lane[kLanes];
    hipEvent_t ev0 = nullptr, ev1 = nullptr; bool timed = false;
    // how the frame is divided (rt_multi_set_split) and the bands of the last balanced split, with what they were computed for
    int split_mode = RT_SPLIT_RUNS;
    bool adaptive_fused = false;         // rt_multi_set_adaptive_fused: a rank's adaptive part in one launch (rt_render_adaptive_fused_on)
    int64_t starts[rt::kMaxSplitParts + 1] = {0}; bool have_split = false; uint64_t split_key[4] = {0, 0, 0, 0};
};

// one buffer with its size, grown on its own demand
static int grow(void** p, int64_t* have, size_t need) { return group_reserve(*have, (int64_t)need, DevGroup().add(p, need)); }
static DevGroup multi_group(rt_multi* M) {
    DevGroup g;
    g.add(&M->d_rand, 0);
    for (Lane& L : M->lane) g.add(&L.d_local, 0).add(&L.d_parts, 0);
    return g;
}

static int multi_new(rt_multi** out, int rank, int nranks) {
    if (!out || nranks < 1 || rank < 0 || rank >= nranks) return RT_EINVAL;
    *out = nullptr;
    rt_multi* M = new (std::nothrow) rt_multi();
    if (!M) return RT_ENOMEM;
    M->rank = rank; M->nranks = nranks;
    int rc = rt_render_ctx_create(&M->ctx);
    if (!rc) { hipError_t e = hipEventCreate(&M->ev0); if (e == hipSuccess) e = hipEventCreate(&M->ev1); rc = (int)e; }
    if (rc) { rt_multi_destroy(M); return rc; }
    *out = M;
    return 0;
}

extern "C" {

int rt_multi_unique_id(void* id_out) {
    if (!id_out) return RT_EINVAL;
    Rccl& R = rccl();
    if (!R.ok) return RT_ENOTSUP;
    NcclId id;
    RT_NCCL(R.GetUniqueId(&id));
    memcpy(id_out, &id, sizeof(id));
    return 0;
}

// What rt_multi_init needs BEFORE it enters the collective ncclCommInitRank, checked without talking to anybody: RCCL bound
// with every entry point, and a context + events on the calling process's current device.  A job calls this on every rank,
// agrees on the answers over its own control plane (gloo, MPI) and only then lets ALL ranks — or none — call rt_multi_init:
// a rank that returned early from rt_multi_init would leave the others blocked inside the collective.
int rt_multi_probe(void) {
    if (!rccl().ok) return RT_ENOTSUP;
    rt_multi* M = nullptr;
    const int rc = multi_new(&M, 0, 1);
    if (rc) return rc;
    return rt_multi_destroy(M);
}

int rt_multi_init(rt_multi** out, int rank, int nranks, const void* unique_id) {
    if (!unique_id) return RT_EINVAL;
    Rccl& R = rccl();
    if (!R.ok) return RT_ENOTSUP;
    int rc = multi_new(out, rank, nranks);
    if (rc) return rc;
    NcclId id;
    memcpy(&id, unique_id, sizeof(id));
    if (R.CommInitRank(&(*out)->comm, nranks, id, rank) != 0) { rt_multi_destroy(*out); *out = nullptr; return RT_ECOMM; }
    return 0;
}

int rt_multi_init_custom(rt_multi** out, int rank, int nranks, rt_gather_fn gather, void* user) {
    if (!gather) return RT_EINVAL;
    const int rc = multi_new(out, rank, nranks);
    if (rc) return rc;
    (*out)->gather = gather; (*out)->user = user;
    return 0;
}

int rt_multi_destroy(rt_multi* M) {
    if (!M) return 0;
    int rc = 0;
    if (M->comm && rccl().ok && rccl().CommDestroy(M->comm) != 0) rc = RT_ECOMM;
    const int r1 = group_free(multi_group(M)); if (!rc) rc = r1;
    if (M->ev0) (void)hipEventDestroy(M->ev0);
    if (M->ev1) (void)hipEventDestroy(M->ev1);
    const int r2 = rt_render_ctx_destroy(M->ctx); if (!rc) rc = r2;
    delete M;
    return rc;
}

int rt_multi_set_split(rt_multi* M, int mode) {
    if (!M || mode < RT_SPLIT_RUNS || mode > RT_SPLIT_BALANCED_CACHED) return RT_EINVAL;
    M->split_mode = mode; M->have_split = false;
    return 0;
}
int rt_multi_set_adaptive_fused(rt_multi* M, int on) {
    if (!M || (on != 0 && on != 1)) return RT_EINVAL;
    M->adaptive_fused = on == 1;
    return 0;
}
int rt_multi_last_split(rt_multi* M, int64_t* starts) {
    if (!M || !starts || !M->have_split) return RT_EINVAL;
    for (int p = 0; p <= M->nranks; ++p) starts[p] = M->starts[p];
    return 0;
}

// lane k's buffers for a part of n_mine elements of `bytes` bytes: on the root the staging slots of `per` elements each, elsewhere the send buffer
static int lane_buffers(rt_multi* M, int k, int64_t n_mine, int64_t per, size_t bytes, int root) {
    Lane& L = M->lane[k];
    if (M->rank == root) return grow(&L.d_parts, &L.parts_bytes, (size_t)per * bytes * (size_t)M->nranks);
    return grow(&L.d_local, &L.local_bytes, (size_t)(n_mine > 0 ? n_mine : 1) * bytes);
}
// this rank's RNG states and colour lane for a part of n_mine pixels
static int multi_buffers(rt_multi* M, int64_t n_mine, int64_t per, size_t px, int root) {
    const int rc = grow(&M->d_rand, &M->rand_bytes, (size_t)(n_mine > 0 ? n_mine : 1) * sizeof(rt_rand_state));
    return rc ? rc : lane_buffers(M, kColour, n_mine, per, px, root);
}

// buffers for frames of this size (rt_multi_render grows them on demand; call this once before timing or graph capture).
// RT_SPLIT_RUNS: exactly what the frame needs.  Balanced splits: the bands' sizes depend on the scene — reserved here for bands of up to
// twice the mean; a frame whose split asks for more grows them in rt_multi_render.
int rt_multi_reserve(rt_multi* M, int max_x, int max_y, int precision, int root) {
    if (!M || max_x <= 0 || max_y <= 0 || root < 0 || root >= M->nranks) return RT_EINVAL;
    if (precision != RT_PRECISION_FP32 && precision != RT_PRECISION_FP16) return RT_EINVAL;
    const size_t px = lane_format(kColour, precision).bytes;
    const rt_partition mine = {M->rank, M->nranks, 0, 0}, first = {0, M->nranks, 0, 0};
    int64_t n_mine = rt_part_pixels(max_x, max_y, mine), per = rt_part_pixels(max_x, max_y, first);
    const bool balanced = M->split_mode != RT_SPLIT_RUNS && M->nranks > 1;
    if (balanced) { n_mine = per * 2; per = per * 2; }
    int rc = multi_buffers(M, n_mine, per, px, root);
    if (!rc) rc = rt_render_ctx_reserve(M->ctx, max_x, max_y, balanced ? rt_partition{0, 1, 0, 0} : mine);      // (a balanced split runs its pilot pass over the whole frame)
    return rc;
}

// One frame on its way to the root: what the entry point was asked for, and what frame_begin decides.
struct Frame {
    int max_x, max_y, precision, root, nlanes;
    void* out[kLanes];                 // the caller's row-major buffers (fb_full, d_spp_full)
    rt_partition mine; bool balanced;  // this rank's part; bands of a balanced split or runs
    int64_t per;                       // elements between the staging slots of two ranks (the largest part)
    void* local[kLanes];               // where this rank renders lane k
};
// elements of rank r's part
static int64_t frame_elems(const rt_multi* M, const Frame& F, int r) {
    return rt_part_pixels(F.max_x, F.max_y, rt_partition{r, M->nranks, F.balanced ? M->starts[r] : 0, F.balanced ? M->starts[r + 1] : 0});
}
// where this rank renders lane k: a single rank's "part" is the whole frame in the reference's row-major layout (rt_partition,
// nparts == 1), straight into the caller's buffer; the root renders straight into its slot of the staging buffer, the others into
// their send buffer
static void* lane_staging(const rt_multi* M, const Frame& F, int k) {
    if (M->nranks == 1) return F.out[k];
    const Lane& L = M->lane[k];
    return M->rank == F.root ? (void*)((char*)L.d_parts + (size_t)F.per * lane_format(k, F.precision).bytes * (size_t)F.root) : L.d_local;
}

// the split, this rank's buffers and staging, its RNG states initialised: everything before the entry point's render call
static int frame_begin(rt_multi* M, Frame& F, const rt_world* world, const rt_octree* d_octree, void* stream) {
    const int max_x = F.max_x, max_y = F.max_y;
    const size_t px = lane_format(kColour, F.precision).bytes;
    const int64_t tiles = (int64_t)((max_x + 7) / 8) * ((max_y + 7) / 8);
    F.balanced = M->split_mode != RT_SPLIT_RUNS && M->nranks > 1 && tiles >= M->nranks;
    F.mine = rt_partition{M->rank, M->nranks, 0, 0};
    F.per = 0;
    int rc = 0;
    RT_TRY(hipEventRecord(M->ev0, (hipStream_t)stream));                  // (this rank's share of the frame starts with the split)
    if (F.balanced) {
        // every rank cuts the frame the same way: the same pilot pass, the same integer arithmetic (rt_split_balanced)
        const uint64_t key[4] = {world->serial, d_octree ? d_octree->serial : 0, ((uint64_t)(uint32_t)max_x << 32) | (uint32_t)max_y,
                                 ((uint64_t)(uint32_t)M->nranks << 32) | (uint32_t)(d_octree ? d_octree->traversal : 0)};
        if (!(M->split_mode == RT_SPLIT_BALANCED_CACHED && M->have_split && memcmp(key, M->split_key, sizeof(key)) == 0)) {
            M->have_split = false;
            if ((rc = rt_split_balanced(M->ctx, world, d_octree, max_x, max_y, M->nranks, M->starts, nullptr, nullptr, nullptr, stream))) return rc;
            memcpy(M->split_key, key, sizeof(key)); M->have_split = true;
        }
        F.mine.tile_begin = M->starts[M->rank]; F.mine.tile_end = M->starts[M->rank + 1];
        for (int r = 0; r < M->nranks; ++r) F.per = std::max<int64_t>(F.per, (M->starts[r + 1] - M->starts[r]) * 64);
        if ((rc = multi_buffers(M, (F.mine.tile_end - F.mine.tile_begin) * 64, F.per, px, F.root))) return rc;
    } else {
        M->have_split = false;
        if ((rc = rt_multi_reserve(M, max_x, max_y, F.precision, F.root))) return rc;
        F.per = rt_part_pixels(max_x, max_y, rt_partition{0, M->nranks, 0, 0});
    }
    // (the further lanes have buffers only where there is an exchange)
    for (int k = kColour + 1; k < F.nlanes && M->nranks > 1; ++k)
        if ((rc = lane_buffers(M, k, rt_part_pixels(max_x, max_y, F.mine), F.per, lane_format(k, F.precision).bytes, F.root))) return rc;
    for (int k = 0; k < F.nlanes; ++k) F.local[k] = lane_staging(M, F, k);
    return rt_render_init(max_x, max_y, (rt_rand_state*)M->d_rand, F.mine, stream);
}

// What goes to the root, in which order.  A custom gather: one call per lane, by every rank, one with nothing to send included.  RCCL:
// the single exchange of the frame, one group — the root receives from its peers in ascending rank, per peer lane by lane, straight
// into the staging slots; a peer sends lane by lane straight out of its render buffers; a rank without elements is left out.
static int frame_exchange(rt_multi* M, const Frame& F, hipStream_t st) {
    const bool root = M->rank == F.root;
    const size_t n_mine = (size_t)frame_elems(M, F, M->rank);
    if (M->gather) {
        for (int k = 0; k < F.nlanes; ++k) {
            const size_t b = lane_format(k, F.precision).bytes;
            const int rc = M->gather(M->user, F.local[k], n_mine * b, root ? M->lane[k].d_parts : nullptr, (size_t)F.per * b, F.root, (void*)st);
            if (rc) return rc > 0 ? RT_ECOMM : rc;
        }
        return 0;
    }
    Rccl& R = rccl();
    RT_NCCL(R.GroupStart());
    int bad = 0;
    if (root) {
        for (int r = 0; r < M->nranks && !bad; ++r) {
            const size_t n = r == F.root ? 0 : (size_t)frame_elems(M, F, r);
            for (int k = 0; k < F.nlanes && n && !bad; ++k) {
                const LaneFormat f = lane_format(k, F.precision);
                bad = R.Recv((char*)M->lane[k].d_parts + (size_t)F.per * f.bytes * (size_t)r, n * f.words, f.dtype, r, M->comm, st);
            }
        }
    } else if (n_mine) {
        for (int k = 0; k < F.nlanes && !bad; ++k) {
            const LaneFormat f = lane_format(k, F.precision);
            bad = R.Send(F.local[k], n_mine * f.words, f.dtype, F.root, M->comm, st);
        }
    }
    if (bad) { (void)R.GroupEnd(); return RT_ECOMM; }
    RT_NCCL(R.GroupEnd());
    return 0;
}

// everything after the entry point's render call: the exchange, and on the root the row-major frame (and count map) from the staging slots
static int frame_end(rt_multi* M, const Frame& F, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    RT_TRY(hipEventRecord(M->ev1, st));
    M->timed = true;
    if (M->nranks == 1) return 0;
    int rc = frame_exchange(M, F, st);
    if (rc || M->rank != F.root) return rc;
    rc = F.balanced ? rt_assemble_split(F.out[kColour], M->lane[kColour].d_parts, F.max_x, F.max_y, M->nranks, M->starts, F.per, F.precision, stream)
                    : rt_assemble(F.out[kColour], M->lane[kColour].d_parts, F.max_x, F.max_y, M->nranks, F.precision, stream);
    if (!rc && F.nlanes > kCounts && F.out[kCounts])
        rc = (int)rt::launch_gather(rt::kGatherI32x1, F.out[kCounts], M->lane[kCounts].d_parts, F.max_x, F.max_y, M->nranks, nullptr, 0, st);
    return rc;
}

int rt_multi_render(rt_multi* M, void* fb_full, int max_x, int max_y, int ns, const rt_world* world, const rt_octree* d_octree, int precision, int root, void* stream) {
    if (!M || !world || max_x <= 0 || max_y <= 0 || ns <= 0 || root < 0 || root >= M->nranks) return RT_EINVAL;
    if (M->rank == root && !fb_full) return RT_EINVAL;
    // the buffers, the RCCL datatype and rt_assemble are sized by `precision`, the render kernel by the world's: they must agree
    // (an fp32 world rendered into binary16-sized buffers would write out of bounds)
    if (precision != world->precision) return RT_EINVAL;
    Frame F = {max_x, max_y, precision, root, 1, {fb_full, nullptr}};
    int rc = frame_begin(M, F, world, d_octree, stream);
    if (!rc) rc = rt_render_on(M->ctx, F.local[kColour], max_x, max_y, ns, world, (rt_rand_state*)M->d_rand, d_octree, F.mine, stream);
    return rc ? rc : frame_end(M, F, stream);
}

// rt_multi_render with adaptive sampling, runs only: every rank runs render_init + rt_render_adaptive_part_on (or, after
// rt_multi_set_adaptive_fused(1), rt_render_adaptive_fused_on) on its runs, then the
// colour parts and the sample-count parts go to the root as the frame's two lanes.
int rt_multi_render_adaptive(rt_multi* M, void* fb_full, int max_x, int max_y, const rt_adaptive* params, const rt_world* world, const rt_octree* d_octree,
                             int precision, int root, int32_t* d_spp_full, void* stream) {
    if (!M || !world || max_x <= 0 || max_y <= 0 || root < 0 || root >= M->nranks || !adaptive_params_ok(params)) return RT_EINVAL;
    if (M->rank == root && !fb_full) return RT_EINVAL;
    if (precision != world->precision) return RT_EINVAL;
    if (world->precision == RT_PRECISION_FP16 || world->arith == RT_ARITH_CONTRACT) return RT_ENOTSUP;
    // balanced bands are cut on a uniform-cost pilot pass: they say nothing about where adaptive sampling spends its samples
    if (M->split_mode != RT_SPLIT_RUNS) return RT_ENOTSUP;
    Frame F = {max_x, max_y, precision, root, 2, {fb_full, d_spp_full}};
    int rc = frame_begin(M, F, world, d_octree, stream);
    // (the part's bits are the same either way: include/rt_amd_fused.h)
    if (!rc) rc = M->adaptive_fused ? rt_render_adaptive_fused_on(M->ctx, F.local[kColour], max_x, max_y, params, world, (rt_rand_state*)M->d_rand, d_octree, (int32_t*)F.local[kCounts], nullptr, F.mine, stream)
                                    : rt_render_adaptive_part_on(M->ctx, F.local[kColour], max_x, max_y, params, world, (rt_rand_state*)M->d_rand, d_octree, (int32_t*)F.local[kCounts], F.mine, stream);
    return rc ? rc : frame_end(M, F, stream);
}

// device time of this rank's own share of the last rt_multi_render (render_init + render, before the exchange), and of
// its render kernel alone; synchronises with the recorded events
int rt_multi_last_render_ms(rt_multi* M, float* call_ms, float* kernel_ms) {
    if (!M || !M->timed) return RT_EINVAL;
    RT_TRY(hipEventSynchronize(M->ev1));
    float ms = 0.f;
    RT_TRY(hipEventElapsedTime(&ms, M->ev0, M->ev1));
    if (call_ms) *call_ms = ms;
    if (kernel_ms) {
        float k[64]; int n = 0;
        const int rc = rt_render_ctx_times(M->ctx, k, 64, &n);
        if (rc) return rc;
        *kernel_ms = n > 0 ? k[n - 1] : 0.f;
    }
    return 0;
}

// One ncclSend + ncclRecv of `bytes` bytes from this rank to itself inside a group, on the caller's stream: checks that
// the RCCL bound at run time moves device memory in this process (what a one-GPU box can check of the RCCL path).
int rt_multi_selftest(rt_multi* M, const void* d_src, void* d_dst, size_t bytes, void* stream) {
    if (!M || !M->comm || !d_src || !d_dst) return RT_EINVAL;
    Rccl& R = rccl();
    RT_NCCL(R.GroupStart());
    const int a = R.Send(d_src, bytes, 0 /* ncclInt8 */, M->rank, M->comm, (hipStream_t)stream);
    const int b = R.Recv(d_dst, bytes, 0, M->rank, M->comm, (hipStream_t)stream);
    RT_NCCL(R.GroupEnd());
    return (a || b) ? RT_ECOMM : 0;
}

}  // extern "C"
