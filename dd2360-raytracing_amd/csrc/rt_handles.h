// rt_handles.h — the opaque handles of include/rt_amd.h as the library's translation units see them (rt_api.hip, rt_build.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cassert>
#include <vector>
#include "rt_device.h"
#include "../host/rt_scene.hpp"
#include "rt_accel.h"
#include "rt_sched_keep.h"

using rt::DevScene; using rt::DevTree; using rt::DevNode; using rt::DevAccel; using rt::AccelHost; using rt::Octree;

// Handles keep their host staging copy; device buffers are created by rt_world_upload / rt_octree_upload
// (called implicitly by the first render/trace that uses the handle).  A handle passed as `const` to a compute call stays
// logically constant: what such a call may create lazily (device copies, the list grid, the default render context) lives
// behind a pointer in a `Lazy` block of its own.
struct rt_octree;

// A group of device buffers that are allocated and freed together.  A handle describes each of its groups ONCE, as a function that
// returns a DevGroup: where every pointer is kept, its bytes at the asked capacity and, for a copy of a host array, that array.
// Whatever grows, uploads or frees device buffers goes through the three functions below.
struct DevBuf { void** at; size_t bytes; const void* src; size_t src_bytes; };      // bytes == 0: freed with the group, allocated elsewhere
struct DevGroup {
    int n = 0; DevBuf b[17];          // (17: the largest group, a tree's)
    DevGroup& add(void* at, size_t bytes) { assert(n < 17); b[n++] = DevBuf{(void**)at, bytes, nullptr, 0}; return *this; }      // at: the address of the (typed) pointer
    // a copy of a host vector; an empty one still gets a buffer (of one element), so no kernel argument is ever null
    template <class V> DevGroup& add_copy(void* at, const V& v) {
        const size_t sz = sizeof(typename V::value_type);
        assert(n < 17);
        b[n++] = DevBuf{(void**)at, (v.empty() ? 1 : v.size()) * sz, v.empty() ? nullptr : v.data(), v.size() * sz};
        return *this;
    }
};
// frees every buffer of the group and nulls its pointer; the first hipFree error is the one returned, the others are still freed
inline int group_free(const DevGroup& g) {
    int rc = 0;
    for (int k = 0; k < g.n; ++k) {
        void*& p = *g.b[k].at;
        if (p) { const hipError_t e = hipFree(p); if (e != hipSuccess && !rc) rc = (int)e; p = nullptr; }
    }
    return rc;
}
// free all, then allocate (and fill) all or none, in the group's order.  The old buffers go first: hipFree waits for the device, so
// launches still queued on them finish.  On any error the group is left empty and the first error is returned.
inline int group_regrow(const DevGroup& g) {
    int rc = group_free(g);
    for (int k = 0; k < g.n && !rc; ++k) {
        const DevBuf& b = g.b[k];
        if (!b.bytes) continue;
        rc = (int)hipMalloc(b.at, b.bytes);
        if (!rc && b.src) rc = (int)hipMemcpy(*b.at, b.src, b.src_bytes, hipMemcpyHostToDevice);
        if (rc) (void)group_free(g);
    }
    return rc;
}
// a group kept at a capacity `have` (g: the group at `need`): regrown when that is too small; 0 while it is empty
inline int group_reserve(int64_t& have, int64_t need, const DevGroup& g) {
    if (have >= need) return 0;
    have = 0;
    const int rc = group_regrow(g);
    if (!rc) have = need;
    return rc;
}

// Per-launch state of rt_render: work counters, scheduling workspace, timing events.  One context serves one launch at a
// time: calls on the same context are ordered by the library (an event recorded behind the render kernel, which the next
// call's stream waits for before it touches the workspace), so two streams sharing a context serialise instead of racing;
// give concurrent frames a context each (rt_render_ctx_create).
struct rt_render_ctx {
    // work counters of the persistent render kernel: a ring of slots (one per launch, 256 B apart), zeroed on the stream
    unsigned int* d_queue = nullptr; unsigned launches = 0;
    // scheduling workspace (tile costs, hand-out order, long-chain flags and list), grown on demand
    int* d_cost = nullptr; unsigned int* d_order = nullptr; unsigned char* d_flags = nullptr; unsigned int* d_long = nullptr; int* d_work = nullptr; int64_t sched_tiles = 0;
    unsigned int* last_queue = nullptr;      // the counters of the latest launch (rt_render_ctx_counters)
    // the kept schedule (rt_sched_keep.h): the key of the scheduling pass whose results lie in d_order / d_flags / d_long, and the words
    // that pass left in its launch's slot (kSchedKeptWords of them, behind the ring in d_queue's allocation) — a launch with an equal
    // key runs no scheduling kernel.  One record per context, shared by rt_render and round 0 of rt_render_adaptive*.
    rt::SchedKeep keep; unsigned int* d_kept = nullptr;
    // the measured pass (rt_sched_keep.h "Feedback"): the iteration count of every buffer element of the launch that computed the record
    // (part of the scheduling workspace: regrown and freed with d_flags), how many elements that launch had, and — behind the kept
    // words — the two words its rebuild leaves (the largest count, the solo cap)
    unsigned short* d_iters = nullptr; int64_t iters_n = 0;
    // tile order of a progressive sequence (rt_render_progressive): the pilot pass that the call with current_sample == 1 runs, kept
    // in buffers of its own and reused by the following passes of the same frame (p_key: the frame's SchedKey with ns = 0 and device = 0)
    int* p_cost = nullptr; unsigned int* p_order = nullptr; int64_t p_tiles = 0; bool p_valid = false; rt::SchedKey p_key;
    bool p_pinned = false;      // a captured progressive pass has baked p_order's address into a hipGraph: the buffers are never freed or moved again
    // rt_render_adaptive: per pixel the luminance sum and sum of squares between rounds, the two lists of active pixels (ping-pong),
    // and one active-pixel count per round; grown on demand
    float* a_sl = nullptr; float* a_q = nullptr; unsigned int* a_list = nullptr; int64_t a_pixels = 0; unsigned int* a_count = nullptr; int64_t a_rounds = 0;
    // rt_adaptive_budget_select / rt_render_adaptive_spend: the selection's histograms, threshold and per-block tie counts (the key bits
    // live in the second half of a_list, which is free outside a render round); grown on demand
    unsigned int* b_ws = nullptr; int64_t b_bytes = 0;
    // HIP events around the dominant kernel of each render call (ring of the last 64), see rt_render_ctx_times
    hipEvent_t ev0[64] = {}, ev1[64] = {}; unsigned ev_head = 0, ev_count = 0; bool ev_ready = false;
    // ordering of successive launches that share this context
    hipEvent_t done = nullptr; hipStream_t last_stream = nullptr; bool has_done = false;
};
static const unsigned kQueueSlots = 64, kQueueStride = 64;     // 256 bytes per launch: counters in the first 128-byte line, read-only thresholds in the second (rt_device.h)

uint64_t rt_next_serial();                  // handles are numbered: a new handle at a recycled address is not mistaken for the old one

struct rt_world {
    uint64_t serial = rt_next_serial();
    int precision = RT_PRECISION_FP32;
    int n = 0;
    std::vector<float4> h_hot, h_geom, h_mat;
    std::vector<int32_t> h_ids, h_kind;
    int list_traversal = RT_TRAVERSAL_FAST;
    int arith = RT_ARITH_IEEE;                 // rt_world_set_arith
    struct Lazy {
        bool uploaded = false;
        DevScene dev{};
        void* d_list_hot = nullptr; void* d_list_id = nullptr; void* d_geom = nullptr; void* d_mat = nullptr; void* d_kind = nullptr;
        void* d_shade = nullptr; void* d_kind8 = nullptr;        // geom and mat interleaved, kind as bytes (DevScene::shade / kind8)
        // hitable_list::hit through the candidate grid: the list as a one-node "tree" (fp32 only; null = plain scan)
        rt_octree* list_tree = nullptr; bool list_tree_tried = false;
        rt_render_ctx ctx;                      // the context rt_render / rt_render_progressive use
        // rt_world_set_geometry has rewritten the device arrays: h_geom / h_hot are behind, and whatever reads them downloads first
        // (world_host_geometry, rt_api.hip)
        bool host_stale = false;
    };
    Lazy* z = nullptr;
};

struct rt_octree {
    uint64_t serial = rt_next_serial();
    int precision = RT_PRECISION_FP32;
    Octree* host = nullptr;
    std::vector<DevNode> h_nodes; std::vector<float4> h_ent_hot; std::vector<int32_t> h_ent_id;
    AccelHost accel;
    int traversal = RT_TRAVERSAL_FAST;
    int build_path = RT_BUILD_HOST;            // rt_octree_build_path: set where rt_build_octree_gpu decides (the list grid's tree is a host build)
    struct Lazy {
        bool uploaded = false;
        DevTree dev{};
        void* d_nodes = nullptr; void* d_ent_hot = nullptr; void* d_ent_id = nullptr;
        void* d_acc[12] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // large_hot, large_brick, cs, hot, brick, memb_start, memb_cell, -, cellnode, bits_index, cellbits, fp16 planes
        // a tree built on the device (rt_build.hip): ONE allocation holds everything above (the pointers point into it), plus
        // the reference-layout arrays that the inspection calls download on demand
        void* d_arena = nullptr;
        const rt_octnode* d_ref_nodes = nullptr; const int32_t* d_leaf_count = nullptr; const int32_t* d_leaf_indices = nullptr;
        int ref_node_count = 0, ref_leaf_count = 0, ref_dropped_full = 0, ref_dropped_outside = 0, ref_spl = 0;
        Octree* host_view = nullptr;            // ... downloaded here when an inspection call first asks for it
        // what the device build keeps for rt_octree_rebuild_gpu (rt_build.hip "memory kept in the handle"): its workspace, the bytes of
        // the workspace and of the two allocations above (d_arena, d_acc[7]), and the lengths the count-dependent arrays of d_arena are
        // laid out for — (cell, sphere) pairs (bucket entries are bounded by them) and leaf buckets.  len_pairs == 0: the arena holds a
        // fresh build's exact sizes; the first rebuild lays it out anew with a quarter of slack.
        void* d_ws = nullptr;
        size_t ws_bytes = 0, a_bytes = 0, b_bytes = 0;
        size_t len_pairs = 0, len_leaf = 0;
        unsigned last_pairs = 0;                // the pairs the last device build counted
        uint64_t rebuilds = 0, regrown = 0, syncs_last = 0;      // rt_octree_rebuild_info
    };
    Lazy* z = nullptr;
    int n_nodes = 0, n_entries = 0;
    int n_world = 0, bit_rows = 1;          // world list size, rows of the membership bitmaps (>= 1)
    int spl = 0;                            // SPHERES_PER_LEAF the tree was built with (rt_octree_rebuild_gpu builds with it again)
};


// rt_adaptive's parameter rule (rt_api.hip), shared with rt_multi_render_adaptive, which refuses before any rank renders or exchanges
bool adaptive_params_ok(const rt_adaptive* P);
