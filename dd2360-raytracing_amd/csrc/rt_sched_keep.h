// rt_sched_keep.h — when a render context may reuse the scheduling pass it ran before (DESIGN.md §5.4 "The kept schedule").
//
// rt_render's scheduling pass (pilot, tile order, long chains, sorted tail: five kernels) reads the world, the tree and how it is
// walked, the frame size, the partition, the sample count, the process-wide knobs of rt_tuning.h and the lane count of the device's
// persistent grid — never the framebuffer or the RNG states.  A context therefore keeps ONE record: the key of the pass whose results
// lie in its workspace (d_order, d_flags, d_long) and in its kept queue words.  This header is the whole decision: plain host C++, no
// HIP, so a stand-alone program exercises every transition on the CPU (tests/test_sched_keep_host.py).
#pragma once
#include <cstdint>
#include "rt_variant.h"

namespace rt {

// everything the scheduling pass reads that can differ between two calls of one process
struct SchedKey {
    uint64_t world = 0, tree = 0;              // handle serials (tree: the caller's octree or the world's list tree; 0 = none)
    int32_t max_x = 0, max_y = 0;
    int32_t part = 0, nparts = 0;              // rt_partition, all four fields
    int64_t tile_begin = 0, tile_end = 0;
    int32_t traversal = 0;                     // the tree's traversal mode (0 without a tree)
    int32_t ns = 0;                            // (0 in the key of a progressive sequence's tile order, as is `device`)
    int32_t half = 0;                          // 1 = a binary16 launch
    int32_t device = 0;
};
inline bool sched_key_equal(const SchedKey& a, const SchedKey& b) {
    return a.world == b.world && a.tree == b.tree && a.max_x == b.max_x && a.max_y == b.max_y && a.part == b.part && a.nparts == b.nparts &&
           a.tile_begin == b.tile_begin && a.tile_end == b.tile_end && a.traversal == b.traversal && a.ns == b.ns && a.half == b.half &&
           a.device == b.device;
}

// the number of queue words a pass leaves for the render kernel: queue[2], queue[4] (long and solo counts) and
// queue[kQueueThr .. kQueueThr + 5] (thresholds, tail mark, head count, head sum, from-end flag)
constexpr int kSchedKeptWords = 8;

enum SchedAction {
    kSchedBypass = 0,       // run the pass exactly as a context without a record would; the record is neither read nor written
    kSchedCompute = 1,      // run the pass, then keep it (sched_keep_commit once its last launch returned success)
    kSchedReuse = 2,        // launch none of the pass's kernels: the workspace and the kept queue words are those of this key
};

struct SchedKeep {
    bool valid = false;         // the workspace and the kept words hold the finished pass of `key`
    bool captured = false;      // a scheduling pass of this context has been captured into a graph: off for the rest of its life
    SchedKey key;
    uint64_t reused = 0, computed = 0;      // calls that reused the record / passes issued (captured ones count where they are captured)
    // the measured pass ("Feedback" below): the launch that computed this record also left every pixel's iteration count in the context's
    // count buffer / the record's pass has been rebuilt from those counts / how often this context did that
    bool has_counts = false, refined = false;
    uint64_t refinements = 0;
};
// whatever ends a record ends its counts: they are counts of that key's pixels
inline void sched_keep_forget(SchedKeep& K) { K.valid = false; K.has_counts = false; K.refined = false; }

// The ONE place that decides, called before the first kernel of a scheduled launch.  Every way a record is dropped or bypassed:
//  - Drop before launching: whatever is not a hit leaves `valid` false BEFORE the pass's first kernel is launched (the pass is about to
//    overwrite the workspace); only sched_keep_commit, after the last launch returned success, sets it again.  An early return between
//    the two therefore leaves no valid record.
//  - Drop on workspace changes: sched_keep_drop, called where the workspace is regrown (ctx_reserve) or freed (ctx_release).  The other
//    writers of d_order / d_flags / d_long were audited: launch_tile_order / launch_tile_order_h from schedule_frame are the only ones
//    (this function runs in front of them, both inside scheduled_round); the progressive path writes p_cost / p_order, rt_split_balanced d_cost / d_work only, the
//    adaptive, budget and refinement rounds none of the three; k_render and k_render_h only read them.
//  - Bypass inside a stream capture: the whole pass is captured as before.  Replays of that graph rewrite the workspace without the
//    host knowing, so the record is dropped and `captured` keeps the context's cache off for good.
//  - Switch: RT_SCHED_CACHE=0 (`enabled` false) runs the pass on every call, kernels and order as without this header.
//  - The progressive path (p_order / p_key / p_pinned) never comes here; it only borrows the key type: p_key is a SchedKey with ns = 0 and
//    device = 0, compared with sched_key_equal.
inline SchedAction sched_keep_decide(SchedKeep& K, const SchedKey& key, bool enabled, bool capturing) {
    if (capturing) K.captured = true;
    if (capturing || K.captured || !enabled) { sched_keep_forget(K); ++K.computed; return kSchedBypass; }
    if (K.valid && sched_key_equal(K.key, key)) { ++K.reused; return kSchedReuse; }
    sched_keep_forget(K); ++K.computed;
    return kSchedCompute;
}
// after the last launch of a kSchedCompute pass (the kept words' copy included) returned success
inline void sched_keep_commit(SchedKeep& K, const SchedKey& key) {
    if (K.captured) return;
    K.key = key; K.valid = true;
}
// the workspace was regrown or freed
inline void sched_keep_drop(SchedKeep& K) { sched_keep_forget(K); }

// ---- Feedback: the pass rebuilt once from the counts of the launch that computed it (DESIGN.md §5.4 "The measured pass") ----------
// A launch that reuses a record has, by the key, just been preceded by a launch that rendered every pixel of this very frame with this
// very sample count: k_render knows each pixel's iteration count when it ends it.  The launch that computes and keeps a pass
// (kSchedCompute) therefore also records those counts, and the FIRST hit of that record runs the pass once more, from the counts instead
// of the pilot's 18 one-sample paths per neighbourhood.  Later hits reuse the rebuilt pass like any other.  One rebuild per record.
//
// The gate — which launches take part at all: binary32, the variants that record counts (rt_variant.h: the sparse-grid kernels, the two whose launches
// end when their longest pixel does), and at least `min_ns` samples (RT_FEEDBACK_MIN_NS): below that chains do not bound
// a launch, and the hits of such launches keep the pilot's words.
inline bool sched_feedback_gate(int ns, int min_ns, int render_variant, bool half) { return !half && ns >= min_ns && variant_records_counts(render_variant); }
// the launch of a kSchedCompute pass that passed the gate was given the count buffer, and its render kernel was launched successfully
inline void sched_keep_counts(SchedKeep& K) { if (K.valid && !K.captured) K.has_counts = true; }
// after sched_keep_decide returned kSchedReuse: is the rebuild due?  (enabled: RT_SCHED_FEEDBACK; gate: sched_feedback_gate of this launch)
inline bool sched_keep_refine_due(const SchedKeep& K, bool enabled, bool gate) {
    return K.valid && K.has_counts && !K.refined && !K.captured && enabled && gate;
}
// before the rebuild's first kernel: it overwrites the workspace, so until sched_keep_refine_commit there is NO valid record — a
// rebuild whose launches did not all succeed leaves the next call a miss (which forgets the counts too)
inline void sched_keep_refine_begin(SchedKeep& K) { K.valid = false; }
// after the rebuild's last launch (the kept words' copy included) returned success; the key is the record's own
inline void sched_keep_refine_commit(SchedKeep& K) {
    if (K.captured || !K.has_counts) return;
    K.valid = true; K.refined = true; ++K.refinements;
}

}  // namespace rt
