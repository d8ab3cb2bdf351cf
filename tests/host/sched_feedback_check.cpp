// Stand-alone check of the measured pass's decision (csrc/rt_sched_keep.h "Feedback") on the CPU: tests/test_sched_feedback_host.py
// compiles it with -fsanitize=address,undefined and runs it.  Exit status 0 = every check held; otherwise the failed lines are printed.
#include <cstdio>
#include "rt_sched_keep.h"

using namespace rt;

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

static SchedKey base_key() {
    SchedKey k;
    k.world = 11; k.tree = 12; k.max_x = 400; k.max_y = 232; k.part = 0; k.nparts = 1; k.traversal = 1; k.ns = 32; k.half = 0; k.device = 0;
    return k;
}
// what rt_render does with the record (rt_api.hip scheduled_round / schedule_frame / render_common): returns 'M' a miss that ran the
// pilot's pass, 'H' a hit that launched nothing, 'R' a hit that rebuilt the pass, 'B' a bypass.  record: the launch is an rt_render
// (k_render MODE 0); pass_ok / render_ok: every launch of the pass (or of the rebuild) / the render kernel's launch succeeded.
static char launch(SchedKeep& K, const SchedKey& key, bool feedback = true, bool gate = true, bool record = true, bool cache = true, bool capturing = false,
                   bool pass_ok = true, bool render_ok = true) {
    const SchedAction a = sched_keep_decide(K, key, cache, capturing);
    const bool take_part = a != kSchedBypass && feedback && gate;
    bool refine = false, recording = false;
    if (a == kSchedReuse && sched_keep_refine_due(K, feedback, take_part)) { refine = true; sched_keep_refine_begin(K); }
    if (a == kSchedCompute && record && take_part) recording = true;
    if (refine) { if (!pass_ok) return 'R'; sched_keep_refine_commit(K); }
    else if (a == kSchedCompute) { if (!pass_ok) return 'M'; sched_keep_commit(K, key); }
    if (render_ok && recording) sched_keep_counts(K);
    return refine ? 'R' : a == kSchedReuse ? 'H' : a == kSchedCompute ? 'M' : 'B';
}

int main() {
    const SchedKey k0 = base_key();
    SchedKey k1 = k0; k1.ns = 33;
    // the gate: binary32, the two sparse-grid kernels, enough samples
    CHECK(sched_feedback_gate(32, 32, 4, false) && sched_feedback_gate(64, 32, 5, false));
    CHECK(!sched_feedback_gate(31, 32, 4, false) && !sched_feedback_gate(16, 32, 5, false));
    CHECK(!sched_feedback_gate(64, 32, 2, false) && !sched_feedback_gate(64, 32, 1, false) && !sched_feedback_gate(64, 32, 0, false));
    CHECK(!sched_feedback_gate(64, 32, 4, true));
    {   // miss + record, hit + rebuild, then plain hits: one rebuild per record
        SchedKeep K;
        CHECK(launch(K, k0) == 'M' && K.valid && K.has_counts && !K.refined && K.refinements == 0);
        CHECK(launch(K, k0) == 'R' && K.valid && K.has_counts && K.refined && K.refinements == 1);
        CHECK(launch(K, k0) == 'H' && launch(K, k0) == 'H' && K.refinements == 1);
        CHECK(K.reused == 3 && K.computed == 1);                  // a rebuilding launch is a hit
        // another key: a miss that forgets the counts and the rebuilt pass, records its own, rebuilds once
        CHECK(launch(K, k1) == 'M' && K.valid && K.has_counts && !K.refined);
        CHECK(launch(K, k1) == 'R' && K.refinements == 2);
        CHECK(launch(K, k0) == 'M' && !K.refined && K.refinements == 2);
        CHECK(K.reused == 4 && K.computed == 3);
    }
    {   // the switch: nothing recorded, nothing rebuilt
        SchedKeep K;
        CHECK(launch(K, k0, false) == 'M' && K.valid && !K.has_counts);
        CHECK(launch(K, k0, false) == 'H' && launch(K, k0, false) == 'H' && K.refinements == 0 && !K.refined);
    }
    {   // outside the gate: the same
        SchedKeep K;
        CHECK(launch(K, k0, true, false) == 'M' && !K.has_counts);
        CHECK(launch(K, k0, true, false) == 'H' && K.refinements == 0);
    }
    {   // a record computed by a launch that stores no counts (round 0 of rt_render_adaptive*) is never rebuilt; one that an rt_render
        // computed is rebuilt by whichever scheduled launch hits it first
        SchedKeep K;
        CHECK(launch(K, k0, true, true, false) == 'M' && K.valid && !K.has_counts);
        CHECK(launch(K, k0) == 'H' && launch(K, k0, true, true, false) == 'H' && K.refinements == 0);
        SchedKeep L;
        CHECK(launch(L, k0) == 'M' && launch(L, k0, true, true, false) == 'R' && L.refinements == 1 && launch(L, k0) == 'H');
    }
    {   // the render kernel of the recording launch was not launched: a valid pass without counts
        SchedKeep K;
        CHECK(launch(K, k0, true, true, true, true, false, true, false) == 'M' && K.valid && !K.has_counts);
        CHECK(launch(K, k0) == 'H' && K.refinements == 0);
    }
    {   // a failed pass leaves no record, hence no counts
        SchedKeep K;
        CHECK(launch(K, k0, true, true, true, true, false, false) == 'M' && !K.valid && !K.has_counts);
        CHECK(launch(K, k0) == 'M' && K.valid && K.has_counts);
    }
    {   // a failed rebuild leaves NO valid record: the next call is a miss, which forgets the counts and records anew
        SchedKeep K;
        CHECK(launch(K, k0) == 'M');
        CHECK(launch(K, k0, true, true, true, true, false, false) == 'R' && !K.valid && !K.refined && K.refinements == 0);
        CHECK(!sched_keep_refine_due(K, true, true));
        CHECK(launch(K, k0) == 'M' && K.valid && K.has_counts && !K.refined && K.computed == 2);
        CHECK(launch(K, k0) == 'R' && K.refinements == 1);
    }
    {   // counts die with the record: a regrown or released workspace
        SchedKeep K;
        CHECK(launch(K, k0) == 'M' && K.has_counts);
        sched_keep_drop(K);
        CHECK(!K.valid && !K.has_counts && !K.refined && !sched_keep_refine_due(K, true, true));
        CHECK(launch(K, k0) == 'M' && launch(K, k0) == 'R');
        sched_keep_drop(K);
        CHECK(!K.valid && !K.has_counts && !K.refined);
        CHECK(launch(K, k0) == 'M' && K.has_counts && K.refinements == 1);
    }
    {   // a capture: bypassed, the record and its counts dropped, and never a rebuild on this context again
        SchedKeep K;
        CHECK(launch(K, k0) == 'M' && launch(K, k0) == 'R');
        CHECK(launch(K, k0, true, true, true, true, true) == 'B' && !K.valid && !K.has_counts && !K.refined && K.captured);
        CHECK(launch(K, k0) == 'B' && launch(K, k0) == 'B' && !K.has_counts && K.refinements == 1);
        sched_keep_counts(K); sched_keep_refine_commit(K);
        CHECK(!K.valid && !K.has_counts && !K.refined && K.refinements == 1);
        SchedKeep L;                                             // captured between the recording launch and the first hit
        CHECK(launch(L, k0) == 'M' && L.has_counts);
        CHECK(launch(L, k0, true, true, true, true, true) == 'B' && launch(L, k0) == 'B' && L.refinements == 0);
    }
    {   // RT_SCHED_CACHE=0: every launch a bypass, nothing recorded
        SchedKeep K;
        CHECK(launch(K, k0, true, true, true, false) == 'B' && launch(K, k0, true, true, true, false) == 'B' && !K.has_counts && K.refinements == 0);
    }
    {   // due only for a valid, counted, not yet rebuilt, uncaptured record with the switch on and the gate passed
        SchedKeep K;
        CHECK(!sched_keep_refine_due(K, true, true));
        K.valid = true; CHECK(!sched_keep_refine_due(K, true, true));
        K.has_counts = true; CHECK(sched_keep_refine_due(K, true, true));
        CHECK(!sched_keep_refine_due(K, false, true) && !sched_keep_refine_due(K, true, false));
        K.captured = true; CHECK(!sched_keep_refine_due(K, true, true)); K.captured = false;
        K.refined = true; CHECK(!sched_keep_refine_due(K, true, true));
        // a commit without counts (the record was dropped in between) validates nothing
        SchedKeep L; sched_keep_refine_commit(L); CHECK(!L.valid && !L.refined && L.refinements == 0);
    }
    if (g_failed) { std::printf("sched_feedback_host: %d checks FAILED\n", g_failed); return 1; }
    std::printf("sched_feedback_host: ok\n");
    return 0;
}
