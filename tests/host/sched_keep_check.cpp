// Stand-alone check of csrc/rt_sched_keep.h (the kept schedule's decision logic) on the CPU: tests/test_sched_keep_host.py compiles it
// with -fsanitize=address,undefined and runs it.  Exit status 0 = every check held; otherwise the failed lines are printed.
#include <cstdio>
#include <cstring>
#include <vector>
#include "rt_sched_keep.h"

using namespace rt;

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

static SchedKey base_key() {
    SchedKey k;
    k.world = 11; k.tree = 12; k.max_x = 603; k.max_y = 403; k.part = 1; k.nparts = 3; k.tile_begin = 64; k.tile_end = 640;
    k.traversal = 1; k.ns = 16; k.half = 0; k.device = 0;
    return k;
}
// what a scheduled launch does with the record: decide, (the pass's launches: `pass_ok`), commit
static SchedAction launch(SchedKeep& K, const SchedKey& key, bool enabled = true, bool capturing = false, bool pass_ok = true) {
    const SchedAction a = sched_keep_decide(K, key, enabled, capturing);
    if (a == kSchedCompute && pass_ok) sched_keep_commit(K, key);
    return a;
}

int main() {
    const SchedKey k0 = base_key();
    // keys that differ in one field at a time: each is a miss after k0, and a hit after itself
    std::vector<SchedKey> other;
    { SchedKey k = k0; k.world = 13; other.push_back(k); }
    { SchedKey k = k0; k.tree = 0; other.push_back(k); }
    { SchedKey k = k0; k.max_x = 604; other.push_back(k); }
    { SchedKey k = k0; k.max_y = 404; other.push_back(k); }
    { SchedKey k = k0; k.part = 2; other.push_back(k); }
    { SchedKey k = k0; k.nparts = 4; other.push_back(k); }
    { SchedKey k = k0; k.tile_begin = 0; other.push_back(k); }
    { SchedKey k = k0; k.tile_end = 641; other.push_back(k); }
    { SchedKey k = k0; k.traversal = 0; other.push_back(k); }
    { SchedKey k = k0; k.ns = 17; other.push_back(k); }
    { SchedKey k = k0; k.half = 1; other.push_back(k); }
    { SchedKey k = k0; k.device = 1; other.push_back(k); }
    CHECK(other.size() == 12);
    CHECK(sched_key_equal(k0, base_key()));
    for (const SchedKey& k : other) {
        CHECK(!sched_key_equal(k0, k) && !sched_key_equal(k, k0));
        SchedKeep K;
        CHECK(launch(K, k0) == kSchedCompute);
        CHECK(launch(K, k0) == kSchedReuse);
        CHECK(launch(K, k) == kSchedCompute);          // one field differs: a miss, and the record is now k's
        CHECK(launch(K, k) == kSchedReuse);
        CHECK(launch(K, k0) == kSchedCompute);         // one record per context: k0 was replaced
        CHECK(K.reused == 2 && K.computed == 3);
    }
    // the key of a progressive sequence's tile order: the same frame with ns = 0 and device = 0 — never equal to a scheduled launch's,
    // equal to itself, and exact where a hash of the partition words could collide (tile_end << 20 against part << 32)
    {
        SchedKey p0 = k0; p0.ns = 0; p0.device = 0;
        CHECK(!sched_key_equal(p0, k0) && sched_key_equal(p0, p0));
        SchedKey a = p0, b = p0;
        a.part = 1; a.tile_begin = 0; a.tile_end = 8192;           // (1 << 32) ^ (8192 << 20)
        b.part = 2; b.tile_begin = 0; b.tile_end = 4096;           // (2 << 32) ^ (4096 << 20): the same word
        CHECK(!sched_key_equal(a, b));
        for (size_t i = 0; i < other.size(); ++i) {                // every other field still tells two frames apart
            SchedKey k = other[i]; k.ns = 0; k.device = 0;
            CHECK(sched_key_equal(k, p0) == (i == 9 || i == 11));  // (9 and 11 differed in ns and device alone)
        }
    }
    // a new context: nothing kept
    { SchedKeep K; CHECK(!K.valid && !K.captured && K.reused == 0 && K.computed == 0); }
    // drop before launching: a miss leaves no valid record until the commit, so a failed pass (an early return) keeps none
    {
        SchedKeep K;
        CHECK(launch(K, k0) == kSchedCompute && K.valid);
        SchedKey k1 = k0; k1.ns = 64;
        CHECK(sched_keep_decide(K, k1, true, false) == kSchedCompute);
        CHECK(!K.valid);                               // dropped before the pass's first kernel
        CHECK(launch(K, k0) == kSchedCompute);         // ... and k0's results are gone with it: the failed pass overwrote them
        CHECK(launch(K, k1, true, false, /*pass_ok=*/false) == kSchedCompute && !K.valid);
        CHECK(launch(K, k1, true, false, false) == kSchedCompute && !K.valid);
        CHECK(launch(K, k1) == kSchedCompute && K.valid);
        CHECK(launch(K, k1) == kSchedReuse);
        CHECK(K.reused == 1 && K.computed == 6);
    }
    // drop on workspace changes (regrown or freed)
    {
        SchedKeep K;
        CHECK(launch(K, k0) == kSchedCompute && launch(K, k0) == kSchedReuse);
        sched_keep_drop(K);
        CHECK(!K.valid);
        CHECK(launch(K, k0) == kSchedCompute && launch(K, k0) == kSchedReuse);
        sched_keep_drop(K); sched_keep_drop(K);        // (dropping nothing is harmless)
        CHECK(launch(K, k0) == kSchedCompute);
        CHECK(K.reused == 2 && K.computed == 3);
    }
    // bypass inside a capture: the record is neither read nor written, and the context never reuses again
    {
        SchedKeep K;
        CHECK(launch(K, k0) == kSchedCompute && launch(K, k0) == kSchedReuse);
        CHECK(launch(K, k0, true, /*capturing=*/true) == kSchedBypass);
        CHECK(K.captured && !K.valid);
        for (int i = 0; i < 3; ++i) { CHECK(launch(K, k0) == kSchedBypass); CHECK(!K.valid); }
        sched_keep_commit(K, k0);                      // (a commit on such a context keeps nothing)
        CHECK(!K.valid && launch(K, k0) == kSchedBypass);
        CHECK(K.reused == 1 && K.computed == 6);
        SchedKeep F;                                   // captured first, before any record
        CHECK(launch(F, k0, true, true) == kSchedBypass && launch(F, k0) == kSchedBypass && F.reused == 0 && F.computed == 2);
    }
    // the switch: off = every call runs the pass, nothing is kept; a record from before is dropped, not resurrected
    {
        SchedKeep K;
        for (int i = 0; i < 3; ++i) CHECK(launch(K, k0, /*enabled=*/false) == kSchedBypass && !K.valid);
        CHECK(K.reused == 0 && K.computed == 3);
        CHECK(launch(K, k0) == kSchedCompute && launch(K, k0) == kSchedReuse);
        CHECK(launch(K, k0, false) == kSchedBypass && !K.valid);
        CHECK(launch(K, k0) == kSchedCompute);
    }
    if (g_failed) { std::printf("%d checks failed\n", g_failed); return 1; }
    std::printf("sched_keep_host: ok\n");
    return 0;
}
