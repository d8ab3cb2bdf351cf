// rt_kernels.hip — hand-written HIP kernels of the render path for gfx950 (MI355X, CDNA4).
//
// Replaces the reference's device code: render_init / render / render_progressive (main.cu:84-142), color()
// (main.cu:43-75), hitTree / traverseTree / intersect_ray_aabb / processHit (acceleration_structure.h:226-342),
// hitable_list::hit (hitable_list.h:16-31), sphere::hit (sphere.h:17-46), the three material::scatter
// (material.h:55-113) and camera::get_ray (camera.h:45-49).
//
// Shape:
//   * one lane = one pixel (the per-pixel XORWOW stream is strictly serial); persistent waves pull pixels from a global
//     queue (one pixel position of 64 different tiles per wave: long chains cluster), most expensive tiles first;
//   * the reference's `for sample { for bounce {..} }` nest is flattened into ONE loop per lane: a lane whose path
//     ended starts its next sample at once instead of idling until the slowest path of the wave finishes;
//   * octree on: candidates come from an exact culling grid (rt_accel.h), the reference's traversal is the fallback; a wave's
//     sphere tests are pooled and dealt out evenly over its 64 lanes — walk_pool on sparse grids (two columns per ray and round),
//     walk_pool_dense on dense ones (one column, four entries per lane and pass, the owner's best hit re-read every pass); the
//     steps the two share (a column's entry range, the owner's ray record, a round's preamble and pick-up, the pre-filter's margin)
//     and the pieces of sphere::hit that several places need (sphere_bc, sphere_offer_t, hit_eligible) are functions of their own;
//     waves holding long pixel chains stop refilling ("thin");
//   * no virtual calls, no device heap, no recursion: materials are a tag + 4 floats, the octree is a pre-order
//     node array with skip links staged in LDS, bucket contents are pre-gathered (centre, r^2) float4 streams;
//   * hitable_list path: the sphere index is wave-uniform, so sphere data comes through scalar loads (SGPR operands).
//
// Numeric contract: every floating-point operation below is one IEEE binary32 operation in the reference's
// order; FMA contraction is off for the whole file (and on the command line); division and sqrt are the
// correctly-rounded forms (hipcc default).  Values that are merely hoisted (a = d.d, radius^2) are bitwise the
// values the reference recomputes.  Two affine maps of the sampling code are explicit fused multiply-adds whose product is exact,
// so their single rounding gives the two-step form's bits (rt_sampling.h: checked for all 2^32 draws).
#include <hip/hip_runtime.h>
#include <float.h>
#include <cstdio>
#include <type_traits>
#include "rt_device.h"
#include "rt_launch.h"
#include "rt_tuning.h"
#include "rt_sampling.h"
#include "rt_adapt_rule.h"

// This file is compiled three times (Makefile).  All three see the device code — what traces a ray, k_render and the other kernel
// templates, of which a unit emits only what its launchers instantiate; the launchers at the end of the file are dealt out:
//   the main unit (rt_kernels.o, RT_TU_MAIN, no SLP vectorisation): everything on trees and every launcher that other files call;
//   RT_TU_LIST (rt_kernels_list.hip, with SLP vectorisation): the hitable_list launchers launch_*_list and nothing else;
//   RT_TU_CONTRACT (rt_kernels_contract.hip): FMA contraction ALLOWED — what nvcc's default -fmad=true does to the reference
//     (Makefile:9) — in namespace rt::fmac, for rt_world_set_arith(RT_ARITH_CONTRACT), never the parity mode: launch_render and
//     the k_render<*, 0|1, *> behind it, list variants included.  The pilot, the ordering pass and everything else stay IEEE.
// A unit exports ONE render launcher, launch_render(A, tree, mode), and — where it holds list kernels — ONE list launcher,
// launch_render_list(A, mode), for the modes with_mode gives it: 0 to 4 in the main and the list unit, 0 and 1 in the contract unit.
// Without RT_SPLIT_LIST (the diagnostic one-unit builds: librt_amd_stats*.so, librt_amd_wpass.so) the main unit holds the list launchers too.
// The kernels that trace no ray live in rt_schedule.hip, rt_adaptive.hip and rt_assemble.hip.
#if defined(RT_TU_CONTRACT)
#pragma clang fp contract(fast)
#define RT_TU_NAMESPACE rt::fmac
#define RT_TU_HAS_LIST 1
#elif defined(RT_TU_LIST)
#pragma clang fp contract(off)
#define RT_TU_NAMESPACE rt
#define RT_TU_HAS_LIST 1
#else
#pragma clang fp contract(off)
#define RT_TU_NAMESPACE rt
#define RT_TU_MAIN 1
#ifndef RT_SPLIT_LIST
#define RT_TU_HAS_LIST 1
#endif
#endif

namespace RT_TU_NAMESPACE {

#define RT_DEV static __device__ __forceinline__

#include "rt_stats.h"      // the diagnostic build's counters (-DRT_STATS): STAT / WPASS / RT_STATS_ONLY — nothing in a product build

// curand (XORWOW) + curand_uniform: x * 2^-32 + 2^-33 — the product is exact, so one fused rounding gives the reference's bits (rt_sampling.h)
RT_DEV float rng_uniform(Rng& s) {
    const uint32_t t = s.v0 ^ (s.v0 >> 2);
    s.v0 = s.v1; s.v1 = s.v2; s.v2 = s.v3; s.v3 = s.v4;
    s.v4 = (s.v4 ^ (s.v4 << 4)) ^ (t ^ (t << 1));
    s.d += 362437u;
    return uniform_from_bits(s.d + s.v4);
}

RT_DEV void rng_seed(Rng& s, unsigned long long seed) {       // curand_init(seed, 0, 0)
    const uint32_t lo = (uint32_t)seed ^ 0xaad26b49u, hi = (uint32_t)(seed >> 32) ^ 0xf7dcefddu;
    const uint32_t t0 = 1099087573u * lo, t1 = 2591861531u * hi;
    s.d = 6615241u + t1 + t0;
    s.v0 = 123456789u + t0; s.v1 = 362436069u ^ t0; s.v2 = 521288629u + t1; s.v3 = 88675123u ^ t1; s.v4 = 5783321u + t0;
}

struct V3 { float x, y, z; };
RT_DEV float dot3(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }     // vec3.h:91, left to right

struct RayF { V3 o, d; };

// pow((1 - cosine), 5) of material.h:14 — contract: binary64 ((x*x)*(x*x))*x rounded once to binary32
RT_DEV float pow5(float x) { const double v = (double)x; const double v2 = v * v; return (float)((v2 * v2) * v); }

// ---------------------------------------------------------------------------------------------------- sphere::hit
// sphere.h:18-21 for a sphere as (centre, r^2): b = oc.d and c = oc.oc - r^2
RT_DEV float2 sphere_bc(const RayF& r, const float4 s) {
    const float ocx = r.o.x - s.x, ocy = r.o.y - s.y, ocz = r.o.z - s.z;
    return make_float2(ocx * r.d.x + ocy * r.d.y + ocz * r.d.z, (ocx * ocx + ocy * ocy + ocz * ocz) - s.w);
}
// One candidate test against (cx,cy,cz,r2).  closest is closest_so_far; on acceptance it is lowered and `best`
// records which entry won.  Operation order of sphere.h:18-41 with a = d.d hoisted by the caller.
RT_DEV void sphere_test(const RayF& r, float a, float cx, float cy, float cz, float r2, int id, float& closest, int& best) {
    const float2 bc = sphere_bc(r, make_float4(cx, cy, cz, r2));
    const float b = bc.x, disc = b * b - a * bc.y;
    if (disc > 0.0f) {
        const float sq = sqrtf(disc);
        float t = (-b - sq) / a;
        if (t < closest && t > 0.001f) { closest = t; best = id; }
        else {
            t = (-b + sq) / a;
            if (t < closest && t > 0.001f) { closest = t; best = id; }
        }
    }
}

// intersect_ray_aabb — acceleration_structure.h:226-244 (comparisons kept literally: NaN/inf fall through as there)
RT_DEV bool ray_box(const RayF& r, float lox, float loy, float loz, float hix, float hiy, float hiz) {
    float tmin = (lox - r.o.x) / r.d.x;
    float tmax = (hix - r.o.x) / r.d.x;
    if (tmin > tmax) { const float t = tmin; tmin = tmax; tmax = t; }
    float tymin = (loy - r.o.y) / r.d.y;
    float tymax = (hiy - r.o.y) / r.d.y;
    if (tymin > tymax) { const float t = tymin; tymin = tymax; tymax = t; }
    if ((tmin > tymax) || (tymin > tmax)) return false;
    if (tymin > tmin) tmin = tymin;
    if (tymax < tmax) tmax = tymax;
    float tzmin = (loz - r.o.z) / r.d.z;
    float tzmax = (hiz - r.o.z) / r.d.z;
    if (tzmin > tzmax) { const float t = tzmin; tzmin = tzmax; tzmax = t; }
    if ((tmin > tzmax) || (tzmin > tmax)) return false;
    return true;
}

// ---------------------------------------------------------------------------------------------------- closest hit
// Every kernel that traces rays takes a RenderArgs as its FIRST argument.  The launch arguments again, read from the kernarg segment at the point of use.  Fields taken from the by-value argument
// live in SGPRs for the whole kernel; the render loop is short of SGPRs (spills cost VALU slots: v_readlane/v_writelane),
// so everything that is only needed between pixels or once per bounce (camera, queue, order, framebuffer, materials) is
// re-read through this pointer (scalar loads, no VALU) — the empty asm keeps the compiler from hoisting those loads.
RT_DEV const RenderArgs* cold_args() {
    auto p = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return (const RenderArgs*)p;
}

RT_DEV float bcast(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
// Minimum over each group of LG = 64, 32 or 16 consecutive lanes, in every lane of the group.  DPP row shifts and row
// broadcasts (~10 cycles a step) instead of dependent ds_bpermute round trips (~100 cycles each): the cooperative paths run in
// waves with nothing else to do while a reduction is in flight.
template <int LG>
RT_DEV float group_min(float v) {
    const int inf = 0x7f800000;
    int x = __float_as_int(v);
#define RT_DPP_MIN(ctrl, rmask) x = __float_as_int(fminf(__int_as_float(x), __int_as_float(__builtin_amdgcn_update_dpp(inf, x, ctrl, rmask, 0xf, false))))
    RT_DPP_MIN(0x111, 0xf);     // row_shr:1
    RT_DPP_MIN(0x112, 0xf);     // row_shr:2
    RT_DPP_MIN(0x114, 0xf);     // row_shr:4
    RT_DPP_MIN(0x118, 0xf);     // row_shr:8   -> lane 15 of each row of 16 holds the row's minimum
    if (LG >= 32) RT_DPP_MIN(0x142, 0xa);     // row_bcast:15 into rows 1 and 3 -> lanes 31 and 63 hold their half's minimum
    if (LG >= 64) RT_DPP_MIN(0x143, 0xc);     // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave's minimum
#undef RT_DPP_MIN
    const int q3 = __builtin_amdgcn_readlane(x, 63);
    if (LG == 64) return __int_as_float(q3);
    const int q1 = __builtin_amdgcn_readlane(x, 31);
    if (LG == 32) return __int_as_float((threadIdx.x & 32) ? q3 : q1);
    const int q0 = __builtin_amdgcn_readlane(x, 15), q2 = __builtin_amdgcn_readlane(x, 47);
    const int g = (threadIdx.x >> 4) & 3;
    return __int_as_float(g == 0 ? q0 : g == 1 ? q1 : g == 2 ? q2 : q3);
}
RT_DEV int wave_min_int(int x) {                              // the same for int32, whole wave
    const int big = 0x7fffffff;
#define RT_DPP_MIN(ctrl, rmask) x = min(x, __builtin_amdgcn_update_dpp(big, x, ctrl, rmask, 0xf, false))
    RT_DPP_MIN(0x111, 0xf); RT_DPP_MIN(0x112, 0xf); RT_DPP_MIN(0x114, 0xf); RT_DPP_MIN(0x118, 0xf); RT_DPP_MIN(0x142, 0xa); RT_DPP_MIN(0x143, 0xc);
#undef RT_DPP_MIN
    return __builtin_amdgcn_readlane(x, 63);
}
RT_DEV int bcast(int v, int l) { return __builtin_amdgcn_readlane(v, l); }

// sphere::hit reduced to "which t would this sphere offer": the near root if it is > t_min, else the far root if that
// is > t_min, else none (+inf).  The reference accepts exactly when that value is < closest_so_far (the far root is
// never below the near root, so a rejected near root in range cannot be followed by an accepted far root).
// sphere_offer_t forms the roots (sphere.h:24-43; sq = sqrtf(disc), disc > 0) for whoever holds b and disc already: the queued
// candidates of the pooled walks, the large spheres; sphere_candidate is the whole test.
RT_DEV float sphere_offer_t(float a, float b, float sq) {
    float cand = __builtin_inff();
    const float t1 = (-b - sq) / a;
    if (t1 > 0.001f) cand = t1;
    else { const float t2 = (-b + sq) / a; if (t2 > 0.001f) cand = t2; }
    return cand;
}
RT_DEV float sphere_candidate(const RayF& r, float a, const float4 s) {
    const float2 bc = sphere_bc(r, s);
    const float b = bc.x, disc = b * b - a * bc.y;
    return disc > 0.0f ? sphere_offer_t(a, b, sqrtf(disc)) : __builtin_inff();
}

// hitable_list::hit over the hittable spheres in list order.
// Full waves: the sphere index `k` is wave-uniform -> scalar loads, every lane tests its own ray against sphere k.
// Thin waves (few live rays, e.g. the tail of a frame): one ray at a time with the 64 lanes testing 64 spheres per step;
// the winner is the smallest offered t, the lowest list index among equal t — exactly what the sequential scan keeps.
RT_DEV void closest_list(const DevScene& S, const RayF& r, float a, bool live, float& closest, int& best) {
    const float4* __restrict__ hot = S.list_hot;
    const int n = S.n_list;
    unsigned long long todo = __ballot(live);
    if ((int)__popcll(todo) * RT_LIST_COOP_COST <= n) {
        const int lane = threadIdx.x & 63;
        while (todo != 0ull) {
            const int L = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            RayF q;
            q.o.x = bcast(r.o.x, L); q.o.y = bcast(r.o.y, L); q.o.z = bcast(r.o.z, L);
            q.d.x = bcast(r.d.x, L); q.d.y = bcast(r.d.y, L); q.d.z = bcast(r.d.z, L);
            const float qa = bcast(a, L);
            float my_t = FLT_MAX; int my_k = 0x7fffffff;
            for (int base = 0; base < n; base += 256) {          // four spheres per lane and pass, their loads in flight together
                float4 sv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int k = base + u * 64 + lane; sv[u] = hot[k < n ? k : n - 1]; }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = base + u * 64 + lane;
                    if (k < n) {
                        const float cand = sphere_candidate(q, qa, sv[u]);
                        if (cand < my_t) { my_t = cand; my_k = k; }
                    }
                }
            }
            const float mn = group_min<64>(my_t);
            const int km = wave_min_int((my_t == mn && my_k != 0x7fffffff) ? my_k : 0x7fffffff);
            if (lane == L && km != 0x7fffffff) { closest = mn; best = S.list_id[km]; }
        }
        return;
    }
    int k = 0;
    for (; k + RT_LIST_BATCH <= n; k += RT_LIST_BATCH) {         // several spheres per pass: their (scalar) loads in flight together
        float4 sv[RT_LIST_BATCH];
#pragma unroll
        for (int q = 0; q < RT_LIST_BATCH; ++q) sv[q] = hot[k + q];
#pragma unroll
        for (int q = 0; q < RT_LIST_BATCH; ++q) sphere_test(r, a, sv[q].x, sv[q].y, sv[q].z, sv[q].w, k + q, closest, best);
    }
    for (; k < n; ++k) {
        const float4 s = hot[k];
        sphere_test(r, a, s.x, s.y, s.z, s.w, k, closest, best);
    }
    if (best >= 0) best = S.list_id[best];
}

// The reference scan: the tree in the reference's depth-first order (pre-order array + skip links), every bucket entry
// of every visited level-3 node.  While-while form: each lane first advances to its next non-empty level-3 node that
// passes the slab test, then scans that node's entries.  `closest`/`best` come in holding the ground-sphere result.
RT_DEV void tree_scan(const float4* s_nodes, const RayF& r, float a, bool live, float& closest, int& best) {
    const DevTree& T = cold_args()->tree;
    if (T.n_nodes == 1) {
        // the list seen as one unbounded node (rt_api.hip build_list_tree): all n_entries spheres are this ray's to test.  Few
        // rays come here (outside the near zone, ties), so one at a time with lanes = spheres as in closest_list — the smallest
        // offered t, the lowest entry among equal t, and only if it beats what the ray holds (the ground was tested first)
        const float4* __restrict__ hot = T.ent_hot;
        const int n = T.n_entries;
        const int lane = threadIdx.x & 63;
        unsigned long long todo = __ballot(live);
        if ((int)__popcll(todo) * RT_LIST_COOP_COST <= n) {
            while (todo != 0ull) {
                const int L = __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                RayF q;
                q.o.x = bcast(r.o.x, L); q.o.y = bcast(r.o.y, L); q.o.z = bcast(r.o.z, L);
                q.d.x = bcast(r.d.x, L); q.d.y = bcast(r.d.y, L); q.d.z = bcast(r.d.z, L);
                const float qa = bcast(a, L);
                float my_t = FLT_MAX; int my_k = 0x7fffffff;
                for (int base = 0; base < n; base += 256) {
                    float4 sv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) { const int k = base + u * 64 + lane; sv[u] = hot[k < n ? k : n - 1]; }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int k = base + u * 64 + lane;
                        if (k < n) {
                            const float cand = sphere_candidate(q, qa, sv[u]);
                            if (cand < my_t) { my_t = cand; my_k = k; }
                        }
                    }
                }
                const float mn = group_min<64>(my_t);
                const int km = wave_min_int((my_t == mn && my_k != 0x7fffffff) ? my_k : 0x7fffffff);
                if (lane == L && km != 0x7fffffff && mn < closest) { closest = mn; best = T.ent_id[km]; }
            }
            return;
        }
    }
    int e_best = -1;
    int node = live ? 0 : T.n_nodes;
    const int n_nodes = T.n_nodes;
    while (true) {
        int e = 0, e_end = 0;
        while (node < n_nodes) {
            const float4 n0 = s_nodes[node * 3 + 0];
            const float4 n1 = s_nodes[node * 3 + 1];
            const float4 n2 = s_nodes[node * 3 + 2];
            const int skip = __float_as_int(n1.z);
            if (ray_box(r, n0.x, n0.y, n0.z, n0.w, n1.x, n1.y)) {
                const int cnt = __float_as_int(n2.x);
                node = node + 1;
                if (cnt > 0) { e = __float_as_int(n1.w); e_end = e + cnt; break; }
            } else {
                node = skip;
            }
        }
        if (e >= e_end) break;          // no node left for this lane (it waits at the loop exit for the rest of the wave)
        while (e < e_end) {                             // four entries per pass, their loads in flight together; tested in order
            const int m = e_end - e;
            const float4 s0 = T.ent_hot[e], s1 = T.ent_hot[m > 1 ? e + 1 : e], s2 = T.ent_hot[m > 2 ? e + 2 : e], s3 = T.ent_hot[m > 3 ? e + 3 : e];
            sphere_test(r, a, s0.x, s0.y, s0.z, s0.w, e, closest, e_best);
            if (m > 1) sphere_test(r, a, s1.x, s1.y, s1.z, s1.w, e + 1, closest, e_best);
            if (m > 2) sphere_test(r, a, s2.x, s2.y, s2.z, s2.w, e + 2, closest, e_best);
            if (m > 3) sphere_test(r, a, s3.x, s3.y, s3.z, s3.w, e + 3, closest, e_best);
            e += m > 4 ? 4 : m;
        }
    }
    if (e_best >= 0) best = T.ent_id[e_best];
}

// Is the sphere stored in a level-3 node that the reference's traversal visits for this ray?  With no zero direction
// component a node's slab test passing implies all its ancestors' tests pass (their intervals contain the child's),
// so the node's own test — the reference's arithmetic — decides.
RT_DEV bool eligible(const float4* s_nodes, const RayF& r, float cand, int sphere STAT_ARG) {
    const DevTree& T = cold_args()->tree;
    STAT(st, ST_ELIG, 1); WPASS(WP_ELIG_FN);
    // Shortcut for spheres stored in several nodes (the big ones): the level-3 cell that contains the hit point.  If the
    // point keeps 0.012 from all six faces of that cell, the hit's t lies inside all three float slab intervals of the
    // cell (rounding errors are ~1e-5), so that node's slab test passes; it remains to see that the sphere is stored
    // there (one bit of its membership bitmap).  Two dependent loads instead of a scan of the membership list.
    {
        const int row = T.acc.bits_index[sphere];
        const float px = r.o.x + cand * r.d.x, py = r.o.y + cand * r.d.y, pz = r.o.z + cand * r.d.z;
        const int ix = (int)floorf((px + kRootHalfXZf) * kInvCellXZf), iy = (int)floorf(py * kInvCellYf), iz = (int)floorf((pz + kRootHalfXZf) * kInvCellXZf);
        if (row >= 0 && ix >= 0 && ix < 8 && iy >= 0 && iy < 8 && iz >= 0 && iz < 8) {
            const int cell = ix * 64 + iy * 8 + iz;
            const int node = T.acc.cellnode[cell];
            const uint32_t word = T.acc.cellbits[row * 16 + (cell >> 5)];
            if (node >= 0 && ((word >> (cell & 31)) & 1u)) {
                const float4 n0 = s_nodes[node * 3 + 0];
                const float4 n1 = s_nodes[node * 3 + 1];
                const float m = 0.012f;
                if (px > n0.x + m && px < n0.w - m && py > n0.y + m && py < n1.x - m && pz > n0.z + m && pz < n1.y - m) return true;
            }
        }
    }
    const int mb = T.acc.memb_start[sphere], me = T.acc.memb_start[sphere + 1];
    for (int k = mb; k < me; ++k) {
        const int node = T.acc.memb_cell[k];
        STAT(st, ST_ELIG_NODES, 1); WPASS(WP_ELIG_LIST);
        const float4 n0 = s_nodes[node * 3 + 0];
        const float4 n1 = s_nodes[node * 3 + 1];
        if (ray_box(r, n0.x, n0.y, n0.z, n0.w, n1.x, n1.y)) return true;
    }
    return false;
}

// Does the hit at `cand` lie inside the sphere's brick (rt_accel.h: the box of level-3 cells that ALL store the sphere, in
// cell coordinates, margins included)?  Then it lies in a stored cell whose three float slab intervals contain the hit's t
// (the hit point keeps 0.002 from the brick's outer faces, rounding moves an interval end by < 1e-5; inner faces are shared
// planes, so the cells' intervals tile the brick's without gaps): that node passes the reference's slab test, and with it
// its ancestors — no division needed.  Approximate arithmetic is fine here: its error is part of the 1e-5.
RT_DEV bool in_brick(const RayF& r, float cand, const float4 blo, const float4 bhi) {
    const float ux = __builtin_fmaf(__builtin_fmaf(cand, r.d.x, r.o.x), kInvCellXZf, 4.0f);      // (x + 11) / 2.75 = x / 2.75 + 4: cell coordinates 0..8
    const float uy = __builtin_fmaf(cand, r.d.y, r.o.y) * kInvCellYf;
    const float uz = __builtin_fmaf(__builtin_fmaf(cand, r.d.z, r.o.z), kInvCellXZf, 4.0f);
    return ux > blo.x && ux < bhi.x && uy > blo.y && uy < bhi.y && uz > blo.z && uz < bhi.z;
}

// blo/bhi, here and below: the candidate's DevAccel::brick pair (brick bounds, world-list index, single storing node or -1)
// The eligibility ladder of a hit at `cand`: inside the brick; else — hit point near an outer face of the brick, or no brick (a bucket was
// full) — the reference's own slab test of the single storing node, or of the nodes `eligible` goes through.  COUNT: `offer` counts the
// single node's test in the diagnostic builds (ST_ELIG, ST_ELIG_NODES, WP_OFFER_RAYBOX), the pooled walks' candidates never did.
template <bool COUNT>
RT_DEV bool hit_eligible(const float4* s_nodes, const RayF& r, float cand, const float4 blo, const float4 bhi STAT_ARG) {
    bool ok = in_brick(r, cand, blo, bhi);
    if (!ok) {
        const int node1 = __float_as_int(bhi.w);
        if (node1 >= 0) {
            if (COUNT) { STAT(st, ST_ELIG, 1); STAT(st, ST_ELIG_NODES, 1); WPASS(WP_OFFER_RAYBOX); }
            const float4 n0 = s_nodes[node1 * 3 + 0];
            const float4 n1 = s_nodes[node1 * 3 + 1];
            ok = ray_box(r, n0.x, n0.y, n0.z, n0.w, n1.x, n1.y);
        } else {
            ok = eligible(s_nodes, r, cand, __float_as_int(blo.w) STAT_PASS);
        }
    }
    return ok;
}
// a large sphere's offer to its own ray
RT_DEV void offer(const DevTree& T, const float4* s_nodes, const RayF& r, float cand, const float4 blo, const float4 bhi, float& best_t, int& best, bool& tie STAT_ARG) {
    STAT(st, ST_OFFERS, 1);
    const int id = __float_as_int(blo.w);
    if (cand < best_t) {
        if (hit_eligible<true>(s_nodes, r, cand, blo, bhi STAT_PASS)) { best_t = cand; best = id; }
    } else if (cand == best_t && id != best && best > 0) {
        tie = true;                      // two different tree spheres at the same float t: visit order decides -> reference scan
    }
}

// Fast path: large spheres directly, small spheres through the (x,z) grid along the ray's projection,
// clipped to the y-slab that holds them, front to back, ending at the column that lies beyond the best hit.  The walks
// (walk_pool for sparse grids, walk_pool_dense for dense ones) pool the sphere tests of a wave's rays and deal them out evenly
// over its 64 lanes; an exact tie between two tree spheres sends the ray to the reference scan.
struct Walk {                // a ray's walk over the grid, in cell units along its major axis
    int i, iend, coff;      // next column, end (exclusive, in travel direction), offset of the x- or z-major grid copy
    float om_c, on_c, slope, dm_c;
    bool fwd, walking;
    unsigned work, cols;    // grid entries this ray's columns have put into the wave's pool, and the columns it stepped through (read by the pilot pass only:
                            // a tile's cost in time — a ray along the horizon crosses hundreds of columns, most of them empty)
};

// last column worth visiting once a hit at best_t is known: the one that holds the hit point.  A sphere that offers a smaller t has its
// own (float) hit point before this one on the line and within R' of its centre — inside its registered extent,
// so it is filed under the column of that point, which the walk has passed or is in.  (Rounds 1-3 walked on until a column's entry
// edge lay R' beyond the hit, and began R' behind the origin: one column too many at either end of every walk — C5 450 -> 354 ms.)
RT_DEV void walk_clip(Walk& W, const DevAccel& A, float best_t) {
    const float fG = (float)A.G, back_c = 2e-3f * A.inv_h;     // (the float error of pm: ~1e-5 cells)
    const float pm = fminf(fmaxf(W.om_c + best_t * W.dm_c, -4.0f), fG + 4.0f);
    if (W.fwd) W.iend = min(W.iend, (int)floorf(pm + back_c) + 1);
    else W.iend = max(W.iend, (int)ceilf(pm - back_c - 1.0f) - 1);
    if (W.fwd ? (W.i >= W.iend) : (W.i <= W.iend)) W.i = W.iend;
}

RT_DEV Walk walk_setup(const DevAccel& A, const RayF& r, float best_t, int best) {
    Walk W;
    W.work = 0u; W.cols = 0u;
    const int G = A.G;
    const float fG = (float)G;
    const float slack = 2e-3f;
    const bool xmajor = fabsf(r.d.x) >= fabsf(r.d.z);
    const float om = xmajor ? r.o.x : r.o.z, on = xmajor ? r.o.z : r.o.x;
    const float dm = xmajor ? r.d.x : r.d.z, dn = xmajor ? r.d.z : r.d.x;
    W.coff = xmajor ? 0 : A.zoff;
    // everything below is in cell units (cell i spans [i, i+1) along either axis)
    W.om_c = (om - A.g0) * A.inv_h; W.on_c = (on - A.g0) * A.inv_h;
    W.dm_c = dm * A.inv_h;
    // the columns that matter are those in which a hit point can lie (a sphere is filed wherever its hit points can be): the stretch of
    // the line inside the spheres' y-slab, from the origin on; s_c covers the float error of these few operations
    const float s_c = slack * A.inv_h;
    // where the line crosses the planes y = ylo / y = yhi, measured along the major axis
    // the walk's own parameters need no exact division: a few ulp are far inside the rasterisation slack
    const float rmy = W.dm_c * __builtin_amdgcn_rcpf(r.d.y);
    const float mA = W.om_c + (A.ylo - r.o.y) * rmy, mB = W.om_c + (A.yhi - r.o.y) * rmy;
    float mlo = fminf(mA, mB) - s_c, mhi = fmaxf(mA, mB) + s_c;
    W.fwd = dm > 0.0f;
    if (W.fwd) mlo = fmaxf(mlo, W.om_c - s_c); else mhi = fminf(mhi, W.om_c + s_c);     // no hit point lies behind the origin (t > t_min > 0)
    int ilo = (int)floorf(fminf(fmaxf(mlo, -1.0f), fG)), ihi = (int)floorf(fminf(fmaxf(mhi, -1.0f), fG));
    W.walking = !(ihi < 0 || ilo > G - 1 || !(mlo <= mhi));
    ilo = max(ilo, 0); ihi = min(ihi, G - 1);
    W.i = W.fwd ? ilo : ihi;
    W.iend = (W.fwd ? ihi : ilo) + (W.fwd ? 1 : -1);
    W.slope = dn * __builtin_amdgcn_rcpf(dm);
    if (best >= 0) walk_clip(W, A, best_t);
    if (W.i == W.iend || (W.fwd ? (W.i > W.iend) : (W.i < W.iend))) W.walking = false;
    return W;
}

// ---------------------------------------------------------------------------------------------------- the walk of a full wave
// Letting every lane test the spheres of ITS columns (rounds 1-2: walk_lanes, removed in round 3 with the cooperative single-ray
// walk once no launch reached them) ran at 47 % busy lanes, 3.5 of 6 test slots used, lanes holding a candidate waiting for a
// vote.  walk_pool spreads the wave's sphere tests evenly instead (the scheme of the binary16 scan, rt_kernels_fp16.hip): per round every walking lane puts the entry ranges of its next RT_POOL_COLS columns
// into the wave's pool (LDS); a prefix over the ranges and a binary search give every lane an equal span of the concatenated
// entries, which it tests — 18-operation discriminant and square-root-free pre-filter as in phase A — against the OWNER's ray
// (LDS) whoever that is; survivors go into a queue of the wave and are resolved 64 at a time (exact roots, brick / slab
// eligibility as in phase B), the owner's best hit kept as a 64-bit key (t bits << 32 | sphere index) by an LDS atomic
// min.  An atomic min that meets an equal t from another sphere flags the exact tie (-> reference scan), as `offer` does.
// Nothing here decides a hit differently: the same candidates' exact values, merged by a minimum instead of one after the other;
// testing MORE spheres than a clipped per-ray walk would (no clipping inside a round) cannot change the minimum (App. A.4).
static_assert(RT_POOL_COLS_THIN >= RT_POOL_COLS, "a thin round takes at least as many columns as a full one");
constexpr int kWalkPool = 64 * RT_POOL_COLS;                  // segments per wave and round
constexpr int kWalkCand = 128;
struct WalkLds {
    uint2 seg[kWalkPool];                // (first entry, count | owner << 26)
    unsigned pref[kWalkPool];            // exclusive prefix of the counts
    float4 ray[128];                     // per owner: (o.x, o.y, o.z, d.x) (d.y, d.z, a, f_abt)
    unsigned long long key[64];          // per owner: bits of the best t << 32 | sphere index (low word ~0: none yet)
    uint4 cq[kWalkCand];                 // candidates: (bits of b, bits of disc, entry, owner)
    unsigned count, tie_lo, tie_hi, pad_;
};
// A thin round (walk_pool, at most kThinWalkers walkers) keeps its walkers' records in `pref` — per walker of rank k two uint4: (lane, next
// column, step, end column) (bits of om_c, on_c, slope; grid offset) — and deals its entries out through `seg`: slot j = (entry, owner).
constexpr int kThinWalkers = 16, kThinCols = 4;
static_assert(kThinWalkers * kThinCols == 64, "a thin round: one lane per (walker, column)");
static_assert(kThinCols == RT_POOL_COLS_THIN, "a thin round takes the columns a round of few walkers took before it");
static_assert(sizeof(unsigned) * kWalkPool >= sizeof(uint4) * 2 * kThinWalkers && sizeof(uint2) * kWalkPool >= sizeof(uint2) * 64, "the thin round's records and slots live in pref and seg");
struct PoolSpan { unsigned cur, end, seg_end, base, sg; int owner; RayF q; float a, abt, atm; };      // a lane's walk through one span of the pool
RT_DEV void walk_sync() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier(); }

// The steps that the two pooled walks share, each written once.  Where a walk still spells one of them out (the thin round's column
// range; walk_pool_dense's owner record, span search and discriminant; the candidate queue of both), every form of the helper that
// was tried changed kernel text there, and text is what these kernels are held to (HISTORY.md, round 26).
// A column's bins (rt_accel.h): Gf fine bins of width 1 / F cells, entries keyed by their centre — the query grows by q_c.
struct ColBins { const int32_t* __restrict__ cs; int Gf; float fF, fGf, fGfm, q_c; };
// The entry range [e0, e1) of column i of a walk (om_c, on_c, slope, coff: Walk); left as it is where the line misses the column's bins.
RT_DEV void column_entries(const ColBins& B, float om_c, float on_c, float slope, int coff, int i, int& e0, int& e1) {
    const float u0 = on_c + ((float)i - om_c) * slope, u1 = u0 + slope;                          // the line at the column's two edges
    const float lo = (fminf(u0, u1) - B.q_c) * B.fF, hi = (fmaxf(u0, u1) + B.q_c) * B.fF;      // in fine bins (F is a power of two)
    if (hi >= 0.0f && lo < B.fGf) {
        const int k0 = (int)fmaxf(lo, 0.0f), k1 = (int)fminf(hi, B.fGfm);
        const unsigned cbase = (unsigned)(coff + i * B.Gf);
        e0 = B.cs[cbase + (unsigned)k0]; e1 = B.cs[cbase + (unsigned)k1 + 1u];
    }
}

// The pooled walks' square-root-free pre-filter (App. A.5), for an entry with disc > 0.  b: the entry's; abt = a * best_t and atm = a * t_min, each
// with its margin towards "keep" (the owner's L.ray record, f_abt; a * (0.001f * 0.9999f - 1e-6f)).  Lm > 0 with Lm^2 > disc: the near root lies
// beyond the best hit; M > 0 with M^2 > disc: the far root lies behind t_min.  The two cannot both be positive (Lm > 0 needs b + kb < -abt,
// M > 0 needs b - kb > -atm, and abt > atm), so the caller makes one test of the larger: the entry is dropped if P > 0 && P * P > disc * 1.0003f.
// (the margins are fused here — one rounding less than the analysis allows for).  The value, not the verdict, is returned: a helper that
// returns the comparison moves the caller's loads behind its branch (HISTORY.md, round 26).
RT_DEV float entry_margin(float b, float abt, float atm) {
    const float ab = fabsf(b);
    const float Lm = __builtin_fmaf(ab, -1e-4f, -b) - abt, M = __builtin_fmaf(ab, -1e-4f, b) + atm;
    return fmaxf(Lm, M);
}

// An owner's ray as its L.ray record holds it, for whoever tests its spheres: origin, direction, a = |d|^2 and abt (entry_margin) as of the round's start.
// (I: int or unsigned as the caller holds the owner — converting the index changes the kernels' text.  walk_pool_dense reads the record itself: there even this form does.)
template <typename I>
RT_DEV void owner_ray(const WalkLds& L, I owner, RayF& q, float& a, float& abt) {
    const float4 r0 = L.ray[2 * owner], r1 = L.ray[2 * owner + 1];
    q.o = {r0.x, r0.y, r0.z}; q.d = {r0.w, r1.x, r1.y}; a = r1.z; abt = r1.w;
}
RT_DEV float margin_atm(float a) { return a * (0.001f * 0.9999f - 1e-6f); }      // entry_margin's atm: a * t_min, lowered
RT_DEV float margin_abt(float a, float best_t) { return __builtin_fmaf(a * best_t, 1.0001f, 1e-6f * a); }      // ... and its abt: a * best_t, raised
// A round begins: this lane's state for whoever tests its spheres (the ray's second half with abt as of now, the best hit as a key), the tie flags cleared ...
RT_DEV void round_begin(WalkLds& L, int lane, const RayF& r, float a, float best_t, int best) {
    L.ray[2 * lane + 1] = make_float4(r.d.y, r.d.z, a, margin_abt(a, best_t));
    L.key[lane] = ((unsigned long long)__float_as_uint(best_t) << 32) | (unsigned)best;
    if (lane == 0) { L.tie_lo = 0u; L.tie_hi = 0u; }
}
// ... and ends, after the fence behind its last candidate: every owner picks up its key and its tie bit
RT_DEV void round_pickup(const WalkLds& L, int lane, float& best_t, int& best, bool& tie) {
    const unsigned long long k = L.key[lane];
    best_t = __uint_as_float((unsigned)(k >> 32)); best = (int)(unsigned)k;
    const unsigned tmask = lane < 32 ? L.tie_lo : L.tie_hi;
    if ((tmask >> (lane & 31)) & 1u) tie = true;
}

// one queued candidate: the exact roots' offer (sphere_offer_t), eligibility as in `offer`, merged into the owner's key
// (q, a: the owner's ray and |d|^2 — a direct round holds them in registers, the queue's candidates fetch them from L.ray)
RT_DEV void pool_candidate_b(const DevTree& T, const float4* s_nodes, WalkLds& L, const uint4 c, const RayF& q, const float a, const float4 blo, const float4 bhi STAT_ARG) {
    const int owner = (int)c.w;
    const float b = __uint_as_float(c.x), disc = __uint_as_float(c.y);
    const unsigned long long k0 = L.key[owner];
    const float best_t = __uint_as_float((unsigned)(k0 >> 32));
    const int best = (int)(unsigned)k0;
    const float cand = sphere_offer_t(a, b, sqrtf(disc));
    if (!(cand <= best_t)) return;
    const int id = __float_as_int(blo.w);
    STAT(st, ST_OFFERS, 1);
    bool tie = false;
    if (cand < best_t) {
        if (hit_eligible<false>(s_nodes, q, cand, blo, bhi STAT_PASS)) {
            const unsigned long long old = atomicMin(&L.key[owner], ((unsigned long long)__float_as_uint(cand) << 32) | (unsigned)id);
            // an equal t from another tree sphere (index > 0: the ground wins its ties in the reference too): the visit order decides
            tie = (unsigned)(old >> 32) == __float_as_uint(cand) && (int)(unsigned)old != id && (int)(unsigned)old > 0;
        }
    } else tie = id != best && best > 0;
    if (tie) { if (owner < 32) atomicOr(&L.tie_lo, 1u << owner); else atomicOr(&L.tie_hi, 1u << (owner - 32)); }
}

RT_DEV void pool_candidate(const DevTree& T, const float4* s_nodes, WalkLds& L, const uint4 c STAT_ARG) {
    // (the brick is asked for before the roots are formed: its round trip overlaps the square root and the divisions — a candidate that
    // cannot win has fetched it for nothing, a chain alone in its wave has one dependent round trip less per candidate)
    const int e = (int)c.z;
    const float4 blo = T.acc.brick[2 * e], bhi = T.acc.brick[2 * e + 1];
    RayF q; float a, abt;
    owner_ray(L, c.w, q, a, abt);
    pool_candidate_b(T, s_nodes, L, c, q, a, blo, bhi STAT_PASS);
}

RT_DEV void pool_drain(const DevTree& T, const float4* s_nodes, WalkLds& L, int lane, unsigned& qn STAT_ARG) {
    walk_sync();
    const unsigned cnt = min(qn, (unsigned)kWalkCand);
    for (unsigned base = 0; base < cnt; base += 64u) {
        STAT(st, ST_B_ROUNDS_WAVE, 1);
        const unsigned i = base + (unsigned)lane;
        if (i < cnt) { STAT(st, ST_B_LANES, 1); pool_candidate(T, s_nodes, L, L.cq[i] STAT_PASS); }
    }
    qn = 0u;
    walk_sync();
}

template <int RT_QUORUM_DEN>
RT_DEV void walk_pool(const DevTree& T, const float4* s_nodes, WalkLds& L, const RayF& r, float a, Walk& W, float& best_t, int& best, bool& tie STAT_ARG) {
    const DevAccel& A = T.acc;
    const int32_t* __restrict__ cs = A.cs;
    const float4* __restrict__ hot = A.hot;
    const int lane = threadIdx.x & 63;
    const int Gf = A.Gf;
    const float fF = (float)A.F, fGf = (float)Gf, fGfm = fGf - 0.5f, q_c = A.rq_c;
    const ColBins B = {cs, Gf, fF, fGf, fGfm, q_c};
    const int step = W.fwd ? 1 : -1;
    bool walking = W.walking && W.i != W.iend;
    const int nw0 = __popcll(__ballot(walking));
    const bool thin_round = RT_POOL_THIN_ROUND && nw0 <= kThinWalkers;      // (walkers only leave: every round of this call has at most 16)
    L.ray[2 * lane] = make_float4(r.o.x, r.o.y, r.o.z, r.d.x);
    while (true) {
        round_begin(L, lane, r, a, best_t, best);
        const unsigned long long wmask = __ballot(walking);
        if (thin_round && walking) {
            const unsigned rank = rank_below(wmask);
            uint4* rec = (uint4*)L.pref;
            rec[2 * rank] = make_uint4((unsigned)lane, (unsigned)W.i, (unsigned)step, (unsigned)W.iend);
            rec[2 * rank + 1] = make_uint4(__float_as_uint(W.om_c), __float_as_uint(W.on_c), __float_as_uint(W.slope), (unsigned)W.coff);
        }
        walk_sync();
        unsigned n_seg = 0u;                                         // (<= 64 x RT_POOL_COLS: the pool cannot overflow)
        bool picked = false;                                         // a round that tested entries: the owners pick up their keys
        bool dealt = false;                                          // the thin round has done the round's tests itself
        if (thin_round) {
            // ---- a thin round (at most 16 walkers entered: a thin wave's chains — the frame's critical path — or a drained wave): lane l
            // forms column (l & 3) of the walker of rank (l >> 2) — phase 1 once, wave-wide, instead of four unrolled copies per walker —
            // and every range's lane writes its entries into consecutive slots: the testing lane reads its slot, no prefix table, no search
            const int nwr = __popcll(wmask);
            const int wk = lane >> 2, c = lane & 3;
            int f0 = 0; unsigned cnt = 0u;                           // the column's first entry and its count
            if (wk < nwr) {
                const uint4* rec = (const uint4*)L.pref;
                const uint4 ra = rec[2 * wk], rb = rec[2 * wk + 1];
                const int wstep = (int)ra.z;
                if (c < ((int)ra.w - (int)ra.y) * wstep) {           // (columns left: a column at or beyond the end is empty)
                    const int wi = (int)ra.y + c * wstep;
                    // (column_entries' steps on the record's values, spelled out)
                    const float w_om = __uint_as_float(rb.x), w_on = __uint_as_float(rb.y), w_slope = __uint_as_float(rb.z);
                    const float u0 = w_on + ((float)wi - w_om) * w_slope, u1 = u0 + w_slope;          // the line at the column's two edges
                    const float lo = (fminf(u0, u1) - q_c) * fF, hi = (fmaxf(u0, u1) + q_c) * fF;      // in fine bins (F is a power of two)
                    if (hi >= 0.0f && lo < fGf) {
                        const int k0 = (int)fmaxf(lo, 0.0f), k1 = (int)fminf(hi, fGfm);
                        const unsigned cbase = (unsigned)((int)rb.w + wi * Gf);
                        const int a0 = cs[cbase + (unsigned)k0], a1 = cs[cbase + (unsigned)k1 + 1u];
                        if (a1 > a0) { f0 = a0; cnt = (unsigned)(a1 - a0); }
                    }
                }
            }
            // the owner steps past the columns taken; its four lanes' counts come back to it (two quad adds, one lane read)
            int qs = (int)cnt;
            qs += __builtin_amdgcn_update_dpp(0, qs, 0xB1, 0xf, 0xf, false);     // quad_perm:[1,0,3,2]
            qs += __builtin_amdgcn_update_dpp(0, qs, 0x4E, 0xf, 0xf, false);     // quad_perm:[2,3,0,1]
            const unsigned rank = rank_below(wmask);
            const int mywork = __builtin_amdgcn_ds_bpermute((int)((rank & 15u) << 4), qs);            // from lane 4 x rank
            if (walking) {
                const int taken = min(kThinCols, (W.iend - W.i) * step);
                STAT(st, ST_COLS, taken);
                W.i += taken * step; W.cols += (unsigned)taken; W.work += (unsigned)mywork;
            }
            unsigned total;
            const unsigned ex = wave_excl_scan(cnt, total);
            RT_STATS_ONLY(n_seg = (unsigned)__popcll(__ballot(cnt != 0u)); TRSTAT_ROUND(lane, n_seg, total); n_seg = 0u;)
            if (total <= 64u) {
                dealt = true;
                if (total != 0u) {
                    picked = true;
                    uint2* slot = (uint2*)L.seg;
                    // (the owner's lane is read again here, not kept from phase 1: a register less across the scan, and k_render<true,1,5> stays without scratch)
#pragma nounroll
                    for (unsigned t = 0u; t < cnt; ++t) slot[ex + t] = make_uint2((unsigned)f0 + t, L.pref[8 * wk]);
                    walk_sync();
                    const bool act = (unsigned)lane < total;
                    STAT(st, ST_A_ITERS_WAVE, 1);
                    unsigned he = 0u; int owner = 0;
                    if (act) { const uint2 sl = slot[lane]; he = sl.x; owner = (int)sl.y; }
                    RayF q; float qa, abt;
                    owner_ray(L, owner, q, qa, abt);
                    const float4 s4 = hot[he], blo = A.brick[2 * he], bhi = A.brick[2 * he + 1];
                    const float atm = margin_atm(qa);
                    STAT(st, ST_TESTS, act ? 1 : 0); STAT(st, ST_A_LANE_STEPS, act ? 1 : 0);
                    const float2 bc = sphere_bc(q, s4);
                    const float b = bc.x, disc = b * b - qa * bc.y;
                    const float P = entry_margin(b, abt, atm);
                    if (act && disc > 0.0f && !(P > 0.0f && P * P > disc * 1.0003f)) {
                        STAT(st, ST_DISCPOS, 1);
                        pool_candidate_b(T, s_nodes, L, make_uint4(__float_as_uint(b), __float_as_uint(disc), he, (unsigned)owner), q, qa, blo, bhi STAT_PASS);
                    }
                    walk_sync();
                }
            } else {
                // more than one entry per lane: the non-empty ranges, compacted, go to the generic loop in its own layout (the records in
                // `pref` are read: phase 2 below may overwrite them after the fence)
                const bool has = cnt != 0u;
                const unsigned long long m = __ballot(has);
                if (has) L.seg[rank_below(m)] = make_uint2((unsigned)f0, cnt | (L.pref[8 * wk] << 26));
                n_seg = (unsigned)__popcll(m);
                walk_sync();
            }
        } else {
        // ---- phase 1: the entry ranges of the next RT_POOL_COLS columns of every walking lane (their cell-start loads in flight together)
        // (a wave with few walkers — a thin wave's chains, the frame's critical path — takes RT_POOL_COLS_THIN columns per round: as
        // many cell-start loads in flight, fewer rounds and their dependent round trips; the pool holds 64 x RT_POOL_COLS ranges)
        const int cols_now = nw0 * RT_POOL_COLS_THIN <= kWalkPool ? RT_POOL_COLS_THIN : RT_POOL_COLS;
        int e0[RT_POOL_COLS_THIN], e1[RT_POOL_COLS_THIN];
#pragma unroll
        for (int c = 0; c < RT_POOL_COLS_THIN; ++c) {
            e0[c] = 0; e1[c] = 0;
            if (c < cols_now && walking && W.i != W.iend) {
                STAT(st, ST_COLS, 1);
                column_entries(B, W.om_c, W.on_c, W.slope, W.coff, W.i, e0[c], e1[c]);
                W.i += step; ++W.cols;
            }
        }
#pragma unroll
        for (int c = 0; c < RT_POOL_COLS_THIN; ++c) {
            if (c >= RT_POOL_COLS && c >= cols_now) break;          // (wave-uniform)
            const bool has = e1[c] > e0[c];
            const unsigned long long m = __ballot(has);
            if (has) {
                const unsigned slot = n_seg + rank_below(m);
                L.seg[slot] = make_uint2((unsigned)e0[c], (unsigned)(e1[c] - e0[c]) | ((unsigned)lane << 26));
                W.work += (unsigned)(e1[c] - e0[c]);
            }
            n_seg += (unsigned)__popcll(m);
        }
        walk_sync();
        RT_STATS_ONLY(if (nw0 <= kThinWalkers && n_seg == 0u) TRSTAT_ROUND(lane, 0u, 0u);)
        }
        if (!dealt && n_seg != 0u) {
            picked = true;
            // ---- phase 2: prefix of the ranges, an equal span of the concatenated entries per lane
            unsigned total = 0u;
            {
                unsigned run = 0u;
#pragma unroll
                for (int k = 0; k < RT_POOL_COLS; ++k) {
                    if (k > 0 && n_seg <= 64u * (unsigned)k) break;          // (wave-uniform: nothing left to count)
                    const unsigned sidx = (unsigned)(k * 64 + lane);
                    const unsigned cnt = sidx < n_seg ? (L.seg[sidx].y & 0x3ffffffu) : 0u;
                    unsigned tot;
                    const unsigned ex = wave_excl_scan(cnt, tot);
                    if (sidx < n_seg) L.pref[sidx] = run + ex;
                    run += tot;
                }
                total = run;
            }
            RT_STATS_ONLY(if (nw0 <= kThinWalkers && !thin_round) TRSTAT_ROUND(lane, n_seg, total);)
            walk_sync();
            // RT_POOL_SPANS spans per lane, stepped through side by side: as many entry loads in flight per lane
            const unsigned C = (total + 64u * RT_POOL_SPANS - 1u) / (64u * RT_POOL_SPANS);
            PoolSpan sp[RT_POOL_SPANS];
#pragma unroll
            for (int j = 0; j < RT_POOL_SPANS; ++j) {
                PoolSpan& S = sp[j];
                const unsigned begin = min((unsigned)(lane + 64 * j) * C, total);
                S.end = min(begin + C, total); S.cur = begin; S.seg_end = begin; S.base = 0u; S.sg = 0u; S.owner = -1;
                S.q.o = {0.f, 0.f, 0.f}; S.q.d = {0.f, 1.f, 0.f}; S.a = 1.0f; S.abt = 0.0f; S.atm = 0.0f;
                if (n_seg <= 4u) {
                    // a thin wave's round: a handful of ranges — three independent LDS reads instead of a chain of eight
                    const unsigned p1 = L.pref[min(1u, n_seg - 1u)], p2 = L.pref[min(2u, n_seg - 1u)], p3 = L.pref[min(3u, n_seg - 1u)];
                    S.sg = (n_seg > 1u && p1 <= begin ? 1u : 0u) + (n_seg > 2u && p2 <= begin ? 1u : 0u) + (n_seg > 3u && p3 <= begin ? 1u : 0u);
                } else if (begin < S.end) {
                    unsigned lo = 0u, hi = n_seg;
#pragma unroll
                    for (int it = 0; it < 8; ++it) {                 // kWalkPool <= 256
                        const unsigned mid = (lo + hi) >> 1;
                        if (hi - lo > 1u) { if (L.pref[mid] <= begin) lo = mid; else hi = mid; }
                    }
                    S.sg = lo;
                }
            }
            // ---- phase 3: the tests
            unsigned qn = 0u;
            if (RT_POOL_DIRECT && RT_POOL_SPANS == 1 && total <= 64u) {
                // A round of at most one entry per lane (a thin wave's chains: the frame's critical path): the entry comes with its brick,
                // and the lane that finds a candidate resolves it on the spot — no queue, and the brick's round trip rides on the entry's
                // (a lone bounce: three dependent cache round trips in the walk become two).
                PoolSpan& S = sp[0];
                const bool act = S.cur < S.end;
                STAT(st, ST_A_ITERS_WAVE, 1);
                unsigned he = 0u;
                if (act) {
                    const uint2 sd = L.seg[S.sg];
                    const unsigned p0 = L.pref[S.sg];
                    he = sd.x - p0 + S.cur;
                    S.owner = (int)(sd.y >> 26);
                    owner_ray(L, S.owner, S.q, S.a, S.abt);
                    S.atm = margin_atm(S.a);
                }
                const float4 s4 = hot[he], blo = A.brick[2 * he], bhi = A.brick[2 * he + 1];
                STAT(st, ST_TESTS, act ? 1 : 0); STAT(st, ST_A_LANE_STEPS, act ? 1 : 0);
                const float2 bc = sphere_bc(S.q, s4);
                const float b = bc.x, disc = b * b - S.a * bc.y;
                const float P = entry_margin(b, S.abt, S.atm);
                if (act && disc > 0.0f && !(P > 0.0f && P * P > disc * 1.0003f)) {
                    STAT(st, ST_DISCPOS, 1);
                    pool_candidate_b(T, s_nodes, L, make_uint4(__float_as_uint(b), __float_as_uint(disc), he, (unsigned)S.owner), S.q, S.a, blo, bhi STAT_PASS);
                }
            } else                                          // (pool_drain below, with nothing queued, is the fence before the owners pick up)
            while (true) {
                bool any = false;
#pragma unroll
                for (int j = 0; j < RT_POOL_SPANS; ++j) any = any || sp[j].cur < sp[j].end;
                if (__ballot(any) == 0ull) break;
                STAT(st, ST_A_ITERS_WAVE, 1);
                bool act[RT_POOL_SPANS]; unsigned he[RT_POOL_SPANS]; float4 s4[RT_POOL_SPANS];
#pragma unroll
                for (int j = 0; j < RT_POOL_SPANS; ++j) {
                    PoolSpan& S = sp[j];
                    act[j] = S.cur < S.end;
                    if (act[j] && S.cur >= S.seg_end) {
                        const uint2 sd = L.seg[S.sg];
                        const unsigned p0 = L.pref[S.sg];
                        ++S.sg;
                        S.seg_end = p0 + (sd.y & 0x3ffffffu);
                        S.base = sd.x - p0;
                        const int ow = (int)(sd.y >> 26);
                        if (ow != S.owner) {
                            S.owner = ow;
                            owner_ray(L, ow, S.q, S.a, S.abt);
                            S.atm = margin_atm(S.a);
                        }
                    }
                    he[j] = act[j] ? S.base + S.cur : 0u;
                    s4[j] = hot[he[j]];
                }
                bool hold[RT_POOL_SPANS]; float hb[RT_POOL_SPANS], hd[RT_POOL_SPANS];
                bool anyhold = false;
#pragma unroll
                for (int j = 0; j < RT_POOL_SPANS; ++j) {
                    const PoolSpan& S = sp[j];
                    STAT(st, ST_TESTS, act[j] ? 1 : 0); STAT(st, ST_A_LANE_STEPS, act[j] ? 1 : 0);
                    const float2 bc = sphere_bc(S.q, s4[j]);
                    const float b = bc.x, disc = b * b - S.a * bc.y;
                    const float P = entry_margin(b, S.abt, S.atm);
                    hold[j] = act[j] && disc > 0.0f && !(P > 0.0f && P * P > disc * 1.0003f);
                    hb[j] = b; hd[j] = disc;
                    anyhold = anyhold || hold[j];
                    if (act[j]) ++sp[j].cur;
                }
                if (__ballot(anyhold) != 0ull) {
#pragma unroll
                    for (int j = 0; j < RT_POOL_SPANS; ++j) {
                        const unsigned long long hm = __ballot(hold[j]);
                        if (hm != 0ull) {
                            const unsigned slot = qn + rank_below(hm);
                            if (hold[j]) {
                                STAT(st, ST_DISCPOS, 1);
                                const uint4 ce = make_uint4(__float_as_uint(hb[j]), __float_as_uint(hd[j]), he[j], (unsigned)sp[j].owner);
                                if (slot < (unsigned)kWalkCand) L.cq[slot] = ce;
                                else pool_candidate(T, s_nodes, L, ce STAT_PASS);
                            }
                            qn += (unsigned)__popcll(hm);
                        }
                    }
                }
                if (qn >= 64u) pool_drain(T, s_nodes, L, lane, qn STAT_PASS);
            }
            pool_drain(T, s_nodes, L, lane, qn STAT_PASS);
        }
        if (picked) {
            round_pickup(L, lane, best_t, best, tie);
        }
        if (walking && best >= 0) walk_clip(W, A, best_t);
        walking = walking && W.i != W.iend;
        const int left = __popcll(__ballot(walking));
        if (left == 0) break;
        if (RT_QUORUM_DEN > 0 && nw0 >= RT_QUORUM_MIN && left * RT_QUORUM_DEN <= nw0) break;     // the stragglers resume next bounce (ts.pending)
    }
    W.walking = walking;
}

// The pooled walk for DENSE grids (C5: ~30 entries per cell, 60-100 per column).  One column per walking lane and round; a lane
// steps through its span RT_DENSE_PB entries at a time (their loads in flight together) and filters
// against the owner's CURRENT best hit, re-read from the wave's LDS every pass — on a dense grid most of a column lies behind the
// first hit, and a filter that only knew the hit of the previous round would send all of it to the candidate queue.  The queue is
// drained from RT_DENSE_DRAIN candidates on, so that a found hit starts rejecting soon.
template <int RT_QUORUM_DEN>
RT_DEV void walk_pool_dense(const DevTree& T, const float4* s_nodes, WalkLds& L, const RayF& r, float a, Walk& W, float& best_t, int& best, bool& tie STAT_ARG) {
    constexpr int PB = RT_DENSE_PB;
    const DevAccel& A = T.acc;
    const int32_t* __restrict__ cs = A.cs;
    const float4* __restrict__ hot = A.hot;
    const int lane = threadIdx.x & 63;
    const int Gf = A.Gf;
    const float fF = (float)A.F, fGf = (float)Gf, fGfm = fGf - 0.5f, q_c = A.rq_c;
    const ColBins B = {cs, Gf, fF, fGf, fGfm, q_c};
    const int step = W.fwd ? 1 : -1;
    bool walking = W.walking && W.i != W.iend;
    const int nw0 = __popcll(__ballot(walking));
    L.ray[2 * lane] = make_float4(r.o.x, r.o.y, r.o.z, r.d.x);
    while (true) {
        round_begin(L, lane, r, a, best_t, best);
        walk_sync();
        // ---- phase 1: the entry range of the next column of every walking lane
        int e0 = 0, e1 = 0;
        if (walking && W.i != W.iend) {
            STAT(st, ST_COLS, 1);
            column_entries(B, W.om_c, W.on_c, W.slope, W.coff, W.i, e0, e1);
            W.i += step; ++W.cols;
        }
        const bool has = e1 > e0;
        const unsigned long long m = __ballot(has);
        const unsigned n_seg = (unsigned)__popcll(m);
        if (has) {
            const unsigned slot = rank_below(m);
            L.seg[slot] = make_uint2((unsigned)e0, (unsigned)(e1 - e0) | ((unsigned)lane << 26));
            W.work += (unsigned)(e1 - e0);
        }
        walk_sync();
        if (n_seg != 0u) {
            // ---- phase 2: prefix of the ranges, an equal span of the concatenated entries per lane
            unsigned total;
            {
                const unsigned cnt = (unsigned)lane < n_seg ? (L.seg[lane].y & 0x3ffffffu) : 0u;
                const unsigned ex = wave_excl_scan(cnt, total);
                if ((unsigned)lane < n_seg) L.pref[lane] = ex;
            }
            walk_sync();
            const unsigned C = (total + 63u) / 64u;
            PoolSpan S;
            const unsigned begin = min((unsigned)lane * C, total);
            S.end = min(begin + C, total); S.cur = begin; S.seg_end = begin; S.base = 0u; S.sg = 0u; S.owner = lane;
            S.q.o = {0.f, 0.f, 0.f}; S.q.d = {0.f, 1.f, 0.f}; S.a = 1.0f; S.abt = 0.0f; S.atm = 0.0f;
            if (begin < S.end) {
                unsigned lo = 0u, hi = n_seg;
#pragma unroll
                for (int it = 0; it < 6; ++it) {                     // n_seg <= 64
                    const unsigned mid = (lo + hi) >> 1;
                    if (hi - lo > 1u) { if (L.pref[mid] <= begin) lo = mid; else hi = mid; }
                }
                S.sg = lo;
            }
            // ---- phase 3: the tests
            unsigned qn = 0u;
            while (true) {
                const bool act = S.cur < S.end;
                if (__ballot(act) == 0ull) break;
                STAT(st, ST_A_ITERS_WAVE, 1);
                if (act && S.cur >= S.seg_end) {
                    const uint2 sd = L.seg[S.sg];
                    const unsigned p0 = L.pref[S.sg];
                    ++S.sg;
                    S.seg_end = p0 + (sd.y & 0x3ffffffu);
                    S.base = sd.x - p0;
                    S.owner = (int)(sd.y >> 26);
                    const float4 r0 = L.ray[2 * S.owner], r1 = L.ray[2 * S.owner + 1];          // (owner_ray without abt, which every pass forms anew below)
                    S.q.o = {r0.x, r0.y, r0.z}; S.q.d = {r0.w, r1.x, r1.y}; S.a = r1.z;
                    S.atm = S.a * (0.001f * 0.9999f - 1e-6f);
                }
                const unsigned nb = act ? min((unsigned)PB, min(S.seg_end, S.end) - S.cur) : 0u;   // (a batch stays within one owner's range)
                const unsigned he0 = act ? S.base + S.cur : 0u;
                const float4* __restrict__ hp = hot + he0;                            // (one address, the batch by immediate offsets)
                float4 s4[PB];
#pragma unroll
                for (int k = 0; k < PB; ++k) s4[k] = hp[k];                           // (padded arrays: reading past a range is harmless, holding is not)
                // the owner's best hit as of now
                const float bt_now = __uint_as_float((unsigned)(L.key[S.owner] >> 32));
                S.abt = margin_abt(S.a, bt_now);
                if (act) { STAT(st, ST_TESTS, nb); STAT(st, ST_A_LANE_STEPS, 1); }
                bool hold[PB]; float hb[PB], hd[PB];
                bool anyhold = false;
#pragma unroll
                for (int k = 0; k < PB; ++k) {
                    const float ocx = S.q.o.x - s4[k].x, ocy = S.q.o.y - s4[k].y, ocz = S.q.o.z - s4[k].z;
                    const float b = ocx * S.q.d.x + ocy * S.q.d.y + ocz * S.q.d.z;
                    const float c = (ocx * ocx + ocy * ocy + ocz * ocz) - s4[k].w;
                    const float disc = b * b - S.a * c;
                    const float P = entry_margin(b, S.abt, S.atm);
                    hold[k] = (unsigned)k < nb && disc > 0.0f && !(P > 0.0f && P * P > disc * 1.0003f);
                    hb[k] = b; hd[k] = disc;
                    anyhold = anyhold || hold[k];
                }
                if (__ballot(anyhold) != 0ull) {
#pragma unroll
                    for (int k = 0; k < PB; ++k) {
                        const unsigned long long hm = __ballot(hold[k]);
                        if (hm != 0ull) {
                            const unsigned slot = qn + rank_below(hm);
                            if (hold[k]) {
                                STAT(st, ST_DISCPOS, 1);
                                const uint4 ce = make_uint4(__float_as_uint(hb[k]), __float_as_uint(hd[k]), he0 + (unsigned)k, (unsigned)S.owner);
                                if (slot < (unsigned)kWalkCand) L.cq[slot] = ce;
                                else pool_candidate(T, s_nodes, L, ce STAT_PASS);
                            }
                            qn += (unsigned)__popcll(hm);
                        }
                    }
                }
                S.cur += nb;
                if (qn >= (unsigned)RT_DENSE_DRAIN) pool_drain(T, s_nodes, L, lane, qn STAT_PASS);
            }
            pool_drain(T, s_nodes, L, lane, qn STAT_PASS);
            round_pickup(L, lane, best_t, best, tie);
        }
        if (walking && best >= 0) walk_clip(W, A, best_t);
        walking = walking && W.i != W.iend;
        const int left = __popcll(__ballot(walking));
        if (left == 0) break;
        if (RT_QUORUM_DEN > 0 && nw0 >= RT_QUORUM_MIN && left * RT_QUORUM_DEN <= nw0) break;
    }
    W.walking = walking;
}

// hitTree (acceleration_structure.h:319-342): ground sphere first, then the tree.
// A pooled walk returns once most of the wave's rays are done (quorum): a lane whose walk is not finished comes back with
// ts.pending set and resumes on the next call with the same ray, while the lanes that are done go on to shade and start new
// rays — the wave does not wait for its longest walk.  `closest`/`best` persist with the caller.
// COOPG selects the walk: 4 = walk_pool (sparse grids), 5 = the same walk, the pre-classified chains start alone in their waves (very sparse grids), 2 = walk_pool_dense, 1 = none — trees without a candidate grid (and the
// reference traversal mode) take the literal scan for every ray.
// The spheres every bounce of every ray meets before its walk — the ground sphere and the first kHotLarge of the grid's large spheres
// (geometry and brick) — are staged in LDS behind the waves' pools by the kernels with a pooled walk: as uniform global loads in the
// serial part of a bounce each cost a full cache round trip (C2 / C3 are as long as their longest pixel: a lone bounce is what counts).
constexpr int kHotLarge = 8;
constexpr int kHotSlots = 1 + 3 * kHotLarge;                   // float4 slots: ground | large_hot[k] | large_brick[2k], [2k + 1]
RT_DEV float4* hot_spheres(const float4* s_nodes, int n_nodes) { return (float4*)((WalkLds*)(s_nodes + n_nodes * 3) + 4); }
template <bool POOL>
RT_DEV void stage_tree_fp32(const DevScene& S, const DevTree& T, float4* s_nodes) {
    const int n4 = T.n_nodes * 3;
    for (int t = threadIdx.x; t < n4; t += 256) s_nodes[t] = T.nodes4[t];
    if (POOL) {
        float4* h = hot_spheres(s_nodes, T.n_nodes);
        const int nl = min(T.acc.n_large, kHotLarge);
        if (threadIdx.x == 0) h[0] = S.ground_valid ? S.list_hot[0] : make_float4(0.f, 0.f, 0.f, 0.f);
        if ((int)threadIdx.x < nl) h[1 + threadIdx.x] = T.acc.large_hot[threadIdx.x];
        if ((int)threadIdx.x < 2 * nl) h[1 + kHotLarge + threadIdx.x] = T.acc.large_brick[threadIdx.x];
    }
    __syncthreads();
}

struct TreeState { Walk W; float g_t; int g_id; bool tie, pending; unsigned work, cols; };
RT_DEV void tree_state_init(TreeState& ts) {
    ts.pending = false; ts.tie = false; ts.g_t = FLT_MAX; ts.g_id = -1; ts.work = 0u; ts.cols = 0u; ts.W.work = 0u; ts.W.cols = 0u;
    ts.W.walking = false; ts.W.i = 0; ts.W.iend = 0; ts.W.coff = 0; ts.W.om_c = 0.f; ts.W.on_c = 0.f; ts.W.slope = 0.f; ts.W.dm_c = 0.f; ts.W.fwd = true;
}

template <int COOPG>
RT_DEV void closest_tree(const DevScene& S, const DevTree& T, const float4* s_nodes, const RayF& r, float a, bool live, float& closest, int& best, TreeState& ts STAT_ARG) {
    const bool fresh = live && !ts.pending;
    STAT(st, ST_RAYS, fresh ? 1 : 0);
    if (fresh) { closest = FLT_MAX; best = -1; }
    if (S.ground_valid && fresh) {
        WPASS(WP_GROUND);
        const float4 g = COOPG != 1 ? hot_spheres(s_nodes, T.n_nodes)[0] : S.list_hot[0];
        int gb = -1;
        // origin outside the sphere (c > 0) and heading away from its centre (b > 0): disc <= fl(b*b), so sqrt(disc) <= b and
        // both roots are <= 0 — the float test cannot pass (no margin involved); saves the exact sqrt and two divisions
        { const float ocx = r.o.x - g.x, ocy = r.o.y - g.y, ocz = r.o.z - g.z;
          const float b = ocx * r.d.x + ocy * r.d.y + ocz * r.d.z;
          const float c = (ocx * ocx + ocy * ocy + ocz * ocz) - g.w;
          if (__ballot(fresh && !(b > 0.0f && c > 0.0f)) != 0ull) sphere_test(r, a, g.x, g.y, g.z, g.w, 0, closest, gb); }
        if (gb == 0) best = 0;
    }
    RT_STATS_ONLY(
    const unsigned long long tG = TICK(); st.cyc[4] += tG;      // (entry stamp is subtracted by the caller's tC0)
    )
    bool slow = fresh;
    if (COOPG != 1 && T.acc.enabled) {
        // preconditions of the exactness argument; any NaN/inf makes a comparison false and sends the ray to the scan.  d.x and d.z must
        // be NORMAL numbers, not merely non-zero: walk_setup divides by the larger of the two through v_rcp_f32, and the reciprocal of a
        // subnormal below 2^-128 is +-inf - an infinite (then NaN) slope skipped every column of an all but vertical ray
        const float zx = r.o.x, zy = r.o.y - 1.0f, zz = r.o.z;
        const bool fast = fresh && (a >= 9.094947e-13f) && (a <= 1.0995116e12f) && (fabsf(r.d.x) >= FLT_MIN) && (fabsf(r.d.z) >= FLT_MIN)
                          && (fabsf(r.d.y) >= 9.094947e-13f) && (zx * zx + zy * zy + zz * zz <= T.acc.zone2);
        slow = fresh && !fast;
        STAT(st, ST_FAST, fast ? 1 : 0); STAT(st, ST_SLOW, slow ? 1 : 0);
        if (fast) {
            ts.g_t = closest; ts.g_id = best; ts.tie = false;
            const float ra = __builtin_amdgcn_rcpf(a);
            for (int k = 0; k < T.acc.n_large; ++k) {
                // same cheap pre-filter as in the walk: exact roots only for a sphere that can still win
                const float4* hs = hot_spheres(s_nodes, T.n_nodes);
                const float4 sp = k < kHotLarge ? hs[1 + k] : T.acc.large_hot[k];
                WPASS(WP_LARGE_K);
                const float2 bc = sphere_bc(r, sp);
                const float b = bc.x, disc = b * b - a * bc.y;
                if (disc > 0.0f) {
                    const float sqa = __builtin_amdgcn_sqrtf(disc);
                    const float m = 1e-4f * ((fabsf(b) + sqa) * ra) + 1e-6f;
                    const bool behind = (sqa - b) * ra + m < 0.001f;
                    const bool beyond = (-b - sqa) * ra - m > closest;
                    if (!behind && !beyond) {
                        WPASS(WP_LARGE_EXACT);
                        const float cand = sphere_offer_t(a, b, sqrtf(disc));
                        offer(T, s_nodes, r, cand, k < kHotLarge ? hs[1 + kHotLarge + 2 * k] : T.acc.large_brick[2 * k], k < kHotLarge ? hs[2 + kHotLarge + 2 * k] : T.acc.large_brick[2 * k + 1], closest, best, ts.tie STAT_PASS);
                    }
                }
            }
            WPASS(WP_SETUP);
            ts.W = walk_setup(T.acc, r, closest, best);
        }
        RT_STATS_ONLY(
        const unsigned long long tL = TICK(); st.cyc[5] += tL - tG;       // large spheres + walk set-up
        )
        const bool walker = fast || (live && ts.pending);
        const int nw = __popcll(__ballot(walker));
        if (nw > 0) {
            // every lane of the wave takes part: lanes without a walk of their own test other lanes' spheres
            WalkLds& L = *((WalkLds*)(s_nodes + T.n_nodes * 3) + (threadIdx.x >> 6));
            Walk Wl = ts.W; Wl.walking = walker && ts.W.walking;
            float bt = walker ? closest : FLT_MAX; int bi = walker ? best : -1; bool tt = false;
            // (sparse grids — C3: 3.6 entries per cell — pool two columns per ray and round; on dense ones — C5: 37 per cell, ~100
            // per column — that walk filters against a stale best hit: 1281 ms against 670 for walk_pool_dense, which re-reads it)
            if (COOPG >= 4) walk_pool<RT_QUORUM_SPARSE>(T, s_nodes, L, r, a, Wl, bt, bi, tt STAT_PASS);
            else walk_pool_dense<RT_QUORUM_DENSE>(T, s_nodes, L, r, a, Wl, bt, bi, tt STAT_PASS);
            if (walker) { ts.work += Wl.work; ts.cols += Wl.cols; Wl.work = 0u; Wl.cols = 0u; ts.W = Wl; closest = bt; best = bi; ts.tie = ts.tie || tt; }
        }
        if (walker) {
            ts.pending = ts.W.walking;
            if (!ts.pending && ts.tie) { closest = ts.g_t; best = ts.g_id; slow = true; STAT(st, ST_TIE, 1); }
        }
    }
    RT_STATS_ONLY(
    const unsigned long long tS0 = TICK(); st.cyc[1] += tS0 - tG;     // fast path (large spheres + setup + walk), wave time
    )
    if (__ballot(slow) != 0ull) { WPASS(WP_SCAN); tree_scan(s_nodes, r, a, slow, closest, best); }
    RT_STATS_ONLY(
    st.cyc[3] += TICK() - tS0;
    )
}

// ---------------------------------------------------------------------------------------------------- sampling
RT_DEV V3 random_in_unit_sphere(Rng& s) {               // material.h:35-41
    V3 p;
    do {
        WPASS(WP_REJ_ITER);
        const float x = rng_uniform(s); const float y = rng_uniform(s); const float z = rng_uniform(s);
        p.x = signed_unit(x); p.y = signed_unit(y); p.z = signed_unit(z);       // 2x - 1, the product exact (rt_sampling.h)
    } while (p.x * p.x + p.y * p.y + p.z * p.z >= 1.0f);
    return p;
}

// camera::get_ray + the two pixel-jitter draws (main.cu:104-106, camera.h:12-18, :45-49)
RT_DEV RayF primary_ray(const rt_camera& c, int i, int j, int max_x, int max_y, Rng& s) {
    const float u = ((float)i + rng_uniform(s)) / (float)max_x;
    const float v = ((float)j + rng_uniform(s)) / (float)max_y;
    float px, py;
    WPASS(WP_PRIMARY);
    do {
        WPASS(WP_DISK_ITER);
        const float x = rng_uniform(s); const float y = rng_uniform(s);
        px = signed_unit(x); py = signed_unit(y);
    } while (px * px + py * py + 0.0f >= 1.0f);
    const float rdx = c.lens_radius * px, rdy = c.lens_radius * py;
    RayF r;
    const float ox = rdx * c.u[0] + rdy * c.v[0], oy = rdx * c.u[1] + rdy * c.v[1], oz = rdx * c.u[2] + rdy * c.v[2];
    r.o.x = c.origin[0] + ox; r.o.y = c.origin[1] + oy; r.o.z = c.origin[2] + oz;
    r.d.x = (((c.lower_left_corner[0] + u * c.horizontal[0]) + v * c.vertical[0]) - c.origin[0]) - ox;
    r.d.y = (((c.lower_left_corner[1] + u * c.horizontal[1]) + v * c.vertical[1]) - c.origin[1]) - oy;
    r.d.z = (((c.lower_left_corner[2] + u * c.horizontal[2]) + v * c.vertical[2]) - c.origin[2]) - oz;
    return r;
}

// material::scatter for the sphere that was hit.  Returns false when the path is absorbed (metal, material.h:72).
RT_DEV bool scatter(const DevScene& S, int sphere, float t, RayF& r, V3& att, Rng& s) {
    const float4 g = S.shade[2 * sphere];
    const float4 m = S.shade[2 * sphere + 1];
    const int kind = S.kind8[sphere];
    V3 p, n;
    p.x = r.o.x + t * r.d.x; p.y = r.o.y + t * r.d.y; p.z = r.o.z + t * r.d.z;            // ray.h:13
    n.x = (p.x - g.x) / g.w; n.y = (p.y - g.y) / g.w; n.z = (p.z - g.z) / g.w;            // sphere.h:29
    // lambertian and metal both draw exactly one random_in_unit_sphere and nothing else: one shared rejection loop
    // (the slowest lane of a wave sets its length) instead of one per material branch; the draw order is unchanged
    V3 q = {0.0f, 0.0f, 0.0f};
    WPASS(WP_SC_ANY);
    if (kind != RT_MAT_DIELECTRIC) q = random_in_unit_sphere(s);
    // metal and dielectric both start from unit_vector(r_in.direction()) (material.h:69, :18): formed once for the lanes of either —
    // a wave that holds both kinds (most do: 15 % metal, 5 % glass) walks through both branches, and paid the square root and the
    // three divisions in each.  Same expression, same operands, same bits.
    float len = 1.0f; V3 ud = {0.0f, 0.0f, 0.0f};
    if (kind != RT_MAT_LAMBERTIAN) {
        len = sqrtf(r.d.x * r.d.x + r.d.y * r.d.y + r.d.z * r.d.z);
        ud.x = r.d.x / len; ud.y = r.d.y / len; ud.z = r.d.z / len;
    }
    if (kind == RT_MAT_LAMBERTIAN) {                                                          // material.h:55-60
        WPASS(WP_SC_LAMB);
        const float tx = (p.x + n.x) + q.x, ty = (p.y + n.y) + q.y, tz = (p.z + n.z) + q.z;
        r.d.x = tx - p.x; r.d.y = ty - p.y; r.d.z = tz - p.z;
        r.o = p;
        att.x *= m.x; att.y *= m.y; att.z *= m.z;
        return true;
    }
    if (kind == RT_MAT_METAL) {                                                               // material.h:68-73
        WPASS(WP_SC_METAL);
        const float k = 2.0f * dot3(ud, n);
        const float rx = ud.x - k * n.x, ry = ud.y - k * n.y, rz = ud.z - k * n.z;
        r.d.x = rx + m.w * q.x; r.d.y = ry + m.w * q.y; r.d.z = rz + m.w * q.z;
        r.o = p;
        att.x *= m.x; att.y *= m.y; att.z *= m.z;
        return dot3(r.d, n) > 0.0f;
    }
    // dielectric — material.h:81-113 (attenuation (1,1,1): the multiply is exact and omitted).  What depends on the sphere alone comes with
    // its record, computed once at upload by the same expressions (world_upload, rt_api.hip): 1 / ri, schlick's r0 squared, ri * ri.
    WPASS(WP_SC_DIEL);
    const float ri = m.w, inv_ri = m.x, r0sq = m.y, ri2 = m.z;
    const float dn = dot3(r.d, n);
    const float k = 2.0f * dn;
    const float rx = r.d.x - k * n.x, ry = r.d.y - k * n.y, rz = r.d.z - k * n.z;            // reflect(dir, normal), dir not normalised
    V3 on; float ni, cosine;
    if (dn > 0.0f) {
        on.x = -n.x; on.y = -n.y; on.z = -n.z; ni = ri;
        cosine = dn / len;
        cosine = sqrtf(1.0f - ri2 * (1.0f - cosine * cosine));
    } else {
        on = n; ni = inv_ri;
        cosine = -dn / len;
    }
    const V3 uv = ud;                                                                         // refract(), material.h:17-31
    const float dt = dot3(uv, on);
    const float disc = 1.0f - ni * ni * (1.0f - dt * dt);
    float fx = 0.0f, fy = 0.0f, fz = 0.0f, reflect_prob;
    if (disc > 0.0f) {
        const float sq = sqrtf(disc);
        fx = ni * (uv.x - dt * on.x) - sq * on.x;
        fy = ni * (uv.y - dt * on.y) - sq * on.y;
        fz = ni * (uv.z - dt * on.z) - sq * on.z;
        const float r0 = r0sq;                                                                // schlick(), material.h:11-15
        reflect_prob = r0 + (1.0f - r0) * pow5(1.0f - cosine);
    } else {
        reflect_prob = 1.0f;
    }
    r.o = p;
    if (rng_uniform(s) < reflect_prob) { r.d.x = rx; r.d.y = ry; r.d.z = rz; }
    else { r.d.x = fx; r.d.y = fy; r.d.z = fz; }
    return true;
}

// background gradient of color() — main.cu:67-72
RT_DEV V3 sky(const RayF& r, const V3& att) {
    WPASS(WP_SKY);
    const float len = sqrtf(r.d.x * r.d.x + r.d.y * r.d.y + r.d.z * r.d.z);
    const float uy = r.d.y / len;
    const float t = 0.5f * (uy + 1.0f);
    const float omt = 1.0f - t;
    V3 c;
    c.x = att.x * (omt + t * 0.5f);
    c.y = att.y * (omt + t * 0.7f);
    c.z = att.z * (omt + t * 1.0f);
    return c;
}

// ---------------------------------------------------------------------------------------------------- kernels
// MODE | entry point                      | a pixel runs                                    | and leaves                        | RenderMode<MODE>
//  0   | rt_render                        | ns samples                                      | its colour: / ns, sqrt            | averages, schedules
//  1   | rt_render_progressive            | one sample, slots taken in chunks of 64 a wave  | the sample, accumulated           | chunked
//  2   | rt_render_adaptive, one round    | ns samples more (ad_list: the active, resumed)  | its sums S_rgb, SL, Q (ad_*)      | schedules, sums, listed
//  3   | rt_render_adaptive_fused         | up to ns = max_spp, adapt_rule after min_spp, min_spp + batch, ... | what the rounds' check kernels write (FusedArgs) | schedules, sums, rule_in_lane
//  4   | rt_render_adaptive_refine_fused  | k_adapt_refine_seed's list, each from the caller's state (k0 samples), rule after k0 + batch, ... | as MODE 3 | ... and listed, resumes
// A pixel is a truncation of its own RNG stream, so which launch structure truncates it changes no bit.  Every line that one mode alone
// needs sits behind `if constexpr` of a RenderMode flag (below), so the other instantiations compile to what they were.
//
// Persistent waves: the grid is sized to what the chip holds at once.  Pixel slots are numbered tile-major
// (slot = local_tile*64 + ly*8 + lx, the 8x8 block shape of the reference); every lane starts on slot
// (wave*64 + lane) and, when its pixel is finished, pulls the next unclaimed slot from a global counter, so no lane
// waits for the slowest pixel of "its" tile.  Which lane renders a pixel does not affect the pixel (the RNG is per pixel).
//
// Long chains.  A pixel is a strictly serial chain of ns x bounces iterations, and a few pixels (crevices between a
// sphere and the ground, glass) need 10-15x the average.  One iteration of a full wave costs ~40 k cycles, of a wave
// with a single live lane ~16 k, so the frame cannot end before (longest chain) x (iteration time of ITS wave).
// Therefore: slots are interleaved over blocks of 64 tiles (the 64 pixels of a tile go to 64 different lanes/waves: long
// pixels cluster); a lane whose pixel shows >= RT_LONG_RATE bounces per sample (checked every RT_LONG_CHECK samples) marks it long;
// a wave holding a long pixel stops refilling its other lanes ("thin" wave, raised issue priority) until that pixel is
// finished, then resumes.  A global counter caps the number of thin waves at a quarter of the grid, so a scene made of long pixels only keeps its throughput.
// What a MODE is, named once (the table above): every test of the mode in k_render reads one of these.
template <int MODE> struct RenderMode {
    static constexpr bool averages = MODE == 0;                  // ends a pixel with its colour: / ns, sqrt
    static constexpr bool chunked = MODE == 1;                   // one sample a launch, accumulated; slots taken in chunks of 64 a wave
    static constexpr bool schedules = MODE != 1;                 // reads what the scheduling pass leaves (tail list, long-chain threshold, solo chains)
    static constexpr bool sums = MODE >= 2;                      // keeps the luminance sums sum_l, sum_q beside the colour sum
    static constexpr bool listed = MODE == 2 || MODE == 4;       // may run over a list of pixels, each resumed from its sums
    static constexpr bool rule_in_lane = MODE == 3 || MODE == 4; // the lane applies adapt_rule at the checkpoints and ends the pixel (FusedArgs)
    static constexpr bool resumes = MODE == 4;                   // always over a list (refine_fused_list), from the caller's state: checkpoints count from k0
};
template <bool TREE, int MODE, int COOPG>
__global__ __launch_bounds__(256, RT_RENDER_WAVES) void k_render(RenderArgs A) {
    using M = RenderMode<MODE>;
    extern __shared__ float4 s_nodes[];
    if (TREE) stage_tree_fp32<COOPG != 1>(A.scene, A.tree, s_nodes);
    const int lane = threadIdx.x & 63;
    // (MODE 4: the list's count lies `elements of the part` words behind its start, rt_device.h)
    const long long n_elems = part_elems(A);
    const long long n_slots = M::resumes ? (long long)refine_fused_list(A)[n_elems] : (M::listed && A.ad_list) ? (long long)*A.ad_count : A.n_local_tiles * 64;
    const int ns = M::chunked ? 1 : A.ns;

    const long long n_waves = (long long)gridDim.x * 4;
    long long slot = 0;
    int i = 0, j = 0; long long idx = 0;
    unsigned int iters = 0;             // bounces spent on the current pixel
    bool is_long = false;               // the current pixel has been classified long
    bool is_med = false;                // ... medium: its wave issues at priority 1
    bool retired = false;               // the queue was empty when this lane last asked
    bool thin = false;                  // wave-uniform: this wave holds a long pixel and does not refill
    bool thin_counted = false;          // wave-uniform: this wave is included in the global thin-wave count
    bool long_done = false;             // the list of pre-classified long chains is exhausted
    // pre-classified long chains are honoured only while they are rare (<= 1/64 of the pixels): a scene made of long
    // chains only must keep its throughput.  The same value is read by every wave, so the decision is grid-wide.
    const unsigned int n_long_raw = A.long_list ? A.queue[2] : 0u, n_solo_raw = A.long_list ? A.queue[4] : 0u;
    const bool use_long = (n_long_raw + n_solo_raw) != 0u && (long long)(n_long_raw + n_solo_raw) * 64 <= n_slots;
    const unsigned int n_long = use_long ? n_long_raw : 0u, n_solo = use_long ? n_solo_raw : 0u;
    bool solo = false, solo_done = false;      // this wave started with one of the longest chains, alone (lane 0); that list is exhausted
    Rng s = {0, 0, 0, 0, 0, 0};
    V3 col = {0.0f, 0.0f, 0.0f};
    V3 att = {1.0f, 1.0f, 1.0f};
    float sum_l = 0.0f, sum_q = 0.0f;   // MODE 2, 3: the pixel's running luminance sum and sum of squares
    RayF r; r.o = {0.f, 0.f, 0.f}; r.d = {0.f, 1.f, 0.f};
    int sample = 0, depth = 0;
    int k0 = 0;                         // MODE 4: the samples the pixel had when this launch took it up
    bool live = false;
    RT_STATS_ONLY(
    unsigned int pix_iters = 0, pix_alone = 0;
    unsigned long long pix_t0 = 0;
    )

    // The next unclaimed slot.  render: one request to the global work counter per lane and pixel (a pixel is ns samples: requests are
    // rare, and the fine grain balances the frame's tail).  render_progressive hands out a pixel per lane and BOUNCE or so: 1.2 M
    // requests per C3 pass, one atomic per wave and iteration on one address — 0.3 ms of a 1.0 ms pass.  There a wave owns its first
    // kProgOwn slots outright (the counter's values start behind all waves' own slots) and then takes the rest in chunks of 64, at
    // the one place of the main loop where the wave is convergent (`refill_progressive`).
    constexpr bool kChunked = M::chunked;
    constexpr long long kProgOwn = RT_PROG_OWN;
    const long long first_free = (kChunked && kProgOwn > 0 && n_waves * kProgOwn <= n_slots) ? n_waves * kProgOwn : 0;
    long long pool_next = 0, pool_end = 0;              // wave-uniform: this wave's current chunk [pool_next, pool_end)
    if (kChunked && first_free > 0) { pool_next = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * kProgOwn; pool_end = pool_next + kProgOwn; }
    auto take_slot = [&]() -> long long {
        return first_free + (long long)atomicAdd(cold_args()->queue, 1u);
    };
    // claim `slot` (skipping slots that fall outside the frame in edge tiles) and set the lane up for that pixel
    auto begin_pixel = [&]() {
        live = false;
        const RenderArgs& A = *cold_args();
#ifdef RT_ONLY_LANE
        if (lane != RT_ONLY_LANE) return;                  // probe build: one pixel chain alone in its wave
#endif
        iters = 0; is_long = false; is_med = false;
        while (slot < n_slots) {
            if constexpr (M::listed) {
                // a resumed round: the list of the pixels still active, in any order (MODE 4: the seed's list, always there)
                const unsigned int* list = M::resumes ? refine_fused_list(A) : A.ad_list;
                if (M::resumes || list) {
                    const unsigned int pid = list[slot];
                    idx = (long long)pid; listed_pixel(A, pid, i, j);
                    live = true; break;
                }
            }
            // Slots are interleaved over blocks of 64 tiles (in hand-out order): consecutive slots are the same pixel
            // position of 64 different tiles, so the pixels of one tile (long chains cluster) never travel together.
            // The END of the queue is handed out per pixel, most expensive 2x2 pilot block first (k_tail_hist / k_tail_scatter): a launch with few pixels
            // per lane ends when its last-started pixels do, and inside a tile of a cheap class sit pixels of three times its mean.
            long long local_tile; int l;
            // On sparse grids that list is handed out FIRST (its first `head` entries, k_tail_scatter: all of it but the blocks outside the
            // frame), then the tiles, most expensive class first: C3 13.9 -> 13.2 ms, C2 10.4 -> 9.3 (rt_tuning.h RT_HEAD_SUM_SPARSE).
            const long long tail0 = (M::schedules && A.tail_list) ? (long long)A.queue[kQueueThr + 2] : 0;
            const long long head = tail0 > 0 ? (long long)A.queue[kQueueThr + 3] : 0;
            if (tail0 > 0 && (slot < head || slot >= tail0 - 1 + head)) {
                // (head taken from the list's cheap END — queue[kQueueThr + 5] — : the sky first, the rest of the list, most expensive first, last)
                const bool from_end = A.queue[kQueueThr + 5] != 0u;
                const long long n_tail = n_slots - (tail0 - 1);
                const long long k = slot < head ? (from_end ? n_tail - head + slot : slot) : (from_end ? slot - (tail0 - 1) - head : slot - (tail0 - 1));
                const unsigned int pid = A.tail_list[k];
                local_tile = (long long)(pid >> 6); l = (int)(pid & 63u);
            } else {
                // (slot_rank of rt_device.h, restated: with the call k_render<true,3,1> takes two other registers)
                constexpr int kIl = COOPG == 2 ? RT_INTERLEAVE_DENSE : (COOPG == 5 ? RT_INTERLEAVE_SOLO : RT_INTERLEAVE);   // tiles whose pixels interleave (consecutive slots: one pixel position of kIl tiles)
                // (k_tile_order starts the tail on a multiple of 64 tiles: a block of kIl tiles that straddled it would skip some pixels and render others twice)
                static_assert(kIl > 0 && 64 % kIl == 0, "RT_INTERLEAVE, RT_INTERLEAVE_DENSE and RT_INTERLEAVE_SOLO must divide 64 (the tail starts on a multiple of 64 tiles)");
                const long long ms = slot - head;                                  // the tiles' own slots
                const long long blk = ms / (64 * kIl);
                const long long tiles_in_blk = (A.n_local_tiles - blk * kIl) < kIl ? (A.n_local_tiles - blk * kIl) : kIl;
                const long long within = ms % (64 * kIl);
                const long long rank = blk * kIl + within % tiles_in_blk;          // position in the hand-out order
                l = (int)(within / tiles_in_blk);
                local_tile = A.order ? (long long)A.order[rank] : rank;
            }
            local_pixel(A, local_tile, l, i, j);
            const bool taken = use_long && A.long_flag[local_tile * 64 + l];      // long chains are handed out separately
            if (i < A.max_x && j < A.max_y && !taken) {
                idx = frame_whole(A) ? (long long)j * A.max_x + i : local_tile * 64 + l;      // (pixel_elem of rt_device.h, restated: the call changes k_render<*,1,*>'s registers)
                live = true;
                RT_STATS_ONLY(
                pix_t0 = __builtin_amdgcn_s_memrealtime();
                )
                break;
            }
            slot = take_slot();
        }
        if (!live) retired = true;
        if (live) {
            rng_load(s, A.rand_state + idx);
            col = {0.0f, 0.0f, 0.0f}; att = {1.0f, 1.0f, 1.0f}; sample = 0; depth = 0;
            if constexpr (M::sums && !M::resumes) { sum_l = 0.0f; sum_q = 0.0f; }
            if constexpr (M::resumes) {                           // where the state stands: k0 is one of the rounds' checkpoints, below max_spp
                const AdaptState K = adapt_state(fused_args(A).state, n_elems);
                const float* S = K.rgb + idx * 3;
                k0 = K.k[idx]; sample = k0;
                col.x = S[0]; col.y = S[1]; col.z = S[2]; sum_l = K.sl[idx]; sum_q = K.q[idx];
            }
            if constexpr (M::listed && !M::resumes) {
                if (A.ad_list) {
                    const float* f = (const float*)A.fb + idx * 3;
                    col.x = f[0]; col.y = f[1]; col.z = f[2]; sum_l = A.ad_sl[idx]; sum_q = A.ad_q[idx];
                }
            }
            r = primary_ray(A.scene.cam, i, j, A.max_x, A.max_y, s);
        }
    };
    // take the next pre-classified long chain, if any is left (lanes 0..RT_LONG_PER_WAVE-1 only)
    // (from_solo: the list of the chains that start one per wave, k_render<true,*,5>)
    auto begin_long_pixel = [&](bool from_solo) -> bool {
        if (!use_long || (from_solo ? solo_done : long_done)) return false;
        const RenderArgs& A = *cold_args();
        long long pid;
        if (from_solo) {
            const unsigned int h = atomicAdd(A.queue + 5, 1u);
            if (h >= n_solo) { solo_done = true; return false; }
            pid = (long long)A.long_list[n_slots - 1 - (long long)h];
        } else {
            const unsigned int h = atomicAdd(A.queue + 3, 1u);
            if (h >= n_long) { long_done = true; return false; }
            // the list is in the pilot's order, the four pixels of a 2x2 block and the blocks of a tile next to each other — and
            // neighbours are chains of like length: a stride (a prime that does not divide the count, so a permutation) puts
            // them into different waves, where each is left alone with its wave once the shorter ones have ended
            pid = (long long)A.long_list[long_list_at(h, n_long)];
        }
        const long long local_tile = pid >> 6;
        const int l = (int)(pid & 63);
        local_pixel(A, local_tile, l, i, j);
        idx = frame_whole(A) ? (long long)j * A.max_x + i : pid;                                   // (pixel_elem, restated as above)
        live = true; iters = 0; is_long = true;
        RT_STATS_ONLY(
        pix_t0 = __builtin_amdgcn_s_memrealtime();
        )
        rng_load(s, A.rand_state + idx);          // (begin_pixel's start, restated: one start_pixel for both changes every k_render's text in seven forms — HISTORY.md, round 30)
        col = {0.0f, 0.0f, 0.0f}; att = {1.0f, 1.0f, 1.0f}; sample = 0; depth = 0;
        if constexpr (M::sums) { sum_l = 0.0f; sum_q = 0.0f; }     // (long chains are listed in round 0 only: never reached by a pixel that resumes)
        r = primary_ray(A.scene.cam, i, j, A.max_x, A.max_y, s);
        return true;
    };
    // rand_state[pixel_index] = local_rand_state; fb[pixel_index] = ...  (main.cu:110-115 / :133-141)
    auto end_pixel = [&]() {
        const RenderArgs& A = *cold_args();
        rng_store(A.rand_state + idx, s);
        float* fb = (float*)A.fb + idx * 3;
        if constexpr (M::sums && !M::rule_in_lane) {
            fb[0] = col.x; fb[1] = col.y; fb[2] = col.z;                 // S_rgb: the check kernel divides and takes the root
            A.ad_sl[idx] = sum_l; A.ad_q[idx] = sum_q;
        } else if constexpr (M::rule_in_lane) {
            // what k_adapt_check / k_adapt_check_keep (rt_adaptive.hip) leave for a pixel that stops after `sample` samples
            // (MODE 4: what k_adapt_refine_check leaves; the state is never NULL there)
            const float kk = (float)(1.0 / (double)(float)sample);
            const FusedArgs F = fused_args(A);
            if (F.state) {
                const AdaptState K = adapt_state(F.state, part_elems(A));
                float* S = K.rgb + idx * 3;
                S[0] = col.x; S[1] = col.y; S[2] = col.z;
                K.sl[idx] = sum_l; K.q[idx] = sum_q; K.k[idx] = sample;
            }
            fb[0] = sqrtf(col.x * kk); fb[1] = sqrtf(col.y * kk); fb[2] = sqrtf(col.z * kk);
            if (F.spp) F.spp[idx] = sample;
        } else if (M::averages) {
            const float k = (float)(1.0 / (double)(float)A.ns);          // vec3::operator/=(real_t): 1.0/t in double (vec3.h:137)
            col.x *= k; col.y *= k; col.z *= k;
            fb[0] = sqrtf(col.x); fb[1] = sqrtf(col.y); fb[2] = sqrtf(col.z);
            // the measured pass: what this pixel cost, for the next launch of the same frame (a function of the pixel alone, not of the schedule)
            if constexpr (TREE && (COOPG == 4 || COOPG == 5)) { if (A.iters_out) A.iters_out[idx] = (unsigned short)(iters < 65535u ? iters : 65535u); }
            RT_STATS_ONLY(
            // diagnostic build: chain length and end / start time (100 MHz ticks mod 2^24) instead of colour
            fb[0] = (float)pix_iters; fb[1] = (float)((__builtin_amdgcn_s_memrealtime() >> 4) & 0xffffffull); fb[2] = (float)((pix_t0 >> 4) & 0xffffffull);
            if (idx < (1ll << 20)) { unsigned int* cd = g_chain_dbg + idx * 8 + 6; cd[0] = (unsigned int)pix_t0; cd[1] = pix_alone; }
            )
        } else {
            if (A.ns == 1) { fb[0] = col.x; fb[1] = col.y; fb[2] = col.z; }
            else { fb[0] += col.x; fb[1] += col.y; fb[2] += col.z; }
        }
    };
    RT_STATS_ONLY(
    Stats st; stats_clear(st);
    const unsigned long long tK0 = TICK(), rK0 = __builtin_amdgcn_s_memrealtime();
    unsigned int dbg_thin_iters = 0, dbg_long = 0;
    unsigned long long th[4] = {0, 0, 0, 0};
    unsigned long long dbg_thin_cyc = 0, dbg_thin_closest = 0, dbg_thin1_cyc = 0; unsigned int dbg_thin1_iters = 0; unsigned long long dbg_t_prev = TICK();
    )
    // start: pre-classified long chains first, RT_LONG_PER_WAVE per wave, in waves that are thin from the beginning
    // (the pre-classified chains alone in their waves: very sparse grids, whose pilot names them, and — <true,0,4> and <true,2,4>, which
    // share a context's record — sparse grids once a measured pass has: a pilot-made pass leaves n_solo = 0 there)
    constexpr bool kSolo = TREE && (COOPG == 5 || (COOPG == 4 && M::schedules));
    if (kSolo && n_solo != 0u && lane == 0 && begin_long_pixel(true)) solo = true;
    if (__ballot(live) == 0ull && lane < RT_LONG_PER_WAVE) begin_long_pixel(false);
    if (__ballot(live) != 0ull) { thin = true; __builtin_amdgcn_s_setprio(3); }
    // (every other lane takes its first pixel at the top of the loop: ONE inlined copy of the pixel switch, not three)

    const unsigned int thin_cap = (unsigned int)(n_waves / RT_THIN_CAP_DEN);
    float closest = FLT_MAX; int best = -1;
    TreeState ts; tree_state_init(ts);
    while (true) {
        // ---- wave-level bookkeeping (uniform)
        const unsigned long long m_live = __ballot(live);
        const unsigned long long m_long = __ballot(live && is_long);
        if (!thin && m_long != 0ull) {
            // try to become a thin wave; if the cap is reached these pixels simply stay ordinary
            unsigned int prev = 0;
            if (lane == 0) prev = atomicAdd(cold_args()->queue + 1, 1u);
            prev = __builtin_amdgcn_readfirstlane(prev);
            if (prev < thin_cap) { thin = true; thin_counted = true; __builtin_amdgcn_s_setprio(3); }       // the chain is on the critical path: win issue arbitration
            else { if (lane == 0) atomicSub(cold_args()->queue + 1, 1u); is_long = false; }
        } else if (thin && m_long == 0ull) {
            thin = false; __builtin_amdgcn_s_setprio(0);
            if (thin_counted && lane == 0) atomicSub(A.queue + 1, 1u);
            thin_counted = false;
        }
        if (RT_MED_RATE > 0 && !thin) { if (__ballot(live && is_med) != 0ull) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0); }
        if (!thin) {
            // idle lanes (their pixel ended while the wave was thin — or, progressive passes, in the previous iteration) go back to the queue
            if (kChunked) {
                const bool need = !live && !retired;
                const unsigned long long mneed = __ballot(need);
                if (mneed != 0ull) {
                    const long long n = (long long)__popcll(mneed);
                    const long long left = pool_end - pool_next;                 // what the current chunk still holds
                    const long long rank = (long long)rank_below(mneed);
                    long long fresh = 0;
                    if (n > left) {                                               // one more chunk for the wave (lane 0 asks)
                        unsigned int b = 0;
                        if (lane == 0) b = atomicAdd(cold_args()->queue, 64u);
                        fresh = first_free + (long long)__builtin_amdgcn_readfirstlane(b);
                    }
                    if (need) slot = rank < left ? pool_next + rank : fresh + (rank - left);
                    if (n > left) { pool_next = fresh + (n - left); pool_end = fresh + 64; } else pool_next += n;
                    if (need) begin_pixel();
                }
            } else if (!live && !retired) { slot = take_slot(); begin_pixel(); }
        }
        // thin implies a live long pixel; otherwise every lane that is not live has just found the queue empty
        if (__ballot(live) == 0ull) break;
        (void)m_live;
        STAT(st, ST_LOOP_ITERS_WAVE, 1);
        RT_STATS_ONLY(
        { const unsigned long long now = TICK(); const int nl2 = __popcll(__ballot(live));
          if (thin) { ++dbg_thin_iters; dbg_thin_cyc += now - dbg_t_prev; if (nl2 <= 2) { ++dbg_thin1_iters; dbg_thin1_cyc += now - dbg_t_prev; } }
          dbg_t_prev = now; }
        )
        RT_STATS_ONLY(
        { const int nl = __popcll(__ballot(live)); STAT(st, nl >= 56 ? ST_LIVE_GE56 : nl >= 32 ? ST_LIVE_32 : nl >= 8 ? ST_LIVE_8 : ST_LIVE_LT8, 1);
          WPASS_CLASS(nl >= 56 ? 0 : nl >= 32 ? 1 : nl >= 8 ? 2 : 3); }
        )
        const float a = dot3(r.d, r.d);
        if (!TREE) { closest = FLT_MAX; best = -1; }
        RT_STATS_ONLY(
        const unsigned long long tC0 = TICK();
        const unsigned long long c4_ = st.cyc[4], c5_ = st.cyc[5], c1_ = st.cyc[1], c3_ = st.cyc[3];
        const bool thin12 = thin && __popcll(__ballot(live)) <= 2;
        )
        if (TREE) closest_tree<COOPG>(A.scene, A.tree, s_nodes, r, a, live, closest, best, ts STAT_PASS);
        else closest_list(A.scene, r, a, live, closest, best);
        RT_STATS_ONLY(
        const unsigned long long tC1 = TICK(); st.cyc[0] += tC1 - tC0; st.cyc[2] += tC0; if (thin) dbg_thin_closest += tC1 - tC0;
        if (TREE && thin12) { th[0] += (st.cyc[4] - c4_) - tC0; th[1] += st.cyc[5] - c5_; th[2] += (st.cyc[1] - c1_) - (st.cyc[5] - c5_); th[3] += st.cyc[3] - c3_; }
        if (live) { ++pix_iters; if (__popcll(__ballot(live)) <= 2) ++pix_alone; }
        )
        if (live && !(TREE && ts.pending)) {
            ++iters;
            bool done;                                     // this sample's path has ended
            float lum = 0.0f;                              // MODE 2, 3, 4: (c.x + c.y) + c.z of the sample (0 for an absorbed path)
            if (best >= 0) {
                const bool cont = scatter(cold_args()->scene, best, closest, r, att, s);
                ++depth;
                done = !cont || depth >= 50;               // absorbed, or 50 bounces used up: contributes (0,0,0)
            } else {
                const V3 c = sky(r, att);
                col.x += c.x; col.y += c.y; col.z += c.z;
                if constexpr (M::sums) lum = (c.x + c.y) + c.z;
                done = true;
            }
            if (done) {
                if constexpr (M::sums) { sum_l += lum; sum_q += lum * lum; }
                (void)lum;
                ++sample; depth = 0; att = {1.0f, 1.0f, 1.0f};
                bool more = sample < ns;
                if constexpr (M::rule_in_lane) {                   // the checkpoints: base, base + batch, ... — base = min_spp, or k0 for a resumed pixel (never below it)
                    const FusedArgs F = fused_args(*cold_args());
                    const int base = M::resumes ? k0 : F.min_spp;
                    if (more && (M::resumes || sample >= base) && (unsigned int)(sample - base) % (unsigned int)F.batch == 0u)
                        more = !adapt_rule(sum_l, sum_q, sample, F.rel_error, F.floor);
                }
                if (more) {
                    RT_STATS_ONLY(
                    if (M::averages && idx < (1ll << 20) && (sample == ns / 3 || sample == 2 * (ns / 3))) {
                        unsigned int* cd = g_chain_dbg + idx * 8 + (sample == ns / 3 ? 0 : 3);
                        cd[0] = (unsigned int)__builtin_amdgcn_s_memrealtime(); cd[1] = pix_iters; cd[2] = pix_alone;
                    }
                    )
                    { const RenderArgs& C = *cold_args(); r = primary_ray(C.scene.cam, i, j, C.max_x, C.max_y, s); }
                    // classify after every 4th sample while enough of the chain is left for it to matter
                    // ... long from RT_LONG_RATE bounces per sample on, or — k_tile_order — when the chain this rate predicts (rate x ns) is a sizeable
                    // part of what ONE lane works through in this launch (queue[kQueueThr]; 0 when no scheduling pass ran)
                    bool now_long = false;
                    // (MODE 4: a resumed pixel's iters count this launch's bounces, so the rates are taken over this launch's samples)
                    const int taken = M::resumes ? sample - k0 : sample;
                    if ((taken & (RT_LONG_CHECK - 1)) == 0 && sample + 8 <= ns) {
                        const unsigned int long_thr = M::schedules ? cold_args()->queue[kQueueThr] : 0u;
                        // (MODE 3: the pass that set the threshold predicted a launch of min_spp samples a pixel — the chain is predicted for as many)
                        unsigned int thr_ns = (unsigned int)ns;
                        if constexpr (M::rule_in_lane && !M::resumes) thr_ns = (unsigned int)fused_args(*cold_args()).min_spp;
                        now_long = iters >= (unsigned int)((COOPG == 2 ? RT_LONG_RATE_DENSE : RT_LONG_RATE) * taken) ||
                                   (long_thr != 0u && (unsigned long long)iters * thr_ns >= (unsigned long long)long_thr * (unsigned int)taken);
                    }
                    if (now_long) {
                        RT_STATS_ONLY(
                        if (!is_long) ++dbg_long;
                        )
                        is_long = true;
                    }
                    else if (RT_MED_RATE > 0 && (taken & 7) == 0 && iters >= (unsigned int)(RT_MED_RATE * taken)) is_med = true;
                } else {
                    WPASS(WP_ENDPIX);
                    end_pixel();
                    RT_STATS_ONLY(
                    pix_iters = 0; pix_alone = 0;
                    )
                    STAT(st, ST_SWITCHES, 1);
                    live = false; is_long = false; is_med = false;
                    if (kSolo && solo && begin_long_pixel(true)) { /* the next of the longest chains, alone again */ }
                    else if (lane < RT_LONG_PER_WAVE && begin_long_pixel(false)) { solo = false; /* next long chain */ }
                    // (otherwise the lane refills at the top of the loop, before the next traversal: the one copy of take_slot + begin_pixel)
                }
            }
        }
    }

    RT_STATS_ONLY(
    for (int q = 0; q < ST_N; ++q) {
        const bool wave_level = (q == ST_LOOP_ITERS_WAVE || (q >= ST_LIVE_GE56 && q <= ST_LIVE_LT8));
        const bool lane_max = (q == ST_A_ITERS_WAVE || q == ST_B_ROUNDS_WAVE);       // single-wave probes: max over lanes = wave count
        if (lane_max) { int m = (int)st.c[q]; for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off)); if (lane == 0) atomicAdd(&g_stats[q], (unsigned long long)m); }
        else if (st.c[q] && (!wave_level || lane == 0)) atomicAdd(&g_stats[q], (unsigned long long)st.c[q]);
    }
    { int nl = (int)dbg_long; for (int off = 32; off > 0; off >>= 1) nl += __shfl_xor(nl, off); dbg_long = (unsigned int)nl; }
    if (lane == 0) {
        const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
        if (wv < 8192) {
            g_wave_dbg[wv * 4 + 0] = __builtin_amdgcn_s_memrealtime();
            g_wave_dbg[wv * 4 + 1] = st.c[ST_LOOP_ITERS_WAVE]; g_wave_dbg[wv * 4 + 2] = dbg_thin_iters; g_wave_dbg[wv * 4 + 3] = dbg_long;
            atomicAdd(&g_stats[TH_GROUND], th[0]); atomicAdd(&g_stats[TH_LARGE_SETUP], th[1]); atomicAdd(&g_stats[TH_WALK], th[2]); atomicAdd(&g_stats[TH_SCAN], th[3]);
            atomicAdd(&g_stats[ST_SPARE0], dbg_thin_cyc); atomicAdd(&g_stats[ST_SPARE1], dbg_thin_closest); atomicAdd(&g_stats[ST_SPARE2], dbg_thin1_cyc); atomicAdd(&g_stats[ST_SPARE3], (unsigned long long)dbg_thin1_iters); atomicAdd(&g_stats[ST_SPARE4], (unsigned long long)dbg_thin_iters);
        }
        atomicAdd(&g_stats[ST_SAMPLES], 1ull);
        const unsigned long long tot = TICK() - tK0;
        atomicAdd(&g_stats[ST_CYC_TOTAL], tot);
        atomicAdd(&g_stats[ST_CYC_CLOSEST], st.cyc[0]); atomicAdd(&g_stats[ST_CYC_WALK_A], st.cyc[1]); atomicAdd(&g_stats[ST_CYC_WALK_B], st.cyc[4] - st.cyc[2]);
        atomicAdd(&g_stats[ST_CYC_SCAN], st.cyc[3]); atomicAdd(&g_stats[ST_CYC_SHADE], tot - st.cyc[0]); atomicAdd(&g_stats[ST_SPARE4 + 1], st.cyc[5]); atomicAdd(&g_stats[ST_SPARE4 + 2], st.cyc[6]);
        atomicAdd(&g_stats[ST_REALTIME], __builtin_amdgcn_s_memrealtime() - rK0);
    }
    )
}

// ---------------------------------------------------------------------------------------------------- scheduling
// Longest-processing-time-first hand-out order for the persistent render kernel.  A pixel is a strictly serial chain
// (ns samples x bounces on one RNG stream); with only a few pixels per resident lane, a long chain picked up late keeps
// a nearly empty wave running.  k_tile_cost traces one PILOT sample per pixel on a private RNG stream and counts its
// bounces: the tile sums feed k_tile_order (rt_schedule.hip: 8 cost classes, most expensive first, stable), and pixels whose pilot path
// neighbourhood reaches RT_PILOT_LONG_SUM bounces (k_long_select, there too) are listed as long chains, which the render kernel starts first, in thin waves.
// All of this changes only WHICH lane renders a pixel and WHEN, never the pixel.
template <bool TREE, int COOPG = 1>
__global__ __launch_bounds__(256) void k_tile_cost(RenderArgs A, int* __restrict__ cost, unsigned char* __restrict__ pilot, int* __restrict__ work) {
    extern __shared__ float4 s_nodes[];
    if (TREE) stage_tree_fp32<COOPG != 1>(A.scene, A.tree, s_nodes);
    const int lane = threadIdx.x & 63;
    // quarter resolution: one pilot pixel per 2x2 block (long chains cluster), its RT_PILOT_SAMPLES samples in adjacent
    // lanes (the pass is as long as its longest serial chain); a wave covers 4 / RT_PILOT_SAMPLES tiles
    constexpr int kPerTile = 16 * RT_PILOT_SAMPLES, kTilesPerWave = 64 / kPerTile;
    static_assert(RT_PILOT_SAMPLES == 1 || RT_PILOT_SAMPLES == 2 || RT_PILOT_SAMPLES == 4, "pilot samples per pixel");
    const long long local_tile = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * kTilesPerWave + lane / kPerTile;
    const bool tile_ok = local_tile < A.n_local_tiles;
    int tx, ty; local_tile_xy(A, tile_ok ? local_tile : 0, tx, ty);
    const int sub = (lane % kPerTile) / RT_PILOT_SAMPLES, smp = lane % RT_PILOT_SAMPLES;
    const int lx = 2 * (sub & 3), ly = 2 * (sub >> 2);
    const int i = tile_px(tx, lx), j = tile_px(ty, ly);
    const bool inside = tile_ok && (i < A.max_x) && (j < A.max_y);
    // PILOT path: one sample per pixel on a private RNG stream (seeded away from the pixel's own 1984 + pixel_index
    // stream, which is not touched), same camera / closest-hit / scatter code as the render kernel; only the number
    // of bounces is kept.
    Rng ps; rng_seed(ps, 0x5deece66dull + (unsigned long long)((long long)j * A.max_x + i) + (unsigned long long)smp * 0x9e3779b97f4a7c15ull);
    RayF r; r.o = {0.f, 0.f, 0.f}; r.d = {0.f, 1.f, 0.f};
    V3 att = {1.0f, 1.0f, 1.0f};
    bool live = inside;
    if (live) r = primary_ray(A.scene.cam, i, j, A.max_x, A.max_y, ps);
    int bounces = 0;
    RT_STATS_ONLY(Stats st; stats_clear(st);)
    float closest = FLT_MAX; int best = -1;
    TreeState ts; tree_state_init(ts);
    int lane_iters = 0;          // passes of this loop the path was alive for: its bounces plus the passes a long walk stayed pending (quorum) — the lane-time it costs
    while (__ballot(live) != 0ull) {
        const float a = dot3(r.d, r.d);
        if (!TREE) { closest = FLT_MAX; best = -1; }
        if (TREE) closest_tree<COOPG>(A.scene, A.tree, s_nodes, r, a, live, closest, best, ts STAT_PASS);
        else closest_list(A.scene, r, a, live, closest, best);
        if (live) ++lane_iters;
        if (live && !(TREE && ts.pending)) {
            ++bounces;
            bool done = true;
            if (best >= 0) { const bool cont = scatter(A.scene, best, closest, r, att, ps); done = !cont || bounces >= RT_PILOT_CAP; }
            if (done) live = false;
        }
    }
    int pix = inside ? bounces : 0;
    for (int off = RT_PILOT_SAMPLES / 2; off > 0; off >>= 1) pix += __shfl_xor(pix, off);       // sum over the pixel's samples
    RT_STATS_ONLY(
    if (tile_ok && smp == 0 && local_tile * 16 + sub < (1 << 20)) g_pilot_dbg[local_tile * 16 + sub] = inside ? pix : -1;
    )
    if (pilot && tile_ok && smp == 0) pilot[local_tile * 16 + sub] = (unsigned char)(pix < 255 ? pix : 255);       // per 2x2 block, for k_long_select
    int w = inside ? bounces : 0;
    for (int off = kPerTile / 2; off > 0; off >>= 1) w += __shfl_xor(w, off);         // sum over the tile's 16 pilot pixels x samples
    if (lane % kPerTile == 0 && tile_ok) cost[local_tile] = w * 4;
    if (work) {                                                                       // (rt_split_balanced: what the tile's walks tested)
        int tw = inside ? (int)ts.work : 0;
        for (int off = kPerTile / 2; off > 0; off >>= 1) tw += __shfl_xor(tw, off);
        int tc = inside ? lane_iters : 0;
        for (int off = kPerTile / 2; off > 0; off >>= 1) tc += __shfl_xor(tc, off);
        if (lane % kPerTile == 0 && tile_ok) { work[local_tile] = tw; work[A.n_local_tiles + local_tile] = tc; }       // [tiles] tests, [tiles] lane passes
        (void)ts.cols;
    }
}

// the closest hit of one ray per lane, stored as an rt_hit_record (k_trace, k_guides): every lane of the block calls it, live or not
// (the tree walk is a wave-wide loop); the tree is already staged in s_nodes
template <bool TREE, int COOPG>
RT_DEV void trace_record(const RenderArgs& A, const float4* s_nodes, const RayF& r, bool live, rt_hit_record* out) {
    const DevScene& S = A.scene; const DevTree& T = A.tree;
    const float a = dot3(r.d, r.d);
    float closest = FLT_MAX; int best = -1;
    RT_STATS_ONLY(Stats st; stats_clear(st);)
    if (TREE) {
        TreeState ts; tree_state_init(ts);
        bool act = live;
        do { closest_tree<COOPG>(S, T, s_nodes, r, a, act, closest, best, ts STAT_PASS); act = live && ts.pending; } while (__ballot(act) != 0ull);
    } else closest_list(S, r, a, live, closest, best);
    if (!live) return;
    rt_hit_record h;
    h.sphere = best; h.t = 0.f; h.p[0] = h.p[1] = h.p[2] = 0.f; h.normal[0] = h.normal[1] = h.normal[2] = 0.f;
    if (best >= 0) {
        const float4 g = S.geom[best];
        h.t = closest;
        h.p[0] = r.o.x + closest * r.d.x; h.p[1] = r.o.y + closest * r.d.y; h.p[2] = r.o.z + closest * r.d.z;
        h.normal[0] = (h.p[0] - g.x) / g.w; h.normal[1] = (h.p[1] - g.y) / g.w; h.normal[2] = (h.p[2] - g.z) / g.w;
    }
    *out = h;
}

// hitTree / hitable_list::hit for a batch of rays (one lane per ray)
template <bool TREE, int COOPG = 1>
__global__ __launch_bounds__(256) void k_trace(RenderArgs A, const float* rays, long long n, rt_hit_record* out) {
    extern __shared__ float4 s_nodes[];
    if (TREE) stage_tree_fp32<COOPG != 1>(A.scene, A.tree, s_nodes);
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = gid < n;
    RayF r; r.o = {0.f, 0.f, 0.f}; r.d = {0.f, 1.f, 0.f};
    if (live) { const float* p = rays + gid * 6; r.o = {p[0], p[1], p[2]}; r.d = {p[3], p[4], p[5]}; }
    trace_record<TREE, COOPG>(A, s_nodes, r, live, out + gid);
}

// rt_render_guides: the first hit of every pixel's centre ray, row-major (pixel_index = j*max_x + i, one lane per pixel).  The ray is
// primary_ray's with both jitter draws replaced by 0.5 and no lens offset: a pinhole at the camera origin.
template <bool TREE, int COOPG = 1>
__global__ __launch_bounds__(256) void k_guides(RenderArgs A, long long n, rt_hit_record* out) {
    extern __shared__ float4 s_nodes[];
    if (TREE) stage_tree_fp32<COOPG != 1>(A.scene, A.tree, s_nodes);
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = gid < n;
    RayF r; r.o = {0.f, 0.f, 0.f}; r.d = {0.f, 1.f, 0.f};
    if (live) {
        const rt_camera& c = A.scene.cam;
        const int i = (int)(gid % A.max_x), j = (int)(gid / A.max_x);
        const float u = ((float)i + 0.5f) / (float)A.max_x;
        const float v = ((float)j + 0.5f) / (float)A.max_y;
        r.o = {c.origin[0], c.origin[1], c.origin[2]};
        r.d.x = ((c.lower_left_corner[0] + u * c.horizontal[0]) + v * c.vertical[0]) - c.origin[0];
        r.d.y = ((c.lower_left_corner[1] + u * c.horizontal[1]) + v * c.vertical[1]) - c.origin[1];
        r.d.z = ((c.lower_left_corner[2] + u * c.horizontal[2]) + v * c.vertical[2]) - c.origin[2];
    }
    trace_record<TREE, COOPG>(A, s_nodes, r, live, out + gid);
}

// ---------------------------------------------------------------------------------------------------- launchers
// LDS of a block of a tree variant's kernels: the nodes, then — pooled walks — one WalkLds per wave and the hot spheres
static size_t variant_lds_bytes(int n_nodes, int variant) {
    return (size_t)n_nodes * sizeof(DevNode) + (variant_pooled(variant) ? 4 * sizeof(WalkLds) + kHotSlots * sizeof(float4) : 0);
}

// blocks of the persistent grid of k_render<TREE, MODE, COOPG> for this launch: what the chip holds (resident_blocks), never more than the work
template <bool TREE, int MODE, int COOPG>
static unsigned grid_blocks(const RenderArgs& A, size_t lds) {
    const unsigned need = (unsigned)((A.n_local_tiles + 3) / 4);
    // the occupancy query costs as much host time as the launch: remembered per thread for the last (device, LDS size) —
    // a progressive loop issues the same launch hundreds of times
    thread_local int c_dev = -1; thread_local size_t c_lds = 0; thread_local unsigned c_cap = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = -2;
    if (dev != c_dev || lds != c_lds || c_cap == 0) { c_cap = resident_blocks((const void*)k_render<TREE, MODE, COOPG>, lds); c_dev = dev; c_lds = lds; }
    return need < c_cap ? need : c_cap;
}
template <bool TREE, int MODE, int COOPG>
static hipError_t launch_k_render(const RenderArgs& A, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL((k_render<TREE, MODE, COOPG>), dim3(grid_blocks<TREE, MODE, COOPG>(A, lds)), dim3(256), lds, st, A);
    return hipGetLastError();
}

// The TWO ladders from what a call chooses at run time to k_render's template arguments, each written once: f is called with a
// std::integral_constant<int, ...> and instantiates what it launches.
// with_walk: a tree variant (render_variant; never kVariantList) to COOPG.
template <class F> static auto with_walk(int variant, F&& f) {
    if (variant == kVariantSolo) return f(std::integral_constant<int, kVariantSolo>{});
    if (variant == kVariantSparse) return f(std::integral_constant<int, kVariantSparse>{});
    if (variant == kVariantDense) return f(std::integral_constant<int, kVariantDense>{});
    return f(std::integral_constant<int, kVariantTree>{});
}
// with_mode: a MODE of k_render to itself, cut to the modes this unit has — the contract unit emits k_render<*, 0|1, *> and nothing
// above.  A mode the unit does not have is hipErrorInvalidValue, never another mode's kernel.
template <class F> static hipError_t with_mode(int mode, F&& f) {
    if (mode == 0) return f(std::integral_constant<int, 0>{});
    if (mode == 1) return f(std::integral_constant<int, 1>{});
#ifndef RT_TU_CONTRACT
    if (mode == 2) return f(std::integral_constant<int, 2>{});
    if (mode == 3) return f(std::integral_constant<int, 3>{});
    if (mode == 4) return f(std::integral_constant<int, 4>{});
#endif
    return hipErrorInvalidValue;
}

// The hitable_list instantiations live in their own translation unit (rt_kernels_list.hip = this file with RT_TU_LIST):
// SLP vectorisation (packed fp32, v_pk_*_f32) makes the list scan 10 % faster and the tree walk 4 % slower on gfx950, so
// the two are compiled with different flags (Makefile).  The contract unit holds its own contracted k_render<false, 0|1, 1>.
#ifdef RT_TU_HAS_LIST
hipError_t launch_render_list(const RenderArgs& A, int mode, hipStream_t st) {
    return with_mode(mode, [&](auto m) { return launch_k_render<false, decltype(m)::value, 1>(A, 0, st); });
}
#ifndef RT_TU_CONTRACT
hipError_t launch_tile_cost_list(const RenderArgs& A, unsigned blocks, int* cost, unsigned char* pilot, hipStream_t st) {
    hipLaunchKernelGGL((k_tile_cost<false>), dim3(blocks), dim3(256), 0, st, A, cost, pilot, (int*)nullptr);
    return hipGetLastError();
}
hipError_t launch_trace_list(const RenderArgs& A, unsigned blocks, const float* rays, long long n, rt_hit_record* out, hipStream_t st) {
    hipLaunchKernelGGL((k_trace<false>), dim3(blocks), dim3(256), 0, st, A, rays, n, out);
    return hipGetLastError();
}
hipError_t launch_guides_list(const RenderArgs& A, unsigned blocks, long long n, rt_hit_record* out, hipStream_t st) {
    hipLaunchKernelGGL((k_guides<false>), dim3(blocks), dim3(256), 0, st, A, n, out);
    return hipGetLastError();
}
#endif
#endif

#ifndef RT_TU_LIST
// ---- the main unit and the contract unit: launch_render, the ONE render launcher a unit exports — k_render<TREE, MODE, COOPG> of the
// variant render_variant names, for every MODE (rt_device.h) the unit has: 0 rt_render, 1 rt_render_progressive, 2 a round of
// rt_render_adaptive, 3 rt_render_adaptive_fused (A.ns = max_spp; FusedArgs), 4 rt_render_adaptive_refine_fused (the list in A.iters_out)
hipError_t launch_render(const RenderArgs& A, bool tree, int mode, hipStream_t st) {
    if (A.n_local_tiles <= 0) return hipSuccess;
    const int variant = render_variant(tree, A.tree.acc);
    if (variant == kVariantList) return RT_TU_NAMESPACE::launch_render_list(A, mode, st);      // (qualified: the contract unit's own, not rt::'s that the argument's namespace offers too)
    const size_t lds = variant_lds_bytes(A.tree.n_nodes, variant);
    return with_mode(mode, [&](auto m) { return with_walk(variant, [&](auto w) { return launch_k_render<true, decltype(m)::value, decltype(w)::value>(A, lds, st); }); });
}
#endif

#ifdef RT_TU_MAIN
// ---- the main unit alone: k_render_init and the IEEE launchers
__global__ __launch_bounds__(256) void k_render_init(rt_rand_state* rand_state, int max_x, int max_y, int tiles_x, int part, int nparts, long long begin, long long end, long long n_local_tiles) {
    const int lane = threadIdx.x & 63;
    const long long local_tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (local_tile >= n_local_tiles) return;
    const AdaptFrame fr{max_x, max_y, tiles_x, part, nparts, begin, end};
    int i, j; local_pixel(fr, local_tile, lane, i, j);
    const bool inside = (i < max_x) && (j < max_y);
    const bool whole = frame_whole(fr);
    if (whole && !inside) return;
    const long long idx = pixel_elem(fr, i, j, local_tile, lane);
    const int pixel_index = j * max_x + i;
    Rng s; rng_seed(s, 1984ull + (unsigned long long)(long long)pixel_index);
    rt_rand_state out;
    rng_store(&out, s);
    out.boxmuller_flag = 0; out.boxmuller_flag_double = 0; out.boxmuller_extra = 0.f; out.pad_ = 0; out.boxmuller_extra_double = 0.0;
    rand_state[idx] = out;
}
hipError_t launch_render_init(rt_rand_state* rs, int max_x, int max_y, int part, int nparts, long long begin, long long end, hipStream_t st) {
    const int tiles_x = (max_x + 7) / 8, tiles_y = (max_y + 7) / 8;
    const long long tiles = (long long)tiles_x * tiles_y;
    const long long local = part_local_tiles(tiles, part, nparts, begin, end);
    if (local <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((local + 3) / 4);
    hipLaunchKernelGGL(k_render_init, dim3(blocks), dim3(256), 0, st, rs, max_x, max_y, tiles_x, part, nparts, begin, end, local);
    return hipGetLastError();
}

// blocks the chip holds at once for one kernel of the render path in blocks of 256 (occupancy query; grid_blocks and
// launch_render_h remember or repeat it): a persistent grid is never larger than that
unsigned resident_blocks(const void* kernel, size_t lds) {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 1024u;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 1024u;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, lds) != hipSuccess || per_cu <= 0) per_cu = 4;
    return (unsigned)(cus * per_cu);
}

// Which walk a call launches — the ONE place that decides (rt_variant.h names the variants and says what each implies): trees with a
// usable candidate grid take the pooled walk their grid's density asks for (rt_accel.h: coop_groups, solo_chains), every other tree
// the per-lane walk.  rt_render, rt_render_progressive, rt_render_adaptive, the pilot, k_trace and k_guides all walk the same way.
int render_variant(bool tree, const DevAccel& acc) {
    if (!tree) return kVariantList;
    if (acc.enabled) return acc.coop_groups >= 4 ? (acc.solo_chains ? kVariantSolo : kVariantSparse) : kVariantDense;
    return kVariantTree;
}

// "k_render<TREE,MODE,COOPG>" as rocprofv3 prints it, from one format; the strings live as long as the library
const char* render_kernel_name(bool tree, int mode, const DevAccel& acc) {
    struct Names {
        char s[5][kVariantSolo + 1][24];      // [mode][variant]
        Names() { for (int m = 0; m < 5; ++m) for (int v = 0; v <= kVariantSolo; ++v) snprintf(s[m][v], sizeof s[m][v], "k_render<%s,%d,%d>", v == kVariantList ? "false" : "true", m, v == kVariantList ? 1 : v); }
    };
    static const Names names;
    return names.s[mode >= 0 && mode < 5 ? mode : 1][render_variant(tree, acc)];
}

// the lanes of rt_render's persistent grid on a tree variant (the scheduling pass wants them before the launch)
static int render_grid_lanes(const RenderArgs& A, int variant) {
    return 256 * (int)with_walk(variant, [&](auto w) { return grid_blocks<true, 0, decltype(w)::value>(A, variant_lds_bytes(A.tree.n_nodes, variant)); });
}

// the pilot pass alone: per tile the bounces (x 4) and — trees with a candidate grid — the grid entries its samples' walks pooled
hipError_t launch_pilot(const RenderArgs& A, bool tree, int* cost, unsigned char* pilot, int* work, hipStream_t st) {
    if (A.n_local_tiles <= 0) return hipSuccess;
    const long long per_block = 4 * (64 / (16 * RT_PILOT_SAMPLES));       // a wave covers 4 / RT_PILOT_SAMPLES tiles
    const unsigned blocks = (unsigned)((A.n_local_tiles + per_block - 1) / per_block);
    const int variant = render_variant(tree, A.tree.acc);
    if (variant == kVariantList) return launch_tile_cost_list(A, blocks, cost, pilot, st);
    // (the pilot paths walk the grid like the render kernel's waves do, through the wave's pool)
    return with_walk(variant, [&](auto w) {
        hipLaunchKernelGGL((k_tile_cost<true, decltype(w)::value>), dim3(blocks), dim3(256), variant_lds_bytes(A.tree.n_nodes, variant), st, A, cost, pilot, work);
        return hipGetLastError();
    });
}

hipError_t launch_tile_order(const RenderArgs& A, bool tree, int* cost, unsigned int* order, unsigned char* flags, unsigned int* long_list, hipStream_t st) {
    if (A.n_local_tiles <= 0) return hipSuccess;
    // flags: 64 bytes per local tile (one per pixel) followed by 16 per local tile (the pilot counts per 2x2 block) and 16 more (k_long_select)
    unsigned char* pilot = flags ? flags + (size_t)A.n_local_tiles * 64 : nullptr;
    const int variant = render_variant(tree, A.tree.acc);
    const bool dense = variant_dense(variant);
    RenderArgs B = A;
    B.n_lanes = tree ? render_grid_lanes(A, variant) : 0;      // (list scans keep the rate rule alone)
    if (dense && A.f_inflight_dense > 0.f) B.f_inflight = A.f_inflight_dense;
    B.head_sum = dense ? A.head_sum_dense : A.head_sum;
    B.head_min_load = dense ? A.head_min_load : 0.f;
    { const hipError_t e = launch_pilot(A, tree, cost, pilot, nullptr, st); if (e != hipSuccess) return e; }
    // (chains in waves of their own: the variant for very sparse grids)
    return launch_select_and_order(B, cost, order, flags, long_list, st, 0, variant_solo_pilot(variant) ? RT_PILOT_SOLO_SUM : 0x7fffffff);
}

// the measured pass (rt_sched_keep.h "Feedback") of a launch on a variant that records counts: launch_tile_order with the recorded
// counts in the pilot's place.  extra: two words of the context ([0] the largest count, [1] the solo cap = waves / solo_cap_den).
hipError_t launch_count_order(const RenderArgs& A, const unsigned short* iters, int* cost, unsigned int* order, unsigned char* flags, unsigned int* long_list,
                              float solo_frac, int solo_cap_den, unsigned int* extra, hipStream_t st) {
    if (A.n_local_tiles <= 0) return hipSuccess;
    const int variant = render_variant(true, A.tree.acc);
    if (!variant_records_counts(variant) || !iters || !flags || !long_list) return hipErrorInvalidValue;
    RenderArgs B = A;
    B.n_lanes = render_grid_lanes(A, variant);
    B.head_sum = A.head_sum; B.head_min_load = 0.f;
    { const hipError_t e = launch_count_cost(B, iters, cost, flags + (size_t)A.n_local_tiles * 64, st); if (e != hipSuccess) return e; }
    const CountedSelect cs{iters, solo_frac, solo_cap_den > 0 ? (unsigned int)(B.n_lanes / 64 / solo_cap_den) : 0u, extra};
    return launch_select_and_order(B, cost, order, flags, long_list, st, 0, 0x7fffffff, &cs);
}

// What launch_trace and launch_guides share — n records, one lane each, in blocks of 256: list(blocks) launches the list scan's kernel,
// walk(w, blocks, lds) the tree kernel of the walk the render kernel would use for this tree (sparse grids: the pooled walk), so that
// per-ray parity checks cover it.
template <class L, class W>
static hipError_t launch_records(const DevTree& T, bool tree, long long n, L&& list, W&& walk) {
    if (n <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (!tree) return list(blocks);
    const int variant = render_variant(true, T.acc);
    return with_walk(variant, [&](auto w) { walk(w, blocks, variant_lds_bytes(T.n_nodes, variant)); return hipGetLastError(); });
}

hipError_t launch_trace(const DevScene& S, const DevTree& T, bool tree, const float* rays, long long n, rt_hit_record* out, hipStream_t st) {
    RenderArgs A{};
    A.scene = S; A.tree = T;
    return launch_records(T, tree, n, [&](unsigned blocks) { return launch_trace_list(A, blocks, rays, n, out, st); },
                          [&](auto w, unsigned blocks, size_t lds) { hipLaunchKernelGGL((k_trace<true, decltype(w)::value>), dim3(blocks), dim3(256), lds, st, A, rays, n, out); });
}

// the guides of a max_x x max_y frame (max_x * max_y < 2^31), launched as launch_trace launches k_trace: the same walk for every tree variant
hipError_t launch_guides(const DevScene& S, const DevTree& T, bool tree, int max_x, int max_y, rt_hit_record* out, hipStream_t st) {
    const long long n = (long long)max_x * max_y;
    RenderArgs A{};
    A.scene = S; A.tree = T; A.max_x = max_x; A.max_y = max_y;
    return launch_records(T, tree, n, [&](unsigned blocks) { return launch_guides_list(A, blocks, n, out, st); },
                          [&](auto w, unsigned blocks, size_t lds) { hipLaunchKernelGGL((k_guides<true, decltype(w)::value>), dim3(blocks), dim3(256), lds, st, A, n, out); });
}

RT_STATS_READERS
#endif

} // namespace RT_TU_NAMESPACE
