// ref_capi.cpp — C entry points over the REFERENCE's own headers, compiled as host C++17 (oracle/Makefile, target `ref`).
// Test infrastructure only: the libraries land in oracle/_ref/ (never committed) and are loaded through ctypes by
// tests/ref_lib.py, so that the CPU oracle (rt_oracle.hpp) can be held to what the reference's text computes.
//
// Everything numeric below happens inside the reference's functions: the constructors sphere / lambertian / metal / dielectric /
// camera, buildOctree, hitable_list::hit, hitTree, material::scatter, camera::get_ray.  This file only moves floats in and out.
// Nothing of main.cu is restated (no color, render or create_world); its own text is built by ref_main_capi.cpp.
// The build defines USE_FP16 or not, and puts a generated copy of acceleration_structure.h, in which only the SPHERES_PER_LEAF
// line differs, first on the include path (that header has a hard #define).
//
// Layout of the arrays: the oracle's (rt_oracle_capi.cpp): geom N x (cx, cy, cz, r), mat N x (albedo rgb, param), kind N
// (0 lambertian, 1 metal, 2 dielectric, -1 ghost slot); cameras are the 22 floats of camera.h:51-56; RNG states are 48 bytes.
#include <cstdint>
#include <cstring>
#include <new>
#include <unistd.h>
#include <unordered_map>
#include <float.h>
#include <curand_kernel.h>
#include "vec3.h"
#include "ray.h"
#include "sphere.h"
#include "hitable_list.h"
#include "camera.h"
#include "material.h"
#include "precision_types.h"
#include "acceleration_structure.h"
#undef pow
#undef tan

namespace {

inline real_t R(float f) { return real_t(f); }
inline float F(real_t x) { return float(x); }
inline vec3 V(const float* f) { return vec3(R(f[0]), R(f[1]), R(f[2])); }
inline void put(float* o, const vec3& v) { o[0] = F(v.e[0]); o[1] = F(v.e[1]); o[2] = F(v.e[2]); }

struct ref_world {
    int n = 0;
    sphere* spheres = nullptr;          // zeroed memory, every slot placement-constructed
    hitable** list = nullptr;
    hitable_list* hl = nullptr;
    hitable* world = nullptr;           // *world is the hitable_list, as main.cu hands it to hitTree
    Octree* tree = nullptr;
    int64_t dropped_full = 0, dropped_outside = 0;
    std::unordered_map<const material*, int> index_of;
};

int sphere_of(const ref_world* W, const material* m) {
    if (!m) return -2;                  // a ghost slot's record: reported, never dereferenced
    auto it = W->index_of.find(m);
    return it == W->index_of.end() ? -3 : it->second;
}

ray ray_of(const float* f) { return ray(V(f), V(f + 3)); }

hit_record rec_of(const ref_world* W, int sph, const float* f) {
    hit_record rec;
    rec.t = R(f[0]); rec.p = V(f + 1); rec.normal = V(f + 4); rec.mat_ptr = W->spheres[sph].mat_ptr;
    return rec;
}

}  // namespace

extern "C" {

// [0] 1 if built with USE_FP16, [1] SPHERES_PER_LEAF, [2] sizeof(sphere), [3] sizeof(curandState)
void ref_build_info(int32_t* out) {
#ifdef USE_FP16
    out[0] = 1;
#else
    out[0] = 0;
#endif
    out[1] = SPHERES_PER_LEAF; out[2] = (int32_t)sizeof(sphere); out[3] = (int32_t)sizeof(curandState);
}

void* ref_world_create(int n, const float* geom, const float* mat, const int32_t* kind) {
    ref_world* W = new ref_world();
    W->n = n;
    W->spheres = (sphere*)std::calloc((size_t)n, sizeof(sphere));
    W->list = new hitable*[n];
    for (int i = 0; i < n; ++i) {
        const float* g = geom + (size_t)i * 4;
        const float* m = mat + (size_t)i * 4;
        material* mp = nullptr;
        if (kind[i] == 0) mp = new lambertian(V(m));
        else if (kind[i] == 1) mp = new metal(V(m), R(m[3]));
        else if (kind[i] == 2) mp = new dielectric(R(m[3]));
        if (mp) { new (&W->spheres[i]) sphere(V(g), R(g[3]), mp); W->index_of[mp] = i; }
        else new (&W->spheres[i]) sphere(vec3(0, 0, 0), 0, nullptr);      // ghost slot: zeroed memory with a valid vptr
        W->list[i] = &W->spheres[i];
    }
    W->hl = new hitable_list(W->list, n);
    W->world = W->hl;
    return W;
}

void ref_world_destroy(void* h) {
    ref_world* W = (ref_world*)h;
    for (auto& kv : W->index_of) ::operator delete((void*)kv.first);      // the materials are trivially destructible
    delete W->tree; delete W->hl; delete[] W->list; std::free(W->spheres);
    delete W;
}

// buildOctree.  out: [0] nodeCount [1] leafCount [2] insertions dropped because the buckets were full [3] spheres outside the root box.
// The reference only prints one line per dropped insertion: the lines are counted (stdout goes to a temporary file meanwhile), and
// the spheres that its own intersects() puts outside the root box are told apart from them.
void ref_build_octree(void* h, int64_t* out) {
    ref_world* W = (ref_world*)h;
    delete W->tree;
    std::fflush(stdout);
    const int saved = dup(1);
    FILE* tmp = std::tmpfile();
    dup2(fileno(tmp), 1);
    W->tree = buildOctree(W->spheres, W->n);
    std::fflush(stdout);
    dup2(saved, 1);
    close(saved);
    std::rewind(tmp);
    int64_t lines = 0;
    for (int c; (c = std::fgetc(tmp)) != EOF;) lines += c == '\n';
    std::fclose(tmp);
    int64_t outside = 0;
    for (int i = 1; i < W->n; ++i) outside += !intersects(W->spheres[i], W->tree->nodes[0].aabb);
    W->dropped_outside = outside; W->dropped_full = lines - outside;
    out[0] = W->tree->nodeCount; out[1] = W->tree->leafCount; out[2] = W->dropped_full; out[3] = W->dropped_outside;
}

// level[585], box[585 * 6], children[585 * 8]: every node of the array, used or not (new Octree() zero-fills the unused ones)
void ref_octree_nodes(void* h, int32_t* level, float* box, int32_t* children) {
    const Octree* T = ((ref_world*)h)->tree;
    for (int i = 0; i < NUMBER_NODES; ++i) {
        const OctNode& n = T->nodes[i];
        level[i] = n.level;
        const real_t b[6] = {n.aabb.x_low, n.aabb.y_low, n.aabb.z_low, n.aabb.x_high, n.aabb.y_high, n.aabb.z_high};
        for (int k = 0; k < 6; ++k) box[i * 6 + k] = F(b[k]);
        for (int k = 0; k < 8; ++k) children[i * 8 + k] = n.children[k];
    }
}

// counts[leafCount], indices[leafCount * SPHERES_PER_LEAF], the leaf array as it stands
void ref_octree_leaves(void* h, int32_t* counts, int32_t* indices) {
    const Octree* T = ((ref_world*)h)->tree;
    for (int l = 0; l < T->leafCount; ++l) {
        counts[l] = T->leaves[l].index_count;
        for (int k = 0; k < SPHERES_PER_LEAF; ++k) indices[(size_t)l * SPHERES_PER_LEAF + k] = T->leaves[l].sphere_indices[k];
    }
}

// closest hit of n rays (6 floats each).  mode 1: hitable_list::hit(r, 0.001f, FLT_MAX) as main.cu:54 calls it; mode 2: hitTree.
// sph: the sphere whose mat_ptr the record carries; -2 where that pointer is null (a ghost slot was hit).
void ref_trace(void* h, int64_t n, const float* rays, int mode, int32_t* hit, int32_t* sph, float* t, float* p, float* nrm) {
    ref_world* W = (ref_world*)h;
    for (int64_t i = 0; i < n; ++i) {
        const ray r = ray_of(rays + i * 6);
        hit_record rec;
        rec.mat_ptr = nullptr;
        const bool got = mode == 2 ? hitTree(W->tree, r, rec, &W->world) : W->world->hit(r, 0.001f, FLT_MAX, rec);
        hit[i] = got ? 1 : 0; sph[i] = got ? sphere_of(W, rec.mat_ptr) : -1; t[i] = got ? F(rec.t) : 0.f;
        for (int k = 0; k < 3; ++k) { p[i * 3 + k] = got ? F(rec.p.e[k]) : 0.f; nrm[i * 3 + k] = got ? F(rec.normal.e[k]) : 0.f; }
    }
}

// material::scatter of sphere sph[i] for n bounces: ray 6 floats, record 7 floats (t, p, normal), state 48 bytes (advanced in place).
// ret: the return value; -1 where the sphere has no material (nothing is called).
void ref_scatter(void* h, int64_t n, const int32_t* sph, const float* rays, const float* recs, void* states, int32_t* ret, float* att, float* out) {
    ref_world* W = (ref_world*)h;
    for (int64_t i = 0; i < n; ++i) {
        const material* m = W->spheres[sph[i]].mat_ptr;
        if (!m) { ret[i] = -1; continue; }
        const ray r = ray_of(rays + i * 6);
        const hit_record rec = rec_of(W, sph[i], recs + i * 7);
        curandState st;
        std::memcpy(&st, (const char*)states + i * 48, 48);
        vec3 a(0, 0, 0);
        ray sc(vec3(0, 0, 0), vec3(0, 0, 0));
        ret[i] = m->scatter(r, rec, a, sc, &st) ? 1 : 0;
        std::memcpy((char*)states + i * 48, &st, 48);
        put(att + i * 3, a); put(out + i * 6, sc.A); put(out + i * 6 + 3, sc.B);
    }
}

// A WITNESS for the tests, not a result: which way a dielectric bounce went, asked of the reference's own refract() and reflect()
// (material.h:17, :43) with the operands dielectric::scatter gives them.  bit 0: the ray leaves the sphere (dot(direction, normal) > 0);
// bit 1: refract() succeeded; bit 2: the scattered direction is reflect(direction, normal), bit for bit.
void ref_dielectric_branch(void* h, int64_t n, const int32_t* sph, const float* rays, const float* recs, const float* scattered, int32_t* out) {
    ref_world* W = (ref_world*)h;
    for (int64_t i = 0; i < n; ++i) {
        const dielectric* m = (const dielectric*)W->spheres[sph[i]].mat_ptr;
        const ray r = ray_of(rays + i * 6);
        const hit_record rec = rec_of(W, sph[i], recs + i * 7);
        const bool leaves = dot(r.direction(), rec.normal) > real_t(0.0f);
        vec3 refracted(0, 0, 0);
        const bool ok = leaves ? refract(r.direction(), -rec.normal, m->ref_idx, refracted)
                               : refract(r.direction(), rec.normal, real_t(1.0f) / m->ref_idx, refracted);
        float want[3], got[3];
        put(want, reflect(r.direction(), rec.normal));
        put(got, V(scattered + i * 6 + 3));
        out[i] = (leaves ? 1 : 0) | (ok ? 2 : 0) | (std::memcmp(want, got, 12) == 0 ? 4 : 0);
    }
}

// camera::camera.  args: lookfrom 3, lookat 3, vup 3, vfov, aspect, aperture, focus_dist.  out: the 22 floats.
void ref_camera(const float* a, float* out) {
    const camera c(V(a), V(a + 3), V(a + 6), R(a[9]), R(a[10]), R(a[11]), R(a[12]));
    put(out, c.origin); put(out + 3, c.lower_left_corner); put(out + 6, c.horizontal); put(out + 9, c.vertical);
    put(out + 12, c.u); put(out + 15, c.v); put(out + 18, c.w); out[21] = F(c.lens_radius);
}

// camera::get_ray(s[i], t[i]) of the camera given by its 22 floats, n times, each from its own 48-byte state
void ref_get_ray(const float* cam, int64_t n, const float* s, const float* t, void* states, float* rays) {
    camera c(vec3(0, 0, 1), vec3(0, 0, 0), vec3(0, 1, 0), 30, 1, 0, 1);
    c.origin = V(cam); c.lower_left_corner = V(cam + 3); c.horizontal = V(cam + 6); c.vertical = V(cam + 9);
    c.u = V(cam + 12); c.v = V(cam + 15); c.w = V(cam + 18); c.lens_radius = R(cam[21]);
    for (int64_t i = 0; i < n; ++i) {
        curandState st;
        std::memcpy(&st, (const char*)states + i * 48, 48);
        const ray r = c.get_ray(R(s[i]), R(t[i]), &st);
        std::memcpy((char*)states + i * 48, &st, 48);
        put(rays + i * 6, r.A); put(rays + i * 6 + 3, r.B);
    }
}

// curand_init(seed[i], 0, 0) into zeroed 48-byte states; one curand_uniform from each state
void ref_curand_init(int64_t n, const uint64_t* seed, void* states) {
    std::memset(states, 0, (size_t)n * 48);
    for (int64_t i = 0; i < n; ++i) {
        curandState st;
        std::memset(&st, 0, sizeof st);
        curand_init(seed[i], 0, 0, &st);
        std::memcpy((char*)states + i * 48, &st, 48);
    }
}
void ref_curand_uniform(int64_t n, void* states, float* out) {
    for (int64_t i = 0; i < n; ++i) {
        curandState st;
        std::memcpy(&st, (const char*)states + i * 48, 48);
        out[i] = curand_uniform(&st);
        std::memcpy((char*)states + i * 48, &st, 48);
    }
}

}  // extern "C"
