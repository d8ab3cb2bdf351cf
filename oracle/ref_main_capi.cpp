// ref_main_capi.cpp — C entry points over the text of the REFERENCE's main.cu above `int main(`, compiled as host C++17
// (oracle/Makefile, target `ref`).  Test infrastructure only: the libraries land in oracle/_ref/ (never committed) and are loaded
// through ctypes by tests/ref_lib.py, so that the CPU oracle's restated loops (rt_oracle.hpp: create_world, render_init, render,
// render_progressive, color, write_ppm) can be held to what the reference's own text computes.
//
// main_body.inc is the generated file: main.cu from its first line up to `int main(`, with only the NUM_SPHERES and SPHERE_RADIUS values
// and the presence of `#define USE_OCTREE` changed (all three are hard #defines there).  It is included below, whole.  A kernel
// "launch" is a plain call with the launch coordinates of ref_shim/cuda_launch.h set first, one thread per call.
//
// Everything numeric happens inside the reference's functions: rand_init, create_world, buildOctree, render_init, render,
// render_progressive (and through them color, get_ray, hit, scatter), output_to_stream.  This file only moves data in and
// out; no loop body of the reference is restated.  The list handed to create_world is zeroed memory, as the slots it leaves unwritten
// are defined to be: spheres of radius 0 at the origin with a null mat_ptr.  In binary32 no ray hits one.  In
// USE_FP16 some do, and color() (main.cu:59) then calls through the null pointer: the reference has no result there.  So that such a
// frame can still be run, every null mat_ptr is pointed at a ghost_witness after create_world: a material of this file that only
// notes that it was reached.  The pixels whose call reached it are reported (ghost[]) and are no part of any comparison.
//
// Layout of the arrays: the oracle's (rt_oracle_capi.cpp): geom N x (cx, cy, cz, r), mat N x (albedo rgb, param), kind N
// (0 lambertian, 1 metal, 2 dielectric, -1 ghost slot); cameras are the 22 floats of camera.h:51-56; RNG states are 48 bytes;
// frames are floats, rows x nx x 3 (in USE_FP16 the exact values of the binary16 frame).
#include <cstdint>
#include <cstring>
#include <sstream>
#include <unistd.h>
#include "cuda_launch.h"
#include "main_body.inc"
#undef pow
#undef tan

namespace {

inline real_t R(float f) { return real_t(f); }
inline float F(real_t x) { return float(x); }
inline vec3 V(const float* f) { return vec3(R(f[0]), R(f[1]), R(f[2])); }
inline void put(float* o, const vec3& v) { o[0] = F(v.e[0]); o[1] = F(v.e[1]); o[2] = F(v.e[2]); }

struct main_scene {
    int nx = 0, ny = 0;
    sphere (*list)[NUM_SPHERES] = nullptr;      // zeroed memory, written by create_world
    hitable* world = nullptr;
    camera* cam = nullptr;
    curandState world_rng;                      // rand_init's state, advanced by create_world
    Octree* tree = nullptr;
};

bool ghost_reached = false;
struct ghost_witness : material {
    bool scatter(const ray&, const hit_record&, vec3&, ray&, curandState*) const override { ghost_reached = true; return false; }
};

void at_pixel(int i, int j) { threadIdx = {0, 0, 0}; blockDim = dim3(1, 1, 1); blockIdx = {(unsigned)i, (unsigned)j, 0}; }

// the frame rows [row0, row0 + rows) as the reference's vec3 array, indexed by the kernels as j * nx + i
struct rows_of {
    vec3* own;
    size_t n;
    float* io;
    rows_of(float* fb, int nx, int rows) : own(new vec3[(size_t)nx * rows]), n((size_t)nx * rows), io(fb) {
        for (size_t k = 0; k < n; ++k) own[k] = V(io + k * 3);
    }
    ~rows_of() {
        for (size_t k = 0; k < n; ++k) put(io + k * 3, own[k]);
        delete[] own;
    }
};

}  // namespace

extern "C" {

// [0] 1 if built with USE_FP16, [1] NUM_SPHERES, [2] 1 if USE_OCTREE, [3] SPHERES_PER_LEAF, [4] sizeof(curandState); radius: SPHERE_RADIUS
void refmain_build_info(int32_t* out, float* radius) {
#ifdef USE_FP16
    out[0] = 1;
#else
    out[0] = 0;
#endif
    out[1] = NUM_SPHERES;
#ifdef USE_OCTREE
    out[2] = 1;
#else
    out[2] = 0;
#endif
    out[3] = SPHERES_PER_LEAF; out[4] = (int32_t)sizeof(curandState);
    *radius = SPHERE_RADIUS;
}

// rand_init<<<1, 1>>> + create_world<<<1, 1>>>(d_list, d_world, d_camera, nx, ny, d_rand_state2)
void* refmain_create(int nx, int ny) {
    main_scene* S = new main_scene();
    S->nx = nx; S->ny = ny;
    S->list = (sphere(*)[NUM_SPHERES])std::calloc(NUM_SPHERES, sizeof(sphere));
    std::memset(&S->world_rng, 0, sizeof S->world_rng);
    at_pixel(0, 0);
    rand_init(&S->world_rng);
    create_world(S->list, &S->world, &S->cam, nx, ny, &S->world_rng);
    for (int i = 0; i < NUM_SPHERES; ++i)
        if (!(*S->list)[i].mat_ptr) (*S->list)[i].mat_ptr = new ghost_witness();
    return S;
}

// what free_world frees, freed here: free_world (compiled above, never called) deletes the materials through `material*`, a base
// without a virtual destructor, which a sized operator delete must not be handed.  The materials are trivially destructible.
void refmain_destroy(void* h) {
    main_scene* S = (main_scene*)h;
    for (int i = 0; i < NUM_SPHERES; ++i) ::operator delete((void*)(*S->list)[i].mat_ptr);
    hitable_list* world = (hitable_list*)S->world;
    delete[] world->list;
    ::operator delete((void*)world);
    delete S->cam;
    delete S->tree;
    std::free(S->list);
    delete S;
}

// the list create_world wrote; a slot it left unwritten (no material) is kind -1
void refmain_spheres(void* h, float* geom, float* mat, int32_t* kind) {
    main_scene* S = (main_scene*)h;
    for (int i = 0; i < NUM_SPHERES; ++i) {
        const sphere& s = (*S->list)[i];
        put(geom + i * 4, s.center); geom[i * 4 + 3] = F(s.radius);
        float* m = mat + i * 4;
        m[0] = m[1] = m[2] = m[3] = 0.f;
        if (dynamic_cast<const ghost_witness*>(s.mat_ptr)) kind[i] = -1;
        else if (const lambertian* l = dynamic_cast<const lambertian*>(s.mat_ptr)) { kind[i] = 0; put(m, l->albedo); }
        else if (const metal* t = dynamic_cast<const metal*>(s.mat_ptr)) { kind[i] = 1; put(m, t->albedo); m[3] = F(t->fuzz); }
        else if (const dielectric* d = dynamic_cast<const dielectric*>(s.mat_ptr)) { kind[i] = 2; m[3] = F(d->ref_idx); }
        else kind[i] = -3;
    }
}

void refmain_world_rng(void* h, void* out48) { std::memcpy(out48, &((main_scene*)h)->world_rng, 48); }

void refmain_camera(void* h, float* out) {
    const camera& c = *((main_scene*)h)->cam;
    put(out, c.origin); put(out + 3, c.lower_left_corner); put(out + 6, c.horizontal); put(out + 9, c.vertical);
    put(out + 12, c.u); put(out + 15, c.v); put(out + 18, c.w); out[21] = F(c.lens_radius);
}

// overwrites the camera's public fields (camera.h:51-56): in USE_FP16 the host build can only take the host branch of camera::camera
void refmain_set_camera(void* h, const float* cam) {
    camera& c = *((main_scene*)h)->cam;
    c.origin = V(cam); c.lower_left_corner = V(cam + 3); c.horizontal = V(cam + 6); c.vertical = V(cam + 9);
    c.u = V(cam + 12); c.v = V(cam + 15); c.w = V(cam + 18); c.lens_radius = R(cam[21]);
}

// buildOctree(cpu_spheres, NUM_SPHERES) on create_world's list, as main() calls it.  out as ref_capi.cpp's ref_build_octree:
// [0] nodeCount [1] leafCount [2] insertions dropped because the buckets were full [3] spheres outside the root box (counted
// from the lines the reference prints; stdout goes to a temporary file meanwhile)
void refmain_build_octree(void* h, int64_t* out) {
    main_scene* S = (main_scene*)h;
    delete S->tree;
    std::fflush(stdout);
    const int saved = dup(1);
    FILE* tmp = std::tmpfile();
    dup2(fileno(tmp), 1);
    S->tree = buildOctree(*S->list, NUM_SPHERES);
    std::fflush(stdout);
    dup2(saved, 1);
    close(saved);
    std::rewind(tmp);
    int64_t lines = 0;
    for (int c; (c = std::fgetc(tmp)) != EOF;) lines += c == '\n';
    std::fclose(tmp);
    int64_t outside = 0;
    for (int i = 1; i < NUM_SPHERES; ++i) outside += !intersects((*S->list)[i], S->tree->nodes[0].aabb);
    out[0] = S->tree->nodeCount; out[1] = S->tree->leafCount; out[2] = lines - outside; out[3] = outside;
}

// render_init<<<blocks, threads>>>(nx, ny, d_rand_state) for the rows [row0, row0 + rows): states rows x nx x 48 bytes
void refmain_render_init(int nx, int ny, int row0, int rows, void* states) {
    curandState* st = (curandState*)states - (ptrdiff_t)row0 * nx;
    for (int j = row0; j < row0 + rows; ++j)
        for (int i = 0; i < nx; ++i) { at_pixel(i, j); render_init(nx, ny, st); }
}

// render<<<blocks, threads>>>(fb, nx, ny, ns, d_camera, d_world, d_rand_state, d_octree, d_list) for the rows [row0, row0 + rows).
// ghost: rows x nx bytes, set to 1 where the pixel's call reached a ghost slot's witness (left as they are elsewhere)
void refmain_render(void* h, float* fb, int ns, int row0, int rows, void* states, uint8_t* ghost) {
    main_scene* S = (main_scene*)h;
    rows_of buf(fb, S->nx, rows);
    vec3* f = buf.own - (ptrdiff_t)row0 * S->nx;
    curandState* st = (curandState*)states - (ptrdiff_t)row0 * S->nx;
    for (int j = row0; j < row0 + rows; ++j)
        for (int i = 0; i < S->nx; ++i) {
            at_pixel(i, j);
            ghost_reached = false;
            render(f, S->nx, S->ny, ns, &S->cam, &S->world, st, S->tree, S->list);
            if (ghost_reached) ghost[(size_t)(j - row0) * S->nx + i] = 1;
        }
}

// render_progressive<<<blocks, threads>>>(fb, nx, ny, current_sample, ...) for the rows [row0, row0 + rows): fb goes in and out
void refmain_render_progressive(void* h, float* fb, int current_sample, int row0, int rows, void* states, uint8_t* ghost) {
    main_scene* S = (main_scene*)h;
    rows_of buf(fb, S->nx, rows);
    vec3* f = buf.own - (ptrdiff_t)row0 * S->nx;
    curandState* st = (curandState*)states - (ptrdiff_t)row0 * S->nx;
    for (int j = row0; j < row0 + rows; ++j)
        for (int i = 0; i < S->nx; ++i) {
            at_pixel(i, j);
            ghost_reached = false;
            render_progressive(f, S->nx, S->ny, current_sample, &S->cam, &S->world, st, S->tree, S->list);
            if (ghost_reached) ghost[(size_t)(j - row0) * S->nx + i] = 1;
        }
}

// output_to_stream(ostream, nx, ny, fb): the bytes; returns their number, copies at most cap of them
int64_t refmain_ppm(float* fb, int nx, int ny, char* out, int64_t cap) {
    std::ostringstream os;
    {
        rows_of buf(fb, nx, ny);
        output_to_stream(os, nx, ny, buf.own);
    }
    const std::string s = os.str();
    if (out) std::memcpy(out, s.data(), (size_t)(cap < (int64_t)s.size() ? cap : (int64_t)s.size()));
    return (int64_t)s.size();
}

}  // extern "C"
