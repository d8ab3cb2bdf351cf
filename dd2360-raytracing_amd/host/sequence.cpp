// sequence.cpp — rt_sequence: an animation rendered end to end on ONE resident world, every stage of the frame loop in the order an
// integrator calls them (INTEGRATION.md "Temporal accumulation over an animation"): move the spheres and the camera, build the tree
// again, guides, adaptive begin, a history-aware budget, rectified temporal accumulation, the history filter, 8-bit levels, one copy
// of 3 bytes a pixel to the host.  mode=progressive is the reference's pass-by-pass viewer (main.cu:222-318, output mode 2) without
// the window: one sample a pass, every `every`-th pass filtered, quantised and written.
//
// A second host program on top of include/rt_amd.h: every render step goes through the C-ABI, nothing is added to it.  The two kernels
// here are the viewer's own: k_animate writes a frame's geometry from the created list by the rule of rt_sequence_motion.hpp, k_upscale
// (upscale > 1) the shown frame from a smaller rendered one by the rule of rt_sequence_upscale.hpp.
// Errors follow rt_main: a message on stderr and exit code 99.  Arguments are key=value tokens in any order; an unknown key, a
// malformed value or a refused combination ends the program BEFORE rt_device_check, so no device is touched.
//
//   mode            animation | progressive                                                            (animation)
//   n nx ny spl radius   NUM_SPHERES, frame size, SPHERES_PER_LEAF, SPHERE_RADIUS of rt_main            (500 64 40 30 0.1)
//   frames          animation: number of frames, >= 1                                                  (4)
//   min_spp max_spp batch rel_error floor   the rt_adaptive of every frame                             (4 8 4 0 0)
//   adaptive        animation: rounds = rt_render_adaptive_begin (round 0, then a launch and a check a batch); fused = the same frame
//                   and state from rt_render_adaptive_fused, one launch with the stop rule inside.  The frames are the same byte
//                   for byte; the `begin` line of timing=1 shows the difference                        (rounds)
//   budget rounds   extra samples a frame = budget * nx * ny, spent by rt_render_adaptive_spend_temporal in `rounds` rounds of
//                   `batch` samples a pick; budget=0: no spend                                         (0 1)
//   budget_max_spp  the spend's cap on a pixel's samples; 0 = max_spp + rounds * batch, which refuses no pick (0)
//   move_every move_step   every move_every-th small sphere moves move_step a frame (rt_sequence_motion.hpp); 0 = static (0 0.02)
//   cam_dx cam_dz   the camera's lookfrom steps by (cam_dx, 0, cam_dz) a frame                          (0 0)
//   max_history tol min_dot reuse_specular   rt_temporal_params                                        (the header's defaults)
//   rect_radius rect_min_count gamma         rt_temporal_rectify; gamma=0 = off                        (the header's defaults)
//   levels sigma_variance   rt_denoise_var_params (progressive: the levels of rt_denoise); levels=0 shows the unfiltered fb
//   passes every    progressive: passes in all; every `every`-th pass and the last one are shown       (10 1)
//   out             file prefix: <out>%04d.ppm, binary P6; out=none writes nothing                      (frame_ | pass_)
//   tree            animation: build = every frame of moved spheres synchronises, frees the tree and calls rt_build_octree_gpu;
//                   rebuild = frame 0 builds, every later one calls rt_octree_rebuild_gpu on the same handle: no free, and no
//                   synchronisation before the stage (the rebuild is ordered on the loop's stream, where every reader of the old
//                   tree was enqueued).  The frames are the same byte for byte                         (build)
//   timing          animation, 1: a table of the stages' device times and the wall time a frame, frame 0 left out (0)
//   upscale         1: the frame is shown as it is rendered.  2..4: samples, history and filter run at nx x ny, the shown frame of
//                   upscale*nx x upscale*ny pixels is rebuilt from it and first-hit guides of both sizes (rt_sequence_upscale.hpp,
//                   kernel k_upscale); levels, copy and file have the shown size.  progressive: needs levels >= 1       (1)
// Binary16 (fp16=1) is refused: the calls of the loop are fp32 only.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <iostream>
#include <string>
#include <vector>
#include <hip/hip_runtime.h>
#include "../../include/rt_amd.h"
#include "rt_sequence_motion.hpp"
#include "rt_sequence_upscale.hpp"

static_assert(RT_SEQ_MAT_NONE == RT_MAT_NONE, "rt_sequence_motion.hpp restates RT_MAT_NONE");
static_assert(sizeof(rt_seq_geom) == 16, "a geometry record is 4 floats");
static_assert(sizeof(rt_seq_hit) == sizeof(rt_hit_record) && sizeof(rt_seq_hit) == 32, "rt_sequence_upscale.hpp restates rt_hit_record");
static_assert(offsetof(rt_seq_hit, sphere) == offsetof(rt_hit_record, sphere), "rt_sequence_upscale.hpp restates rt_hit_record");

#define checkHipErrors(val) check_hip((int)(val), #val, __FILE__, __LINE__)
static void check_hip(int result, char const* const func, const char* const file, int const line) {
    if (result) {
        std::cerr << "HIP error = " << static_cast<int>(result) << " (" << rt_error_string(result) << ") at " << file << ":" << line << " '" << func << "' \n";
        (void)hipDeviceReset();
        exit(99);
    }
}

// This frame's geometry from the created list's: one lane a sphere, one 16-byte load, one byte of mask, one 16-byte store.
// base, dir and out hold n elements; out is none of the world's own arrays (rt_world_set_geometry reads it afterwards).
__global__ __launch_bounds__(256) void k_animate(rt_seq_geom* out, const rt_seq_geom* base, const signed char* dir, int n, int f, float move_step) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;                  // (n < 2^31 - 256, checked with the arguments)
    if (i >= n) return;
    out[i] = rt_seq_move(base[i], (int)dir[i], f, move_step);
}

// The shown frame of s*nx x s*ny pixels from the low frame by the rule of rt_sequence_upscale.hpp: one lane a high pixel, 16x16 pixels
// a block, the blocks of a row one after the other in a one-dimensional grid (a frame of few columns has more rows of blocks than a
// grid's second dimension holds).  A lane reads one word of its own high guide, the sphere word and the 12 bytes of colour of up to four
// low pixels — the lanes of a block share (16/s + 2)^2 of them, which the vector cache serves — and stores 12 bytes.  out holds
// 3 * s*nx * s*ny floats and is none of the inputs; c, g hold the low frame, G the high guides.
__global__ __launch_bounds__(256) void k_upscale(float* out, const float* c, const rt_seq_hit* g, const rt_seq_hit* G, int nx, int ny, int s,
                                                 int blocks_x) {
    const int NX = s * nx, NY = s * ny;                                      // (both within int, checked with the arguments)
    const int by = (int)(blockIdx.x / (unsigned)blocks_x), bx = (int)(blockIdx.x - (unsigned)by * (unsigned)blocks_x);
    const int I = bx * 16 + (int)threadIdx.x, J = by * 16 + (int)threadIdx.y;
    if (I >= NX || J >= NY) return;
    const size_t P = (size_t)J * (size_t)NX + (size_t)I;
    float px[3];
    (void)rt_seq_upscale_pixel(c, g, nx, ny, s, I, J, G[P].sphere, px);
    out[P * 3] = px[0];
    out[P * 3 + 1] = px[1];
    out[P * 3 + 2] = px[2];
}

namespace {

struct Options {
    std::string mode = "animation", out, tree = "build", adaptive = "rounds";
    int n = 500, nx = 64, ny = 40, spl = 30, frames = 4;
    float radius = 0.1f;
    int min_spp = 4, max_spp = 8, batch = 4;
    float rel_error = 0.f, floor = 0.f;
    long long budget = 0;
    int rounds = 1, budget_max_spp = 0;
    int move_every = 0;
    float move_step = 0.02f, cam_dx = 0.f, cam_dz = 0.f;
    rt_temporal_params temporal = {RT_TEMPORAL_DEFAULT_MAX_HISTORY, RT_TEMPORAL_DEFAULT_REUSE_SPECULAR, RT_TEMPORAL_DEFAULT_POSITION_TOLERANCE,
                                   RT_TEMPORAL_DEFAULT_NORMAL_MIN_DOT};
    rt_temporal_rectify rectify = {RT_TEMPORAL_RECTIFY_DEFAULT_RADIUS, RT_TEMPORAL_RECTIFY_DEFAULT_MIN_COUNT, RT_TEMPORAL_RECTIFY_DEFAULT_GAMMA};
    int levels = RT_DENOISE_VAR_DEFAULT_LEVELS;
    float sigma_variance = RT_DENOISE_VAR_DEFAULT_SIGMA_VARIANCE;
    int passes = 10, every = 1;
    int timing = 0, fp16 = 0, upscale = 1;
    bool out_given = false;
};

[[noreturn]] void refuse(const std::string& key, const std::string& why) {
    std::cerr << "rt_sequence: " << key << ": " << why << "\n";
    exit(99);
}

void parse_value(const std::string& key, const std::string& v, int* out) {
    char* end = nullptr;
    const long x = strtol(v.c_str(), &end, 10);
    if (v.empty() || *end || x < INT32_MIN || x > INT32_MAX) refuse(key, "'" + v + "' is not an integer");
    *out = (int)x;
}
void parse_value(const std::string& key, const std::string& v, long long* out) {
    char* end = nullptr;
    *out = strtoll(v.c_str(), &end, 10);
    if (v.empty() || *end) refuse(key, "'" + v + "' is not an integer");
}
void parse_value(const std::string& key, const std::string& v, float* out) {
    char* end = nullptr;
    *out = strtof(v.c_str(), &end);
    if (v.empty() || *end || !std::isfinite(*out)) refuse(key, "'" + v + "' is not a finite number");
}

Options parse(int argc, char** argv) {
    Options o;
    for (int a = 1; a < argc; a++) {
        const std::string tok = argv[a];
        const size_t eq = tok.find('=');
        if (eq == std::string::npos || eq == 0) refuse(tok, "arguments are key=value");
        const std::string key = tok.substr(0, eq), v = tok.substr(eq + 1);
#define KEY(name, field) if (key == name) { parse_value(key, v, &(field)); continue; }
        if (key == "mode") { o.mode = v; continue; }
        if (key == "out") { o.out = v; o.out_given = true; continue; }
        if (key == "tree") { o.tree = v; continue; }
        if (key == "adaptive") { o.adaptive = v; continue; }
        KEY("n", o.n) KEY("nx", o.nx) KEY("ny", o.ny) KEY("spl", o.spl) KEY("radius", o.radius) KEY("frames", o.frames)
        KEY("min_spp", o.min_spp) KEY("max_spp", o.max_spp) KEY("batch", o.batch) KEY("rel_error", o.rel_error) KEY("floor", o.floor)
        KEY("budget", o.budget) KEY("rounds", o.rounds) KEY("budget_max_spp", o.budget_max_spp)
        KEY("move_every", o.move_every) KEY("move_step", o.move_step) KEY("cam_dx", o.cam_dx) KEY("cam_dz", o.cam_dz)
        KEY("max_history", o.temporal.max_history) KEY("tol", o.temporal.position_tolerance) KEY("min_dot", o.temporal.normal_min_dot)
        KEY("reuse_specular", o.temporal.reuse_specular)
        KEY("rect_radius", o.rectify.radius) KEY("rect_min_count", o.rectify.min_count) KEY("gamma", o.rectify.gamma)
        KEY("levels", o.levels) KEY("sigma_variance", o.sigma_variance) KEY("passes", o.passes) KEY("every", o.every)
        KEY("timing", o.timing) KEY("fp16", o.fp16) KEY("upscale", o.upscale)
#undef KEY
        refuse(key, "unknown key");
    }
    return o;
}

// every refusal, on the host: the ranges of the library's own checks with the key named, then those checks themselves
void validate(Options& o) {
    const bool progressive = o.mode == "progressive";
    if (!progressive && o.mode != "animation") refuse("mode", "'" + o.mode + "' is neither animation nor progressive");
    if (o.tree != "build" && o.tree != "rebuild") refuse("tree", "'" + o.tree + "' is neither build nor rebuild");
    if (o.adaptive != "rounds" && o.adaptive != "fused") refuse("adaptive", "'" + o.adaptive + "' is neither rounds nor fused");
    if (progressive && o.adaptive != "rounds") refuse("adaptive", "mode=progressive takes one sample a pass: no adaptive frame");
    if (progressive && o.tree != "build") refuse("tree", "nothing moves in mode=progressive: the tree is built once");
    if (o.fp16 != 0) refuse("fp16", "binary16 is not offered: the calls of the loop are fp32 only");
    if (o.n < 1 || o.n >= INT32_MAX - 256) refuse("n", "needs 1 .. 2^31 - 257 spheres");
    if (o.nx < 1) refuse("nx", "needs a positive size");
    if (o.ny < 1) refuse("ny", "needs a positive size");
    if (o.spl < 1) refuse("spl", "needs at least one sphere a leaf");
    if (o.upscale < 1 || o.upscale > RT_SEQ_UPSCALE_MAX) refuse("upscale", "needs 1 .. " + std::to_string(RT_SEQ_UPSCALE_MAX) + " (1 = the frame is shown as it is rendered)");
    if (o.upscale > 1) {
        if (o.nx > INT32_MAX / o.upscale || o.ny > INT32_MAX / o.upscale) refuse("upscale", "upscale * nx or upscale * ny is beyond int");
        const rt_levels_params shown = {RT_DENOISE_INPUT_GAMMA, 1, RT_LEVELS_RGB8, 1};
        if (rt_frame_levels_check(o.upscale * o.nx, o.upscale * o.ny, RT_PRECISION_FP32, &shown))
            refuse("upscale", "rt_frame_levels_check refuses a shown frame of upscale * nx x upscale * ny pixels");
        if (progressive && o.levels == 0) refuse("upscale", "the rule blends gamma values: progressive passes with levels=0 hold sample sums, needs levels >= 1");
    }
    if (o.timing < 0 || o.timing > 1) refuse("timing", "is 0 or 1");
    if (!o.out_given) o.out = progressive ? "pass_" : "frame_";
    if (o.levels < 0 || o.levels > RT_DENOISE_MAX_LEVELS) refuse("levels", "needs 0 .. " + std::to_string(RT_DENOISE_MAX_LEVELS));
    const rt_levels_params lp = {RT_DENOISE_INPUT_GAMMA, 1, RT_LEVELS_RGB8, 1};
    if (rt_frame_levels_check(o.nx, o.ny, RT_PRECISION_FP32, &lp)) refuse("nx", "rt_frame_levels_check refuses a frame of nx x ny pixels");
    if (progressive) {
        if (o.passes < 1) refuse("passes", "needs at least one pass");
        if (o.every < 1) refuse("every", "needs at least 1");
        if (o.timing) refuse("timing", "the stage table belongs to mode=animation");
        const rt_denoise_params dp = {RT_DENOISE_INPUT_SUM, 1, o.levels, RT_DENOISE_DEFAULT_NORMAL_POW_LOG2, RT_DENOISE_DEFAULT_SIGMA_POSITION,
                                      RT_DENOISE_DEFAULT_SIGMA_COLOR};
        if (o.levels > 0 && rt_denoise_check(o.nx, o.ny, &dp)) refuse("levels", "rt_denoise_check refuses the filter");
        return;
    }
    if (o.frames < 1) refuse("frames", "needs at least one frame");
    if (o.timing && o.frames < 2) refuse("timing", "frame 0 is left out of the table: needs frames >= 2");
    if (o.min_spp < 2) refuse("min_spp", "needs at least 2 samples");
    if (o.max_spp < o.min_spp) refuse("max_spp", "is below min_spp");
    if (o.batch < 1) refuse("batch", "needs at least 1");
    if ((o.max_spp - o.min_spp) % o.batch != 0) refuse("batch", "does not divide max_spp - min_spp");
    if (o.rel_error < 0.f) refuse("rel_error", "is negative");
    if (o.floor < 0.f) refuse("floor", "is negative");
    if (o.budget < 0) refuse("budget", "is negative");
    if (o.budget > 0) {
        if (o.rounds < 1) refuse("rounds", "a budget needs at least one round");
        if (o.budget_max_spp < 0) refuse("budget_max_spp", "is negative");
        if (o.budget > INT64_MAX / ((long long)o.nx * o.ny)) refuse("budget", "budget * nx * ny overflows");
        if (o.budget_max_spp == 0) {
            const long long cap = (long long)o.max_spp + (long long)o.rounds * o.batch;
            if (cap > INT32_MAX) refuse("rounds", "max_spp + rounds * batch overflows");
            o.budget_max_spp = (int)cap;
        }
        const rt_budget b = {o.budget * o.nx * o.ny, o.rounds, o.batch, o.budget_max_spp, o.floor};
        if (rt_adaptive_budget_check(&b)) refuse("budget", "rt_adaptive_budget_check refuses budget, rounds, batch, budget_max_spp or floor");
    }
    if (o.move_every < 0) refuse("move_every", "is negative");
    if (o.temporal.max_history < 0) refuse("max_history", "is negative");
    if (o.temporal.reuse_specular < 0 || o.temporal.reuse_specular > 1) refuse("reuse_specular", "is 0 or 1");
    if (!(o.temporal.position_tolerance > 0.f)) refuse("tol", "needs a positive tolerance");
    if (o.temporal.normal_min_dot < -1.f || o.temporal.normal_min_dot > 1.f) refuse("min_dot", "needs -1 .. 1");
    if (rt_temporal_check(o.nx, o.ny, &o.temporal)) refuse("tol", "rt_temporal_check refuses max_history, tol, min_dot, reuse_specular or the frame size");
    if (o.rectify.radius < 1 || o.rectify.radius > 2) refuse("rect_radius", "needs 1 or 2");
    const int window = (2 * o.rectify.radius + 1) * (2 * o.rectify.radius + 1);
    if (o.rectify.min_count < 2 || o.rectify.min_count > window) refuse("rect_min_count", "needs 2 .. (2 * rect_radius + 1)^2");
    if (o.rectify.gamma < 0.f) refuse("gamma", "is negative");
    if (rt_temporal_rectify_check(&o.rectify)) refuse("gamma", "rt_temporal_rectify_check refuses rect_radius, rect_min_count or gamma");
    if (o.sigma_variance < 0.f) refuse("sigma_variance", "is negative");
    const rt_denoise_var_params vp = {o.levels, RT_DENOISE_VAR_DEFAULT_NORMAL_POW_LOG2, RT_DENOISE_VAR_DEFAULT_PREFILTER,
                                      RT_DENOISE_VAR_DEFAULT_SIGMA_POSITION, o.sigma_variance};
    if (o.levels > 0 && rt_denoise_adaptive_check(o.nx, o.ny, &vp)) refuse("sigma_variance", "rt_denoise_adaptive_check refuses levels or sigma_variance");
}

// "P6\n<nx> <ny>\n255\n" and the RGB8 levels, top row first: the bytes rt_write_image(RT_IMAGE_P6) writes for the frame
void write_p6(const std::string& prefix, int index, int nx, int ny, const unsigned char* levels) {
    char name[32];
    snprintf(name, sizeof name, "%04d.ppm", index);
    const std::string path = prefix + name;
    FILE* f = fopen(path.c_str(), "wb");
    bool ok = f && fprintf(f, "P6\n%d %d\n255\n", nx, ny) > 0 && fwrite(levels, 1, (size_t)nx * ny * 3, f) == (size_t)nx * ny * 3;
    if (f) ok = fclose(f) == 0 && ok;
    if (!ok) {
        std::cerr << "rt_sequence: cannot write " << path << "\n";
        exit(99);
    }
}

// (the upscale stage and its line exist for upscale > 1 only)
const char* const STAGES[] = {"animate + setters", "tree rebuild", "guides", "begin", "spend", "accumulate", "filter", "upscale", "levels + copy"};
enum { ANIMATE, TREE, GUIDES, BEGIN, SPEND, ACCUMULATE, FILTER, UPSCALE, LEVELS, NSTAGES };

// the high guides of the same world, tree and camera, then the shown frame from the low one (rt_sequence_upscale.hpp)
void upscale_frame(float* d_up, const float* d_show, const rt_hit_record* d_hits, rt_hit_record* d_hits_up, const rt_world* world, const rt_octree* tree,
                   int nx, int ny, int s, bool trace_guides, hipStream_t stream) {
    const int NX = s * nx, NY = s * ny;
    if (trace_guides) checkHipErrors(rt_render_guides(world, tree, NX, NY, d_hits_up, stream));
    const unsigned blocks_x = (unsigned)((NX + 15) / 16), blocks_y = (unsigned)((NY + 15) / 16);   // at most 2^30 pixels: below 2^31 blocks
    hipLaunchKernelGGL(k_upscale, dim3(blocks_x * blocks_y), dim3(16, 16), 0, stream, d_up, d_show, reinterpret_cast<const rt_seq_hit*>(d_hits),
                       reinterpret_cast<const rt_seq_hit*>(d_hits_up), nx, ny, s, (int)blocks_x);
    checkHipErrors(hipGetLastError());
}

struct Scene {
    std::vector<rt_sphere> list;
    rt_camera camera;
    rt_world* world = nullptr;
};

Scene create_scene(const Options& o) {
    Scene s;
    rt_rand_state rs;
    checkHipErrors(rt_rand_init(&rs));
    s.list.resize(o.n);
    int created = 0;
    checkHipErrors(rt_create_world(s.list.data(), o.n, o.radius, &s.camera, o.nx, o.ny, &rs, RT_PRECISION_FP32, &created));
    checkHipErrors(rt_world_create(s.list.data(), o.n, &s.camera, RT_PRECISION_FP32, &s.world));
    checkHipErrors(rt_world_upload(s.world));
    return s;
}

void report_drops(const rt_octree* tree) {
    int full = 0, outside = 0;
    checkHipErrors(rt_octree_info(tree, nullptr, nullptr, nullptr, &full, &outside));
    if (full || outside) std::cerr << "octree: " << full << " insertions dropped (leaf nodes full), " << outside << " outside the root box\n";
}

template <class T> T* device_alloc(size_t count) {
    void* p = nullptr;
    checkHipErrors(hipMalloc(&p, count * sizeof(T)));
    return static_cast<T*>(p);
}

int run_animation(const Options& o) {
    const rt_partition whole = {0, 1, 0, 0};
    const size_t px = (size_t)o.nx * o.ny;
    const bool spheres_move = o.move_every > 0, camera_moves = o.cam_dx != 0.f || o.cam_dz != 0.f;
    const rt_adaptive adaptive = {o.min_spp, o.max_spp, o.batch, o.rel_error, o.floor};
    const rt_budget budget = {o.budget * o.nx * o.ny, o.rounds, o.batch, o.budget_max_spp, o.floor};
    const rt_denoise_var_params filter = {o.levels, RT_DENOISE_VAR_DEFAULT_NORMAL_POW_LOG2, RT_DENOISE_VAR_DEFAULT_PREFILTER,
                                          RT_DENOISE_VAR_DEFAULT_SIGMA_POSITION, o.sigma_variance};
    const rt_levels_params lp = {RT_DENOISE_INPUT_GAMMA, 1, RT_LEVELS_RGB8, 1};
    const int s = o.upscale, NX = s * o.nx, NY = s * o.ny;                    // the shown frame; upscale=1: the rendered one
    const size_t shown_px = (size_t)NX * NY;

    Scene S = create_scene(o);
    rt_world* const world = S.world;
    hipStream_t stream;
    checkHipErrors(hipStreamCreate(&stream));

    // every buffer of the loop, once
    float* fb = device_alloc<float>(px * 3);
    float* d_show = o.levels > 0 ? device_alloc<float>(px * 3) : fb;
    rt_rand_state* d_rand = device_alloc<rt_rand_state>(px);
    char* d_state = device_alloc<char>(px * RT_ADAPTIVE_STATE_BYTES);
    int32_t* d_spp = device_alloc<int32_t>(px);
    char* d_work = device_alloc<char>(px * RT_DENOISE_WORK_BYTES);
    unsigned char* d_levels = device_alloc<unsigned char>(shown_px * 3);
    float* d_up = s > 1 ? device_alloc<float>(shown_px * 3) : nullptr;
    rt_hit_record* d_hits_up = s > 1 ? device_alloc<rt_hit_record>(shown_px) : nullptr;
    char* d_hist[2];
    rt_hit_record* d_hits[2];
    rt_seq_geom* d_geom[2];
    for (int b = 0; b < 2; b++) {
        d_hist[b] = device_alloc<char>(px * RT_TEMPORAL_HISTORY_BYTES);
        d_hits[b] = device_alloc<rt_hit_record>(px);
        d_geom[b] = device_alloc<rt_seq_geom>(o.n);
    }
    rt_seq_geom* d_base = device_alloc<rt_seq_geom>(o.n);
    signed char* d_dir = device_alloc<signed char>(o.n);
    unsigned char* h_levels = nullptr;
    int32_t* h_spp = nullptr;
    checkHipErrors(hipHostMalloc(reinterpret_cast<void**>(&h_levels), shown_px * 3));
    checkHipErrors(hipHostMalloc(reinterpret_cast<void**>(&h_spp), px * sizeof(int32_t)));

    // the motion mask, from the created list; the created geometry is the base of every frame and frame 0's own
    std::vector<signed char> dir(o.n);
    for (int i = 0; i < o.n; i++) dir[i] = (signed char)rt_seq_dir(i, o.move_every, S.list[i].material, S.list[i].radius);
    checkHipErrors(hipMemcpyAsync(d_dir, dir.data(), (size_t)o.n, hipMemcpyHostToDevice, stream));
    checkHipErrors(rt_world_get_geometry(world, &d_base->x, stream));
    checkHipErrors(rt_world_get_geometry(world, &d_geom[0]->x, stream));
    checkHipErrors(rt_render_init(o.nx, o.ny, d_rand, whole, stream));      // once: the RNG states continue from frame to frame
    checkHipErrors(hipStreamSynchronize(stream));                            // (dir is a host vector: the copy has read it)

    hipEvent_t ev[NSTAGES][2];
    double sum_ms[NSTAGES] = {}, max_ms[NSTAGES] = {}, wall_sum = 0.0, wall_max = 0.0;
    if (o.timing)
        for (auto& pair : ev)
            for (auto& e : pair) checkHipErrors(hipEventCreate(&e));
    auto mark = [&](int stage, int end) { if (o.timing) checkHipErrors(hipEventRecord(ev[stage][end], stream)); };

    rt_camera cam[2] = {S.camera, S.camera};
    rt_octree* tree = nullptr;
    for (int f = 0; f < o.frames; f++) {
        const int c = f & 1, l = c ^ 1;
        const auto wall0 = std::chrono::steady_clock::now();
        cam[c] = S.camera;
        if (f > 0 && camera_moves) {
            const float lookat[3] = {0.f, 0.f, 0.f}, vup[3] = {0.f, 1.f, 0.f};   // create_world's camera (rt_scene.hpp, world_camera) from another place
            float lookfrom[3];
            rt_seq_lookfrom(f, o.cam_dx, o.cam_dz, lookfrom);
            checkHipErrors(rt_camera_init(&cam[c], lookfrom, lookat, vup, 30.0f, (float)o.nx / (float)o.ny, 0.1f, 10.0f, RT_PRECISION_FP32));
        }
        // 1. this frame's geometry and camera
        mark(ANIMATE, 0);
        if (f > 0 && spheres_move) {
            hipLaunchKernelGGL(k_animate, dim3((unsigned)((o.n + 255) / 256)), dim3(256), 0, stream, d_geom[c], d_base, d_dir, o.n, f, o.move_step);
            checkHipErrors(hipGetLastError());
            checkHipErrors(rt_world_set_geometry(world, &d_geom[c]->x, stream));
        }
        if (f > 0 && camera_moves) checkHipErrors(rt_world_set_camera(world, &cam[c]));
        mark(ANIMATE, 1);
        // 2. the tree of this geometry; the old one may still be read by the last frame's launches
        mark(TREE, 0);
        if (f == 0 || spheres_move) {
            if (f > 0 && o.tree == "rebuild") {
                checkHipErrors(rt_octree_rebuild_gpu(tree, world, stream));     // every launch that reads the old tree is on this stream
            } else {
                checkHipErrors(hipStreamSynchronize(stream));
                checkHipErrors(rt_free_octree(tree));
                tree = nullptr;
                checkHipErrors(rt_build_octree_gpu(world, o.spl, &tree, stream));
            }
            report_drops(tree);
            if (o.timing && rt_octree_build_path(tree) != RT_BUILD_DEVICE)
                std::cerr << "timing: frame " << f << ": the device build declined this geometry, the tree was built on the host\n";
        }
        mark(TREE, 1);
        // 3. - 7. guides, samples, history, filter
        mark(GUIDES, 0);
        checkHipErrors(rt_render_guides(world, tree, o.nx, o.ny, d_hits[c], stream));
        mark(GUIDES, 1);
        mark(BEGIN, 0);
        if (o.adaptive == "fused") checkHipErrors(rt_render_adaptive_fused(fb, o.nx, o.ny, &adaptive, world, d_rand, tree, d_spp, d_state, whole, stream));
        else checkHipErrors(rt_render_adaptive_begin(fb, o.nx, o.ny, &adaptive, world, d_rand, tree, d_spp, d_state, whole, stream));
        mark(BEGIN, 1);
        mark(SPEND, 0);
        if (o.budget > 0) {
            const rt_temporal_inputs in = {f ? d_hist[l] : nullptr, d_hits[c], d_hits[l], &cam[l]};
            checkHipErrors(rt_render_adaptive_spend_temporal(fb, o.nx, o.ny, &budget, &in, &o.temporal, world, d_rand, tree, d_spp, d_state, nullptr, stream));
        }
        mark(SPEND, 1);
        mark(ACCUMULATE, 0);
        checkHipErrors(rt_temporal_accumulate_rectified(d_hist[c], f ? d_hist[l] : nullptr, d_hits[c], f ? d_hits[l] : nullptr, f ? &cam[l] : nullptr,
                                                        (f && spheres_move) ? &d_geom[l]->x : nullptr, d_state, world, o.nx, o.ny, &o.temporal, &o.rectify, stream));
        mark(ACCUMULATE, 1);
        mark(FILTER, 0);
        if (o.levels > 0) checkHipErrors(rt_denoise_history(d_show, fb, o.nx, o.ny, d_hits[c], d_hist[c], &filter, d_work, stream));
        mark(FILTER, 1);
        // 8. upscale > 1: the shown frame from the filtered low one and the guides of both sizes, traced anew every frame
        if (s > 1) {
            mark(UPSCALE, 0);
            upscale_frame(d_up, d_show, d_hits[c], d_hits_up, world, tree, o.nx, o.ny, s, true, stream);
            mark(UPSCALE, 1);
        }
        // 9. what leaves the device: 3 bytes a shown pixel (and the sample counts, for the report)
        mark(LEVELS, 0);
        checkHipErrors(rt_frame_levels(d_levels, s > 1 ? d_up : d_show, NX, NY, RT_PRECISION_FP32, &lp, stream));
        checkHipErrors(hipMemcpyAsync(h_levels, d_levels, shown_px * 3, hipMemcpyDeviceToHost, stream));
        mark(LEVELS, 1);
        checkHipErrors(hipMemcpyAsync(h_spp, d_spp, px * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        checkHipErrors(hipStreamSynchronize(stream));
        const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();

        double total = 0.0;
        for (size_t p = 0; p < px; p++) total += h_spp[p];
        std::cerr << "frame " << f << ": mean samples per pixel: " << total / (double)px;   // samples are taken at the low size only
        if (s > 1) std::cerr << " (per low pixel, " << o.nx << "x" << o.ny << ")";
        std::cerr << "\n";
        if (o.out != "none") write_p6(o.out, f, NX, NY, h_levels);
        if (o.timing && f > 0) {
            for (int st = 0; st < NSTAGES; st++) {
                if (st == UPSCALE && s == 1) continue;
                float ms = 0.f;
                checkHipErrors(hipEventElapsedTime(&ms, ev[st][0], ev[st][1]));
                sum_ms[st] += ms;
                if (ms > max_ms[st]) max_ms[st] = ms;
            }
            wall_sum += wall_ms;
            if (wall_ms > wall_max) wall_max = wall_ms;
        }
    }

    if (o.timing) {
        // device time between each stage's two events (host work between them included: the tree rebuild synchronises), frames 1 .. frames-1;
        // the wall time runs from the frame's first call to the return of its last synchronisation, before the report and the file
        const int m = o.frames - 1;
        double stages = 0.0;
        char line[160];
        if (s > 1) snprintf(line, sizeof line, "timing: %dx%d shown at %dx%d, n=%d, frames 1..%d (frame 0 left out)\n", o.nx, o.ny, NX, NY, o.n, m);
        else snprintf(line, sizeof line, "timing: %dx%d, n=%d, frames 1..%d (frame 0 left out)\n", o.nx, o.ny, o.n, m);
        std::cerr << line;
        for (int st = 0; st < NSTAGES; st++) {
            if (st == UPSCALE && s == 1) continue;
            snprintf(line, sizeof line, "timing: %-18s mean %9.3f ms  max %9.3f ms\n", STAGES[st], sum_ms[st] / m, max_ms[st]);
            std::cerr << line;
            stages += sum_ms[st] / m;
        }
        snprintf(line, sizeof line, "timing: %-18s mean %9.3f ms\n", "sum of stages", stages);
        std::cerr << line;
        snprintf(line, sizeof line, "timing: %-18s mean %9.3f ms  max %9.3f ms\n", "wall per frame", wall_sum / m, wall_max);
        std::cerr << line;
        snprintf(line, sizeof line, "timing: %-18s mean %9.3f ms\n", "wall - stages", wall_sum / m - stages);
        std::cerr << line;
        for (auto& pair : ev)
            for (auto& e : pair) checkHipErrors(hipEventDestroy(e));
    }

    checkHipErrors(hipStreamSynchronize(stream));
    checkHipErrors(rt_free_octree(tree));
    checkHipErrors(rt_free_world(world));
    void* const device_buffers[] = {fb, d_rand, d_state, d_spp, d_work, d_levels, d_hist[0], d_hist[1], d_hits[0], d_hits[1], d_geom[0], d_geom[1], d_base, d_dir};
    for (void* p : device_buffers) checkHipErrors(hipFree(p));
    if (d_show != fb) checkHipErrors(hipFree(d_show));
    if (s > 1) {
        checkHipErrors(hipFree(d_up));
        checkHipErrors(hipFree(d_hits_up));
    }
    checkHipErrors(hipHostFree(h_levels));
    checkHipErrors(hipHostFree(h_spp));
    checkHipErrors(hipStreamDestroy(stream));
    return 0;
}

// the reference viewer's loop (main.cu:222-318) without the window: a plain loop, one sample a pass
int run_progressive(const Options& o) {
    const rt_partition whole = {0, 1, 0, 0};
    const size_t px = (size_t)o.nx * o.ny;
    Scene S = create_scene(o);
    rt_world* const world = S.world;
    hipStream_t stream;
    checkHipErrors(hipStreamCreate(&stream));
    float* fb = device_alloc<float>(px * 3);
    float* d_show = o.levels > 0 ? device_alloc<float>(px * 3) : fb;
    rt_rand_state* d_rand = device_alloc<rt_rand_state>(px);
    rt_hit_record* d_hits = device_alloc<rt_hit_record>(px);
    char* d_work = device_alloc<char>(px * RT_DENOISE_WORK_BYTES);
    const int up = o.upscale, NX = up * o.nx, NY = up * o.ny;                // the shown frame; upscale=1: the rendered one
    const size_t shown_px = (size_t)NX * NY;
    unsigned char* d_levels = device_alloc<unsigned char>(shown_px * 3);
    float* d_up = up > 1 ? device_alloc<float>(shown_px * 3) : nullptr;
    rt_hit_record* d_hits_up = up > 1 ? device_alloc<rt_hit_record>(shown_px) : nullptr;
    unsigned char* h_levels = nullptr;
    checkHipErrors(hipHostMalloc(reinterpret_cast<void**>(&h_levels), shown_px * 3));

    rt_octree* tree = nullptr;
    checkHipErrors(rt_build_octree_gpu(world, o.spl, &tree, stream));
    report_drops(tree);
    checkHipErrors(rt_render_init(o.nx, o.ny, d_rand, whole, stream));
    checkHipErrors(rt_render_guides(world, tree, o.nx, o.ny, d_hits, stream));   // once: nothing moves
    if (up > 1) checkHipErrors(rt_render_guides(world, tree, NX, NY, d_hits_up, stream));   // the shown frame's, once as well
    for (int s = 1; s <= o.passes; s++) {
        checkHipErrors(rt_render_progressive(fb, o.nx, o.ny, s, world, d_rand, tree, whole, stream));
        if (s % o.every != 0 && s != o.passes) continue;
        rt_levels_params lp = {RT_DENOISE_INPUT_SUM, s, RT_LEVELS_RGB8, 1};      // levels=0: the viewer's sqrt(fb / s)
        if (o.levels > 0) {
            const rt_denoise_params dp = {RT_DENOISE_INPUT_SUM, s, o.levels, RT_DENOISE_DEFAULT_NORMAL_POW_LOG2, RT_DENOISE_DEFAULT_SIGMA_POSITION,
                                          RT_DENOISE_DEFAULT_SIGMA_COLOR};
            checkHipErrors(rt_denoise(d_show, fb, o.nx, o.ny, d_hits, &dp, d_work, stream));
            lp.input = RT_DENOISE_INPUT_GAMMA;                                   // the filter wrote the gamma frame
        }
        if (up > 1) upscale_frame(d_up, d_show, d_hits, d_hits_up, world, tree, o.nx, o.ny, up, false, stream);   // (levels > 0: d_show is the gamma frame)
        checkHipErrors(rt_frame_levels(d_levels, up > 1 ? d_up : d_show, NX, NY, RT_PRECISION_FP32, &lp, stream));
        checkHipErrors(hipMemcpyAsync(h_levels, d_levels, shown_px * 3, hipMemcpyDeviceToHost, stream));
        checkHipErrors(hipStreamSynchronize(stream));
        std::cerr << "pass " << s << " shown\n";
        if (o.out != "none") write_p6(o.out, s, NX, NY, h_levels);
    }

    checkHipErrors(hipStreamSynchronize(stream));
    checkHipErrors(rt_free_octree(tree));
    checkHipErrors(rt_free_world(world));
    void* const device_buffers[] = {fb, d_rand, d_hits, d_work, d_levels};
    for (void* p : device_buffers) checkHipErrors(hipFree(p));
    if (d_show != fb) checkHipErrors(hipFree(d_show));
    if (up > 1) {
        checkHipErrors(hipFree(d_up));
        checkHipErrors(hipFree(d_hits_up));
    }
    checkHipErrors(hipHostFree(h_levels));
    checkHipErrors(hipStreamDestroy(stream));
    return 0;
}

} // namespace

int main(int argc, char** argv) {
    Options o = parse(argc, argv);
    validate(o);
    const bool progressive = o.mode == "progressive";
    std::cerr << "rt_sequence: " << o.mode << ", " << o.nx << "x" << o.ny << ", " << o.n << " spheres of radius " << o.radius << ", "
              << (progressive ? o.passes : o.frames) << (progressive ? " passes" : " frames");
    if (o.upscale > 1) std::cerr << ", shown at " << o.upscale * o.nx << "x" << o.upscale * o.ny;
    std::cerr << "\n";
    checkHipErrors(rt_device_check(nullptr));
    const int rc = progressive ? run_progressive(o) : run_animation(o);
    (void)hipDeviceReset();
    return rc;
}
