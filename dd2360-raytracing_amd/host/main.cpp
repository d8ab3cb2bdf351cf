// main.cpp — host program of the MI355X render path; the counterpart of the reference's main() (main.cu:347-477).
//
// Same sequence, same stderr lines, same output modes (0 = PPM to stdout, 1 = none, 3 = output.ppm; mode 2, the
// OpenGL viewer, is out of scope here: rt_sequence mode=progressive, host/sequence.cpp, is its headless counterpart), same error convention (message + exit code 99), but every step goes through the
// C-ABI of include/rt_amd.h.  The reference's compile-time knobs become optional trailing arguments:
//   rt_main [output_mode] [NUM_SPHERES] [nx] [ny] [ns] [USE_OCTREE 0|1] [SPHERES_PER_LEAF] [SPHERE_RADIUS] [USE_FP16 0|1] [BUILD_ON_GPU 0|1]
// with the reference's values as defaults (main.cu:22-24, :348-350; acceleration_structure.h:15).  BUILD_ON_GPU 1 replaces
// buildOctree + upload (main.cu:405-417) by rt_build_octree_gpu: the same tree, built on the device.
// Adaptive sampling (no reference counterpart) takes four more optional arguments:
//   ... [REL_ERROR] [MIN_SPP] [BATCH] [FLOOR]
// REL_ERROR > 0 renders through rt_render_adaptive with max_spp = ns: MIN_SPP defaults to 4 (ns if smaller), BATCH to the largest of
// 4, 2, 1 that divides ns - MIN_SPP, FLOOR to 0.  Without REL_ERROR (or with 0) the program does exactly what it does without them.
// Denoising (no reference counterpart) takes one more:
//   ... [DENOISE]
// DENOISE > 0: after the render, rt_render_guides + rt_denoise (GAMMA input, DENOISE levels, the header's default weights) filter the
// frame before it is written.  0 or absent: exactly the program without it.  fp32 only: USE_FP16 1 with DENOISE > 0 is an error.
// The variance-guided filter (no reference counterpart) takes one more:
//   ... [DENOISE_SIGMA_VARIANCE]
// > 0 together with REL_ERROR > 0 and DENOISE > 0: the frame is rendered through rt_render_adaptive_begin, which keeps every pixel's
// sums, and filtered by rt_denoise_adaptive (DENOISE levels, this sigma_variance, the header's other defaults).  0 or absent: exactly
// the program without it.  A positive value without a positive REL_ERROR and a positive DENOISE is an error.
#include <iostream>
#include <string>
#include <vector>
#include <cstdlib>
#include <time.h>
#include <hip/hip_runtime.h>
#include "../../include/rt_amd.h"

// limited version of the reference's checkCudaErrors (main.cu:27-37)
#define checkHipErrors(val) check_hip((int)(val), #val, __FILE__, __LINE__)
static void check_hip(int result, char const* const func, const char* const file, int const line) {
    if (result) {
        std::cerr << "HIP error = " << static_cast<int>(result) << " (" << rt_error_string(result) << ") at " << file << ":" << line << " '" << func << "' \n";
        (void)hipDeviceReset();
        exit(99);
    }
}

int main(int argc, char** argv) {
    int output_mode = 0;                 // 0 = to stdout (default), 1 = disabled, 3 = to file
    int num_spheres = 8000;              // NUM_SPHERES
    int nx = 1200, ny = 800, ns = 10;
    int use_octree = 1;                  // USE_OCTREE
    int spheres_per_leaf = 30;           // SPHERES_PER_LEAF
    float sphere_radius = 0.1f;          // SPHERE_RADIUS
    int use_fp16 = 0;                    // USE_FP16
    int build_on_gpu = 0;
    float rel_error = 0.f, floor_lum = 0.f;   // adaptive sampling (rt_render_adaptive): off
    int min_spp = -1, batch = -1;
    int denoise_levels = 0;              // rt_denoise: off
    float denoise_sigma_variance = 0.f;  // rt_denoise_adaptive: off
    const int tx = 8, ty = 8;
    if (argc > 1) output_mode = std::stoi(argv[1]);
    if (argc > 2) num_spheres = std::stoi(argv[2]);
    if (argc > 3) nx = std::stoi(argv[3]);
    if (argc > 4) ny = std::stoi(argv[4]);
    if (argc > 5) ns = std::stoi(argv[5]);
    if (argc > 6) use_octree = std::stoi(argv[6]);
    if (argc > 7) spheres_per_leaf = std::stoi(argv[7]);
    if (argc > 8) sphere_radius = std::stof(argv[8]);
    if (argc > 9) use_fp16 = std::stoi(argv[9]);
    if (argc > 10) build_on_gpu = std::stoi(argv[10]);
    if (argc > 11) rel_error = std::stof(argv[11]);
    if (argc > 12) min_spp = std::stoi(argv[12]);
    if (argc > 13) batch = std::stoi(argv[13]);
    if (argc > 14) floor_lum = std::stof(argv[14]);
    if (argc > 15) denoise_levels = std::stoi(argv[15]);
    if (argc > 16) denoise_sigma_variance = std::stof(argv[16]);
    const bool adaptive = rel_error > 0.f;
    if (min_spp < 0) min_spp = ns < 4 ? ns : 4;
    if (batch < 0) batch = (ns - min_spp) % 4 == 0 ? 4 : ((ns - min_spp) % 2 == 0 ? 2 : 1);
    const int precision = use_fp16 ? RT_PRECISION_FP16 : RT_PRECISION_FP32;
    if (denoise_levels > 0 && use_fp16) {
        std::cerr << "DENOISE needs a binary32 frame (USE_FP16 0)\n";
        return 99;
    }

    const bool denoise_var = denoise_sigma_variance > 0.f;
    if (denoise_var && !(adaptive && denoise_levels > 0)) {
        std::cerr << "DENOISE_SIGMA_VARIANCE needs adaptive sampling and the filter (REL_ERROR > 0 and DENOISE > 0)\n";
        return 99;
    }

    std::cerr << "Rendering a " << nx << "x" << ny << " image with " << ns << " samples per pixel ";
    std::cerr << "in " << tx << "x" << ty << " blocks.\n";
    std::cerr << "Number of spheres: " << num_spheres << "\n";
    std::cerr << "Sphere radius: " << sphere_radius << "\n";
    std::cerr << (use_octree ? "Use octree: ON\n" : "Use octree: OFF\n");
    std::cerr << "Output mode: " << output_mode << "\n";
    if (adaptive)
        std::cerr << "Adaptive sampling: " << min_spp << " to " << ns << " samples per pixel in steps of " << batch << ", relative error " << rel_error
                  << ", floor " << floor_lum << "\n";
    if (denoise_levels > 0) std::cerr << "Denoising: " << denoise_levels << " levels\n";
    if (denoise_var) std::cerr << "Variance-guided weights: sigma_variance " << denoise_sigma_variance << "\n";

    checkHipErrors(rt_device_check(nullptr));
    const rt_partition whole = {0, 1};
    const size_t num_pixels = (size_t)nx * ny;
    const size_t fb_size = num_pixels * 3 * (use_fp16 ? 2 : 4);

    // allocate FB and random state
    void* fb = nullptr;
    checkHipErrors(hipMalloc(&fb, fb_size));
    rt_rand_state* d_rand_state = nullptr;
    checkHipErrors(hipMalloc(reinterpret_cast<void**>(&d_rand_state), num_pixels * sizeof(rt_rand_state)));

    // world RNG, world of hitables & the camera
    rt_rand_state rand_state2;
    checkHipErrors(rt_rand_init(&rand_state2));
    std::vector<rt_sphere> list(num_spheres);
    rt_camera camera;
    int created = 0;
    checkHipErrors(rt_create_world(list.data(), num_spheres, sphere_radius, &camera, nx, ny, &rand_state2, precision, &created));
    rt_world* d_world = nullptr;
    checkHipErrors(rt_world_create(list.data(), num_spheres, &camera, precision, &d_world));
    checkHipErrors(rt_world_upload(d_world));

    // build octree and upload it
    rt_octree* d_octree = nullptr;
    if (use_octree) {
        if (build_on_gpu) checkHipErrors(rt_build_octree_gpu(d_world, spheres_per_leaf, &d_octree, nullptr));
        else checkHipErrors(rt_build_octree(list.data(), num_spheres, spheres_per_leaf, precision, &d_octree));
        int dropped_full = 0, dropped_outside = 0;
        checkHipErrors(rt_octree_info(d_octree, nullptr, nullptr, nullptr, &dropped_full, &dropped_outside));
        if (dropped_full || dropped_outside)   // the reference prints one line per drop to stdout, corrupting mode 0; here: stderr, once
            std::cerr << "octree: " << dropped_full << " insertions dropped (leaf nodes full), " << dropped_outside << " outside the root box\n";
        checkHipErrors(rt_octree_upload(d_octree));
    }
    checkHipErrors(hipDeviceSynchronize());

    clock_t start, stop;
    start = clock();
    checkHipErrors(rt_render_init(nx, ny, d_rand_state, whole, nullptr));
    checkHipErrors(hipDeviceSynchronize());
    int32_t* d_spp = nullptr;
    void* d_state = nullptr;             // every pixel's sums and sample count, for rt_denoise_adaptive
    if (adaptive) {
        const rt_adaptive params = {min_spp, ns, batch, rel_error, floor_lum};
        checkHipErrors(hipMalloc(reinterpret_cast<void**>(&d_spp), num_pixels * sizeof(int32_t)));
        if (denoise_var) {
            checkHipErrors(hipMalloc(&d_state, num_pixels * RT_ADAPTIVE_STATE_BYTES));
            checkHipErrors(rt_render_adaptive_begin(fb, nx, ny, &params, d_world, d_rand_state, d_octree, d_spp, d_state, whole, nullptr));
        } else {
            checkHipErrors(rt_render_adaptive(fb, nx, ny, &params, d_world, d_rand_state, d_octree, d_spp, nullptr));
        }
    } else {
        checkHipErrors(rt_render(fb, nx, ny, ns, d_world, d_rand_state, d_octree, whole, nullptr));
    }
    checkHipErrors(hipDeviceSynchronize());
    stop = clock();
    const double timer_seconds = static_cast<double>(stop - start) / CLOCKS_PER_SEC;
    std::cerr << "took " << timer_seconds << " seconds.\n";
    if (adaptive) {
        std::vector<int32_t> spp(num_pixels);
        checkHipErrors(hipMemcpy(spp.data(), d_spp, num_pixels * sizeof(int32_t), hipMemcpyDeviceToHost));
        double total = 0.0;
        for (int32_t k : spp) total += k;
        std::cerr << "mean samples per pixel: " << total / (double)num_pixels << "\n";
        checkHipErrors(hipFree(d_spp));
    }

    if (denoise_var) {
        // guides of the pixel centres, then the variance-guided filter in place on the state the render left
        const rt_denoise_var_params params = {denoise_levels, RT_DENOISE_VAR_DEFAULT_NORMAL_POW_LOG2, RT_DENOISE_VAR_DEFAULT_PREFILTER,
                                              RT_DENOISE_VAR_DEFAULT_SIGMA_POSITION, denoise_sigma_variance};
        rt_hit_record* d_hits = nullptr;
        void* d_work = nullptr;
        checkHipErrors(hipMalloc(reinterpret_cast<void**>(&d_hits), num_pixels * sizeof(rt_hit_record)));
        checkHipErrors(hipMalloc(&d_work, num_pixels * RT_DENOISE_WORK_BYTES));
        checkHipErrors(rt_render_guides(d_world, d_octree, nx, ny, d_hits, nullptr));
        checkHipErrors(rt_denoise_adaptive(fb, fb, nx, ny, d_hits, d_state, &params, d_work, nullptr));
        checkHipErrors(hipDeviceSynchronize());
        checkHipErrors(hipFree(d_work));
        checkHipErrors(hipFree(d_hits));
        checkHipErrors(hipFree(d_state));
    } else if (denoise_levels > 0) {
        // guides of the pixel centres, then the filter in place (fb_out == fb_in), default weights
        const rt_denoise_params params = {RT_DENOISE_INPUT_GAMMA, 1, denoise_levels, RT_DENOISE_DEFAULT_NORMAL_POW_LOG2,
                                          RT_DENOISE_DEFAULT_SIGMA_POSITION, RT_DENOISE_DEFAULT_SIGMA_COLOR};
        rt_hit_record* d_hits = nullptr;
        void* d_work = nullptr;
        checkHipErrors(hipMalloc(reinterpret_cast<void**>(&d_hits), num_pixels * sizeof(rt_hit_record)));
        checkHipErrors(hipMalloc(&d_work, num_pixels * RT_DENOISE_WORK_BYTES));
        checkHipErrors(rt_render_guides(d_world, d_octree, nx, ny, d_hits, nullptr));
        checkHipErrors(rt_denoise(fb, fb, nx, ny, d_hits, &params, d_work, nullptr));
        checkHipErrors(hipDeviceSynchronize());
        checkHipErrors(hipFree(d_work));
        checkHipErrors(hipFree(d_hits));
    }

    if (output_mode == 0 || output_mode == 3) {
        std::vector<char> host(fb_size);
        checkHipErrors(hipMemcpy(host.data(), fb, fb_size, hipMemcpyDeviceToHost));
        checkHipErrors(rt_write_ppm(output_mode == 3 ? "output.ppm" : nullptr, nx, ny, host.data(), precision));
    }

    // clean up
    checkHipErrors(hipDeviceSynchronize());
    checkHipErrors(rt_free_octree(d_octree));
    checkHipErrors(rt_free_world(d_world));
    checkHipErrors(hipFree(d_rand_state));
    checkHipErrors(hipFree(fb));
    (void)hipDeviceReset();
    return 0;
}
