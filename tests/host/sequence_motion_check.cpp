// sequence_motion_check.cpp — test program (tests/test_sequence_host.py compiles it with g++ -ffp-contract=off and
// -fsanitize=address,undefined and runs it; not part of the product).  Evaluates the motion rule of rt_sequence
// (dd2360-raytracing_amd/host/rt_sequence_motion.hpp) on a small hand-made list and prints everything as bits: the list itself, and
// for move_every 1, 3 and 0 the mask and the geometry of frames 0, 1, 3 and 1000; then the lookfrom of the same frames.
// tests/sequence_model.py computes the same from the printed list, and the test compares the bits.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include "rt_sequence_motion.hpp"

static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}

struct Slot {
    int material;
    rt_seq_geom g;
};

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const Slot list[] = {
        {0, {0.f, -1000.f, -1.f, 1000.f}},     // the ground
        {2, {0.f, 1.f, 0.f, 1.f}},             // a unit sphere
        {0, {-0.f, 0.1f, 2.5f, 0.1f}},         // -0 in a coordinate that moves (move_every 1: +x ... )
        {1, {1.25f, -0.f, -3.f, 0.1f}},        // -0 in a coordinate that is copied
        {-1, {7.f, 7.f, 7.f, 0.1f}},           // a ghost slot
        {0, {4.5f, nan, -0.f, 0.1f}},          // NaN in a coordinate that is copied, -0 in z
        {2, {-2.f, 0.1f, 1e-3f, 0.1f}},
        {0, {3.f, 0.1f, 16777216.f, 0.1f}},    // a coordinate whose spacing is above every step
        {1, {nan, 0.1f, 0.5f, 0.5f}},          // radius 0.5 is not < 0.5: never moves, NaN copied
        {0, {0.3f, 0.1f, -0.7f, 0.4999f}},
        {-1, {nan, -0.f, 0.f, 0.f}},           // a ghost slot holding NaN and -0
        {0, {-5.5f, 0.1f, 5.5f, 0.1f}},
        {1, {8.f, 0.1f, -8.f, 0.1f}},
    };
    const int n = (int)(sizeof list / sizeof list[0]);
    const float move_step = 0.02f, cam_dx = 0.05f, cam_dz = -0.03f;
    const int frames[] = {0, 1, 3, 1000}, every[] = {1, 3, 0};
    printf("step %08x %08x %08x\n", bits(move_step), bits(cam_dx), bits(cam_dz));
    for (int i = 0; i < n; i++)
        printf("in %d %d %08x %08x %08x %08x\n", i, list[i].material, bits(list[i].g.x), bits(list[i].g.y), bits(list[i].g.z), bits(list[i].g.r));
    for (int me : every) {
        for (int i = 0; i < n; i++) printf("dir %d %d %d\n", me, i, rt_seq_dir(i, me, list[i].material, list[i].g.r));
        for (int f : frames)
            for (int i = 0; i < n; i++) {
                const rt_seq_geom g = rt_seq_move(list[i].g, rt_seq_dir(i, me, list[i].material, list[i].g.r), f, move_step);
                printf("geom %d %d %d %08x %08x %08x %08x\n", me, f, i, bits(g.x), bits(g.y), bits(g.z), bits(g.r));
            }
    }
    for (int f : frames) {
        float from[3];
        rt_seq_lookfrom(f, cam_dx, cam_dz, from);
        printf("lookfrom %d %08x %08x %08x\n", f, bits(from[0]), bits(from[1]), bits(from[2]));
    }
    printf("sequence_motion_check: ok\n");
    return 0;
}
