// rt_sequence_motion.hpp — the motion rule of rt_sequence (host/sequence.cpp), written once: which spheres of the created list move,
// where a sphere is in frame f, and where the camera stands.  The host program, its kernel k_animate and the stand-alone check
// tests/host/sequence_motion_check.cpp all evaluate these inlines; tests/sequence_model.py is the numpy model, bit for bit.
// Nothing of the library is included, so a plain C++ compiler takes the header as it is.
//
// Numeric contract: every value is one IEEE binary32 operation (compile with -ffp-contract=off; under clang the pragma below says
// it again).  A field that the rule does not change is COPIED: no multiply by 0 or 1, so -0 and NaN survive.
#ifndef RT_SEQUENCE_MOTION_HPP
#define RT_SEQUENCE_MOTION_HPP

#if defined(__HIPCC__)
#define RT_SEQ_HD __host__ __device__
#else
#define RT_SEQ_HD
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// one record of rt_world_set_geometry / rt_world_get_geometry: (cx, cy, cz, radius), 16 bytes
struct alignas(16) rt_seq_geom {
    float x, y, z, r;
};

#define RT_SEQ_MAT_NONE (-1)   // RT_MAT_NONE of rt_amd.h: a ghost slot of the world list (sequence.cpp asserts the two agree)

// The mask, from the CREATED list: sphere i moves along direction (i / move_every) & 3 — +x, +z, -x, -z — when move_every > 0, i is a
// multiple of it, the slot is filled and the sphere is a small one; -1 = it never moves.  The ground (radius 1000), the three unit
// spheres and ghost slots stay.
RT_SEQ_HD inline int rt_seq_dir(int i, int move_every, int material, float radius) {
    if (move_every > 0 && i % move_every == 0 && material != RT_SEQ_MAT_NONE && radius < 0.5f) return (i / move_every) & 3;
    return -1;
}

// the distance every moving sphere has covered in frame f: one rounding
RT_SEQ_HD inline float rt_seq_time(int f, float move_step) { return (float)f * move_step; }

// frame f's record of a sphere from its record in the created list: one add or one subtract on one coordinate, everything else
// copied.  Frame 0 sets nothing (-0 + 0 would be +0).
RT_SEQ_HD inline rt_seq_geom rt_seq_move(rt_seq_geom c0, int dir, int f, float move_step) {
    rt_seq_geom g = c0;
    if (f == 0) return g;
    const float t = rt_seq_time(f, move_step);
    if (dir == 0) g.x = c0.x + t;
    else if (dir == 1) g.z = c0.z + t;
    else if (dir == 2) g.x = c0.x - t;
    else if (dir == 3) g.z = c0.z - t;
    return g;
}

// lookfrom of frame f: create_world's (13, 2, 3) stepped by (cam_dx, 0, cam_dz) a frame, each component one multiply and one add
RT_SEQ_HD inline void rt_seq_lookfrom(int f, float cam_dx, float cam_dz, float out[3]) {
    const float sx = (float)f * cam_dx, sz = (float)f * cam_dz;
    out[0] = 13.0f + sx;
    out[1] = 2.0f;
    out[2] = 3.0f + sz;
}

#endif // RT_SEQUENCE_MOTION_HPP
