"""Worlds AT the workspace limit of the device tree build (csrc/rt_build.hip, gpubuild::build), and the smallest worlds.

rt_build_octree_gpu sizes its workspace for cap = 16 n + 65536 (level-3 cell, sphere) pairs; k_pairs counts the pairs and writes one
only while its slot is below cap; with more, the build declines and rt_build_octree_gpu builds on the host from the world's staging
copy.  create_world scenes and random_world stay far below: a sphere of radius 0.1 touches one to eight of the 512 cells.  A sphere of
radius > 8.25 centred on the root box touches all 512.

  at_cap    slot 0 the ground; 133 concentric shells at (0, 1, 0) with radii 9 + i / 64 (slots 1..133: 512 pairs each); 16 spheres of
            radius 1 / 64, each at the centre of a level-3 cell of its own (slots 134..149: one pair each); 11 spheres at (50, 50, 50),
            outside the root box (slots 150..160: no pair).  n = 161, pairs = 133 * 512 + 16 = 68112 = cap: the device must build it.
  over_cap  slot 150 is a 17th one-cell sphere instead: pairs = 68113 = cap + 1: the device must decline.
  small     at_cap with every shell radius times 1 / 64 (0.14 .. 0.17: a shell touches the eight cells around (0, 1, 0)): far below
            the limit.  geometry(small) and geometry(over_cap) move one resident world across the limit and back: the lists differ in
            geometry only.
Every cell then has 133 or 134 members: SPHERES_PER_LEAF 17 fills eight buckets in each of the 512 cells and drops nothing (leafCount
4097, the most a tree can have), SPHERES_PER_LEAF 16 keeps the first 128 of every cell (the five outermost shells and every one-cell
sphere are in no leaf).  The shells' materials cycle dielectric / metal / lambertian from the innermost out, so that the outermost
shell (slot 133) and the outermost one a tree of SPHERES_PER_LEAF 16 stores (slot 128, a metal) both let a path go on to the shells
behind them.  Every value is a binary16 number: the binary16 twin of a world is the same list.  create_world's camera, 13.4 from
(0, 1, 0), lies outside all shells (the largest radius is 11.0625).

  ground, inside, outside   n = 1 (the ground alone), and n = 2 with the one sphere inside / outside the root box.

`pairs_model(spheres, fp16)` is k_pairs' count in numpy, in float32 or binary16: the nine planes per axis of the 512 level-3 boxes by
the float midpoint rule of full_tree_boxes (csrc/rt_octgeom.h) and the comparison of sphere_touches_box, open on low x, closed
elsewhere, one rounding per operation.  `cap(n)` is the limit.

A helper module (no tests, not a conftest): tests/test_build_limit_worlds_host.py shows on the CPU that every world sits where its
name says, tests/test_gpu_build_limits.py runs them through rt_build_octree_gpu."""
import functools

import numpy as np

import material_edge_worlds as mw

F = np.float32
MAT_NONE, LAMBERTIAN, METAL, DIELECTRIC = mw.MAT_NONE, mw.LAMBERTIAN, mw.METAL, mw.DIELECTRIC
sphere_dtype = mw.sphere_dtype
NX, NY, NS = 43, 21, 4                                     # edge tiles in both directions
N_RAYS, N_AIMED = 4096, 512
N_SHELLS, N_CELL, N_OUT = 133, 16, 11
SHELLS = np.arange(1, 1 + N_SHELLS)                        # slots of the shells, innermost first
ONE_CELL = np.arange(1 + N_SHELLS, 1 + N_SHELLS + N_CELL)  # slots of the one-cell spheres (over_cap: and slot MOVED)
MOVED = 1 + N_SHELLS + N_CELL                              # the slot that is outside the box in at_cap and a one-cell sphere in over_cap
ROOT = ((-11.0, 11.0), (0.0, 2.0), (-11.0, 11.0))          # acceleration_structure.h:203
NAMES = ("at_cap", "over_cap", "small")
SMALLEST = ("ground", "inside", "outside")


def cap(n):
    """the pairs the device build's workspace holds"""
    return 16 * n + 65536


# ---------------------------------------------------------------------------------------------------- the model
def planes(fp16):
    """per axis the nine planes of the level-3 boxes, as float32 images of real_t: the root box halved three times, each midpoint
    low + (high - low) / 2 computed in float32 and rounded to real_t"""
    R = np.float16 if fp16 else F

    def halve(lo, hi, depth):
        if depth == 0:
            return [lo]
        mid = F(R(lo + (hi - lo) / F(2)))
        return halve(lo, mid, depth - 1) + halve(mid, hi, depth - 1)
    return [np.array(halve(F(R(lo)), F(R(hi)), 3) + [F(R(hi))], F) for lo, hi in ROOT]


def pairs_model(sp, fp16):
    """dict(per_sphere: the level-3 cells every sphere of the list touches (0 for slot 0, which buildOctree leaves out), pairs: their
    sum, outside: the spheres behind slot 0 that do not touch the root box)"""
    R = np.float16 if fp16 else F
    c, r = sp["center"].astype(R), sp["radius"].astype(R)
    touched, root = [], np.ones(len(sp), bool)
    for axis in range(3):
        p = planes(fp16)[axis].astype(R)
        lo = (p[None, :-1] - r[:, None]).astype(R)         # one rounding: the box grown by the radius
        hi = (p[None, 1:] + r[:, None]).astype(R)
        x = c[:, axis, None]
        t = ((x > lo) if axis == 0 else (x >= lo)) & (x <= hi)
        touched.append(t.sum(axis=1))
        rlo, rhi = (p[0] - r).astype(R), (p[-1] + r).astype(R)
        root &= ((c[:, axis] > rlo) if axis == 0 else (c[:, axis] >= rlo)) & (c[:, axis] <= rhi)
    per = touched[0] * touched[1] * touched[2] * root
    per[0] = 0
    return dict(per_sphere=per, pairs=int(per.sum()), outside=int((~root[1:]).sum()))


# ---------------------------------------------------------------------------------------------------- the worlds
GROUND = mw.GROUND
KINDS = (DIELECTRIC, METAL, LAMBERTIAN)


def _cell_centre(k):
    """the centre of the k-th chosen level-3 cell: spread over the box, no two in one cell"""
    ix, iy, iz = (3 * k + 1) % 8, (5 * k + 2 + k // 8) % 8, (7 * k + 3) % 8
    return (-11.0 + 2.75 * (ix + 0.5), 0.25 * (iy + 0.5), -11.0 + 2.75 * (iz + 0.5))


@functools.lru_cache(None)
def _built(name):
    if name in SMALLEST:
        recs = [GROUND]
        if name == "inside":
            recs.append(((0.5, 0.25, 0.75), 0.25, LAMBERTIAN, (0.75, 0.5, 0.25), 0.0))
        elif name == "outside":
            recs.append(((50.0, 50.0, 50.0), 1.0, METAL, (0.75, 0.5, 0.25), 0.25))
    else:
        assert name in NAMES, name
        scale = 1.0 / 64.0 if name == "small" else 1.0
        recs = [GROUND]
        for i in range(N_SHELLS):
            kind = KINDS[i % 3]
            alb = (0.25 + 0.125 * (i % 5), 0.5, 0.875 - 0.125 * (i % 3))
            param = 0.25 * (i % 2) if kind == METAL else 1.5 if kind == DIELECTRIC else 0.0
            recs.append(((0.0, 1.0, 0.0), (9.0 + i / 64.0) * scale, kind, alb, param))
        for k in range(N_CELL + N_OUT):
            alb = (0.875, 0.25 + 0.125 * (k % 4), 0.125)
            if k < N_CELL or (k == N_CELL and name == "over_cap"):
                recs.append((_cell_centre(k), 1.0 / 64.0, LAMBERTIAN, alb, 0.0))
            else:
                recs.append(((50.0, 50.0, 50.0), 1.0, LAMBERTIAN, alb, 0.0))
    sp = np.zeros(len(recs), sphere_dtype)
    for i, rec in enumerate(recs):
        sp[i] = rec
    for f in ("center", "radius", "albedo", "param"):          # the binary16 twin is the same list
        assert np.array_equal(sp[f], sp[f].astype(np.float16).astype(F)), (name, f)
    sp.setflags(write=False)
    return sp


def spheres(name):
    """the binding's sphere records of a world (the same for both precisions)"""
    return _built(name).copy()


def geometry(name):
    """(cx, cy, cz, radius) per slot: what rt_world_set_geometry takes"""
    sp = _built(name)
    return np.ascontiguousarray(np.concatenate([sp["center"], sp["radius"][:, None]], 1), F)


def camera(rt, fp16, nx=NX, ny=NY):
    """create_world's camera for this frame size, from the library (host only), as a camera_dtype record"""
    W = rt.World(22, nx, ny, precision=rt.FP16 if fp16 else rt.FP32)
    cam = W.camera.copy()
    W.close()
    return cam


def gpu_world(rt, name_or_spheres, fp16, nx=NX, ny=NY):
    sp = spheres(name_or_spheres) if isinstance(name_or_spheres, str) else name_or_spheres
    return rt.World(len(sp), nx, ny, precision=rt.FP16 if fp16 else rt.FP32, spheres=sp, camera=camera(rt, fp16, nx, ny))


def oracle(rt, name, fp16, spl, nx=NX, ny=NY):
    """the oracle's scene of a world, rendered and traced through its octree"""
    return mw.oracle(_built(name), camera(rt, fp16, nx, ny).view(F).ravel(), nx, ny, tree=True, spl=spl, fp16=fp16)


# ---------------------------------------------------------------------------------------------------- rays
def rays(fp16):
    """N_RAYS rays: world_cases.random_rays (origins in the box - inside every shell -, at the camera, far away, around the box),
    the last N_AIMED of them replaced by rays from 12 to 40 (binary16: 12 to 16) away from (0, 1, 0) - outside every shell - aimed at a
    point of the root box; binary16 numbers for a binary16 world"""
    from world_cases import random_rays
    r = random_rays(N_RAYS, 4100)
    rng = np.random.default_rng(4200)
    d = rng.normal(size=(N_AIMED, 3))
    d[:, 1] = np.abs(d[:, 1])
    o = np.array([0.0, 1.0, 0.0]) + d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(12.0, 16.0 if fp16 else 40.0, (N_AIMED, 1))
    tgt = rng.uniform([-11.0, 0.0, -11.0], [11.0, 2.0, 11.0], (N_AIMED, 3))
    d = tgt - o
    if fp16:                                               # (b * b of a longer ray overflows binary16: unit directions from close by)
        d /= np.linalg.norm(d, axis=1)[:, None]
    r[-N_AIMED:] = np.concatenate([o, d], 1).astype(F)
    if fp16:
        r = r.astype(np.float16).astype(F)
    return np.ascontiguousarray(r, F)
