"""Worlds, ray sets and cameras that several test files and tools share.  numpy only: the host-only modules import this file, and
`rt` is whatever the caller passes (the binding, or a namespace with its dtype and constants)."""
import math

import numpy as np


def random_rays(n, seed):
    """rays that exercise the scene: origins around/inside the sphere field, at the camera, far away on the ground;
    directions random, some axis-aligned (zero components -> inf/NaN slab arithmetic)."""
    rng = np.random.default_rng(seed)
    o = np.empty((n, 3), np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    k = n // 4
    o[:k] = rng.uniform([-11, 0, -11], [11, 2, 11], (k, 3))
    o[k:2 * k] = np.array([13, 2, 3], np.float32) + rng.normal(scale=0.05, size=(k, 3))
    tgt = rng.uniform([-11, 0, -11], [11, 0.3, 11], (k, 3))
    d[k:2 * k] = tgt - o[k:2 * k]
    o[2 * k:3 * k] = rng.uniform([-300, 0, -300], [300, 40, 300], (k, 3))
    tgt = rng.uniform([-11, 0, -11], [11, 1, 11], (k, 3))
    d[2 * k:3 * k] = tgt - o[2 * k:3 * k]
    o[3 * k:] = rng.uniform([-12, -0.5, -12], [12, 3, 12], (n - 3 * k, 3))
    # axis-aligned / zero-component directions
    z = rng.integers(0, n, n // 50)
    d[z, rng.integers(0, 3, z.size)] = 0.0
    z = rng.integers(0, n, n // 100)
    d[z] = 0.0
    d[z, rng.integers(0, 3, z.size)] = rng.choice([-1.0, 1.0], z.size)
    return np.ascontiguousarray(np.concatenate([o, d], 1), np.float32)


def lattice_rays(info, centers, radii, n, seed, g0=None):
    """rays ON the candidate grid's lattice (tests/test_gpu_strips.py says why); g0: the grid's origin where it is not the root box's
    (a list whose grid follows its spheres further out)"""
    rng = np.random.default_rng(seed)
    G, h = info["grid_dim"], float(info["cell_size"])
    if g0 is None:
        g0 = -(11.0 + 5.0 * h)                                # build_accel: half = root half-width + 2 Rlim + 2 h, Rlim = 1.5 h
    F = 8
    o = np.zeros((n, 3), np.float64)
    d = np.zeros((n, 3), np.float64)
    # origins: x and z on column edges / fine-bin edges / an ulp off them, y anywhere in and around the spheres' slab
    i = rng.integers(0, G * F + 1, (n, 2))
    on_col = rng.random((n, 2)) < 0.5
    i = np.where(on_col, (i // F) * F, i)
    o[:, 0] = g0 + i[:, 0] * (h / F)
    o[:, 2] = g0 + i[:, 1] * (h / F)
    o[:, 1] = rng.choice([0.0, 1e-4, 0.1, 0.2, 0.2, 0.4, 0.4001, 0.7, 2.0], n)
    # a third of the origins at a sphere's centre or on its surface along an axis
    k = n // 3
    pick = rng.integers(1, len(radii), k)
    o[:k] = centers[pick]
    on_surface = rng.random(k) < 0.6
    axis = rng.integers(0, 3, k)
    sign = rng.choice([-1.0, 1.0], k)
    o[np.arange(k)[on_surface], axis[on_surface]] += (sign * radii[pick])[on_surface]
    # directions
    kind = rng.integers(0, 8, n)
    ang = rng.uniform(0, 2 * np.pi, n)
    d[:, 0] = np.cos(ang); d[:, 2] = np.sin(ang); d[:, 1] = rng.normal(scale=0.2, size=n)
    m = kind == 0; d[m, 2] = rng.choice([1e-30, -1e-30, 1e-12, -1e-7], m.sum()); d[m, 0] = rng.choice([-1.0, 1.0], m.sum())     # along x, all but flat in z
    m = kind == 1; d[m, 0] = rng.choice([1e-30, -1e-30, 1e-12, -1e-7], m.sum()); d[m, 2] = rng.choice([-1.0, 1.0], m.sum())     # along z
    m = kind == 2; d[m, 0] = rng.choice([-1.0, 1.0], m.sum()); d[m, 2] = d[m, 0] * rng.choice([-1.0, 1.0], m.sum())               # |dx| == |dz|: the major axis' tie
    m = kind == 3; d[m, 1] = rng.choice([1e-30, -1e-30, 1e-9, -1e-6, 1e-3], m.sum())                                               # all but horizontal
    m = kind == 4; d[m, 0] *= 1e-6; d[m, 2] *= 1e-6; d[m, 1] = rng.choice([-1.0, 1.0], m.sum())                                    # all but vertical
    m = kind == 5; d[m] *= rng.choice([1e-9, 1e-4, 1e4, 1e9], m.sum())[:, None]                                                    # |d|^2 at and beyond the walk's preconditions
    return np.ascontiguousarray(np.concatenate([o, d], 1), np.float32)


def random_world(rt, seed, n, nx, ny, big=6, air=0.3, outside=0.05, ghosts=0.03):
    """a caller-built world (not create_world): spheres of many sizes, in the air, overlapping, some outside the
    octree's root box (dropped with the reference's 'not in range' message), some ghost slots, every material"""
    rng = np.random.default_rng(seed)
    sp = np.zeros(n, rt.sphere_dtype)
    sp["center"][:, 0] = rng.uniform(-10.5, 10.5, n)
    sp["center"][:, 2] = rng.uniform(-10.5, 10.5, n)
    sp["radius"] = rng.choice([0.03, 0.05, 0.1, 0.1, 0.1, 0.15, 0.2, 0.3], n)
    sp["center"][:, 1] = sp["radius"]
    up = rng.random(n) < air
    sp["center"][up, 1] = rng.uniform(0.0, 1.9, up.sum())
    bigs = rng.choice(np.arange(1, n), big, replace=False)
    sp["radius"][bigs] = rng.uniform(0.6, 1.4, big)
    sp["center"][bigs, 1] = rng.uniform(0.2, 1.2, big)
    out = rng.random(n) < outside
    sp["center"][out, 0] = rng.uniform(11.5, 14.0, out.sum())
    sp["material"] = rng.choice([rt.MAT_LAMBERTIAN, rt.MAT_LAMBERTIAN, rt.MAT_METAL, rt.MAT_DIELECTRIC], n)
    sp["albedo"] = rng.uniform(0.05, 1.0, (n, 3))
    sp["param"] = np.where(sp["material"] == rt.MAT_METAL, rng.uniform(0, 1, n), np.where(sp["material"] == rt.MAT_DIELECTRIC, 1.5, 0.0))
    g = rng.random(n) < ghosts
    g[0] = False
    sp["material"][g] = rt.MAT_NONE
    sp["center"][g] = 0; sp["radius"][g] = 0; sp["albedo"][g] = 0; sp["param"][g] = 0
    sp[0] = ((0.0, -1000.0, -1.0), 1000.0, rt.MAT_LAMBERTIAN, (0.5, 0.5, 0.5), 0.0)      # ground stays slot 0 (hitTree tests it first)
    cam = rt.camera_init((rng.uniform(8, 14), rng.uniform(1, 4), rng.uniform(-4, 4)), (0, 0.3, 0), (0, 1, 0), 35.0,
                         np.float32(nx) / np.float32(ny), 0.05, 10.0)
    return sp, cam


def orbit_camera(rt, deg, nx, ny):
    """create_world's camera (lookfrom (13, 2, 3), 30 degrees, aperture 0.1, focus 10) with lookfrom turned about the y axis"""
    th = math.radians(deg)
    lookfrom = (13 * math.cos(th) + 3 * math.sin(th), 2.0, -13 * math.sin(th) + 3 * math.cos(th))
    return rt.camera_init(lookfrom, (0, 0, 0), (0, 1, 0), 30.0, nx / ny, 0.1, 10.0)


def half_bits(t):
    """a binary16 device tensor's patterns"""
    return t.cpu().numpy().view(np.uint16)


def f32_to_half_bits(a):
    """the binary16 patterns of float values (the oracle returns exact float images of its binary16 values)"""
    return np.ascontiguousarray(a, np.float32).astype(np.float16).view(np.uint16)
