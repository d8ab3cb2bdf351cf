"""Worlds for the branches of the shading code that create_world and world_cases.random_world never reach: several refractive
indices in one world (below, at and above 1; 0, negative, inf and NaN), negative radii (hollow glass shells, inward-facing rooms the
camera cannot see out of), albedo 0 and 1e30, fuzz exactly 0 and 1, a radius of 0 and of NaN, a lens radius of 0, slot 0 as a ghost
and as the room itself.

Plain deterministic numpy builders (a helper module, not a conftest): `world(name, nx, ny, ...)` returns (spheres, camera) — the
spheres as a structured array with the layout of rt_amd.sphere_dtype, the camera as the 22 floats of rt_camera / camera.h — for
rt_amd.World(spheres=, camera=) through `gpu_world` and for OracleScene(custom=) through `oracle`.  The same floats go to both sides.

Used by tests/test_material_edge_worlds_host.py (the oracle alone: every world reaches the branch it is named for) and
tests/test_gpu_material_edges.py (the kernels against the oracle, bit for bit)."""
import numpy as np

F = np.float32
MAT_NONE, LAMBERTIAN, METAL, DIELECTRIC = -1, 0, 1, 2
sphere_dtype = np.dtype([("center", "<f4", 3), ("radius", "<f4"), ("material", "<i4"), ("albedo", "<f4", 3), ("param", "<f4")])

INDICES = (1.5, 1.0, 2.0 / 3.0, 2.4, 0.3)
ROOMS = {"white_room": (LAMBERTIAN, (1.0, 1.0, 1.0), 0.0), "mirror_room": (METAL, (0.97, 0.97, 0.97), 0.0),
         "tir_room": (DIELECTRIC, (1.0, 1.0, 1.0), 0.3)}
ROOM_CENTER, ROOM_RADIUS = (0.0, 0.5, -0.5), -8.0
# (name, variant) of every world the tests run
WORLDS = [("glass_indices", None), ("shells", None), ("shells", "solid"), ("shells", "hollow"), ("white_room", None), ("mirror_room", None),
          ("tir_room", None), ("extremes", None), ("extremes", "ghost0")]
# lookfrom, lookat, vup, vfov, aperture, focus distance: at (0, 1, 4.5), looking down -z; the rooms and the open scenes through an
# almost-pinhole lens, `extremes` through a lens of radius exactly 0 (the disk is still drawn, then scaled by 0)
CAMERA = dict(lookfrom=(0.0, 1.0, 4.5), lookat=(0.0, 1.0, 3.5), vup=(0.0, 1.0, 0.0), vfov=60.0, aperture=0.02, focus=4.0)
GROUND = ((0.0, -1000.0, -1.0), 1000.0, LAMBERTIAN, (0.5, 0.5, 0.5), 0.0)
GHOST = ((0.0, 0.0, 0.0), 0.0, MAT_NONE, (0.0, 0.0, 0.0), 0.0)


# ---------------------------------------------------------------------------------------------------- camera
def _unit(a):
    return a / np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], -(a[0] * b[2] - a[2] * b[0]), a[0] * b[1] - a[1] * b[0]], F)


def camera_floats(nx, ny, aperture=None):
    """camera::camera (camera.h:22-44) for CAMERA in binary32, one rounding per operation as oracle/rt_oracle.hpp make_camera does it:
    origin, lower_left_corner, horizontal, vertical, u, v, w, lens_radius.  The view is axis-aligned, so every vector operation is
    exact or a single correctly rounded numpy operation."""
    c = CAMERA
    aperture = c["aperture"] if aperture is None else aperture
    lookfrom, lookat, vup = (np.array(c[k], F) for k in ("lookfrom", "lookat", "vup"))
    aspect = F(nx) / F(ny)
    lens_radius = F(aperture) / F(2.0)
    theta = F(c["vfov"]) * F(3.14159265358979323846) / F(180.0)
    arg = theta / F(2.0)
    half_height = F(np.tan(np.float64(arg)))
    half_width = aspect * half_height
    focus = F(c["focus"])
    w = _unit(lookfrom - lookat)
    u = _unit(_cross(vup, w))
    v = _cross(w, u)
    llc = ((lookfrom - (half_width * focus) * u) - (half_height * focus) * v) - focus * w
    horizontal = ((F(2.0) * half_width) * focus) * u
    vertical = ((F(2.0) * half_height) * focus) * v
    return np.concatenate([lookfrom, llc, horizontal, vertical, u, v, w, [lens_radius]]).astype(F)


def library_camera(rt, nx, ny, aperture=None, precision=0):
    """the same camera from the library's rt_camera_init"""
    c = CAMERA
    aspect = float(F(nx) / F(ny)) if precision == 0 else float(np.float16(nx) / np.float16(ny))
    cam = rt.camera_init(c["lookfrom"], c["lookat"], c["vup"], c["vfov"], aspect, c["aperture"] if aperture is None else aperture,
                         c["focus"], precision=precision)
    return cam.view(F).ravel().copy()


# ---------------------------------------------------------------------------------------------------- spheres
def _pack(recs):
    sp = np.zeros(len(recs), sphere_dtype)
    for i, r in enumerate(recs):
        sp[i] = r
    return sp


def _room_field(seed, n=300):
    """slots 1..n-1 of the rooms: spheres all over the view volume, every material, albedo channels that are exactly 0, 0.5 or 1, fuzz
    exactly 0, 0.5 or 1, five refractive indices; every second dielectric is followed by a concentric shell of radius -0.9 r with the
    same index (hollow glass); 3 % ghost slots"""
    rng = np.random.default_rng(seed)
    recs = [None]
    glass = 0
    while len(recs) < n:
        if rng.random() < 0.03:
            recs.append(GHOST)
            continue
        c = tuple(float(v) for v in rng.uniform([-5, -2, -5], [5, 3, 3]))
        r = float(rng.choice([0.1, 0.2, 0.3, 0.5]))
        kind = int(rng.choice([LAMBERTIAN, METAL, DIELECTRIC, DIELECTRIC]))
        alb = tuple(float(v) for v in rng.choice([0.0, 0.5, 1.0, 1.0], 3))
        param = float(rng.choice([0.0, 0.5, 1.0])) if kind == METAL else float(rng.choice(INDICES)) if kind == DIELECTRIC else 0.0
        recs.append((c, r, kind, alb, param))
        if kind == DIELECTRIC:
            glass += 1
            if glass % 2 == 0 and len(recs) < n:
                recs.append((c, -0.9 * r, DIELECTRIC, alb, param))
    return recs


def _open_scene(seed, shells, variant, n=300):
    """ground; three big glass balls between the camera and the field; a front row of nine glass beads (r = 0.2) close to the camera;
    75 more dielectrics, 15 of each index in four sizes (3 % of all slots are ghosts and take a few of them: the host test guards
    >= 10 of each index); lambertian and metal spheres as random_world draws them.

    shells: dielectrics get a concentric partner of negative radius right behind them in the list — every one of r <= 0.2 a partner of
    -0.5 r, every second larger one -0.9 r or -0.5 r in turn.  buildOctree grows a node's box by the radius, so a negative radius
    shrinks it: a shell stays in the tree only if its centre lies deeper than |r| inside a leaf cell, and the cells are 0.25 high.
    Therefore the small dielectrics float at the mid-height of a cell (y = 0.125 + 0.25 k), where |r| <= 0.1 fits: those shells are
    in the tree, the larger ones only in the list.  Four free-standing negative-radius spheres (lambertian and metal, one pair large,
    one pair small enough for the tree) stand in view, and a variant puts the camera inside a solid glass ball or inside the cavity of
    a hollow one."""
    rng = np.random.default_rng(seed)
    recs = [GROUND,
            ((-1.7, 0.8, 1.6), 0.8, DIELECTRIC, (0.3, 0.6, 0.9), 1.5),
            ((0.0, 0.8, 1.0), 0.8, DIELECTRIC, (0.3, 0.6, 0.9), 2.0 / 3.0),
            ((1.7, 0.8, 1.6), 0.8, DIELECTRIC, (0.3, 0.6, 0.9), 2.4)]
    for k in range(9):
        recs.append(((-1.4 + 0.35 * k, (0.375, 0.625, 0.875)[k % 3], 3.0), 0.2, DIELECTRIC, (0.9, 0.6, 0.3), INDICES[k % 5]))
    glass = []
    for k in range(75):
        r = (0.1, 0.2, 0.3, 0.5)[(k // 5) % 4]
        glass.append((r, INDICES[k % 5]))
    order = rng.permutation(n - len(recs))
    for slot in order:
        if rng.random() < 0.03:
            recs.append(GHOST)
            continue
        x, z = float(rng.uniform(-5, 5)), float(rng.uniform(-5, 3))
        if slot < len(glass):
            r, ri = glass[slot]
            kind, alb, param = DIELECTRIC, tuple(float(v) for v in rng.uniform(0.05, 1.0, 3)), ri
        else:
            r = float(rng.choice([0.1, 0.15, 0.2, 0.3]))
            kind = int(rng.choice([LAMBERTIAN, LAMBERTIAN, METAL]))
            alb = tuple(float(v) for v in rng.uniform(0.05, 1.0, 3))
            param = float(rng.uniform(0, 1)) if kind == METAL else 0.0
        y = float(rng.uniform(0.0, 1.9)) if rng.random() < 0.3 else r
        if kind == DIELECTRIC and r <= 0.2:
            y = 0.125 + 0.25 * int(rng.integers(0, 8))
        recs.append(((x, y, z), r, kind, alb, param))
    if not shells:
        return recs
    out, k = [], 0
    for rec in recs:
        out.append(rec)
        if rec[2] == DIELECTRIC:
            if rec[1] <= 0.2:
                out.append((rec[0], -0.5 * rec[1], DIELECTRIC, rec[3], rec[4]))
                continue
            if k % 2 == 0:
                out.append((rec[0], (-0.9, -0.5)[(k // 2) % 2] * rec[1], DIELECTRIC, rec[3], rec[4]))
            k += 1
    out.append(((-0.9, 0.45, 2.6), -0.45, LAMBERTIAN, (0.9, 0.8, 0.2), 0.0))
    out.append(((0.9, 0.45, 2.6), -0.45, METAL, (0.9, 0.9, 0.9), 0.1))
    out.append(((-0.3, 0.375, 3.5), -0.1, LAMBERTIAN, (0.9, 0.8, 0.2), 0.0))
    out.append(((0.3, 0.375, 3.5), -0.1, METAL, (0.9, 0.9, 0.9), 0.1))
    if variant in ("solid", "hollow"):
        out.append((CAMERA["lookfrom"], 0.6, DIELECTRIC, (1.0, 1.0, 1.0), 1.5))
        if variant == "hollow":
            out.append((CAMERA["lookfrom"], -0.54, DIELECTRIC, (1.0, 1.0, 1.0), 1.5))
    else:
        assert variant is None, variant
    return out


def _extremes(seed, variant, n=300):
    """albedo channels of 0, 0.5, 1 and 1e30 (two bounces overflow the attenuation; inf * 0 is a NaN sample), fuzz exactly 0 and 1,
    dielectrics with ref_idx 0, -1.5, +inf and NaN in the front row, a lambertian of radius 0 at a representable centre, spheres of
    radius NaN and inf (never hit; the accelerator builds must keep them out of their grids), and — variant ghost0 — no ground: slot 0
    is a ghost"""
    assert variant in (None, "ghost0"), variant
    rng = np.random.default_rng(seed)
    inf, nan = float("inf"), float("nan")
    recs = [GROUND if variant is None else GHOST]
    for x, ri in ((-2.25, 0.0), (-0.75, -1.5), (0.75, inf), (2.25, nan)):
        recs.append(((x, 0.5, 1.5), 0.5, DIELECTRIC, (1.0, 1.0, 1.0), ri))
    recs += [((-1.5, 0.3, 2.75), 0.3, LAMBERTIAN, (1e30, 1e30, 1e30), 0.0), ((-0.9, 0.3, 2.75), 0.3, LAMBERTIAN, (1e30, 0.5, 0.0), 0.0),
             ((1.5, 0.3, 2.75), 0.3, LAMBERTIAN, (0.0, 1e30, 1.0), 0.0), ((0.9, 0.3, 2.75), 0.3, METAL, (1e30, 1e30, 1e30), 1.0),
             ((0.0, 0.3, 2.75), 0.3, LAMBERTIAN, (0.0, 0.0, 0.0), 0.0),
             ((0.5, 0.75, 2.0), 0.0, LAMBERTIAN, (0.5, 0.5, 0.5), 0.0),
             ((-3.0, 1.0, -2.0), nan, LAMBERTIAN, (0.5, 0.5, 0.5), 0.0), ((3.0, 1.0, -2.0), inf, METAL, (0.5, 0.5, 0.5), 0.0)]
    while len(recs) < n:
        c = tuple(float(v) for v in rng.uniform([-5, 0, -5], [5, 2, 1]))
        r = float(rng.choice([0.1, 0.2, 0.3]))
        kind = int(rng.choice([LAMBERTIAN, LAMBERTIAN, METAL, DIELECTRIC]))
        alb = tuple(float(v) for v in rng.choice([0.0, 0.5, 1.0, 1e30], 3, p=[0.2, 0.4, 0.3, 0.1]))
        param = float(rng.choice([0.0, 1.0])) if kind == METAL else 1.5 if kind == DIELECTRIC else 0.0
        recs.append((c, r, kind, alb, param))
    return recs


def spheres(name, variant=None):
    if name in ROOMS:
        assert variant is None, variant
        recs = _room_field(7)
        kind, alb, param = ROOMS[name]
        recs[0] = (ROOM_CENTER, ROOM_RADIUS, kind, alb, param)
        return _pack(recs)
    if name == "glass_indices":
        assert variant is None, variant
        return _pack(_open_scene(3, False, None))
    if name == "shells":
        return _pack(_open_scene(3, True, variant))
    if name == "extremes":
        return _pack(_extremes(5, variant))
    raise KeyError(name)


def world(name, nx, ny, variant=None, rt=None):
    """(spheres, the camera's 22 floats); rt given: the camera comes from the library's rt_camera_init"""
    aperture = 0.0 if name == "extremes" else None
    cam = camera_floats(nx, ny, aperture) if rt is None else library_camera(rt, nx, ny, aperture)
    return spheres(name, variant), cam


def half_world(rt, name, nx, ny, variant=None):
    """the world in binary16: every sphere value rounded to binary16, the camera from rt_camera_init in binary16 arithmetic"""
    sp = spheres(name, variant)
    for f in ("center", "radius", "albedo", "param"):
        sp[f] = np.asarray(sp[f], F).astype(np.float16).astype(F)
    return sp, library_camera(rt, nx, ny, 0.0 if name == "extremes" else None, precision=rt.FP16)


def with_index(sp, ri=1.5):
    """the same geometry, every dielectric's ref_idx replaced"""
    out = sp.copy()
    out["param"][out["material"] == DIELECTRIC] = ri
    return out


def with_positive_radii(sp):
    out = sp.copy()
    out["radius"] = np.abs(out["radius"])
    return out


def negative(sp):
    """indices of the hittable negative-radius spheres"""
    return np.flatnonzero((sp["material"] != MAT_NONE) & (sp["radius"] < 0))


def oracle(sp, cam, nx, ny, tree=False, spl=30, fp16=False):
    from oracle_lib import OracleScene
    geom = np.concatenate([sp["center"], sp["radius"][:, None]], 1)
    mat = np.concatenate([sp["albedo"], sp["param"][:, None]], 1)
    return OracleScene(len(sp), nx, ny, fp16=fp16, use_octree=tree, spl=spl, custom=(geom, mat, sp["material"], np.asarray(cam, F).ravel()))


def gpu_world(rt, sp, cam, nx, ny, precision=0):
    assert rt.sphere_dtype == sphere_dtype
    return rt.World(len(sp), nx, ny, precision=precision, spheres=sp, camera=np.asarray(cam, F).ravel().view(rt.camera_dtype))


# ---------------------------------------------------------------------------------------------------- rays
def edge_rays(sp, n, seed):
    """n rays for the hit-record tests: world_cases.random_rays rescaled to the field (half its width); a quarter of the origins
    inside negative-radius spheres or in the glass between a shell and its outer sphere (inside the dielectrics where the world has no
    negative radius); 2 % aimed exactly through the centre of a radius-0 sphere, origin, direction and centre all representable."""
    from world_cases import random_rays
    rng = np.random.default_rng(seed)
    rays = random_rays(n, seed)
    rays[:, [0, 2, 3, 5]] *= F(0.5)
    neg = negative(sp)
    hosts = neg if neg.size else np.flatnonzero((sp["material"] == DIELECTRIC) & (sp["radius"] > 0))
    k = n // 4
    pick = hosts[rng.integers(0, hosts.size, k)]
    c, r = sp["center"][pick].astype(np.float64), np.abs(sp["radius"][pick].astype(np.float64))
    d = rng.normal(size=(k, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    rad = r * rng.uniform(0.0, 0.98, k)
    if neg.size:
        # a shell follows its outer sphere in the list: every second such origin lies in the glass between the two
        outer = np.maximum(pick - 1, 0)
        shell = (pick > 0) & (sp["center"][outer] == sp["center"][pick]).all(axis=1) & (sp["radius"][outer] > 0) & (rng.random(k) < 0.5)
        ro = sp["radius"][outer].astype(np.float64)
        rad = np.where(shell, r + (ro - r) * rng.uniform(0.02, 0.98, k), rad)
    rays[:k, 0:3] = c + d * rad[:, None]
    rays[:k, 3:6] = rng.normal(size=(k, 3))
    zero = np.flatnonzero((sp["material"] != MAT_NONE) & (sp["radius"] == 0))
    if zero.size:
        m = n // 50
        c = sp["center"][zero[rng.integers(0, zero.size, m)]]
        d = rng.integers(-8, 9, (m, 3)).astype(F) * F(0.125)
        d[(d == 0).all(axis=1)] = F(1.0)
        steps = rng.integers(1, 9, m).astype(F)
        rays[k:k + m, 0:3] = c - d * steps[:, None]
        rays[k:k + m, 3:6] = d
    return np.ascontiguousarray(rays, F)
