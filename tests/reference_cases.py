"""The worlds, ray sets and the lockstep walk with which the oracle is held to a build of the reference's own headers
(tests/test_reference_pins_host.py), from which tests/golden/make_reference_golden.py records its fixtures, and which the fixture
tests rebuild (tests/test_reference_fixtures_host.py, tests/test_gpu_reference_fixtures.py).  A helper module: no tests here.

A "side" is anything with trace(rays, mode) and scatter(sphere, rays, recs, states): ref_lib.RefWorld or oracle_lib.OracleScene."""
import hashlib
import types

import numpy as np

import material_edge_worlds as mw
import oracle_lib
from denoise_model import guide_rays
from world_cases import lattice_rays, random_rays, random_world

F = np.float32
NX, NY = 64, 40
MAX_DEPTH = 50                       # main.cu:47
GX, GY = 12, 8                       # the frame whose pixel-centre rays open every recorded ray set (rt_render_guides' rays)

# name -> (kind of world, arguments, SPHERES_PER_LEAF of its tree)
CREATED = {"created_22": (22, 30), "created_500": (500, 30), "created_10000": (10000, 32)}
RANDOM = {"random_1": (1, 300, 30), "random_2": (2, 3000, 40), "random_3": (3, 12000, 64)}
EDGE = {"%s%s" % (n, "_" + v if v else ""): (n, v) for n, v in mw.WORLDS}
NAMES = list(CREATED) + list(RANDOM) + list(EDGE)
# more trees: buckets of 3 and 4 that overflow
SMALL_BUCKETS = [("created_10000", 3), ("random_3", 4), ("random_2", 3), ("created_10000", 4)]


def half(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, F).astype(np.float16).astype(F)


_host_rt = types.SimpleNamespace(sphere_dtype=mw.sphere_dtype, MAT_NONE=-1, MAT_LAMBERTIAN=0, MAT_METAL=1, MAT_DIELECTRIC=2,
                                 camera_init=lambda *a: oracle_lib.make_camera(*a))


def world(name, fp16=False):
    """(geom N x 4, mat N x 4, kind N, camera 22 floats, spl) — in binary16 every value is the binary16 image of the fp32 world's"""
    if name in CREATED:
        n, spl = CREATED[name]
        S = oracle_lib.OracleScene(n, 1200, 800, fp16=fp16)
        geom, mat, kind = S.spheres()
        cam = S.camera()
    else:
        if name in RANDOM:
            seed, n, spl = RANDOM[name]
            sp, cam = random_world(_host_rt, seed, n, 72, 48)
        else:
            spl = 30
            sp, cam = mw.world(EDGE[name][0], NX, NY, EDGE[name][1])
        geom = np.concatenate([sp["center"], sp["radius"][:, None]], 1).astype(F)
        mat = np.concatenate([sp["albedo"], sp["param"][:, None]], 1).astype(F)
        kind, cam = sp["material"].astype(np.int32), np.asarray(cam, F).ravel()
        if fp16:
            geom, mat, cam = half(geom), half(mat), half(cam)
    return geom, mat, kind, cam, spl


def tag(name, fp16):
    return "%s_%s" % (name, "fp16" if fp16 else "fp32")


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def world_of(gold, name, fp16):
    """the world, checked against the digest taken when the fixtures were recorded"""
    w = world(name, fp16)
    assert np.array_equal(sha(*w[:4]), gold["hits"][tag(name, fp16) + "_world_sha"]), "the world builder of %s changed: re-record the fixtures" % name
    return w


def as_spheres(geom, mat, kind):
    sp = np.zeros(kind.size, mw.sphere_dtype)
    sp["center"], sp["radius"], sp["material"], sp["albedo"], sp["param"] = geom[:, :3], geom[:, 3], kind, mat[:, :3], mat[:, 3]
    return sp


def oracle_side(w, fp16=False, spl=None, tree=True):
    geom, mat, kind, cam, wspl = w
    return oracle_lib.OracleScene(kind.size, NX, NY, fp16=fp16, use_octree=tree, spl=spl or wspl, custom=(geom, mat, kind, cam))


def reference_side(w, fp16=False, spl=None):
    import ref_lib
    geom, mat, kind, cam, wspl = w
    return ref_lib.RefWorld(geom, mat, kind, fp16=fp16, spl=spl or wspl)


# ---------------------------------------------------------------------------------------------------- rays
def ray_set(name, w, n):
    """GX * GY pixel-centre rays of the world's camera, then n rays on the lattice of the candidate strips (created worlds: the grid
    is given here as 64 columns over the root box, the seams of the tree's own cells among them), random_rays or edge_rays"""
    geom, mat, kind, cam, _ = w
    c = np.zeros(1, np.dtype([("origin", "<f4", 3), ("lower_left_corner", "<f4", 3), ("horizontal", "<f4", 3), ("vertical", "<f4", 3)]))
    c["origin"], c["lower_left_corner"], c["horizontal"], c["vertical"] = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    head = guide_rays(c[0], GX, GY)
    if n == 0:
        return head
    if name in CREATED:
        info = dict(grid_dim=64, cell_size=22.0 / 64)
        rest = lattice_rays(info, geom[:, :3].astype(np.float64), geom[:, 3].astype(np.float64), n, 4242 + kind.size)
    elif name in RANDOM:
        rest = random_rays(n, 500 + RANDOM[name][0])
    else:
        rest = mw.edge_rays(as_spheres(geom, mat, kind), n, 11)
    return np.ascontiguousarray(np.concatenate([head, rest]), F)


def camera_samples(cam, npaths, fp16, uniform, init, get_ray):
    """npaths camera rays as render() makes them (main.cu:104-106) for pixel p % (NX * NY) of an NX x NY frame, seed 1984 + p:
    two draws for (s, t), then get_ray.  uniform / init / get_ray belong to ONE side; returns (rays, states after)."""
    p = np.arange(npaths)
    st = init(1984 + p.astype(np.uint64))
    i, j = (p % NX).astype(F), ((p // NX) % NY).astype(F)
    du, st = uniform(st)
    dv, st = uniform(st)
    if fp16:
        with np.errstate(over="ignore"):
            s = ((i + du).astype(np.float16) / np.float16(NX)).astype(F)
            t = ((j + dv).astype(np.float16) / np.float16(NY)).astype(F)
    else:
        s, t = (i + du) / F(NX), (j + dv) / F(NY)
    return (s, t) + tuple(get_ray(cam, s, t, st))


def trace(side, rays, mode, threads=8):
    """side.trace(rays, mode), the rays split over a few threads where there is work for them (the libraries only read the world;
    ctypes releases the interpreter lock)"""
    rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
    if rays.shape[0] * side.n < 200_000:
        return side.trace(rays, mode)
    from concurrent.futures import ThreadPoolExecutor
    if mode == 2 and hasattr(side, "build_octree"):
        side.build_octree()                          # (built on first use: before the threads, not by each of them)
    parts = [p for p in np.array_split(rays, threads) if len(p)]
    with ThreadPoolExecutor(threads) as ex:
        outs = list(ex.map(lambda p: side.trace(p, mode), parts))
    return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}


def recs_of(h):
    return np.concatenate([h["t"][:, None], h["p"], h["normal"]], 1).astype(F)


def walk(ref, rays, states, kinds, other=None, on_bounce=None):
    """Lockstep paths: for up to MAX_DEPTH bounces the reference side traces every live ray through the list and through the tree
    and scatters from the record of the tree (even paths) or the list (odd paths); `other`, if given, does the same from the same
    inputs and on_bounce(depth, live, inputs, ref_out, other_out) compares.  The walk continues along the REFERENCE's outputs.
    A path ends on a miss, a false return, a ghost slot's record (see test_reference_pins_host.py), or a dielectric bounce whose draw is exactly 1.0 (there the reference
    may return an uninitialised direction: counted in stats['excluded'], its direction not compared).  Returns stats."""
    import ref_lib
    rays, states = np.array(rays, F), np.array(states, np.uint32)
    live = np.arange(rays.shape[0])
    stats = dict(bounces=0, records=0, excluded=0, ghost_records=0, depth_limit=0, absorbed=0, misses=0)
    for depth in range(MAX_DEPTH):
        if live.size == 0:
            break
        r = rays[live]
        tl, tt = trace(ref, r, 1), trace(ref, r, 2)
        otl, ott = (trace(other, r, 1), trace(other, r, 2)) if other is not None else (None, None)
        stats["records"] += 2 * live.size
        odd = (live % 2) == 1
        pick = {k: np.where(odd if tl[k].ndim == 1 else odd[:, None], tl[k], tt[k]) for k in tl}
        ghost = pick["sphere"] == -2
        stats["ghost_records"] += int(ghost.sum())
        go = (pick["hit"] == 1) & ~ghost
        stats["misses"] += int((pick["hit"] == 0).sum())
        idx = np.flatnonzero(go)
        sph, rin, rec, st = pick["sphere"][idx], r[idx], recs_of(pick)[idx], states[live][idx]
        draw = ref_lib.curand_uniform(st, ref.fp16)[0]
        ub = (kinds[sph] == mw.DIELECTRIC) & (draw == F(1.0))
        out = ref.scatter(sph, rin, rec, st)
        oout = other.scatter(sph, rin, rec, st) if other is not None else None
        stats["bounces"] += idx.size
        stats["excluded"] += int(ub.sum())
        stats["absorbed"] += int((out[0] == 0).sum())
        if on_bounce is not None:
            on_bounce(depth, live, dict(rays=r, list=tl, tree=tt, olist=otl, otree=ott, idx=idx, sphere=sph, rin=rin, rec=rec, states=st, excluded=ub),
                      out, oout)
        keep = (out[0] == 1) & ~ub
        rays[live[idx]] = out[2]
        states[live[idx]] = out[3]
        live = live[idx][keep]
    stats["depth_limit"] = int(live.size)
    return stats
