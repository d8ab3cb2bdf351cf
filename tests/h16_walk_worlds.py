"""Worlds and rays AT the rules of the binary16 tree walk (csrc/rt_kernels_fp16.hip, closest_tree), and a numpy model of that walk.

closest_tree replaces the reference's per-ray hitTree by a wave-wide scheme: level-2 expansions pooled up to kTask = 384, big segments
(a level-3 node of >= kSmallPairs = 8 pairs) up to kBig = 128, small ones up to kSmall = 256, spans of kPP = 10 pairs per lane and pass,
a candidate queue of kCand = 128 records, packed two-sphere tests with a NaN half padding an odd node, and an atomicMin on
(t bits << 32 | entry index + 1) that has to reproduce "the first visited sphere among equal t".  Random rays almost never sit at any
of these; the worlds and ray sets here do, and `model` shows on the CPU where every input sits.

Every coordinate, radius and ray component is an exact binary16 number (asserted where the arrays are built): the binary16 twin of a
world is the same list.  The level-3 cells are 2.75 x 0.25 x 2.75, cell (ix, iy, iz) starting at (-11 + 2.75 ix, 0.25 iy, -11 + 2.75 iz).

A sphere of radius 1/64 is hit in binary16 only from close by: c = dot(oc, oc) - r^2 loses r^2 = 2^-12 once |oc|^2 >= 1/2.  Rays that
must HIT such spheres from outside the root box therefore start just above it, at y = 2 + 1/64, over cells of the top layer (iy = 7).

Worlds (slot 0 the ground, SPHERES_PER_LEAF 30):
  leaf_sizes  seven cells of the top layer hold exactly 1, 2, 13, 14, 15, 16 and 17 one-cell spheres of radius 1/64 - 1, 1, 7, 7, 8, 8
              and 9 pairs: small, small, small, small, big, big, big, a NaN half in the odd ones.  The spheres of a cell lie on a line,
              1/16 apart.  The cell of 17 is cell (7, 7, 7), the last node of the tree's pre-order: its 9 pairs end the pair array and
              every pass of 10 pairs over it reads past the array's end.
  twins       pairs of spheres with identical centre and radius and different materials: the halves of one pair (a cell holding the two);
              two pairs of one cell (entries 0 and 2); a twin on the plane x = 0, which sits in the two cells to either side - the
              earlier cell in pre-order decides; and a twin of slot 0 in slot 1, where slot 0 must win.  Slot 0 of THIS world is a ground
              of radius 100 at (0, -100, 0): the radius 1000 of create_world's ground squares to +inf in binary16, c = inf - inf is a
              NaN, and that sphere never offers anything to a binary16 ray - no tie could be had with it.
  stack       cell (3, 7, 4) holds 16 concentric spheres of radii 1/64 .. 16/64 around its centre.  Those of radius >= 1/8 reach the cell
              below, (3, 6, 4), which holds 9 (5 pairs: small); nothing else is touched.
  tmin        spheres of radius 1/4, 1/2 and 1/8 whose axis points are binary16 numbers, and 49 tiny spheres of radius j / 2^20,
              j = 512 .. 560, centred ON the box floor y = 0 (so that the surface point (x, r, z) is a binary16 number).  real_t(0.001f)
              is 1049 / 2^20.  In binary16 r^2 of a tiny sphere is a subnormal, a multiple of 2^-24, so the far root of a ray from the
              surface through the centre is r + sqrt(k 2^-24) and not 2 r: with k = 4 the radii 536, 537 and 538 / 2^20 put it one ulp
              below, at and one ulp above t_min (the radii 524 .. 525 / 2^20, whose 2 r brackets t_min, are in the sweep as well).

Ray sets: `aimed` (64-ray waves from above the box at one cell, every lane through it; `aimed_mix`: the seven cells' sets interleaved
lane by lane), `surface_rays` (tmin), `on_planes` (one or two
direction components +-0, origins exactly on box planes: 0/0 and +-inf slab parameters), `flood` (rays that pass every node of the tree,
alone and mixed with sky rays in one wave), `BATCHES` (launch sizes).

`model(tree, spheres, rays)` is closest_tree's input seen from the reference: everything numpy, binary16 with one rounding per operation
(numpy's float16 arithmetic rounds the float32 result once, as rt_real.h does); the tree is the LIBRARY's host tree (`host_tree`: Octree
.nodes() / .leaves()), so insert() is not restated.

A helper module (no tests, not a conftest): tests/test_h16_walk_worlds_host.py shows on the CPU that every input sits where its name
says and holds the model to the oracle; tests/test_gpu_h16_walk.py runs everything through the kernels."""
import collections
import functools

import numpy as np

import build_limit_worlds as bw
import material_edge_worlds as mw

F, H = np.float32, np.float16
LAMBERTIAN, METAL, DIELECTRIC = mw.LAMBERTIAN, mw.METAL, mw.DIELECTRIC
SPL = 30
CREATED_N, CREATED_SPL = 10000, 32                          # rt.World(10000, ..., precision=FP16): the flood's and on_planes' second world
NX, NY, NS = 32, 24, 4                                      # the frames
K_TASK, K_BIG, K_SMALL, K_SMALL_PAIRS, K_PP, K_CAND = 384, 128, 256, 8, 10, 128      # rt_tuning.h / rt_kernels_fp16.hip, restated
T_MIN = H(F(0.001))                                        # real_t(0.001f)
WORLDS = ("leaf_sizes", "twins", "stack", "tmin")
LEAF_CELLS = collections.OrderedDict([(1, (0, 7, 0)), (2, (1, 7, 5)), (13, (3, 7, 2)), (14, (4, 7, 6)), (15, (6, 7, 1)), (16, (5, 7, 4)),
                                      (17, (7, 7, 7))])
STACK_CELL = (3, 7, 4)
TWIN_CELLS = {"pair": (1, 7, 1), "two_pairs": (5, 7, 2), "two_cells": ((3, 7, 5), (4, 7, 5))}
GROUND100 = ((0.0, -100.0, 0.0), 100.0, LAMBERTIAN, (0.5, 0.5, 0.5), 0.0)
TINY_J = np.arange(512, 561)
BATCHES = (1, 63, 64, 65, 129)
FAR = -49152.0
# lookfrom, lookat of the frames: create_world's lens (vfov 30, aperture 0.1) moved to where the special cells are
CAMERAS = {"leaf_sizes": ((9.625, 2.0, 10.0), (9.625, 1.875, 9.625)), "twins": ((0.25, 2.0, 4.5), (0.0, 1.875, 4.125)),
           "stack": ((-0.875, 2.25, 1.875), (-1.375, 1.875, 1.375)), "tmin": ((1.0, 0.75, 3.5), (0.5, 0.5, 3.0))}


def exact16(a):
    """a as float32, asserted to hold binary16 numbers only"""
    a = np.ascontiguousarray(a, F)
    with np.errstate(over="ignore"):
        assert np.array_equal(a, a.astype(H).astype(F), equal_nan=True), "not a binary16 number"
    return a


def cell_lo(cell):
    return (-11.0 + 2.75 * cell[0], 0.25 * cell[1], -11.0 + 2.75 * cell[2])


def cell_centre(cell):
    lo = cell_lo(cell)
    return (lo[0] + 1.375, lo[1] + 0.125, lo[2] + 1.375)


def preorder_key(cell):
    """the position of a level-3 cell in the tree's pre-order: the octant (4 x-high + 2 y-high + z-high) of every level, root first"""
    key = 0
    for level in (2, 1, 0):
        key = key * 8 + 4 * ((cell[0] >> level) & 1) + 2 * ((cell[1] >> level) & 1) + ((cell[2] >> level) & 1)
    return key


# ---------------------------------------------------------------------------------------------------- the worlds
def _albedo(k):
    return (0.25 + 0.125 * (k % 5), 0.5, 0.875 - 0.125 * (k % 3))


def leaf_member_centre(size, j):
    c = cell_centre(LEAF_CELLS[size])
    return (c[0] - 0.5 + j / 16.0, c[1], c[2])


@functools.lru_cache(None)
def _built(name):
    recs = [mw.GROUND]
    if name == "leaf_sizes":
        for size in LEAF_CELLS:
            for j in range(size):
                kind = (LAMBERTIAN, METAL, DIELECTRIC)[(j + size) % 3]
                recs.append((leaf_member_centre(size, j), 1.0 / 64.0, kind, _albedo(j), 0.25 if kind == METAL else 1.5 if kind == DIELECTRIC else 0.0))
    elif name == "twins":
        recs = [GROUND100, (GROUND100[0], GROUND100[1], METAL, (0.875, 0.25, 0.125), 0.0)]       # slot 1: the ground's twin
        a, b = cell_centre(TWIN_CELLS["pair"]), cell_centre(TWIN_CELLS["two_pairs"])
        c = (0.0, 1.875, cell_centre(TWIN_CELLS["two_cells"][0])[2])
        recs += [(a, 1.0 / 16.0, LAMBERTIAN, _albedo(0), 0.0), (a, 1.0 / 16.0, METAL, _albedo(1), 0.25),                      # slots 2, 3
                 (b, 1.0 / 16.0, LAMBERTIAN, _albedo(2), 0.0), ((b[0] + 0.5, b[1], b[2]), 1.0 / 64.0, LAMBERTIAN, _albedo(3), 0.0),
                 (b, 1.0 / 16.0, DIELECTRIC, _albedo(4), 1.5),                                                                # slots 4, 5, 6
                 (c, 1.0 / 16.0, METAL, _albedo(5), 0.0), (c, 1.0 / 16.0, LAMBERTIAN, _albedo(6), 0.0)]                       # slots 7, 8
    elif name == "stack":
        c = cell_centre(STACK_CELL)
        for k in range(1, 17):
            kind = (DIELECTRIC, LAMBERTIAN, METAL)[k % 3]
            recs.append((c, k / 64.0, kind, _albedo(k), 0.25 if kind == METAL else 1.5 if kind == DIELECTRIC else 0.0))
    elif name == "tmin":
        recs += [((-4.0, 1.0, -4.0), 0.25, LAMBERTIAN, _albedo(0), 0.0), ((4.0, 1.0, 4.0), 0.5, METAL, _albedo(1), 0.0),
                 ((0.5, 0.5, 3.0), 0.125, DIELECTRIC, _albedo(2), 1.5)]
        for i, j in enumerate(TINY_J):
            recs.append(((0.25 + i / 32.0, 0.0, 1.0), float(j) / 2.0 ** 20, LAMBERTIAN, _albedo(i), 0.0))
    else:
        raise KeyError(name)
    sp = np.zeros(len(recs), mw.sphere_dtype)
    for i, rec in enumerate(recs):
        sp[i] = rec
    for f in ("center", "radius", "albedo", "param"):
        exact16(sp[f])
    sp.setflags(write=False)
    return sp


TWIN_SLOTS = {"ground": (0, 1), "pair": (2, 3), "two_pairs": (4, 6), "two_cells": (7, 8)}
TMIN_REGULAR, TMIN_TINY0 = (1, 2, 3), 4


def spheres(name):
    return _built(name).copy()


def camera(rt, name, nx=NX, ny=NY):
    """the 22 floats of the frame's camera, from the library's rt_camera_init in binary16 arithmetic"""
    lookfrom, lookat = CAMERAS[name]
    dist = float(np.sqrt(sum((a - b) ** 2 for a, b in zip(lookfrom, lookat))))
    cam = rt.camera_init(lookfrom, lookat, (0.0, 1.0, 0.0), 30.0, float(H(nx) / H(ny)), 0.1, dist, precision=rt.FP16)
    return cam.view(F).ravel().copy()


def pixel_rays(cam, nx=NX, ny=NY):
    """the rays from the camera's origin through the pixel centres, rounded to binary16: what a frame's camera looks at"""
    i, j = np.meshgrid((np.arange(nx) + 0.5) / nx, (np.arange(ny) + 0.5) / ny)
    d = cam[3:6] + i.reshape(-1, 1) * cam[6:9] + j.reshape(-1, 1) * cam[9:12] - cam[0:3]
    return np.concatenate([np.tile(cam[0:3], (nx * ny, 1)), d], 1).astype(H).astype(F)


def gpu_world(rt, name, nx=NX, ny=NY):
    return mw.gpu_world(rt, _built(name), camera(rt, name, nx, ny), nx, ny, precision=rt.FP16)


def oracle(rt, name, nx=NX, ny=NY):
    return mw.oracle(_built(name), camera(rt, name, nx, ny), nx, ny, tree=True, spl=SPL, fp16=True)


# ---------------------------------------------------------------------------------------------------- the library's tree
Tree = collections.namedtuple("Tree", "level parent box members first pairs n_pairs")


def host_tree(O):
    """The library's HOST tree (Octree.nodes() / .leaves(), reference numbering) in the visit order of traverseTree: per node of the
    pre-order its level, the position of its parent, its box, and for a level-3 node its members - the sphere indices of its leaves in
    order (acceleration_structure.h:282-295 stops at the first missing leaf) - with the pair layout that follows from them: a node's
    pairs = (members + 1) // 2, laid out one node after the other in this order."""
    nodes = O.nodes()
    counts, idx = O.leaves()
    level, parent, box, members = [], [], [], []

    def visit(n, par):
        pos = len(level)
        level.append(int(nodes["level"][n])); parent.append(par); box.append(nodes["aabb"][n].copy())
        if nodes["level"][n] == 3:
            m = []
            for leaf in nodes["children"][n]:
                if leaf == 0:
                    break
                m += idx[leaf, :counts[leaf]].tolist()
            members.append(np.array(m, np.int64))
            return
        members.append(np.zeros(0, np.int64))
        for ch in nodes["children"][n]:
            if ch != 0:
                visit(int(ch), pos)
    visit(0, -1)
    pairs = np.array([(len(m) + 1) // 2 for m in members])
    first = np.concatenate([[0], np.cumsum(pairs)[:-1]])
    return Tree(np.array(level), np.array(parent), exact16(np.array(box, F)), members, first, pairs, int(pairs.sum()))


def cell_of(tree, pos):
    """(ix, iy, iz) of a level-3 node"""
    b = tree.box[pos]
    return (int(round((b[0] + 11.0) / 2.75)), int(round(b[1] / 0.25)), int(round((b[2] + 11.0) / 2.75)))


def node_at(tree, cell):
    for pos in np.flatnonzero(tree.level == 3):
        if cell_of(tree, pos) == tuple(cell):
            return int(pos)
    raise KeyError(cell)


# ---------------------------------------------------------------------------------------------------- the model
def _h(a):
    return np.asarray(a).astype(H)


def _offers(o, d, a, c, r2):
    """sphere::hit (sphere.h:17-43) of rays [k] against spheres [m] in binary16: (discriminant > 0, near root, far root, offer,
    discriminant) as [k, m] arrays; the operation order is pair_math's, the roots are FLOAT arithmetic on the converted operands rounded once
    (sphere.h:25 and :36 under USE_FP16).  offer: the near root if > t_min, else the far root if > t_min, else +inf"""
    with np.errstate(all="ignore"):
        ocx, ocy, ocz = (o[:, None, i] - c[None, :, i] for i in range(3))
        dx, dy, dz = (d[:, None, i] for i in range(3))
        b = (ocx * dx + ocy * dy) + ocz * dz
        cc = ((ocx * ocx + ocy * ocy) + ocz * ocz) - r2[None, :]
        disc = b * b - a[:, None] * cc
        pos = disc > H(0)
        nb, A, df = -b.astype(F), a[:, None].astype(F), disc.astype(F)
        sq16 = np.sqrt(df).astype(H).astype(F)
        t1 = ((nb - sq16) / A).astype(H)
        t2 = ((nb + np.sqrt(df)) / A).astype(H)
        offer = np.where(t1 > T_MIN, t1, np.where(t2 > T_MIN, t2, H(np.inf))).astype(F)
        offer = np.where(pos & (offer < np.inf), offer, F(np.inf))
    return pos, t1, t2, offer, disc


def model(tree, sp, rays):
    """closest_tree's input for an [n, 6] ray array, seen from the reference.  Per ray:
      visited        [nodes, n] - the nodes traverseTree visits: the node's box and every ancestor's pass intersect_ray_aabb, with the
                     kernel's quotients rf((plane - o) / d) and the reference's comparisons, NaN and +-inf included
      nan_params     the NaN quotients among the 27 plane parameters of the ray
      nan_node_pass / nan_node_fail   tested nodes (parent visited) with a NaN among their six parameters that pass / fail
      sphere, t      the model's own record: the smallest offered t, the first in visit order among equals, slot 0 first (-1, 0: none)
      ground_t       what slot 0 offers (+inf: nothing)
      offers         dict of flat arrays over every (ray, visited entry) with a positive discriminant: ray, entry (index in the pair
                     array's entry order: 2 * first pair of the node + position), node, sphere, t1, t2, t (the offer, +inf: none)
      positives, zeros, negatives, nans   the visited entries of the ray by the sign of their discriminant (sphere.h:18-22)
    Per wave (64 consecutive rays, as k_trace_h groups them): tasks (level-2 nodes that passed), big and small (segments), pairs,
    positives."""
    rays = exact16(rays).reshape(-1, 6)
    full = rays
    # (the flood repeats its rays: each distinct one once - distinct by BITS: -0 is not +0 in a divisor)
    bits, inverse = np.unique(full.view(np.uint32), axis=0, return_inverse=True)
    rays, inverse = bits.view(F), np.asarray(inverse).ravel()
    n = len(rays)
    o, d = _h(rays[:, :3]), _h(rays[:, 3:])
    c_all, r_all = _h(sp["center"]), _h(sp["radius"])
    with np.errstate(all="ignore"):
        a = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        r2_all = r_all * r_all
        planes = bw.planes(True)
        Q = [((_h(planes[ax])[:, None] - o[None, :, ax]) / d[None, :, ax]).astype(F) for ax in range(3)]       # [9, n] per axis
    nan_params = sum(np.isnan(q).sum(axis=0) for q in Q)
    nn = len(tree.level)
    visited = np.zeros((nn, n), bool)
    nan_pass, nan_fail = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for pos in range(nn):
        bx = tree.box[pos]
        par = visited[tree.parent[pos]] if tree.parent[pos] >= 0 else np.ones(n, bool)
        q = []
        for ax in range(3):
            for side in (0, 3):
                k = np.flatnonzero(planes[ax] == bx[ax + side])
                assert k.size == 1, (pos, bx)
                q.append(Q[ax][k[0]])
        with np.errstate(invalid="ignore"):
            def slab(lo, hi):
                sw = lo > hi
                return np.where(sw, hi, lo), np.where(sw, lo, hi)
            tmin, tmax = slab(q[0], q[1])
            tymin, tymax = slab(q[2], q[3])
            ok = ~((tmin > tymax) | (tymin > tmax))
            tmin = np.where(tymin > tmin, tymin, tmin)
            tmax = np.where(tymax < tmax, tymax, tmax)
            tzmin, tzmax = slab(q[4], q[5])
            ok &= ~((tmin > tzmax) | (tzmin > tmax))
        visited[pos] = par & ok
        has_nan = np.isnan(np.array(q)).any(axis=0) & par
        nan_pass += has_nan & ok
        nan_fail += has_nan & ~ok
    # slot 0, then the visited level-3 nodes in order
    best = np.full(n, np.inf, F)
    sphere = np.full(n, -1, np.int64)
    _, _, _, g, _ = _offers(o, d, a, c_all[:1], r2_all[:1])
    hit0 = g[:, 0] < np.inf
    best[hit0], sphere[hit0] = g[hit0, 0], 0
    positives = np.zeros(n, np.int64)
    signs = {k: np.zeros(n, np.int64) for k in ("zero", "negative", "nan")}
    off = {k: [] for k in ("ray", "entry", "node", "sphere", "t1", "t2", "t")}
    for pos in np.flatnonzero(tree.level == 3):
        K = np.flatnonzero(visited[pos])
        m = tree.members[pos]
        if K.size == 0 or m.size == 0:
            continue
        p, t1, t2, offer, disc = _offers(o[K], d[K], a[K], c_all[m], r2_all[m])
        positives[K] += p.sum(axis=1)
        with np.errstate(invalid="ignore"):
            signs["zero"][K] += (disc == 0).sum(axis=1); signs["negative"][K] += (disc < 0).sum(axis=1); signs["nan"][K] += np.isnan(disc).sum(axis=1)
        j = offer.argmin(axis=1)                                       # (the first among equals)
        tm = offer[np.arange(K.size), j]
        upd = tm < best[K]                                             # sphere.h:29: temp < closest_so_far
        best[K[upd]], sphere[K[upd]] = tm[upd], m[j[upd]]
        kk, mm = np.nonzero(p)
        off["ray"].append(K[kk]); off["entry"].append(2 * tree.first[pos] + mm); off["node"].append(np.full(kk.size, pos))
        off["sphere"].append(m[mm]); off["t1"].append(t1[kk, mm]); off["t2"].append(t2[kk, mm]); off["t"].append(offer[kk, mm])
    l2, l3 = tree.level == 2, tree.level == 3
    big3, small3 = l3 & (tree.pairs >= K_SMALL_PAIRS), l3 & (tree.pairs > 0) & (tree.pairs < K_SMALL_PAIRS)
    per_ray = dict(tasks=visited[l2].sum(axis=0), big=visited[big3].sum(axis=0), small=visited[small3].sum(axis=0),
                   pairs=(visited[l3] * tree.pairs[l3][:, None]).sum(axis=0), positives=positives)
    # back to the launch's rays
    out = dict(visited=visited[:, inverse], nan_params=nan_params[inverse], nan_node_pass=nan_pass[inverse], nan_node_fail=nan_fail[inverse],
               sphere=sphere[inverse], t=np.where(sphere >= 0, best, F(0))[inverse].astype(F), positives=positives[inverse],
               ground_t=g[inverse, 0], zeros=signs["zero"][inverse], negatives=signs["negative"][inverse], nans=signs["nan"][inverse])
    flat = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in off.items()}
    out["offers_unique"] = flat                                        # (rays numbered among the DISTINCT rays: `unique_of` maps a launch's ray)
    out["unique_of"] = inverse
    nw = (len(full) + 63) // 64
    for k, v in per_ray.items():
        w = np.zeros(nw * 64, np.int64)
        w[:len(full)] = v[inverse]
        out["wave_" + k] = w.reshape(nw, 64).sum(axis=1)
    return out


def offers_of(m, ray):
    """the positive-discriminant entries of one ray of the launch, in visit order: dict of arrays (entry, node, sphere, t1, t2, t)"""
    f = m["offers_unique"]
    sel = np.flatnonzero(f["ray"] == m["unique_of"][ray])
    sel = sel[np.argsort(f["entry"][sel], kind="stable")]
    return {k: f[k][sel] for k in f if k != "ray"}


# ---------------------------------------------------------------------------------------------------- rays
V_Y = 9.0 / 64.0                                           # height of an aimed ray's origin above the target: y = 1.875 + 9/64 = 2 + 1/64
SCALES = (1.0, 2.0, 4.0, 8.0, 0.5, 0.25, 16.0, 3.0)


def _aimed_at(targets, vy=V_Y, step=1.0 / 64.0):
    """len(SCALES) waves of 64 rays: lane i starts at its target + v, v = (((i % 8) - 4) / 64, 9 / 64, ((i // 8) - 4) / 64) - above the
    root box - and heads along -v times the wave's scale, through the target.  targets: [64, 3]"""
    i = np.arange(64)
    v = np.stack([((i % 8) - 4) * step, np.full(64, vy), ((i // 8) - 4) * step], 1)
    out = [np.concatenate([targets + v, -v * s], 1) for s in SCALES]
    return exact16(np.concatenate(out))


def aimed(world, cell):
    """64-ray waves aimed at one cell of leaf_sizes (cell: the member count), stack or twins (cell: the arrangement) from above the box:
    lane i aims at the centre of member i % count (stack, twins: at the common centre)"""
    if world == "leaf_sizes":
        t = np.array([leaf_member_centre(cell, i % cell) for i in range(64)])
    elif world == "stack":
        t = np.tile(np.array(cell_centre(STACK_CELL)), (64, 1))
    elif world == "twins":
        t = np.tile(_built("twins")["center"][TWIN_SLOTS[cell][0]].astype(np.float64), (64, 1))
    else:
        raise KeyError(world)
    return _aimed_at(t)


def stack_inside():
    """stack: the aimed waves from INSIDE the stack, 5/64 to 0.09 from its centre: the record is the shell of radius 4/64 or 5/64 just
    ahead of the origin, and the shells below 1/8 are in the stack's cell alone - the cell below, which holds the larger shells a second time,
    cannot supply it"""
    return _aimed_at(np.tile(np.array(cell_centre(STACK_CELL)), (64, 1)), vy=5.0 / 64.0, step=1.0 / 128.0)


def ground_rays():
    """twins: rays from inside the box down onto the ground of radius 100 around (0, 0, 0), where it rises into the bottom cells"""
    rng = np.random.default_rng(8100)
    n = 1024
    o = np.stack([rng.integers(-16, 17, n) / 8.0, rng.integers(1, 9, n) / 8.0, rng.integers(-16, 17, n) / 8.0], 1)
    d = np.stack([rng.integers(-4, 5, n) / 16.0, -np.ones(n), rng.integers(-4, 5, n) / 16.0], 1)
    return exact16(np.concatenate([o, d], 1))


def surface_rays():
    """tmin: unit-direction rays that start exactly ON a sphere: from each of the six axis points of the three regular spheres along all
    six axis directions (outward, inward, four tangents); from the top (x, r, z) of every tiny sphere down (inward, through the
    centre), up (outward) and along +-x (tangent, over the neighbours' tops); from its bottom (x, -r, z), below the box, up and down"""
    sp = _built("tmin")
    axes = [np.array(v, np.float64) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    out = []
    for s in TMIN_REGULAR:
        c, r = sp["center"][s].astype(np.float64), float(sp["radius"][s])
        for p in axes:
            for dd in axes:
                out.append(np.concatenate([c + r * p, dd]))
    for s in range(TMIN_TINY0, len(sp)):
        c, r = sp["center"][s].astype(np.float64), float(sp["radius"][s])
        for p, dirs in ((axes[2], (axes[3], axes[2], axes[0], axes[1])), (axes[3], (axes[2], axes[3]))):
            for dd in dirs:
                out.append(np.concatenate([c + r * p, dd]))
    return exact16(np.array(out))


def on_planes(n=3072, seed=8200):
    """Directions with one or two components +0 or -0; the origin lies exactly on one of the nine planes of such an axis - 0/0, a NaN
    parameter - and, for two thirds of the rays, on a plane of a second axis or of all three (a corner of a cell); every other plane of
    a zero axis has a parameter of +-inf.  The remaining coordinates are binary16 numbers inside the box."""
    rng = np.random.default_rng(seed)
    planes = bw.planes(True)
    for p in planes:                                        # all 27 plane values are binary16 numbers: an origin can lie ON each
        assert len(exact16(p)) == 9
    o = rng.uniform([-11, 0, -11], [11, 2, 11], (n, 3)).astype(H).astype(np.float64)
    d = rng.normal(size=(n, 3)).astype(H).astype(np.float64)
    d[d == 0] = 1.0
    for i in range(n):
        zero = rng.permutation(3)[:1 + i % 2]
        d[i, zero] = rng.choice([0.0, -0.0], zero.size)
        on = [zero[0]] + [ax for ax in range(3) if ax != zero[0]][:(i // 2) % 3]
        for ax in on:
            o[i, ax] = planes[ax][rng.integers(0, 9)]
    return exact16(np.concatenate([o, d], 1))


def sky_rays(n):
    """rays at the sky whose LINE misses the root box too (intersect_ray_aabb has no t >= 0 test): they finish in the walk's first round"""
    i = np.arange(n)
    return exact16(np.stack([30.0 + (i % 16) / 8.0, np.full(n, 3.0), 30.0 + (i // 16) / 8.0, np.full(n, 0.5), np.ones(n), np.full(n, 0.25)], 1))


FLOOD_MIXED = (1, 16, 63, 64)
FLOOD_WITH_HITTERS = (16, 60)


def flood():
    """The first four blocks of test_fp16_rays_that_pass_every_node_of_the_tree (tests/test_gpu_parity.py) - origins at -49152, where
    every box plane lies at the same rounded distance: 512 rays that pass every node, 2048 degenerate on x, 2048 on x and z, 256 with
    direction components of 0.5, 1 and 2 - 76 full waves, then two waves each in which only 1, 16, 63 or 64 lanes are rays that pass
    every node (spread over the wave) and the others point at the sky: 84 waves; then two waves each in which 16 or 60 lanes pass
    every node and the OTHERS are rays from create_world's camera at its three spheres of radius 1: rays of the flood
    offer nothing - their discriminants are NaN - so only these lanes can show a segment that a full pool dropped: 88 waves"""
    from world_cases import random_rays
    rng = np.random.default_rng(5)
    far = F(FAR)
    every = np.array([far, far, far, 1, 1, 1], F)
    a = np.tile(every, (512, 1))
    b = random_rays(2048, 11); b[:, 0] = far; b[:, 3] = np.abs(b[:, 3]) + 0.5
    c = random_rays(2048, 12); c[:, 0] = far; c[:, 2] = far; c[:, 3] = 1.0; c[:, 5] = 1.0
    d = np.tile(every, (256, 1)); d[:, 3:] *= rng.choice([0.5, 1.0, 2.0], (256, 3)).astype(F)
    blocks = [a, b, c, d]
    for cnt in FLOOD_MIXED:
        for rep in range(2):
            w = sky_rays(64)
            lanes = (np.arange(cnt) * (64 // cnt) + rep) % 64 if cnt < 63 else np.arange(cnt) + (rep if cnt == 63 else 0)
            w[lanes] = every
            blocks.append(w)
    # (from create_world's camera at the three spheres of radius 1 that every created world has, (-4, 1, 0), (0, 1, 0), (4, 1, 0))
    tgt = np.array([[-4.0, 1.0, 0.0], [0.0, 1.0, 0.0], [4.0, 1.0, 0.0]])[np.arange(256) % 3] + rng.uniform(-0.4, 0.4, (256, 3))
    hitters = np.concatenate([np.tile([13.0, 2.0, 3.0], (256, 1)), tgt - [13.0, 2.0, 3.0]], 1).astype(F)
    for k, cnt in enumerate(FLOOD_WITH_HITTERS):
        for rep in range(2):
            w = hitters[(2 * k + rep) * 64:(2 * k + rep + 1) * 64].copy()
            w[(np.arange(cnt) * (64 // cnt) + rep) % 64 if cnt < 63 else np.arange(cnt) + rep] = every
            blocks.append(w)
    with np.errstate(over="ignore"):
        r = np.concatenate(blocks).astype(F).astype(H).astype(F)
    return exact16(r)


FLOOD_FULL_WAVES = 76


# ---------------------------------------------------------------------------------------------------- the cases
# (world, ray set): every pair the host test pins and the GPU test runs; "created" is rt.World(10000, ..., precision=FP16), SPL 32
CASES = ([("leaf_sizes", "aimed%d" % s) for s in LEAF_CELLS] + [("leaf_sizes", "aimed_mix"), ("leaf_sizes", "on_planes"), ("created", "on_planes"), ("created", "flood"),
         ("stack", "aimed"), ("stack", "inside"), ("tmin", "surface")] + [("twins", k) for k in ("pair", "two_pairs", "two_cells", "ground")])
IDS = ["%s-%s" % c for c in CASES]


def library_world(rt, world, nx=NX, ny=NY):
    """(rt.World, SPHERES_PER_LEAF) of a world of this module or of "created" """
    if world == "created":
        return rt.World(CREATED_N, nx, ny, precision=rt.FP16), CREATED_SPL
    return gpu_world(rt, world, nx, ny), SPL


@functools.lru_cache(None)
def host_side(rt, world):
    """(the library's host tree as host_tree gives it, the sphere records, the oracle's scene, rt_octree_info of the host build), once"""
    from oracle_lib import OracleScene
    W, spl = library_world(rt, world)
    O = rt.Octree(W, spl)
    S = OracleScene(CREATED_N, NX, NY, fp16=True, use_octree=True, spl=spl) if world == "created" else oracle(rt, world)
    sp = W.spheres.copy()
    for f in ("center", "radius"):
        exact16(sp[f])
    return host_tree(O), sp, S, O.info()


@functools.lru_cache(None)
def host_case(rt, world, rayset):
    """(rays, the model, the oracle's hitTree records) of a case, once; read-only"""
    tree, sp, S, _ = host_side(rt, world)
    rays = case_rays(world, rayset)
    ref = S.trace(rays, mode=2)
    for a in ref.values():
        a.setflags(write=False)
    return rays, model(tree, sp, rays), ref


@functools.lru_cache(None)
def case_rays(world, rayset):
    if rayset == "on_planes":
        r = on_planes()
    elif rayset == "flood":
        r = flood()
    elif rayset == "surface":
        r = surface_rays()
    elif rayset == "ground":
        r = ground_rays()
    elif rayset == "inside":
        r = stack_inside()
    elif rayset == "aimed_mix":
        # lane i of every wave from the set aimed at cell i % 7: big segments of 8, 8 and 9 pairs next to small ones in one pool - the
        # lanes' equal spans (C = ceil(pairs / 64)) no longer end where segments end, and a pass must stop at every segment's end
        sets = [aimed(world, s) for s in LEAF_CELLS]
        r = np.stack([sets[i % len(sets)][i] for i in range(len(sets[0]))])
    elif world == "leaf_sizes":
        r = aimed(world, int(rayset[5:]))
    elif world == "stack":
        r = aimed(world, None)
    else:
        r = aimed(world, rayset)
    r.setflags(write=False)
    return r
