"""Worlds and rays AT the thresholds of the candidate grid (csrc/rt_accel.h, csrc/rt_build.hip, closest_tree), which create_world scenes
and world_cases.random_world never come near: radii a few float steps either side of the radius at which a sphere leaves the grid
(R' = Rlim), centres a few float steps either side of the centre bound 17.5, column ranges and fine bins either side of a floor(),
hittable counts 63 / 64, large counts 64 / 65 and 0 / 8 / 9, the clamps of the cell size, in-tree counts either side of the dense
rule and of the solo rule; ray origins a few float steps either side of the near zone's sphere |o - (0,1,0)| = 24, aimed at grazing
spheres on the far side (|o - c| up to 41.5, the case K2 is sized for), |d|^2 and |d.y| at 2^-40 / 2^40 and their float neighbours,
subnormal and zero d.x / d.z.

A helper module (no tests, not a conftest).  Three parts:
  * `model(spheres, mode, stored)`: the classification of build_accel in numpy float64, restated from DESIGN.md 5.2 / 5.3 / App. A;
  * `world(name, variant)`: deterministic builders, (spheres, camera) with the layout of rt_amd.sphere_dtype / the 22 camera floats;
  * `zone_rays`, `precondition_rays`, `lattice_rays_for` and `fast_path` (the kernel's precondition test in numpy float32).
Used by tests/test_grid_threshold_worlds_host.py and tests/test_gpu_grid_thresholds.py; `python tests/grid_threshold_worlds.py`
prints the counts kept in profiles/r14/grid_thresholds.txt.

Two of the thresholds in build_accel cannot decide anything, and the builders show that instead of reaching them:
  * `!inside` alone never files a sphere as large.  A sphere that passes the other three rules has R' <= Rlim = 1.5 h and (list) |x|, |z|
    <= reach, (tree) |x|, |z| <= 11 + r < 11 + R'; the grid spans reach + 2 Rlim + 2 h = reach + 5 h to either side and `inside` asks for
    |x| + R' < reach + 4 h at the least.  `centre_bound` therefore puts its `inside` probes among spheres beyond the centre bound
    (large either way) - the model still says on which side each lies.
  * the lower clamp h >= 0.05 never binds: R' >= sqrt(K2) + 1e-5 + 2e-3 = 0.0595 for radius 0, so h >= 0.7 * 2 * 0.0595 = 0.083.
    `tiny` (every radius 1e-3) has the smallest cell a world can have; the host test asserts that floor instead of the clamp."""
import functools

import numpy as np

import material_edge_worlds as mw
import oracle_lib
from world_cases import lattice_rays

F = np.float32
NX, NY = 64, 40
MAT_NONE, LAMBERTIAN, METAL, DIELECTRIC = mw.MAT_NONE, mw.LAMBERTIAN, mw.METAL, mw.DIELECTRIC
sphere_dtype = mw.sphere_dtype

# ---------------------------------------------------------------------------------------------------- the model
U = 2.0 ** -24
ZONE, CENTRE_BOUND, SLACK, ROOT_HALF = 24.0, 17.5, 2e-3, 11.0          # App. A.1; the reference's root box spans +-11 in x and z
SPARSE_CELL, DENSE_CELL, FINE, SOLO_DENSITY = 1.0, 0.7, 8, 1.0        # rt_tuning.h
MIN_LIST, MAX_LIST_LARGE, HOT_LARGE = 64, 64, 8
K2 = 2.0 * 16.1 * U * (ZONE + CENTRE_BOUND) * (ZONE + CENTRE_BOUND)    # 16.1 u |o - c|^2 at |o - c| = 41.5, twice over (App. A.1)


def inflated(r2):
    """R' of a sphere of squared radius r2: the ball a ray's line must cross for the float test to be able to pass, plus the slack"""
    return np.sqrt(r2 * (1.0 + 1e-6) + K2) + 1e-5 + SLACK


def stored_set(counts, indices):
    """the spheres a tree stores, from the leaves' (counts, indices) of Octree.leaves() or OracleScene.octree()"""
    counts, indices = np.asarray(counts), np.asarray(indices)
    return np.unique(indices[np.arange(indices.shape[1])[None, :] < counts[:, None]])


def model(sp, mode, stored=None):
    """The grid of a world: mode "list" (members: the hittable spheres behind slot 0) or "tree" (members: the hittable spheres of
    `stored`, slot 0 left out).  Every quantity in float64 from the float32 centres and the float32 product radius * radius."""
    assert mode in ("list", "tree")
    n = len(sp)
    member = np.zeros(n, bool)
    if mode == "list":
        member[1:] = True
    else:
        member[np.asarray(stored, np.int64)] = True
        member[0] = False
    member &= sp["material"] != MAT_NONE
    idx = np.flatnonzero(member)
    m = dict(mode=mode, members=idx, enabled=False, G=0, h=0.0, grid_entries=0, n_large=0, large=np.zeros(0, np.int64), cells=0.0,
             coop_groups=0, solo_chains=0, dense=False)
    if idx.size == 0:
        return m
    x, y, z = (sp["center"][idx, k].astype(np.float64) for k in range(3))
    r2 = (sp["radius"][idx] * sp["radius"][idx]).astype(F).astype(np.float64)
    # cell size: the inflated diameter of the median sphere, within [0.05, 1]; narrower where more than 8 spheres per cell are expected
    rmed = np.sort(np.sqrt(r2))[idx.size // 2]
    h0 = min(1.0, max(0.05, 2.0 * float(inflated(rmed * rmed))))
    g = np.ceil(2.0 * (ROOT_HALF + 5.0 * h0) / h0)
    dense = bool(4.0 * idx.size > 8.0 * g * g)
    h = max(0.05, (DENSE_CELL if dense else SPARSE_CELL) * h0)
    rlim = 1.5 * h
    rp = inflated(r2)
    dc = np.sqrt(x * x + (y - 1.0) * (y - 1.0) + z * z)
    fits = (r2 >= 0.0) & ~(rp > rlim) & (dc <= CENTRE_BOUND)
    # extent: the root box; a list's grid follows its grid spheres out to the centre bound
    reach = ROOT_HALF
    if mode == "list" and fits.any():
        reach = max(reach, float(np.abs(x[fits]).max()), float(np.abs(z[fits]).max()))
    half = reach + 2.0 * rlim + 2.0 * h
    G = int(np.ceil(2.0 * half / h))
    g0 = -half
    lo, hi = g0 + h, g0 + (G - 1) * h
    inside = (x - rp > lo) & (x + rp < hi) & (z - rp > lo) & (z + rp < hi)
    large = ~fits | ~inside
    k = ~large
    col = lambda v: np.clip(np.floor(v).astype(np.int64), 0, G - 1)
    ix0, ix1 = col((x - rp - g0) / h - 1e-4), col((x + rp - g0) / h + 1e-4)
    iz0, iz1 = col((z - rp - g0) / h - 1e-4), col((z + rp - g0) / h + 1e-4)
    fine = lambda c: np.clip(np.floor((c - g0) / h * float(FINE)).astype(np.int64), 0, G * FINE - 1)
    cells = float(((ix1 - ix0 + 1) * (iz1 - iz0 + 1))[k].sum())
    n_large = int(large.sum())
    m.update(h0=h0, g_rule=float(g), dense=dense, h=h, Rlim=rlim, reach=reach, G=G, g0=g0, Rp=rp, dc=dc, inside=inside, is_large=large,
             large=idx[large], grid=idx[k], ix0=ix0, ix1=ix1, iz0=iz0, iz1=iz1, bx=fine(x), bz=fine(z), cells=cells,
             grid_entries=int((ix1 - ix0 + 1)[k].sum()), n_large=n_large,
             ylo=F((y - rp)[k].min() - 1e-4) if k.any() else F(-1e-4), yhi=F((y + rp)[k].max() + 1e-4) if k.any() else F(1e-4),
             rmax=F((rp[k].max() if k.any() else 0.0) + 1e-4),
             coop_groups=4 if cells <= 8.0 * G * G else 1, solo_chains=int(cells <= SOLO_DENSITY * G * G))
    # a tree's grid is on as soon as the tree stores a sphere; a list gets one from 64 hittable spheres on, with at most 64 large ones
    m["enabled"] = True if mode == "tree" else bool(idx.size >= MIN_LIST and n_large <= MAX_LIST_LARGE)
    return m


def cell_starts(m):
    """DevAccel::cs of the model's grid: per column and fine bin the first entry, once with the columns along x (a sphere in every
    column ix0..ix1 under the bin of its centre's z) and, behind all of those, once along z; each part ends with its total"""
    G, Gf = m["G"], m["G"] * FINE
    g = ~m["is_large"]
    cx, cz = np.zeros(G * Gf + 1, np.int64), np.zeros(G * Gf + 1, np.int64)
    for lo, hi, b, c in ((m["ix0"][g], m["ix1"][g], m["bz"][g], cx), (m["iz0"][g], m["iz1"][g], m["bx"][g], cz)):
        for a, e, k in zip(lo, hi, b):
            c[np.arange(a, e + 1) * Gf + k + 1] += 1
    cx, cz = np.cumsum(cx), np.cumsum(cz)
    return np.concatenate([cx, cx[-1] + cz]).astype(np.int32)


def info_of(m):
    """what World.list_accel_info() / Octree.accel_info() report for the model's grid"""
    on = m["enabled"]
    d = dict(grid_dim=m["G"] if on else 0, cell_size=float(F(m["h"])) if on else 0.0, grid_entries=m["grid_entries"] if on else 0,
             large_spheres=m["n_large"] if on else 0)
    if m["mode"] == "list":
        d["enabled"] = on
    return d


def variant_of(m):
    """the last template argument of the k_render a world's frames go through: 2 (dense walk), 4 (pooled walk), 5 (pooled walk, chains
    start alone), 1 (no grid)"""
    if not m["enabled"]:
        return 1
    return (5 if m["solo_chains"] else 4) if m["coop_groups"] >= 4 else 2


def kernel_name(m, mode=0):
    if not m["enabled"]:
        return "k_render<%s,%d,1>" % ("false" if m["mode"] == "list" else "true", mode)
    return "k_render<true,%d,%d>" % (mode, variant_of(m))


# ---------------------------------------------------------------------------------------------------- float32 neighbours
def step32(x, k):
    """x moved k float32 steps away from zero (k < 0: towards it)"""
    x = np.atleast_1d(np.asarray(x, F))
    mag = (np.abs(x).view(np.int32) + np.asarray(k, np.int32)).astype(np.int32)
    return np.copysign(mag.view(F), x)


def first_float(pred, lo, hi):
    """the smallest positive float32 in (lo, hi] at which the monotone predicate holds (pred(lo) false, pred(hi) true)"""
    a, b = int(F(lo).view(np.int32)), int(F(hi).view(np.int32))
    assert not pred(F(lo)) and pred(F(hi))
    while b - a > 1:
        mid = (a + b) // 2
        if pred(np.int32(mid).view(F)):
            b = mid
        else:
            a = mid
    return np.int32(b).view(F)


# ---------------------------------------------------------------------------------------------------- worlds
# (name, variant, modes, SPHERES_PER_LEAF of the tree)
WORLDS = [("rlim", None, ("list", "tree"), 30), ("centre_bound", None, ("list",), 30),
          ("counts", "h63", ("list",), 30), ("counts", "h64", ("list",), 30), ("counts", "l64", ("list",), 30), ("counts", "l65", ("list",), 30),
          ("counts", "t0", ("tree",), 30), ("counts", "t8", ("tree",), 30), ("counts", "t9", ("tree",), 30),
          ("clamps", "tiny", ("list", "tree"), 30), ("clamps", "huge", ("tree",), 30), ("clamps", "one", ("list", "tree"), 30),
          ("clamps", "none", ("tree",), 30),
          ("switches", "coop", ("tree",), 64), ("switches", "sparse", ("tree",), 64), ("switches", "dense", ("tree",), 64),
          ("switches", "solo", ("tree",), 64), ("switches", "nosolo", ("tree",), 64)]
CASES = [(n, v, mode, spl) for n, v, modes, spl in WORLDS for mode in modes]
SPL_OF = {(n, v): spl for n, v, _, spl in WORLDS}
GROUND = ((0.0, -1000.0, -1.0), 1000.0, LAMBERTIAN, (0.5, 0.5, 0.5), 0.0)
# lookfrom of the three cameras: the world's own (inside the near zone), one at distance 30 from (0,1,0) (every primary ray takes the
# scan, every secondary ray the walk), one at distance exactly 24 (256 + 64 + 256 = 576: the lens offsets fall to either side)
LOOKFROM = {"own": (13.0, 2.0, 3.0), "outside": (24.0, 1.0, 18.0), "edge": (16.0, 9.0, 16.0)}


def camera(which="own", nx=NX, ny=NY, vfov=35.0):
    return oracle_lib.make_camera(LOOKFROM[which], (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), vfov, float(F(nx) / F(ny)), 0.05, 10.0)


class _Slots:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.recs, self.probes = [GROUND], {}

    def add(self, centres, radii, probe=None):
        centres = np.asarray(centres, np.float64).reshape(-1, 3)
        radii = np.broadcast_to(np.asarray(radii, np.float64), (len(centres),))
        first = len(self.recs)
        for c, r in zip(centres, radii):
            kind = int(self.rng.choice([LAMBERTIAN, LAMBERTIAN, METAL, DIELECTRIC]))
            alb = tuple(float(v) for v in self.rng.uniform(0.05, 1.0, 3))
            param = float(self.rng.uniform(0, 1)) if kind == METAL else 1.5 if kind == DIELECTRIC else 0.0
            self.recs.append((tuple(float(v) for v in c), float(r), kind, alb, param))
        if probe:
            self.probes.setdefault(probe, []).extend(range(first, len(self.recs)))
        return np.arange(first, len(self.recs))

    def ghosts(self, k):
        self.recs += [mw.GHOST] * k

    def field(self, k, r=0.1, ext=10.0, air=0.3, probe=None):
        """k ordinary spheres: resting on the ground or in the air below y = 1.9, inside the root box"""
        c = np.empty((k, 3))
        c[:, 0], c[:, 2] = self.rng.uniform(-ext, ext, k), self.rng.uniform(-ext, ext, k)
        c[:, 1] = r
        up = self.rng.random(k) < air
        c[up, 1] = self.rng.uniform(r, 1.9 - r, int(up.sum()))
        return self.add(c, r, probe)

    def outside(self, k, r=0.1):
        """k spheres beyond the root box (buildOctree drops them), on all four sides"""
        far = self.rng.uniform(11.5, 14.0, k) * self.rng.choice([-1.0, 1.0], k)
        along = self.rng.uniform(-10.0, 10.0, k)
        swap = self.rng.random(k) < 0.5
        c = np.stack([np.where(swap, along, far), np.full(k, r), np.where(swap, far, along)], 1)
        return self.add(c, r)

    def done(self):
        sp = np.zeros(len(self.recs), sphere_dtype)
        for i, r in enumerate(self.recs):
            sp[i] = r
        return sp, {k: np.array(v, np.int64) for k, v in self.probes.items()}


def _rlim():
    """200 spheres of radius 0.1 (the median: h = 2 R'(0.1) ~ 0.235, Rlim = 1.5 h ~ 0.352); 40 probes whose float32 radii are the 20
    floats below and the 20 from the first radius on at which R' > Rlim (~0.345); spheres of radius 0.1 whose x lies two float steps
    below / at / above the values at which a column bound (ix0, ix1) or the fine bin of the centre steps to the next integer"""
    S = _Slots(101)
    S.field(200)
    px, pz = np.meshgrid(np.linspace(-8.4, 8.4, 8), np.linspace(-7.0, 7.0, 5))
    probes = S.add(np.stack([px.ravel(), np.full(40, 0.345), pz.ravel()], 1), 0.3451, "rlim")
    sp, _ = S.done()
    rlim = model(sp, "list")["Rlim"]
    edge = first_float(lambda r: float(inflated(np.float64(F(r) * F(r)))) > rlim, 0.2, 0.5)
    radii = step32(np.full(40, edge, F), np.arange(-20, 20))
    for i, r in zip(probes, radii):
        c, _, kind, alb, param = S.recs[i]
        S.recs[i] = ((c[0], float(r), c[2]), float(r), kind, alb, param)
    m = model(S.done()[0], "list")
    g0, h, rp = m["g0"], m["h"], float(inflated(np.float64(F(0.1) * F(0.1))))
    rules = {"ix0": lambda v, k: np.floor((np.float64(v) - rp - g0) / h - 1e-4) >= k, "ix1": lambda v, k: np.floor((np.float64(v) + rp - g0) / h + 1e-4) >= k,
             "bx": lambda v, k: np.floor((np.float64(v) - g0) / h * float(FINE)) >= k}
    row = 0
    for name, rule in rules.items():
        for col in (57, 70, 83):                                   # columns of the grid right of x = 0 (g0 ~ -12.2, h ~ 0.235)
            k = col * FINE if name == "bx" else col
            xb = first_float(lambda v: bool(rule(v, k)), 0.05, 10.9)
            xs = step32(np.full(4, xb, F), np.arange(-2, 2))
            S.add(np.stack([xs.astype(np.float64), np.full(4, 0.1), np.full(4, -9.0 + 2.0 * row)], 1), 0.1, "floor_" + name)
            row += 1
    return S.done()


def _centre_bound():
    """200 ordinary spheres in the middle (the median radius stays 0.1); three rings of spheres of radius 0.1 at y = 0.1, 1 and 6 whose
    distance dc from (0,1,0) is, per ring position, the last three floats of the varied coordinate with dc <= 17.5 and the first three
    with dc > 17.5; four centres at dc == 17.5 exactly; `inside` probes beyond the bound (see the module's docstring)"""
    S = _Slots(202)
    S.field(200)
    S.add([(17.5, 1.0, 0.0), (0.0, 1.0, -17.5), (10.5, 1.0, 14.0), (-14.0, 1.0, 10.5)], 0.1, "exact")
    dist = lambda c: float(np.sqrt(c[0] * c[0] + (c[1] - 1.0) * (c[1] - 1.0) + c[2] * c[2]))
    for ring, yy in enumerate((0.1, 1.0, 6.0)):
        rho = np.sqrt(CENTRE_BOUND ** 2 - (float(F(yy)) - 1.0) ** 2)
        for j in range(5):
            th = 0.3 + 0.41 * ring + j * 2.0 * np.pi / 5.0
            c = np.array([F(rho * np.cos(th)), F(yy), F(rho * np.sin(th))], np.float64)
            ax = 0 if abs(c[0]) >= abs(c[2]) else 2

            def beyond(v, c=c, ax=ax):
                q = c.copy()
                q[ax] = np.float64(v)
                return dist(q) > CENTRE_BOUND
            vb = first_float(beyond, 0.5 * abs(c[ax]), abs(c[ax]) + 1.0)
            for steps, probe in ((np.arange(-3, 0), "within"), (np.arange(0, 3), "beyond")):
                pts = np.tile(c, (3, 1))
                pts[:, ax] = np.copysign(step32(np.full(3, vb, F), steps).astype(np.float64), c[ax])
                S.add(pts, 0.1, probe)
    m = model(S.done()[0], "list")
    g0, h, G, rp = m["g0"], m["h"], m["G"], float(inflated(np.float64(F(0.1) * F(0.1))))
    # (-v, 1, 0): inside as long as -v - R' > g0 + h;  (0, 1, v): inside as long as v + R' < g0 + (G - 1) h
    for ax, fails in ((0, lambda v: not (-np.float64(v) - rp > g0 + h)), (2, lambda v: not (np.float64(v) + rp < g0 + (G - 1) * h))):
        vb = first_float(fails, 17.6, 25.0)
        for steps, probe in ((np.arange(-3, 0), "inside"), (np.arange(0, 3), "not_inside")):
            pts = np.zeros((3, 3))
            pts[:, 1] = 1.0
            pts[:, ax] = step32(np.full(3, vb, F), steps).astype(np.float64) * (-1.0 if ax == 0 else 1.0)
            S.add(pts, 0.1, probe)
    return S.done()


def _counts(variant):
    S = _Slots(303)
    if variant in ("h63", "h64"):
        # 70 slots: the ground, 64 spheres, five ghosts (h64); one more sphere is a ghost in h63
        S.field(69, ext=4.0)
        for slot in (7, 19, 33, 48, 60) + ((40,) if variant == "h63" else ()):
            S.recs[slot] = mw.GHOST
        return S.done()
    S.field(200)
    if variant in ("l64", "l65"):
        # 65 slots of radius 0.5 (R' > Rlim ~ 0.352), the last one a ghost in l64
        gx, gz = np.meshgrid(np.linspace(-9.0, 9.0, 13), np.linspace(-8.0, 8.0, 5))
        S.add(np.stack([gx.ravel(), np.full(65, 0.5), gz.ravel()], 1), 0.5, "large")
        k = 64 if variant == "l64" else 65
    else:
        # nine slots of radius 0.5 inside the root box, the last 9, 1 or 0 of them ghosts
        k = {"t0": 0, "t8": 8, "t9": 9}[variant]
        S.add(np.stack([np.linspace(-8.0, 8.0, 9), np.full(9, 0.5), np.linspace(-6.0, 6.0, 9)[::-1]], 1), 0.5, "large")
    big = S.probes["large"]
    for slot in big[k:]:
        S.recs[slot] = mw.GHOST
    S.probes["large"] = big[:k]
    return S.done()


def _clamps(variant):
    S = _Slots(404)
    if variant == "tiny":
        S.field(300, r=1e-3, ext=3.0, air=1.0)                  # (in the air: resting on the ground they vanish in its float noise)
    elif variant == "huge":
        k = 80
        c = np.stack([S.rng.uniform(-9.0, 9.0, k), S.rng.uniform(0.5, 1.5, k), S.rng.uniform(-9.0, 9.0, k)], 1)
        S.add(c, 2.0, "huge")
    elif variant == "one":
        S.add([(0.5, 0.1, 0.75)], 0.1, "one")
        S.outside(70)
    else:
        assert variant == "none", variant
        S.outside(71)
    return S.done()


@functools.lru_cache(None)
def _switch_counts():
    """in-tree counts at which the rules switch, from the model on the recipes' own spheres: (last sparse N of `4 N > 8 g^2` for equal
    radii 0.35, last solo N of `cells <= ncell` for equal radii 0.1)"""
    S = _Slots(505)
    S.field(100, r=0.35, ext=10.4)
    g = model(S.done()[0], "list")["g_rule"]
    last_sparse = int(2.0 * g * g)
    S = _Slots(606)
    S.field(4000, ext=10.4)
    sp = S.done()[0]
    m = model(sp, "list")
    assert not m["dense"] and m["n_large"] == 0
    per = ((m["ix1"] - m["ix0"] + 1) * (m["iz1"] - m["iz0"] + 1)).astype(np.float64)
    last_solo = int(np.flatnonzero(np.cumsum(per) <= SOLO_DENSITY * m["G"] * m["G"]).max()) + 1
    return last_sparse, last_solo


def _switches(variant):
    """Equal radii, so the cell size does not move with the count.
      coop / sparse / dense: radius 0.35 (h = 2 R': every sphere covers exactly 2 x 2 cells unless it sits on a column edge).  `coop` and
        `sparse` store the last count of the sparse rule, `dense` one sphere more (h shrinks to 0.7 of it).  In `coop` no sphere sits
        on an edge: cells == 8 ncell exactly, the last value of the pooled walk (variant 4); `sparse` and `dense` move sphere 1 onto a
        column edge of the sparse grid (three columns): cells = 8 ncell + 2 sends `sparse` to the dense walk (variant 2).
      solo / nosolo: radius 0.1, the last count with cells <= ncell (chains start alone, variant 5) and one sphere more (variant 4)."""
    last_sparse, last_solo = _switch_counts()
    if variant in ("coop", "sparse", "dense"):
        S = _Slots(505)
        S.field(last_sparse + 1, r=0.35, ext=10.4)
        sp, probes = S.done()
        if variant != "coop":
            m = model(sp[:-1], "list")
            assert not m["dense"]
            rp = float(inflated(np.float64(F(0.35) * F(0.35))))
            sp["center"][1, 0] = F(m["g0"] + rp + 25.0 * m["h"])
    else:
        assert variant in ("solo", "nosolo"), variant
        S = _Slots(606)
        S.field(last_solo + 1, ext=10.4)
        sp, probes = S.done()
    if variant in ("coop", "sparse", "solo"):                      # the pairs differ by their last sphere: a ghost here
        sp[-1] = mw.GHOST
    return sp, probes


@functools.lru_cache(None)
def _built(name, variant):
    if name == "rlim":
        sp, probes = _rlim()
    elif name == "centre_bound":
        sp, probes = _centre_bound()
    else:
        sp, probes = {"counts": _counts, "clamps": _clamps, "switches": _switches}[name](variant)
    sp.setflags(write=False)
    return sp, probes


def world(name, variant=None, nx=NX, ny=NY, cam="own"):
    """(spheres, the camera's 22 floats)"""
    return _built(name, variant)[0].copy(), camera(cam, nx, ny, 60.0 if name == "centre_bound" else 35.0)


def probes(name, variant=None):
    """the named groups of sphere indices a world places at its thresholds"""
    return _built(name, variant)[1]


def oracle(sp, cam, tree=False, spl=30, nx=NX, ny=NY):
    return mw.oracle(sp, cam, nx, ny, tree=tree, spl=spl)


def stored_by_oracle(sp, cam, spl):
    t = oracle(sp, cam, True, spl).octree()
    return stored_set(t["counts"], t["indices"])


# ---------------------------------------------------------------------------------------------------- rays
TWO40, TWOM40 = F(2.0 ** 40), F(2.0 ** -40)
TINY = F(2.0 ** -126)                 # the smallest normal float32: d.x and d.z of a walking ray are normal numbers


def fast_path(rays):
    """closest_tree's preconditions in numpy float32, in the kernel's operation order: the terms and their conjunction"""
    r = np.ascontiguousarray(rays, F).reshape(-1, 6)
    ox, oy, oz, dx, dy, dz = (r[:, k] for k in range(6))
    with np.errstate(all="ignore"):
        a = dx * dx + dy * dy + dz * dz
        zy = oy - F(1.0)
        q = ox * ox + zy * zy + oz * oz
        t = dict(a_lo=a >= TWOM40, a_hi=a <= TWO40, dx=np.abs(dx) >= TINY, dz=np.abs(dz) >= TINY, dy=np.abs(dy) >= TWOM40, zone=q <= F(ZONE * ZONE))
    t["fast"] = t["a_lo"] & t["a_hi"] & t["dx"] & t["dz"] & t["dy"] & t["zone"]
    t["a"], t["q"] = a, q
    return t


# kinds of a group's rays: 0 through the centre, 99 tangent, +-k (k = 1..8) at r (1 +- k 2^-20) from it, +-(100 + j) (j = 1..6) at
# sqrt(r^2 +- ZONE_BAND[j - 1] of the discriminant's error bound 16.1 u |o - c|^2) - where the float test of a sphere much smaller than that
# bound (`tiny`) changes its mind
ZONE_BAND = np.array([0.003, 0.01, 0.03, 0.1, 0.3, 0.6])             # fractions of the error bound of the kinds +-(101..106); K2 covers 2
ZONE_KINDS = np.array([0, 99] + [s * k for k in range(1, 9) for s in (1, -1)] + [s * (100 + j) for j in range(1, len(ZONE_BAND) + 1) for s in (1, -1)])
ZONE_GROUP = len(ZONE_KINDS)


def zone_rays_meta(sp, n, seed, prefer=None):
    """(rays, meta).  Groups of ZONE_GROUP rays share an origin on (or 1 to 4 float steps inside / outside) the sphere |o - (0,1,0)| = 24 and a
    target sphere on the far side of the field: one ray through its centre, one tangent, and twins passing the centre at
    r (1 + k 2^-20) and r (1 - k 2^-20), k = 1..8, and at the edge of the discriminant's error (ZONE_KINDS).  prefer: sphere indices that half of the groups take their target from.
    meta: group, kind (ZONE_KINDS) and target per ray."""
    rng = np.random.default_rng(seed)
    ng = max(1, n // ZONE_GROUP)
    ctr = np.array([0.0, 1.0, 0.0])
    o = rng.normal(size=(ng, 3))
    o[::8, 1] = -np.abs(o[::8, 1])                                  # (an origin below the ground sees nothing but the ground: one in eight)
    o[1::8, 1] *= 0.02                                              # all but level with the field
    up = np.arange(ng) % 8 > 1
    o[up, 1] = np.abs(o[up, 1])
    o = ctr + ZONE * o / np.linalg.norm(o, axis=1)[:, None]
    exact = np.array([(24, 1, 0), (-24, 1, 0), (0, 25, 0), (0, -23, 0), (0, 1, 24), (0, 1, -24)], np.float64)
    at = np.arange(0, ng, max(1, ng // 60))[:60]
    o[at] = exact[np.arange(at.size) % 6]
    o = o.astype(F)
    # 1 to 4 float steps outward (s > 0) or inward (s < 0) in every coordinate that is not (nearly) the centre's; s = 0: as it is
    s = rng.integers(-4, 5, ng)
    for ax in (0, 2):
        far = np.abs(o[:, ax]) > 1.0
        o[far, ax] = step32(o[far, ax], s[far])
    yy = o[:, 1]
    far = np.abs(yy - F(1.0)) > 1.0
    out = np.where((yy < 0) | (yy > 1), s, -s)
    o[far, 1] = step32(yy[far], out[far])
    o64 = o.astype(np.float64)
    # targets: hittable spheres of positive radius behind the centre as seen from the origin
    cand = np.flatnonzero((sp["material"] != MAT_NONE) & (sp["radius"] > 0) & np.isfinite(sp["radius"]))
    cand = cand[cand > 0]
    tgt = cand[rng.integers(0, cand.size, ng)]
    if prefer is not None and len(prefer):
        use = rng.random(ng) < 0.5
        tgt = np.where(use, np.asarray(prefer)[rng.integers(0, len(prefer), ng)], tgt)
    for _ in range(16):
        near = ((sp["center"][tgt].astype(np.float64) - ctr) * (o64 - ctr)).sum(axis=1) >= 0
        if not near.any():
            break
        tgt[near] = cand[rng.integers(0, cand.size, int(near.sum()))]
    c, r = sp["center"][tgt].astype(np.float64), sp["radius"][tgt].astype(np.float64)
    w = c - o64
    wl = np.linalg.norm(w, axis=1)
    e = np.cross(w, rng.normal(size=(ng, 3)))
    e /= np.linalg.norm(e, axis=1)[:, None]
    kinds = ZONE_KINDS
    kk = kinds[None, :]
    band = np.sqrt(np.maximum(r[:, None] ** 2 + np.sign(kk) * ZONE_BAND[np.clip(np.abs(kk) - 101, 0, len(ZONE_BAND) - 1)] * 16.1 * U * wl[:, None] ** 2, 0.0))
    off = np.where(kk == 0, 0.0, np.where(kk == 99, r[:, None], np.where(np.abs(kk) > 100, band, r[:, None] * (1.0 + kk * 2.0 ** -20))))
    # the line from o along w + e * shift passes the centre at distance `off`
    shift = off * wl[:, None] / np.sqrt(np.maximum(wl[:, None] ** 2 - off ** 2, 1e-300))
    d = w[:, None, :] + e[:, None, :] * shift[:, :, None]
    rays = np.concatenate([np.broadcast_to(o64[:, None, :], d.shape), d], 2).reshape(-1, 6)
    group, kind = np.repeat(np.arange(ng), ZONE_GROUP), np.tile(kinds, ng)
    pad = n - len(rays)
    if pad > 0:                                                     # fill up with centre rays
        extra = np.arange(pad) % ng * ZONE_GROUP
        rays, group, kind = np.concatenate([rays, rays[extra]]), np.concatenate([group, group[extra]]), np.concatenate([kind, kind[extra]])
    rays, group, kind = rays[:n], group[:n], kind[:n]
    return np.ascontiguousarray(rays, F), dict(group=group, kind=kind, target=tgt[group])


def zone_rays(sp, n, seed, prefer=None):
    return zone_rays_meta(sp, n, seed, prefer)[0]


def _scene_rays(rng, k, low=False):
    """k scene-like rays in float64: origins in the field (low: inside the layer of spheres that rest on the ground), unit directions
    towards points near the ground"""
    o = rng.uniform([-10.0, 0.02, -10.0], [10.0, 0.22 if low else 2.0, 10.0], (k, 3))
    t = rng.uniform([-10.0, 0.0, -10.0], [10.0, 0.3, 10.0], (k, 3))
    d = t - o
    return o, d / np.linalg.norm(d, axis=1)[:, None]


def _search_a(dxy, target, zsign):
    """per ray the float32 d.z >= 0 at which float32 (dx dx + dy dy) + dz dz first reaches `target` (vectorised bisection over the
    float32 bit patterns; the sum is monotone in dz)"""
    base = dxy[:, 0] * dxy[:, 0] + dxy[:, 1] * dxy[:, 1]
    lo = np.zeros(len(dxy), np.int64)
    hi = np.sqrt(target.astype(np.float64)).astype(F).view(np.int32).astype(np.int64) + 16
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        z = mid.astype(np.int32).view(F)
        ok = base + z * z >= target
        hi, lo = np.where(ok, mid, hi), np.where(ok, lo, mid)
    return hi.astype(np.int32).view(F) * zsign


PRECONDITION_FAMILIES = ("a_low", "a_high", "dy", "dx", "dz", "vertical", "plain")


def precondition_rays_meta(n, seed):
    """(rays, meta): scene-like rays at the walk's preconditions.  meta: family per ray (index into PRECONDITION_FAMILIES).
      a_low / a_high: directions scaled by 2^-20 / 2^20 whose float32 a = d.d is the float below 2^-40 (2^40), 2^-40 (2^40) itself, or the
                      float above - found by a search over d.z, which holds less than a quarter of a;
      dy:             all but horizontal rays through the layer of spheres, |d.y| the float below 2^-40, 2^-40, the float above;
      dx / dz:        that component the smallest normal float32, the largest or the smallest subnormal, +0 or -0, the other axis dominant;
      vertical:       d.y = +-1 with d.x and d.z the smallest normal float32, subnormal or (d.x) zero - the walk divides by the larger;
      plain:          the same kind of ray scaled by 2^-10 .. 2^10."""
    rng = np.random.default_rng(seed)
    fam = np.arange(n) % len(PRECONDITION_FAMILIES)
    rays = np.zeros((n, 6), F)
    tiny = np.array([2.0 ** -126, 2.0 ** -126 - 2.0 ** -149, 2.0 ** -149, 0.0, -0.0])
    for f, name in enumerate(PRECONDITION_FAMILIES):
        at = np.flatnonzero(fam == f)
        k = at.size
        if name in ("a_low", "a_high"):
            # directions whose z component holds 3 % to 22 % of the squared length
            o, d = _scene_rays(rng, 8 * k + 64)
            keep = np.flatnonzero((d[:, 2] ** 2 >= 0.03) & (d[:, 2] ** 2 <= 0.22))[:k]
            assert keep.size == k
            o, d = o[keep], d[keep]
            scale, centre = (2.0 ** -20, TWOM40) if name == "a_low" else (2.0 ** 20, TWO40)
            targets = np.array([np.nextafter(centre, F(0)), centre, np.nextafter(centre, F(np.inf))], F)[np.arange(k) % 3]
            dxy = (d[:, :2] * scale).astype(F)
            dz = _search_a(dxy, targets, np.sign(d[:, 2]).astype(F))
            rays[at] = np.concatenate([o.astype(F), dxy, dz[:, None]], 1)
        elif name == "dy":
            o, d = _scene_rays(rng, k, low=True)
            v = np.array([np.nextafter(TWOM40, F(0)), TWOM40, np.nextafter(TWOM40, F(1))], F)[np.arange(k) % 3]
            d[:, 1] = v.astype(np.float64) * rng.choice([-1.0, 1.0], k)
            rays[at] = np.concatenate([o, d], 1).astype(F)
        elif name in ("dx", "dz"):
            o, d = _scene_rays(rng, k)
            ax, other = (0, 2) if name == "dx" else (2, 0)
            d[:, other] = rng.choice([-1.0, 1.0], k)
            d[:, ax] = tiny[np.arange(k) % 5] * rng.choice([-1.0, 1.0], k)
            rays[at] = np.concatenate([o, d], 1).astype(F)
        elif name == "vertical":
            o = rng.uniform([-10.0, 0.3, -10.0], [10.0, 3.0, 10.0], (k, 3))
            d = np.zeros((k, 3))
            d[:, 1] = -1.0
            d[::7, 1] = 1.0
            d[:, 0] = tiny[rng.integers(0, 5, k)] * rng.choice([-1.0, 1.0], k)
            d[:, 2] = tiny[rng.integers(0, 4, k)] * rng.choice([-1.0, 1.0], k)
            rays[at] = np.concatenate([o, d], 1).astype(F)
        else:
            o, d = _scene_rays(rng, k)
            d *= 2.0 ** rng.integers(-10, 11, k)[:, None]
            rays[at] = np.concatenate([o, d], 1).astype(F)
    return np.ascontiguousarray(rays, F), dict(family=fam)


def precondition_rays(n, seed):
    return precondition_rays_meta(n, seed)[0]


def lattice_rays_for(m, sp, n, seed):
    """world_cases.lattice_rays on the model's grid: g0, G and h of the world's own grid - a list's grid reaches past the root box -
    (no grid: 64 columns over the root box)"""
    on = m["enabled"] and m["G"] > 0
    info = dict(grid_dim=m["G"], cell_size=m["h"]) if on else dict(grid_dim=64, cell_size=2.0 * ROOT_HALF / 64)
    return lattice_rays(info, sp["center"].astype(np.float64), sp["radius"].astype(np.float64), n, seed, g0=m["g0"] if on else -ROOT_HALF)


def preferred_targets(name, variant=None):
    """the spheres half of a world's zone_rays groups aim at: centre_bound's spheres at the centre bound, the one sphere `one` stores in
    its tree (the other 70 lie outside the root box: through the tree nothing else can be grazed); None elsewhere"""
    p = probes(name, variant)
    if name == "centre_bound":
        return np.concatenate([p["within"], p["beyond"], p["exact"]])
    if (name, variant) == ("clamps", "one"):
        return p["one"]
    return None


def ray_families(name, variant, sp, m, n):
    """the four ray sets of a world, by name"""
    from world_cases import random_rays
    return {"zone": zone_rays(sp, n, 7100, preferred_targets(name, variant)), "precondition": precondition_rays(n, 7200),
            "lattice": lattice_rays_for(m, sp, n, 7300), "random": random_rays(n, 7400)}


# ---------------------------------------------------------------------------------------------------- the record
def grazing_flips(sp, meta, ref, fast):
    """among the k / -k twins of zone_rays whose both rays take the fast path: the pairs in which exactly one ray hits the target"""
    kind, tgt = meta["kind"], meta["target"]
    plus = np.flatnonzero((kind >= 1) & (kind != 99))
    plus = plus[plus + 1 < len(kind)]
    plus = plus[kind[plus + 1] == -kind[plus]]
    both = fast[plus] & fast[plus + 1]
    on = ref["sphere"] == tgt
    return int((both & (on[plus] != on[plus + 1])).sum()), int(both.sum())


def band_hits(meta, ref):
    """per fraction f of ZONE_BAND: (rays that pass their target at sqrt(r^2 + f * 16.1 u |o - c|^2), those of them the float test lets hit it)"""
    out = []
    for j in range(1, len(ZONE_BAND) + 1):
        at = meta["kind"] == 100 + j
        out.append((int(at.sum()), int((ref["sphere"][at] == meta["target"][at]).sum())))
    return out


def report(n=24000):
    lines = ["world / mode: spheres, grid on, G, h, large / grid spheres, kernel; per ray family: rays, fast, slow, hits (zone: grazing flips among fast twins)"]
    bands = np.zeros((len(ZONE_BAND), 2), np.int64)
    for name, variant, mode, spl in CASES:
        sp, cam = world(name, variant)
        S = oracle(sp, cam, mode == "tree", spl)
        m = model(sp, mode, stored_by_oracle(sp, cam, spl) if mode == "tree" else None)
        label = "%s%s/%s" % (name, "_" + variant if variant else "", mode)
        lines.append("%-22s N %5d  on %d  G %3d  h %.6f  large %3d  grid %4d  entries %5d  cells/ncell %.3f  %s" % (
            label, len(sp), m["enabled"], m["G"], m["h"], m["n_large"], len(m.get("grid", [])), m["grid_entries"],
            m["cells"] / max(1, m["G"] ** 2), kernel_name(m)))
        for fam, rays in ray_families(name, variant, sp, m, n).items():
            ref = S.trace(rays, mode=2 if mode == "tree" else 1)
            fast = fast_path(rays)["fast"]
            extra = ""
            if fam == "zone":
                meta = zone_rays_meta(sp, n, 7100, preferred_targets(name, variant))[1]
                extra = "  flips %d of %d fast twins" % grazing_flips(sp, meta, ref, fast)
                bands += np.array(band_hits(meta, ref))
            lines.append("    %-12s rays %6d  fast %6d  slow %6d  hits %6d%s" % (fam, len(rays), fast.sum(), (~fast).sum(), ref["hit"].sum(), extra))
    lines.append("zone_rays of all cases, rays passing their target at sqrt(r^2 + f * 16.1 u |o - c|^2) and how many of them the oracle's float test lets hit it "
                 "(K2 covers f = 2; the rasterisation slack 0.002 alone covers f = 0.24 at r = 0.1):")
    for f, (rays, hits) in zip(ZONE_BAND, bands):
        lines.append("    f = %-5g rays %6d  hit their target %6d" % (f, rays, hits))
    return "\n".join(lines)


if __name__ == "__main__":
    print(report())
