"""The worlds and rays of tests/grid_threshold_worlds.py on the CPU (not gpu):
  * the builders are deterministic;
  * build_accel (the product's host build, through World.list_accel_info / Octree.accel_info / rt_render_kernel_name) files every world
    as the independent float64 model does: grid on or off, G, h as float32, entries, large spheres, kernel variant;
  * each world reaches the threshold it is named for (the margins are conditions: a recipe that misses one is retuned, never the margin);
  * on the oracle alone, the ray families hit, fall to both sides of every precondition of the walk, and graze, so the comparisons of
    tests/test_gpu_grid_thresholds.py cannot pass vacuously;
  * where oracle/_ref/ is present, the oracle's records on these worlds and rays are the reference build's, bit for bit.
Every figure is printed before it is asserted.

Two thresholds cannot be reached by any world, and what is asserted instead is (grid_threshold_worlds' docstring has the algebra):
  * `inside`: centre_bound's probes lie to either side of it, but all of them beyond the centre bound - no sphere is ever large because
    of `inside` alone (test_inside_never_decides shows it on every world of this module);
  * the 0.05 clamp of the cell size: `tiny` has the smallest h a world can have, 2 R'(r^2 -> 0) = 0.119 (0.083 under the dense rule)."""
import functools

import numpy as np
import pytest

import grid_threshold_worlds as gw
import ref_lib
import reference_cases as rc
from bitcmp import same_nan_as_ref

N_RAYS = 24000
IDS = ["%s%s-%s" % (n, "_" + v if v else "", mode) for n, v, mode, _ in gw.CASES]


@functools.lru_cache(None)
def case(name, variant, mode, spl):
    """(spheres, camera, model from the ORACLE's tree) of a case, built once"""
    sp, cam = gw.world(name, variant)
    m = gw.model(sp, mode, gw.stored_by_oracle(sp, cam, spl) if mode == "tree" else None)
    sp.setflags(write=False)
    return sp, cam, m


@functools.lru_cache(None)
def traced(name, variant, mode, spl):
    """{family: (rays, the oracle's records)}"""
    sp, cam, m = case(name, variant, mode, spl)
    S = gw.oracle(sp, cam, mode == "tree", spl)
    out = {}
    for fam, rays in gw.ray_families(name, variant, sp, m, N_RAYS).items():
        ref = rc.trace(S, rays, 2 if mode == "tree" else 1)
        rays.setflags(write=False)
        out[fam] = (rays, ref)
    return out


def test_the_builders_are_deterministic():
    first = {}
    for name, variant, _, _ in gw.WORLDS:
        sp, cam = gw.world(name, variant)
        first[name, variant] = (sp.tobytes(), cam.tobytes())
        hittable = int((sp["material"][1:] != gw.MAT_NONE).sum())
        assert sp["material"][0] != gw.MAT_NONE and sp["radius"][0] == 1000.0
        assert hittable >= 64 or (name, variant) == ("counts", "h63"), (name, variant, hittable)
    gw._built.cache_clear()
    gw._switch_counts.cache_clear()
    for name, variant, _, _ in gw.WORLDS:
        sp, cam = gw.world(name, variant)
        assert (sp.tobytes(), cam.tobytes()) == first[name, variant], (name, variant)
    sp = gw.world("rlim")[0]
    for build in (lambda: gw.zone_rays(sp, 5000, 3), lambda: gw.precondition_rays(5000, 3)):
        assert build().tobytes() == build().tobytes()


def test_lattice_rays_default_origin_is_unchanged():
    """the optional g0 of world_cases.lattice_rays: leaving it out, or passing the root-box formula, gives the same bytes"""
    from world_cases import lattice_rays
    sp = gw.world("rlim")[0]
    c, r = sp["center"].astype(np.float64), sp["radius"].astype(np.float64)
    info = dict(grid_dim=104, cell_size=0.2347186952829361)
    a = lattice_rays(info, c, r, 4000, 9)
    assert a.tobytes() == lattice_rays(info, c, r, 4000, 9, g0=-(11.0 + 5.0 * info["cell_size"])).tobytes()
    assert a.tobytes() != lattice_rays(info, c, r, 4000, 9, g0=-18.0).tobytes()


# ---------------------------------------------------------------------------------------------------- the host build against the model
@pytest.mark.parametrize("name,variant,mode,spl", gw.CASES, ids=IDS)
def test_host_build_files_the_world_as_the_model_does(rt, name, variant, mode, spl):
    sp, cam, m = case(name, variant, mode, spl)
    W = rt.World(len(sp), gw.NX, gw.NY, spheres=sp, camera=cam.view(rt.camera_dtype))
    if mode == "tree":
        O = rt.Octree(W, spl)
        assert np.array_equal(gw.stored_set(*O.leaves()), gw.stored_by_oracle(sp, cam, spl))     # the model's input, from either build
        assert O.info()["dropped_full"] == 0
        info = O.accel_info()
    else:
        O = None
        info = W.list_accel_info()
    print(name, variant, mode, info, rt.render_kernel_name(W, O, 0), "cells / ncell %.6f" % (m["cells"] / max(1, m["G"] ** 2)))
    assert info == gw.info_of(m)
    assert np.float32(info["cell_size"]) == (np.float32(m["h"]) if m["enabled"] else 0.0)
    for k in (0, 1):
        assert rt.render_kernel_name(W, O, k) == gw.kernel_name(m, k)
    if m["enabled"]:
        # the model is consistent in itself: columns in range, every member filed exactly once
        assert m["n_large"] + len(m["grid"]) == len(m["members"])
        g = ~m["is_large"]
        assert (m["ix0"][g] <= m["ix1"][g]).all() and (m["iz0"][g] <= m["iz1"][g]).all()
        assert ((m["bx"] >= 0) & (m["bx"] < m["G"] * gw.FINE)).all()


# ---------------------------------------------------------------------------------------------------- each world reaches its threshold
def by_index(m, key, idx):
    pos = np.searchsorted(m["members"], idx)
    assert np.array_equal(m["members"][pos], idx)
    return m[key][pos]


@pytest.mark.parametrize("mode", ["list", "tree"])
def test_rlim_probes_straddle_the_large_radius(mode):
    sp, cam, m = case("rlim", None, mode, 30)
    p = gw.probes("rlim")
    large = by_index(m, "is_large", p["rlim"])
    r = sp["radius"][p["rlim"]]
    print("rlim/%s: h %.6f Rlim %.6f, probe radii %.9g .. %.9g, %d of %d large" % (mode, m["h"], m["Rlim"], r.min(), r.max(), large.sum(), large.size))
    assert large.size == 40 and large.sum() == 20
    assert np.array_equal(np.diff(r.view(np.int32)), np.ones(39, np.int32))            # 40 consecutive floats
    assert not large[:20].any() and large[20:].all()
    assert abs(m["h"] - 0.235) < 0.001 and abs(float(r[20]) - 0.345) < 0.001
    assert np.sort(sp["radius"][m["members"]])[len(m["members"]) // 2] == np.float32(0.1)                   # the median radius
    # the floor probes: two spheres to either side of each step of a column bound / of the centre's fine bin
    for key in ("ix0", "ix1", "bx"):
        v = by_index(m, key, p["floor_" + key]).reshape(3, 4)
        print("rlim/%s: floor probes of %s" % (mode, key), v.tolist())
        assert (v[:, 0] == v[:, 1]).all() and (v[:, 2] == v[:, 3]).all() and (v[:, 2] == v[:, 1] + 1).all()


def test_centre_bound_probes_straddle_17_5_and_the_grid_follows_them():
    sp, cam, m = case("centre_bound", None, "list", 30)
    p = gw.probes("centre_bound")
    within, beyond, exact = (by_index(m, "dc", p[k]) for k in ("within", "beyond", "exact"))
    print("centre_bound: reach %.6f, G %d; dc of the probes within %.9f .. %.9f, beyond %.9f .. %.9f; %d / %d probes; large %d" % (
        m["reach"], m["G"], within.min(), within.max(), beyond.min(), beyond.max(), within.size, beyond.size, m["n_large"]))
    assert within.size >= 10 and beyond.size >= 10
    assert (within <= 17.5).all() and (within > 17.5 - 1e-5).all() and (beyond > 17.5).all() and (beyond < 17.5 + 1e-5).all()
    assert (exact == 17.5).all() and exact.size == 4
    assert not by_index(m, "is_large", p["within"]).any() and not by_index(m, "is_large", p["exact"]).any()
    assert by_index(m, "is_large", p["beyond"]).all()
    assert m["reach"] > 11 and m["reach"] == 17.5
    assert {0.1, 1.0, 6.0} == set(np.round(sp["center"][p["within"], 1].astype(np.float64), 6).tolist())
    ins, out = by_index(m, "inside", p["inside"]), by_index(m, "inside", p["not_inside"])
    print("centre_bound: %d probes inside, %d not inside the stretched grid" % (ins.sum(), (~out).sum()))
    assert ins.size >= 3 and ins.all() and out.size >= 3 and not out.any()
    assert np.sort(sp["radius"][m["members"]])[len(m["members"]) // 2] == np.float32(0.1)                   # the median radius
    assert m["n_large"] <= gw.MAX_LIST_LARGE and m["enabled"]


def test_inside_never_decides():
    """no member of any world is large because of `inside` alone (the module docstring of grid_threshold_worlds has the reason)"""
    for c in gw.CASES:
        m = case(*c)[2]
        if len(m["members"]) == 0:
            continue
        alone = ~m["inside"] & ~(m["Rp"] > m["Rlim"]) & ~(m["dc"] > gw.CENTRE_BOUND)
        assert not alone.any(), c


def test_counts_sit_on_either_side_of_their_switches():
    m63, m64 = case("counts", "h63", "list", 30)[2], case("counts", "h64", "list", 30)[2]
    a, b = gw.world("counts", "h63")[0], gw.world("counts", "h64")[0]
    print("counts: hittable %d / %d, enabled %d / %d" % (len(m63["members"]), len(m64["members"]), m63["enabled"], m64["enabled"]))
    assert len(m63["members"]) == 63 and len(m64["members"]) == 64 and not m63["enabled"] and m64["enabled"]
    diff = np.flatnonzero([x.tobytes() != y.tobytes() for x, y in zip(a, b)])
    assert diff.size == 1 and a["material"][diff[0]] == gw.MAT_NONE and (a["material"] == gw.MAT_NONE).sum() == 6
    l64, l65 = case("counts", "l64", "list", 30)[2], case("counts", "l65", "list", 30)[2]
    print("counts: large %d / %d, enabled %d / %d" % (l64["n_large"], l65["n_large"], l64["enabled"], l65["enabled"]))
    assert l64["n_large"] == 64 and l65["n_large"] == 65 and l64["enabled"] and not l65["enabled"]
    for v, k in (("t0", 0), ("t8", 8), ("t9", 9)):
        m = case("counts", v, "tree", 30)[2]
        print("counts %s: %d large spheres in the tree's grid (LDS slots: %d)" % (v, m["n_large"], gw.HOT_LARGE))
        assert m["n_large"] == k and m["enabled"] and np.array_equal(m["large"], gw.probes("counts", v).get("large", np.zeros(0, np.int64)))


def test_clamps():
    floor = 2.0 * float(gw.inflated(np.float64(np.float32(1e-3) * np.float32(1e-3))))
    for mode in ("list", "tree"):
        m = case("clamps", "tiny", mode, 30)[2]
        print("clamps tiny/%s: h %.6f (2 R' of radius 1e-3: %.6f; of radius 0: %.6f; the clamp: 0.05)" % (mode, m["h"], floor, 2.0 * float(gw.inflated(0.0))))
        assert m["h"] == floor and not m["dense"] and m["n_large"] == 0
    # (the clamp itself is out of reach: the smallest h of any world, dense rule included, stays above it)
    assert gw.DENSE_CELL * 2.0 * float(gw.inflated(0.0)) > 0.05
    m = case("clamps", "huge", "tree", 30)[2]
    print("clamps huge: h %.6f (2 R' = %.4f), %d members, %d large, %d entries, enabled %d" % (m["h"], 2.0 * m["Rp"].max(), len(m["members"]), m["n_large"], m["grid_entries"], m["enabled"]))
    assert m["h"] == 1.0 and 2.0 * m["Rp"].min() > 1.0 and m["enabled"] and m["grid_entries"] == 0 and m["n_large"] == len(m["members"]) >= 64
    assert m["ylo"] == np.float32(-1e-4) and m["yhi"] == np.float32(1e-4) and m["rmax"] == np.float32(1e-4)
    m = case("clamps", "one", "tree", 30)[2]
    assert len(m["members"]) == 1 and m["enabled"] and m["members"][0] == gw.probes("clamps", "one")["one"][0]
    m = case("clamps", "none", "tree", 30)[2]
    assert len(m["members"]) == 0 and not m["enabled"]


def test_switch_pairs_straddle_their_rules_and_reach_every_variant():
    coop, sparse, dense, solo, nosolo = (case("switches", v, "tree", 64)[2] for v in ("coop", "sparse", "dense", "solo", "nosolo"))
    for v, m in zip(("coop", "sparse", "dense", "solo", "nosolo"), (coop, sparse, dense, solo, nosolo)):
        print("switches %s: in tree %d, 8 g^2 / 4 = %.1f, dense %d, cells %.0f, ncell %d, variant %d" % (
            v, len(m["members"]), 2.0 * m["g_rule"] ** 2, m["dense"], m["cells"], m["G"] ** 2, gw.variant_of(m)))
    n = len(sparse["members"])
    assert len(dense["members"]) == n + 1 and len(coop["members"]) == n and 3300 <= n <= 3500
    assert 4.0 * n <= 8.0 * sparse["g_rule"] ** 2 < 4.0 * (n + 1) and not sparse["dense"] and not coop["dense"] and dense["dense"]
    assert dense["h"] == max(0.05, gw.DENSE_CELL * sparse["h"])
    assert coop["cells"] == 8.0 * coop["G"] ** 2 and sparse["cells"] == coop["cells"] + 2                 # the last value of the pooled walk, and past it
    assert (gw.variant_of(coop), gw.variant_of(sparse), gw.variant_of(dense)) == (4, 2, 4)
    n = len(solo["members"])
    assert len(nosolo["members"]) == n + 1 and solo["cells"] <= solo["G"] ** 2 < nosolo["cells"] and nosolo["cells"] - solo["cells"] <= 9
    assert (gw.variant_of(solo), gw.variant_of(nosolo)) == (5, 4)
    reached = {gw.variant_of(case(*c)[2]) for c in gw.CASES}
    assert {2, 4, 5} <= reached and 1 in reached


# ---------------------------------------------------------------------------------------------------- the rays, on the oracle alone
def test_zone_origins_fall_to_both_sides_of_the_near_zone():
    sp = gw.world("centre_bound")[0]
    p = gw.probes("centre_bound")
    rays, meta = gw.zone_rays_meta(sp, N_RAYS, 7100, gw.preferred_targets("centre_bound"))
    t = gw.fast_path(rays)
    o = rays[:, :3].astype(np.float64)
    dist = np.linalg.norm(o - [0.0, 1.0, 0.0], axis=1)
    reach = np.linalg.norm(o - sp["center"][meta["target"]], axis=1)
    exact = (t["q"] == np.float32(576.0))
    print("zone_rays: |o - (0,1,0)| in [%.7f, %.7f]; %d rays in the zone, %d outside, %d with the float32 sum exactly 576; |o - c| up to %.3f, %d above 41" % (
        dist.min(), dist.max(), t["zone"].sum(), (~t["zone"]).sum(), exact.sum(), reach.max(), (reach > 41.0).sum()))
    assert np.abs(dist - 24.0).max() < 3e-5
    assert t["zone"].sum() >= 100 and (~t["zone"]).sum() >= 100 and exact.sum() >= 100
    grid = np.isin(meta["target"], np.concatenate([p["within"], p["exact"]]))               # targets the grid files: |o - c| <= 24 + 17.5
    walk = grid & t["fast"]                                                                   # ... and the ray takes the walk
    print("zone_rays: %d rays at grid spheres of the centre bound, %d of them on the fast path: |o - c| up to %.4f, %d above 41" % (
        grid.sum(), walk.sum(), reach[walk].max(), (reach[walk] > 41.0).sum()))
    assert (reach[walk] > 41.0).sum() >= 100 and 41.4 < reach[walk].max() <= 41.5 + 1e-4
    kinds = set(meta["kind"].tolist())
    assert kinds == set(gw.ZONE_KINDS.tolist()) and {0, 99, 1, -1, 8, -8} <= kinds


def test_precondition_rays_fall_to_both_sides_of_every_precondition():
    rays, meta = gw.precondition_rays_meta(N_RAYS, 7200)
    t = gw.fast_path(rays)
    fam = {name: meta["family"] == k for k, name in enumerate(gw.PRECONDITION_FAMILIES)}
    lo, hi = gw.TWOM40, gw.TWO40
    nb = lambda v: (np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(np.inf)))
    for name, term, values, of in (("a_low", "a_lo", nb(lo), t["a"]), ("a_high", "a_hi", nb(hi), t["a"]), ("dy", "dy", nb(lo), np.abs(rays[:, 4]))):
        got = of[fam[name]]
        counts = [int((got == v).sum()) for v in values]
        print("precondition_rays %s: %d rays, at the float below / at / above the bound: %s; pass %d, fail %d" % (
            name, fam[name].sum(), counts, t[term][fam[name]].sum(), (~t[term][fam[name]]).sum()))
        assert sum(counts) == fam[name].sum() and min(counts) >= 100
        assert t[term][fam[name]].sum() >= 100 and (~t[term][fam[name]]).sum() >= 100
    for name, col in (("dx", 3), ("dz", 5)):
        v = np.abs(rays[fam[name], col])
        counts = [int((v == np.float32(2.0 ** -126)).sum()), int(((v > 0) & (v < np.float32(2.0 ** -126))).sum()), int((v == 0).sum())]
        print("precondition_rays %s: smallest normal %d, subnormal %d, zero %d" % (name, *counts))
        assert min(counts) >= 100 and sum(counts) == fam[name].sum()
    v = fam["vertical"]
    both_sub = (np.abs(rays[v, 3]) < np.float32(2.0 ** -126)) & (np.abs(rays[v, 5]) < np.float32(2.0 ** -126)) & (rays[v, 3] != 0) & (rays[v, 5] != 0)
    print("precondition_rays vertical: %d rays, %d with d.x and d.z both subnormal, fast %d, slow %d" % (v.sum(), both_sub.sum(), t["fast"][v].sum(), (~t["fast"][v]).sum()))
    assert both_sub.sum() >= 100 and t["fast"][v].sum() >= 100 and (~t["fast"][v]).sum() >= 100
    assert t["fast"][fam["plain"]].all()


@pytest.mark.parametrize("name,variant,mode,spl", gw.CASES, ids=IDS)
def test_the_ray_families_hit_and_graze(name, variant, mode, spl):
    sp, cam, m = case(name, variant, mode, spl)
    for fam, (rays, ref) in traced(name, variant, mode, spl).items():
        fast = gw.fast_path(rays)["fast"]
        print("%s %s %s %-12s: %d rays, %d fast, %d slow, %d hits" % (name, variant, mode, fam, len(rays), fast.sum(), (~fast).sum(), ref["hit"].sum()))
        assert len(rays) == N_RAYS and ref["hit"].mean() >= 0.05
        assert fast.sum() >= 100 and (~fast).sum() >= 100
    rays, ref = traced(name, variant, mode, spl)["zone"]
    again, meta = gw.zone_rays_meta(sp, N_RAYS, 7100, gw.preferred_targets(name, variant))
    assert again.tobytes() == rays.tobytes()
    flips, twins = gw.grazing_flips(sp, meta, ref, gw.fast_path(rays)["fast"])
    on_target = int((ref["sphere"] == meta["target"]).sum())
    print("%s %s %s zone: %d records on the ray's own target, %d grazing flips among %d fast twins" % (name, variant, mode, on_target, flips, twins))
    if mode == "tree" and len(m["members"]) == 0:
        assert flips == 0 and on_target == 0                     # a tree that stores no sphere: there is nothing to graze
    else:
        assert flips >= 50


# ---------------------------------------------------------------------------------------------------- the oracle against the reference build
@pytest.mark.parametrize("name,variant,mode,spl", gw.CASES, ids=IDS)
def test_oracle_records_are_the_reference_builds(name, variant, mode, spl):
    s = ref_lib.status()
    if s == "absent":
        pytest.skip("neither oracle/_ref/ nor the reference's sources are here")
    assert s == "ok", "the reference's sources are here but oracle/_ref/ is incomplete: run `make -C oracle ref`"
    sp, cam, m = case(name, variant, mode, spl)
    geom = np.concatenate([sp["center"], sp["radius"][:, None]], 1).astype(np.float32)
    mat = np.concatenate([sp["albedo"], sp["param"][:, None]], 1).astype(np.float32)
    R = rc.reference_side((geom, mat, sp["material"].astype(np.int32), cam, spl))
    if mode == "tree":
        tree, _ = R.build_octree()
        assert np.array_equal(gw.stored_set(tree["counts"], tree["indices"]), gw.stored_by_oracle(sp, cam, spl))
    for fam, (rays, ref) in traced(name, variant, mode, spl).items():
        got = rc.trace(R, rays, 2 if mode == "tree" else 1)
        assert (got["sphere"] != -2).all(), fam                   # no ghost slot's record in binary32
        assert np.array_equal(got["hit"], ref["hit"]) and np.array_equal(got["sphere"], ref["sphere"]), fam
        for f in ("t", "p", "normal"):
            assert same_nan_as_ref(got[f], ref[f]), (fam, f)
