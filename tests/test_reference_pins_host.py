"""The CPU oracle (oracle/rt_oracle.hpp) against a CPU build of the REFERENCE's own headers (`make -C oracle ref`: oracle/ref_capi.cpp
over the nine unmodified headers, in fp32 and in USE_FP16, one library per SPHERES_PER_LEAF).  Not marked gpu.

Every comparison is bit equality; a NaN compares as "NaN where the reference has NaN" (bitcmp.same_nan_as_ref).  No tolerance
appears anywhere.  Worlds: create_world at N = 22, 500 and 10000, three random_world worlds, the nine of material_edge_worlds.WORLDS
(tests/reference_cases.py), each in both precisions.  Compared: buildOctree (every node, leaf, count and drop counter), hit records
through hitable_list::hit and hitTree, one-bounce material::scatter along lockstep paths (hit record, return value, attenuation,
scattered ray, all 12 words of the RNG state), camera::camera in fp32 and camera::get_ray in both.

Left out, with reasons:
  * camera::camera in USE_FP16.  camera.h:27-35 branches on __CUDA_ARCH__: the device takes hsin / hcos, the host tan.  The oracle
    follows the DEVICE branch (rt_oracle.hpp TanHalf<h16>), the host build can only take the other.  get_ray has no such branch and is
    compared in both precisions, from the same 22 floats.
  * a dielectric bounce whose draw is exactly 1.0: when refract() failed, dielectric::scatter (material.h:104-111) then returns an
    uninitialised `refracted`.  Such a bounce is recognised from the draw alone (the reference's own RNG word), its direction is not
    compared, and it is counted: the count is asserted to be 0 on every world of this file (about 2^-25 per draw).
  * a record of a GHOST slot.  create_world leaves slots of the list unwritten; as zeroed memory they are spheres of
    radius 0 at the origin with no material.  In binary32 nothing hits them.  In binary16 the rounding of b*b - a*c lets a ray that
    passes the origin within a few percent of its distance "hit" one, and color() (main.cu:59) would call through the null mat_ptr.
    This project defines ghost slots as unhittable (oracle, host code and kernels skip them).  The reference's
    ghost records are therefore reported by the driver (sphere -2), left out of the comparison of that ray and path, and counted:
    0 in binary32 on every world, and in binary16 under 1 % of the records (a radius-0 sphere catches directions within about
    2^-5 of its own, 2.4e-4 of the sphere of directions, and no world has more than a dozen ghosts in view).
  * the loops of main.cu (color, render, create_world): tests/test_reference_main_host.py, over a build of main.cu's own text.

The live tests skip only where neither oracle/_ref/ nor the reference's sources exist (a clean checkout elsewhere: the fixtures of
tests/test_reference_fixtures_host.py stand in); sources without libraries are a failure."""
import numpy as np
import pytest

import material_edge_worlds as mw
import oracle_lib
import ref_lib
import reference_cases as rc
from bitcmp import f32_bits, same_nan_as_ref

F = np.float32


@pytest.fixture(scope="module", autouse=True)
def built():
    s = ref_lib.status()
    if s == "absent":
        pytest.skip("neither oracle/_ref/ nor the reference's sources are here")
    assert s == "ok", "the reference's sources are here but oracle/_ref/ is incomplete: run `make -C oracle ref` (__graft_entry__.build() does)"


_worlds = {}


def sides(name, fp16, spl=None):
    """(world arrays, reference side, oracle side), built once per module"""
    k = (name, fp16, spl)
    if k not in _worlds:
        w = rc.world(name, fp16)
        _worlds[k] = (w, rc.reference_side(w, fp16, spl), rc.oracle_side(w, fp16, spl))
    return _worlds[k]


CASES = [(n, f) for n in rc.NAMES for f in (False, True)]


# ---------------------------------------------------------------------------------------------------- the stand-in headers
def test_the_stand_in_rng_gives_the_recorded_known_answers():
    """SURVEY App. A.1 (taken at survey time from the same definitions): seed 1984 state words and first uniforms, seed 1985 uniforms"""
    st = ref_lib.curand_init([1984, 1985])
    assert [int(x) for x in st[0, :6]] == [0x0e2ad815, 0x3b8fc912, 0x21a9ae18, 0xf8a42704, 0xdcd8f87c, 0x348c3b16]
    assert not st[:, 6:].any()
    u = []
    for _ in range(4):
        d, st = ref_lib.curand_uniform(st)
        u.append(d)
    u = f32_bits(np.array(u))
    assert u[:, 0].tolist() == [0x3e48b09e, 0x3ee873b3, 0x3eb7ce17, 0x3f39620a]
    assert u[:, 1].tolist() == [0x3eb57405, 0x3f5a9bd8, 0x3ecb5bc7, 0x3f78538f]


# ---------------------------------------------------------------------------------------------------- octree
def compare_trees(name, fp16, spl):
    w, ref, orc = sides(name, fp16, spl)
    t, info = ref.build_octree()
    o, oinfo = orc.octree(), orc.info()
    for k in ("node_count", "leaf_count", "dropped_full", "dropped_outside"):
        assert info[k] == oinfo[k], (k, info, oinfo)
    words = 0
    for k in ("level", "box", "children", "counts", "indices"):
        assert t[k].shape == o[k].shape and t[k].dtype == o[k].dtype, k
        assert same_nan_as_ref(t[k], o[k]) if k == "box" else np.array_equal(t[k], o[k]), k
        words += t[k].size
    print("%s %s spl %d: %d octree words, %d nodes, %d leaves, dropped %d full / %d outside" % (
        name, "fp16" if fp16 else "fp32", ref.spl, words, info["node_count"], info["leaf_count"], info["dropped_full"], info["dropped_outside"]))
    return info


@pytest.mark.parametrize("name,fp16", CASES)
def test_build_octree(name, fp16):
    info = compare_trees(name, fp16, None)
    if name.startswith("random"):
        assert info["dropped_outside"] > 0


@pytest.mark.parametrize("name,spl", rc.SMALL_BUCKETS)
@pytest.mark.parametrize("fp16", [False, True])
def test_build_octree_with_overflowing_buckets(name, spl, fp16):
    assert compare_trees(name, fp16, spl)["dropped_full"] > 0


def test_every_bucket_size_is_used():
    used = {rc.world(n)[4] for n in rc.NAMES} | {s for _, s in rc.SMALL_BUCKETS}
    assert used == set(ref_lib.SPLS)


# ---------------------------------------------------------------------------------------------------- hit records
@pytest.mark.parametrize("name,fp16", CASES)
def test_hit_records(name, fp16):
    """pixel-centre rays, then the lattice rays of test_gpu_strips (created worlds), random_rays or edge_rays: list and tree"""
    w, ref, orc = sides(name, fp16)
    big = w[2].size >= 3000
    rays = rc.ray_set(name, w, (2000 if big else 20000) // (10 if fp16 else 1))
    if fp16:
        rays = rc.half(rays)
    for mode in (1, 2):
        a, b = rc.trace(ref, rays, mode), rc.trace(orc, rays, mode)
        assert (a["sphere"] != -2).all(), "the reference hit a ghost slot"
        assert np.array_equal(a["hit"], b["hit"]) and np.array_equal(a["sphere"], b["sphere"]), mode
        for k in ("t", "p", "normal"):
            assert same_nan_as_ref(b[k], a[k]), (mode, k)
        print("%s %s %s: %d hit records compared, %d hits" % (name, "fp16" if fp16 else "fp32", ("", "list", "tree")[mode], len(rays), a["hit"].sum()))
        assert a["hit"].sum() > len(rays) // 50


# ---------------------------------------------------------------------------------------------------- lockstep paths
def witnesses(name, W):
    """what the reference's own walk must have reached in the world of that name (W: the counts gathered from its side)"""
    need = []
    if name.startswith(("created", "random", "glass_indices", "shells")):
        need += ["refracted", "reflected_by_draw"]
    if name.startswith("glass_indices") or name == "tir_room":
        need += ["total_internal_reflection"]
    if name.startswith("shells"):
        need += ["shell_entered", "shell_left"]
    if name in ("white_room", "mirror_room", "tir_room"):
        need += ["depth_limit"]
    if name.startswith(("created_500", "created_10000", "random", "extremes", "tir_room")):      # (created_22 has no fuzzy metal in view)
        need += ["metal_absorbed"]
    if name.startswith("extremes"):
        need += ["nan_direction", "odd_index_hit", "huge_albedo"]
    if name == "extremes_ghost0":
        need += ["miss_downwards"]
    if name in ("shells_solid", "shells_hollow"):
        need += ["starts_inside_glass"]
    return [k for k in need if not W.get(k)]


@pytest.mark.parametrize("name,fp16", CASES)
def test_lockstep_paths(name, fp16):
    w, ref, orc = sides(name, fp16)
    geom, mat, kind, cam, _ = w
    npaths = (2048 if name.startswith("extremes") else 512) if fp16 else 4096      # (extremes: its four odd indices are seldom hit)
    s, t, rays, st = rc.camera_samples(cam, npaths, fp16, lambda x: ref_lib.curand_uniform(x, fp16), lambda x: ref_lib.curand_init(x, fp16),
                                       lambda *a: ref_lib.get_ray(*a, fp16=fp16))
    # the oracle's camera rays from the same (s, t) and the same states
    st0 = ref_lib.curand_init(1984 + np.arange(npaths, dtype=np.uint64), fp16)
    for _ in range(2):
        st0 = ref_lib.curand_uniform(st0, fp16)[1]
    orays, ost = oracle_lib.get_ray(cam, s, t, st0, fp16=fp16)
    assert same_nan_as_ref(orays, rays) and np.array_equal(ost, st)
    if fp16 and name not in rc.EDGE and name != "random_3":      # (random_3's camera happens to stand close: its camera paths do bounce)
        # binary16 from create_world's and random_world's far cameras: b * b overflows and nearly every camera ray misses everything
        # (SURVEY fact 8).  So that scatter is compared there too, as many paths again start on the world's ray set, inside the field
        more = rc.half(rc.ray_set(name, w, npaths))[rc.GX * rc.GY:]
        rays = np.concatenate([rays, more])
        st = np.concatenate([st, ref_lib.curand_init(5000 + np.arange(npaths, dtype=np.uint64), fp16)])
    W = {}
    inside = (kind == mw.DIELECTRIC) & (np.linalg.norm(geom[:, :3].astype(np.float64) - cam[:3], axis=1) < np.abs(geom[:, 3]))

    def count(k, n):
        W[k] = W.get(k, 0) + int(n)

    def on_bounce(depth, live, x, out, oout):
        for mode, a, b in (("list", x["list"], x["olist"]), ("tree", x["tree"], x["otree"])):
            real = a["sphere"] != -2
            count("ghost_records_" + mode, (~real).sum())
            assert np.array_equal(a["hit"][real], b["hit"][real]) and np.array_equal(a["sphere"][real], b["sphere"][real]), (depth, mode)
            for k in ("t", "p", "normal"):
                assert same_nan_as_ref(b[k][real], a[k][real]), (depth, mode, k)
        ret, att, sc, sta = out
        oret, oatt, osc, osta = oout
        ok = ~x["excluded"]
        assert np.array_equal(ret, oret), depth
        assert same_nan_as_ref(oatt, att) and same_nan_as_ref(osc[:, :3], sc[:, :3]) and same_nan_as_ref(osc[ok, 3:], sc[ok, 3:]), depth
        assert np.array_equal(osta, sta), depth
        # witnesses, from the reference's side
        sph, kd = x["sphere"], kind[x["sphere"]]
        d = np.flatnonzero(kd == mw.DIELECTRIC)
        if d.size:
            br = ref.dielectric_branch(sph[d], x["rin"][d], x["rec"][d], sc[d])
            leaves, refr_ok, took_reflected = (br & 1) != 0, (br & 2) != 0, (br & 4) != 0
            count("refracted", (refr_ok & ~took_reflected).sum())
            count("reflected_by_draw", (refr_ok & took_reflected).sum())
            count("total_internal_reflection", (~refr_ok).sum())
            shell = geom[sph[d], 3] < 0
            # a negative radius turns the normal inward: "leaves" (dot > 0) is there a ray that ENTERS the cavity
            count("shell_entered", (shell & refr_ok & ~took_reflected & leaves).sum())
            count("shell_left", (shell & refr_ok & ~took_reflected & ~leaves).sum())
            if depth == 0:
                count("starts_inside_glass", inside[sph[d]].sum())
        count("metal_absorbed", ((kd == mw.METAL) & (ret == 0)).sum())
        count("nan_direction", np.isnan(sc[:, 3:]).any(axis=1).sum())
        count("odd_index_hit", np.isin(sph, (1, 2, 3, 4)).sum())
        count("huge_albedo", (att > 1e29).any(axis=1).sum())
        if depth == 0:
            miss = x["list"]["hit"] == 0
            count("miss_downwards", (miss & (x["rays"][:, 4] < 0)).sum())

    stats = rc.walk(ref, rays, st, kind, other=orc, on_bounce=on_bounce)
    W["depth_limit"] = stats["depth_limit"]
    print("%s %s: %d paths, %d hit records, %d bounces compared, %d excluded, %d ghost records; %s" % (
        name, "fp16" if fp16 else "fp32", len(rays), stats["records"], stats["bounces"], stats["excluded"], stats["ghost_records"], sorted(W.items())))
    assert stats["excluded"] == 0
    ghosts = W["ghost_records_list"] + W["ghost_records_tree"]
    assert ghosts == 0 if not fp16 else ghosts * 100 < stats["records"]
    # not vacuous: a bounce for every second path; a quarter of that where binary16 overflow ends most paths at once
    assert stats["bounces"] >= (npaths // 8 if fp16 and name not in rc.EDGE else npaths // 2)
    if not fp16 or name in rc.EDGE:                     # (the far cameras' binary16 walks are too short to be asked for every branch)
        assert witnesses(name, W) == [], (witnesses(name, W), W)


# ---------------------------------------------------------------------------------------------------- camera
@pytest.mark.parametrize("nx,ny,aperture", [(64, 40, None), (61, 35, None), (64, 40, 0.0), (131, 99, None)])
def test_camera_constructor_fp32(nx, ny, aperture):
    """all 22 floats, at the four frame shapes of test_the_closed_form_camera_is_the_librarys; and create_world's camera"""
    c = mw.CAMERA
    args = (c["lookfrom"], c["lookat"], c["vup"], c["vfov"], float(F(nx) / F(ny)), c["aperture"] if aperture is None else aperture, c["focus"])
    ref = ref_lib.camera(*args)
    assert np.array_equal(f32_bits(oracle_lib.make_camera(*args)), f32_bits(ref))
    assert np.array_equal(f32_bits(mw.camera_floats(nx, ny, aperture)), f32_bits(ref))
    args = ((13, 2, 3), (0, 0, 0), (0, 1, 0), 30.0, float(F(nx) / F(ny)), 0.1, 10.0)
    assert np.array_equal(f32_bits(oracle_lib.make_camera(*args)), f32_bits(ref_lib.camera(*args)))
    assert np.array_equal(f32_bits(oracle_lib.OracleScene(22, nx, ny).camera()), f32_bits(ref_lib.camera(*args)))


@pytest.mark.parametrize("fp16", [False, True])
def test_get_ray(fp16):
    """20 000 (s, t), some outside [0, 1], from the same 22 floats and states: open lens, lens radius 0, create_world's camera"""
    rng = np.random.default_rng(9)
    n = 20000
    s, t = rng.uniform(-0.1, 1.1, n).astype(F), rng.uniform(-0.1, 1.1, n).astype(F)
    st = ref_lib.curand_init(rng.integers(0, 2 ** 40, n).astype(np.uint64), fp16)
    for cam in (mw.camera_floats(64, 40), mw.camera_floats(64, 40, 0.0), oracle_lib.OracleScene(22, 1200, 800, fp16=fp16).camera()):
        if fp16:
            cam, s, t = rc.half(cam), rc.half(s), rc.half(t)
        a, sa = ref_lib.get_ray(cam, s, t, st, fp16)
        b, sb = oracle_lib.get_ray(cam, s, t, st, fp16)
        assert same_nan_as_ref(b, a) and np.array_equal(sa, sb)
        assert (sa != st).any()
