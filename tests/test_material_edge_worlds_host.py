"""The worlds of tests/material_edge_worlds.py on the CPU oracle alone (that the oracle's bounces in these worlds are the reference's is
tests/test_reference_pins_host.py's business): each one really reaches the branch it is named for, so the GPU
comparisons of tests/test_gpu_material_edges.py cannot pass vacuously.  The bounds are conditions with wide margins over what the
oracle gives (every test prints its figures; 64 x 40, 16 spp, list / tree: about 47 / 48 rays per sample in the white and the mirror
room, 17 / 16 in tir_room; extremes: hundreds of NaN and of infinite pixels, over two thirds finite).  A recipe that misses one is
retuned, not the bound.

What the oracle says about negative radii in the octree shapes the `shells` recipe: buildOctree grows a node's box by the radius
(acceleration_structure.h:82-93), so a negative radius SHRINKS it, and a shell is stored only where its centre lies deeper than |r|
inside a leaf cell (0.25 high).  It vanishes silently otherwise — no child box matches, and nothing is counted as dropped.  `shells`
therefore floats its small hollow beads at the mid-height of a cell; the conditions below hold through the tree as through the list.
Slot 0 — the rooms' wall — is tested outside the tree and is always there."""
import numpy as np
import pytest

import material_edge_worlds as mw
from bitcmp import f32_bits

NX, NY, NS = 64, 40, 16


def render(name, variant=None, tree=False, sp=None):
    s, cam = mw.world(name, NX, NY, variant)
    fb, _, c = mw.oracle(s if sp is None else sp, cam, NX, NY, tree=tree).render(NS, nthreads=8, counters=True)
    return fb, c["rays"] / c["samples"]


def differing(a, b):
    return float((f32_bits(a) != f32_bits(b)).any(axis=2).mean())


def test_the_builders_are_deterministic_and_large_enough_for_the_candidate_grid():
    for name, variant in mw.WORLDS:
        a, cam_a = mw.world(name, NX, NY, variant)
        b, cam_b = mw.world(name, NX, NY, variant)
        assert a.tobytes() == b.tobytes() and cam_a.tobytes() == cam_b.tobytes()
        assert (a["material"][1:] != mw.MAT_NONE).sum() >= 64, name
        assert (a["material"] == mw.MAT_NONE).sum() >= 1 or name == "extremes", name
    cam = mw.camera_floats(NX, NY)
    assert cam.shape == (22,) and cam[21] == np.float32(0.01)
    assert mw.world("extremes", NX, NY)[1][21] == 0.0                          # lens_radius == 0
    assert mw.world("extremes", NX, NY, "ghost0")[0]["material"][0] == mw.MAT_NONE


def test_glass_indices_has_every_index_in_several_sizes():
    sp = mw.spheres("glass_indices")
    glass = sp[sp["material"] == mw.DIELECTRIC]
    for ri in mw.INDICES:
        at = glass[glass["param"] == np.float32(ri)]
        assert len(at) >= 10 and len(np.unique(at["radius"])) >= 3, ri
    assert (glass["radius"] >= 0.8).sum() == 3
    sh = mw.spheres("shells")
    neg = mw.negative(sh)
    partners = neg[(sh["material"][neg] == mw.DIELECTRIC)]
    assert len(partners) >= len(glass) // 2 - 3
    assert (sh["center"][partners] == sh["center"][partners - 1]).all() and (sh["param"][partners] == sh["param"][partners - 1]).all()
    ratio = np.round(sh["radius"][partners].astype(np.float64) / sh["radius"][partners - 1], 3)
    assert set(ratio.tolist()) == {-0.9, -0.5}
    assert set(sh["material"][neg].tolist()) == {mw.LAMBERTIAN, mw.METAL, mw.DIELECTRIC}


@pytest.mark.parametrize("tree", [False, True])
def test_white_room_is_black_and_every_path_runs_to_the_depth_limit(tree):
    fb, rays = render("white_room", tree=tree)
    print("white_room tree=%d: %.2f rays per sample, %d black pixels" % (tree, rays, (fb == 0).all(axis=2).sum()))
    assert rays >= 40
    assert (f32_bits(fb) == 0).all()


def test_mirror_room_paths_run_to_the_depth_limit():
    for tree in (False, True):
        fb, rays = render("mirror_room", tree=tree)
        print("mirror_room tree=%d: %.2f rays per sample" % (tree, rays))
        assert rays >= 40


def test_tir_room_mixes_paths_that_end_at_the_limit_with_paths_that_leave():
    sp, cam = mw.world("tir_room", NX, NY)
    for tree in (False, True):
        S = mw.oracle(sp, cam, NX, NY, tree=tree)
        fb, _, c = S.render(NS, nthreads=8, counters=True)
        rays = c["rays"] / c["samples"]
        black = float((fb == 0).all(axis=2).mean())
        st = S.render_init()
        one = np.zeros((NY, NX, 3), np.float32)
        zero = lit = 0
        for _ in range(NS):
            S.render_progressive(one, 1, st, nthreads=8)
            zero += int((one == 0).all(axis=2).sum())
            lit += int((one != 0).any(axis=2).sum())
        zero, lit = zero / (NS * NX * NY), lit / (NS * NX * NY)
        print("tir_room tree=%d: %.2f rays per sample, black pixels %.4f, one-sample colours zero %.4f non-zero %.4f" % (tree, rays, black, zero, lit))
        assert 5 <= rays <= 30
        assert black <= 0.05
        assert zero >= 0.03 and lit >= 0.30


@pytest.mark.parametrize("name,variant", [("glass_indices", None), ("shells", None), ("shells", "solid"), ("shells", "hollow")])
def test_open_scenes_tell_a_wrong_index_and_a_wrong_radius_sign_apart(name, variant):
    """no NaN pixel; the frame differs from the same world with every index 1.5 — and, where the world has negative radii (glass_indices
    has none: its |r| twin is itself), from the same world with every radius replaced by its absolute value — in >= 5 % of the pixels"""
    sp = mw.spheres(name, variant)
    for tree in (False, True):
        fb, _ = render(name, variant, tree)
        assert not np.isnan(fb).any()
        d = differing(fb, render(name, variant, tree, sp=mw.with_index(sp))[0])
        print("%s/%s tree=%d: differs from index 1.5 in %.3f of the pixels" % (name, variant, tree, d))
        assert d >= 0.05
        if name == "shells":
            d = differing(fb, render(name, variant, tree, sp=mw.with_positive_radii(sp))[0])
            print("%s/%s tree=%d: differs from |radius| in %.3f of the pixels" % (name, variant, tree, d))
            assert d >= 0.05


def test_shells_are_seen_through_the_tree_too():
    """the tree keeps the small shells: its `shells` frame is not the `glass_indices` frame, and its leaves hold negative radii"""
    a, b = render("glass_indices", tree=True)[0], render("shells", tree=True)[0]
    d = differing(a, b)
    sp, cam = mw.world("shells", NX, NY)
    t = mw.oracle(sp, cam, NX, NY, tree=True).octree()
    stored = np.unique(t["indices"][np.arange(t["indices"].shape[1])[None, :] < t["counts"][:, None]])
    kept = np.intersect1d(stored, mw.negative(sp))
    print("shells through the tree: differs from glass_indices in %.3f of the pixels; %d of %d negative-radius spheres are stored" % (
        d, kept.size, mw.negative(sp).size))
    assert d >= 0.05
    assert kept.size >= 20 and {mw.LAMBERTIAN, mw.METAL, mw.DIELECTRIC} <= set(sp["material"][kept].tolist())


def test_camera_inside_glass_changes_the_whole_frame():
    base = render("shells")[0]
    for variant in ("solid", "hollow"):
        assert differing(base, render("shells", variant)[0]) >= 0.9


@pytest.mark.parametrize("variant", [None, "ghost0"])
def test_extremes_has_nan_infinite_and_finite_pixels(variant):
    for tree in (False, True):
        fb, _ = render("extremes", variant, tree)
        px = fb.reshape(-1, 3)
        nan = np.isnan(px).any(axis=1)
        inf = np.isinf(px).any(axis=1)
        finite = np.isfinite(px).all(axis=1)
        print("extremes/%s tree=%d: %d NaN, %d infinite, %d finite pixels" % (variant, tree, nan.sum(), inf.sum(), finite.sum()))
        assert nan.sum() >= 10 and inf.sum() >= 10 and finite.sum() >= px.shape[0] // 2


@pytest.mark.parametrize("name,variant", [("shells", None), ("shells", "hollow"), ("tir_room", None)])
def test_the_ray_set_hits_negative_radius_spheres_and_their_normals_point_inward(name, variant):
    """through the list and through the tree"""
    sp, cam = mw.world(name, NX, NY, variant)
    rays = mw.edge_rays(sp, 100_000, 11)
    S = mw.oracle(sp, cam, NX, NY, tree=True)
    for mode in (1, 2):
        ref = S.trace(rays, mode=mode)
        s = ref["sphere"]
        neg = (s >= 0) & (sp["radius"][np.maximum(s, 0)] < 0)
        print("%s/%s %s: %.3f of the records hit a negative-radius sphere" % (name, variant, ("", "list", "tree")[mode], neg.mean()))
        assert neg.mean() >= 0.05
        d = np.einsum("ij,ij->i", ref["normal"][neg].astype(np.float64), ref["p"][neg].astype(np.float64) - sp["center"][s[neg]])
        assert (d < 0).all()


def test_the_ray_set_reaches_the_radius_zero_sphere_exactly():
    sp = mw.spheres("extremes")
    zero = np.flatnonzero((sp["material"] != mw.MAT_NONE) & (sp["radius"] == 0))
    assert zero.size == 1
    rays = mw.edge_rays(sp, 100_000, 11).astype(np.float64)
    k, m = 25_000, 2_000
    o, d = rays[k:k + m, :3], rays[k:k + m, 3:]
    t = (sp["center"][zero[0]].astype(np.float64) - o) / np.where(d == 0, np.nan, d)
    # origin + t * direction is the centre, exactly, with one integer t per ray
    assert (np.nanmax(t, axis=1) == np.nanmin(t, axis=1)).all() and (np.nanmin(t, axis=1) >= 1).all()
