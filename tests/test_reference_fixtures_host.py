"""The recorded results of the reference's own functions (tests/golden/reference_*.npz, written by golden/make_reference_golden.py from
a CPU build of the reference's headers) against the CPU oracle and the host code.  Not marked gpu, and it never skips: this is the pin
that stays where the reference itself is absent.  Bit equality, "NaN where the reference has NaN" (bitcmp.same_nan_as_ref).

reference_frames.npz holds whole frames of main.cu's own render loops (tests/reference_frames.py, recorded from the main libraries
of oracle/ref_main_capi.cpp): the oracle's render / render_progressive / create_world and the host code's rt_create_world are held to it.

The last tests re-record from the live libraries, where oracle/_ref/ is built, and hold the files to what they give now."""
import os

import numpy as np
import pytest

import oracle_lib
import ref_lib
import reference_cases as rc
import reference_frames as rf
from bitcmp import f32_bits, same_nan_as_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PRECISIONS = [False, True]


@pytest.fixture(scope="module")
def gold():
    return {f: np.load(os.path.join(GOLD, "reference_%s.npz" % f)) for f in ("hits", "bounces", "octrees")}


@pytest.fixture(scope="module")
def frames():
    return np.load(os.path.join(GOLD, "reference_frames.npz"))


def tree_cases():
    return [(n, None) for n in rc.NAMES] + list(rc.SMALL_BUCKETS)


@pytest.mark.parametrize("fp16", PRECISIONS)
@pytest.mark.parametrize("name", rc.NAMES)
def test_oracle_hit_records(gold, name, fp16):
    w = rc.world_of(gold, name, fp16)
    rays = gold["hits"][name + "_rays"]
    assert len(rays) >= rc.GX * rc.GY + 32
    if fp16:
        rays = rc.half(rays)
    S = rc.oracle_side(w, fp16)
    hits = 0
    for mode, m in ((1, "list"), (2, "tree")):
        got = S.trace(rays, mode)
        k = "%s_%s_" % (rc.tag(name, fp16), m)
        assert np.array_equal(got["sphere"], gold["hits"][k + "sphere"]), m
        for f in ("t", "p", "normal"):
            assert same_nan_as_ref(got[f], gold["hits"][k + f]), (m, f)
        hits += int((got["sphere"] >= 0).sum())
    assert hits > 0 or (fp16 and name == "created_22")           # (binary16 from the far camera: b * b overflows)


@pytest.mark.parametrize("fp16", PRECISIONS)
@pytest.mark.parametrize("name", rc.NAMES)
def test_oracle_bounces_and_camera_rays(gold, name, fp16):
    w = rc.world_of(gold, name, fp16)
    g, k = gold["bounces"], rc.tag(name, fp16) + "_"
    S = rc.oracle_side(w, fp16)
    n = g[k + "sphere"].size
    wide = lambda s: np.concatenate([s, np.zeros((len(s), 6), np.uint32)], 1)
    if n:
        ret, att, out, st = S.scatter(g[k + "sphere"], g[k + "rin"], g[k + "rec"], wide(g[k + "s0"]))
        assert np.array_equal(ret, g[k + "ret"])
        assert same_nan_as_ref(att, g[k + "att"]) and same_nan_as_ref(out, g[k + "out"])
        assert np.array_equal(st, wide(g[k + "s1"]))
    else:
        assert fp16 and name.startswith("created")               # (no camera ray hits anything there)
    # the camera rays the walks started from: seed 1984 + p, two draws, get_ray
    s_t, want = g[k + "camera_s_t"], g[k + "camera_rays"]
    st = np.zeros((len(s_t), 12), np.uint32)
    for p in range(len(s_t)):
        oracle_lib.lib().orc_xorwow_init(st[p].ctypes.data, 1984 + p)
        oracle_lib.lib().orc_uniform(st[p].ctypes.data)
        oracle_lib.lib().orc_uniform(st[p].ctypes.data)
    rays, _ = oracle_lib.get_ray(w[3], s_t[:, 0], s_t[:, 1], st, fp16=fp16)
    assert same_nan_as_ref(rays, want)


@pytest.mark.parametrize("fp16", PRECISIONS)
@pytest.mark.parametrize("name,spl", tree_cases())
def test_oracle_octree(gold, name, spl, fp16):
    w = rc.world_of(gold, name, fp16)
    S = rc.oracle_side(w, fp16, spl)
    k = "%s_spl%d_" % (rc.tag(name, fp16), spl or w[4])
    t, info = S.octree(), S.info()
    assert [info[f] for f in ("node_count", "leaf_count", "dropped_full", "dropped_outside")] == gold["octrees"][k + "counts"].tolist()
    assert np.array_equal(rc.sha(*(t[f] for f in ("level", "box", "children", "counts", "indices"))), gold["octrees"][k + "sha"])


@pytest.mark.parametrize("fp16", PRECISIONS)
@pytest.mark.parametrize("name,spl", tree_cases())
def test_host_code_octree(rt, gold, name, spl, fp16):
    """rt_build_octree (host/rt_scene.hpp), the tree the product renders through: the same nodes, leaves and counts"""
    w = rc.world_of(gold, name, fp16)
    spl = spl or w[4]
    W = rt.World(w[2].size, rc.NX, rc.NY, precision=rt.FP16 if fp16 else rt.FP32, spheres=rc.as_spheres(*w[:3]), camera=w[3].view(rt.camera_dtype))
    O = rt.Octree(W, spl)
    k = "%s_spl%d_" % (rc.tag(name, fp16), spl)
    info = O.info()
    assert [info[f] for f in ("node_count", "leaf_count", "dropped_full", "dropped_outside")] == gold["octrees"][k + "counts"].tolist()
    nodes = O.nodes()
    counts, idx = O.leaves()
    assert np.array_equal(rc.sha(nodes["level"], nodes["aabb"], nodes["children"], counts, idx), gold["octrees"][k + "sha"])


def test_the_fixtures_are_small_and_cover_every_world(gold):
    for f in ("hits", "bounces", "octrees"):
        assert os.path.getsize(os.path.join(GOLD, "reference_%s.npz" % f)) <= os.path.getsize(os.path.join(GOLD, "frames.npz"))
    for name in rc.NAMES:
        for fp16 in PRECISIONS:
            assert rc.tag(name, fp16) + "_tree_t" in gold["hits"] and rc.tag(name, fp16) + "_ret" in gold["bounces"]
    assert len([k for k in gold["octrees"].files if k.endswith("_sha")]) == 2 * len(tree_cases())


# ---------------------------------------------------------------------------------------------------- frames of main.cu's own loops
def test_the_frame_fixtures_are_small_and_cover_every_case(frames):
    assert os.path.getsize(os.path.join(GOLD, "reference_frames.npz")) <= os.path.getsize(os.path.join(GOLD, "frames.npz"))
    assert sorted(frames.files) == sorted(c.name + "_" + f for c in rf.CASES for f in ("frame", "states_sha", "list_sha", "camera", "params", "ghost"))
    for c in rf.CASES:
        assert np.array_equal(frames[c.name + "_params"], rf.params_of(c)), c.name
        shape = (c.passes, c.ny, c.nx, 3) if c.passes else (len(rf.rows_of(c)), c.nx, 3)
        assert frames[c.name + "_frame"].shape == shape and frames[c.name + "_frame"].dtype == (np.float16 if c.fp16 else np.float32)
        g = frames[c.name + "_ghost"]
        assert g.dtype == bool and g.shape == shape[-3:-1] and g.sum() * 100 < g.size and (c.fp16 or not g.any())
    assert {(c.fp16, c.octree) for c in rf.RENDER} == {(False, False), (False, True), (True, False), (True, True)}


@pytest.mark.parametrize("case", rf.CASES, ids=lambda c: c.name)
def test_oracle_frames(frames, case):
    """create_world's list and camera, the frame (the sum after each progressive pass) and the RNG states afterwards"""
    S = rf.oracle_scene(case)
    assert np.array_equal(rf.list_digest(*S.spheres()), frames[case.name + "_list_sha"])
    assert np.array_equal(f32_bits(S.camera()), f32_bits(frames[case.name + "_camera"]))
    got, g = rf.run(S, case), frames[case.name + "_ghost"]
    want = frames[case.name + "_frame"].astype(np.float32)
    assert same_nan_as_ref(got["frame"][..., ~g, :], want[..., ~g, :])
    assert np.array_equal(rf.state_digest(got["states"], g), frames[case.name + "_states_sha"])


@pytest.mark.parametrize("case", rf.CASES, ids=lambda c: c.name)
def test_host_code_create_world(rt, frames, case):
    """rt_rand_init + rt_create_world (host/rt_scene.hpp), the world the product renders: the reference's list, the camera rendered with"""
    W = rt.World(case.n, case.nx, case.ny, precision=rt.FP16 if case.fp16 else rt.FP32)
    assert np.array_equal(rf.list_digest_of_world(W), frames[case.name + "_list_sha"])
    assert np.array_equal(f32_bits(W.camera.view(np.float32)), f32_bits(frames[case.name + "_camera"]))


@pytest.mark.parametrize("case", rf.CASES, ids=lambda c: c.name)
def test_a_case_reaches_all_three_materials(case):
    """a check on the cases themselves: the oracle's walk through each calls material::scatter on a lambertian, a metal and a
    dielectric.  (How often, against the camera rays it starts, is the recorder's to assert: golden/make_reference_golden.py.)"""
    rays, scatters = rf.oracle_content(case)
    print("%s: %d camera rays, scatter calls %s" % (case.name, rays, scatters))
    assert rays == len(rf.rows_of(case)) * case.nx * case.ns * max(case.passes, 1)
    assert all(scatters[m] > 0 for m in ("lambertian", "metal", "dielectric"))


def test_the_live_main_libraries_still_give_the_frames(frames):
    if ref_lib.status() == "absent":
        pytest.skip("neither oracle/_ref/ nor the reference's sources are here")
    assert ref_lib.status() == "ok", "the reference's sources are here but oracle/_ref/ is incomplete: run `make -C oracle ref`"
    import sys
    sys.path.insert(0, GOLD)
    import make_reference_golden as mk
    d = mk.record_frames(both_builds=False)
    assert sorted(d) == sorted(frames.files)
    for k, v in d.items():
        a, b = np.asarray(v), frames[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_the_live_libraries_still_give_the_fixtures(gold):
    if ref_lib.status() == "absent":
        pytest.skip("neither oracle/_ref/ nor the reference's sources are here")
    assert ref_lib.status() == "ok", "the reference's sources are here but oracle/_ref/ is incomplete: run `make -C oracle ref`"
    import sys
    sys.path.insert(0, GOLD)
    import make_reference_golden as mk
    for f, d in mk.record().items():
        g = gold[f[len("reference_"):-len(".npz")]]
        assert sorted(d) == sorted(g.files), f
        for k, v in d.items():
            a, b = np.asarray(v), g[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (f, k)
