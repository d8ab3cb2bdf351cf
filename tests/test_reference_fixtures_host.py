"""The recorded results of the reference's own functions (tests/golden/reference_*.npz, written by golden/make_reference_golden.py from
a CPU build of the reference's headers) against the CPU oracle and the host code.  Not marked gpu, and it never skips: this is the pin
that stays where the reference itself is absent.  Bit equality, "NaN where the reference has NaN" (bitcmp.same_nan_as_ref).

The last test re-records from the live libraries, where oracle/_ref/ is built, and holds the files to what they give now."""
import os

import numpy as np
import pytest

import oracle_lib
import ref_lib
import reference_cases as rc
from bitcmp import same_nan_as_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PRECISIONS = [False, True]


@pytest.fixture(scope="module")
def gold():
    return {f: np.load(os.path.join(GOLD, "reference_%s.npz" % f)) for f in ("hits", "bounces", "octrees")}


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
