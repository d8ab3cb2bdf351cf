"""Records tests/golden/reference_{hits,bounces,octrees}.npz from the libraries of `make -C oracle ref` — a build of the REFERENCE's
own headers (oracle/ref_capi.cpp) — and never from the oracle: run it where oracle/_ref/ exists.

    python tests/golden/make_reference_golden.py          # rewrites the three files

The files hold data the reference's functions computed, for every world of tests/reference_cases.py in both precisions:
  reference_hits.npz      a ray set per world (the GX x GY pixel-centre rays of its camera, then lattice / random / edge rays) and the
                          records of hitable_list::hit and hitTree: sphere, t, p, normal
  reference_bounces.npz   bounces picked from lockstep walks along the reference: sphere, ray, record and RNG state in; return value,
                          attenuation, scattered ray and RNG state out (the first 6 state words: the others stay 0)
  reference_octrees.npz   buildOctree: the four counts and one SHA-256 over level, box, children, counts, indices (as worlds.npz does)
plus a SHA-256 of each world's own arrays, so that a changed world builder is told apart from a changed result.
tests/test_reference_fixtures_host.py holds the oracle and the host code to them, tests/test_gpu_reference_fixtures.py the kernels."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ref_lib                       # noqa: E402
import reference_cases as rc         # noqa: E402

N_RAYS = 64                          # after the GX * GY pixel-centre rays
N_PATHS, N_BOUNCES = 128, 48
FILES = ("reference_hits.npz", "reference_bounces.npz", "reference_octrees.npz")


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def tag(name, fp16):
    return "%s_%s" % (name, "fp16" if fp16 else "fp32")


def tree_cases():
    return [(n, f, None) for n in rc.NAMES for f in (False, True)] + [(n, f, s) for n, s in rc.SMALL_BUCKETS for f in (False, True)]


def record():
    """the three files' contents as dicts of arrays"""
    hits, bounces, trees = {}, {}, {}
    for name in rc.NAMES:
        for fp16 in (False, True):
            w = rc.world(name, fp16)
            geom, mat, kind, cam, spl = w
            k = tag(name, fp16)
            hits[k + "_world_sha"] = sha(geom, mat, kind, cam)
            ref = rc.reference_side(w, fp16)
            # hit records
            rays = rc.ray_set(name, rc.world(name, False), N_RAYS)
            if fp16:
                rays = rc.half(rays)
            else:
                hits[name + "_rays"] = rays
            for mode, m in ((1, "list"), (2, "tree")):
                h = rc.trace(ref, rays, mode)
                assert (h["sphere"] != -2).all(), "a ghost slot's record: pick other rays"
                for f in ("sphere", "t", "p", "normal"):
                    hits["%s_%s_%s" % (k, m, f)] = h[f]
            # bounces
            rec = dict(sphere=[], rin=[], rec=[], s0=[], ret=[], att=[], out=[], s1=[])

            def keep(depth, live, x, out, oout):
                ok = ~x["excluded"]
                for key, v in (("sphere", x["sphere"]), ("rin", x["rin"]), ("rec", x["rec"]), ("s0", x["states"]), ("ret", out[0]),
                               ("att", out[1]), ("out", out[2]), ("s1", out[3])):
                    rec[key].append(v[ok])

            s, t, r0, st = rc.camera_samples(cam, N_PATHS, fp16, lambda x: ref_lib.curand_uniform(x, fp16), lambda x: ref_lib.curand_init(x, fp16),
                                             lambda *a: ref_lib.get_ray(*a, fp16=fp16))
            stats = rc.walk(ref, r0, st, kind, on_bounce=keep)
            assert stats["excluded"] == 0
            rec = {key: np.concatenate(v) for key, v in rec.items()}
            n = rec["sphere"].size
            pick = np.sort(np.random.default_rng(17).permutation(n)[:N_BOUNCES])
            assert not rec["s0"][:, 6:].any() and not rec["s1"][:, 6:].any()
            for key, v in rec.items():
                bounces["%s_%s" % (k, key)] = v[pick][:, :6] if key in ("s0", "s1") else v[pick]
            bounces[k + "_camera_s_t"] = np.stack([s, t], 1)[:16]
            bounces[k + "_camera_rays"] = r0[:16]
    for name, fp16, spl in tree_cases():
        w = rc.world(name, fp16)
        t, info = rc.reference_side(w, fp16, spl).build_octree()
        k = tag(name, fp16) + "_spl%d" % (spl or w[4])
        trees[k + "_sha"] = sha(*(t[f] for f in ("level", "box", "children", "counts", "indices")))
        trees[k + "_counts"] = np.array([info[f] for f in ("node_count", "leaf_count", "dropped_full", "dropped_outside")], np.int64)
    return dict(zip(FILES, (hits, bounces, trees)))


if __name__ == "__main__":
    assert ref_lib.status() == "ok", "oracle/_ref/ is not built: make -C oracle ref"
    for f, d in record().items():
        np.savez_compressed(os.path.join(HERE, f), **d)
        print("%s: %d arrays, %d bytes" % (f, len(d), os.path.getsize(os.path.join(HERE, f))))
