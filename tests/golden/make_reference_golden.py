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
tests/test_reference_fixtures_host.py holds the oracle and the host code to them, tests/test_gpu_reference_fixtures.py the kernels.

It also records tests/golden/reference_frames.npz from the main libraries (oracle/ref_main_capi.cpp over main.cu's own text above
`int main(`), for every case of tests/reference_frames.py:
  <case>_frame        render: the rows x nx x 3 frame (whole small frames, the listed rows of the 1200 x 800 ones), binary16 cases as
                      float16; render_progressive: passes x ny x nx x 3, the sum buffer after each pass
  <case>_states_sha   SHA-256 of the six state words of those pixels afterwards          <case>_list_sha   of create_world's list
  <case>_camera       the 22 floats rendered with          <case>_params   reference_frames.params_of          <case>_ghost   the pixels
                      where the reference reached a slot create_world left unwritten and has no result (ref_main_capi.cpp)
A case is recorded only if the driver built at -O0 and at -O2 gives the same bytes (after a dielectric draw of exactly 1.0 the
reference reads an uninitialised direction: such a frame is no fixture), and the oracle's walk through it calls scatter on all three
materials.  The file is written with fixed zip dates, so a second run reproduces it byte for byte.  The run then asserts that every
case calls scatter more often than it starts camera rays, which 11 of the 16 cases do not (see the end of this file).
tests/test_reference_fixtures_host.py holds the oracle to it, tests/test_gpu_reference_frames.py the render kernels."""
import hashlib
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ref_lib                       # noqa: E402
import reference_cases as rc         # noqa: E402
import reference_frames as rf        # noqa: E402

N_RAYS = 64                          # after the GX * GY pixel-centre rays
N_PATHS, N_BOUNCES = 128, 48
FILES = ("reference_hits.npz", "reference_bounces.npz", "reference_octrees.npz")
FRAMES = "reference_frames.npz"


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


def record_frames(verbose=False, both_builds=True):
    """reference_frames.npz's contents: everything from the main libraries; the oracle is asked only what the inputs walk through.
    both_builds False leaves out the -O0 run (the test that re-records: the file it compares with was written with it)"""
    out = {}
    for c in rf.CASES:
        R = rf.reference_scene(c)
        a = rf.run(R, c)
        b = rf.run(rf.reference_scene(c, opt=0), c) if both_builds else a
        for k in ("frame", "states", "ghost"):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), "%s: %s differs between the -O0 and the -O2 build" % (c.name, k)
        assert not a["states"][:, 6:].any()
        assert a["ghost"].sum() * 100 < a["ghost"].size and (c.fp16 or not a["ghost"].any()), c.name
        rays, scatters = rf.oracle_content(c)
        assert all(scatters[m] > 0 for m in ("lambertian", "metal", "dielectric")), (c.name, scatters)
        frame = a["frame"]
        if c.fp16:
            with np.errstate(over="raise"):
                half = frame.astype(np.float16)
            assert np.array_equal(half.astype(np.float32).view(np.uint32)[~np.isnan(frame)], frame.view(np.uint32)[~np.isnan(frame)])
            frame = half
        out[c.name + "_frame"] = frame
        out[c.name + "_states_sha"] = rf.state_digest(a["states"], a["ghost"])
        out[c.name + "_list_sha"] = rf.list_digest(*R.spheres())
        out[c.name + "_camera"] = R.camera()
        out[c.name + "_params"] = rf.params_of(c)
        out[c.name + "_ghost"] = a["ghost"]
        if verbose:
            print("%-22s %6d camera rays, scatter calls %s (%.2f per camera ray), %d ghost pixels, %d NaN pixels" % (
                c.name, rays, scatters, sum(scatters.values()) / rays, a["ghost"].sum(), np.isnan(a["frame"]).any(-1).sum()))
        if sum(scatters.values()) <= rays:
            thin.append(c.name)
    return out


thin = []                            # the cases whose walk calls scatter no more often than it starts camera rays


def write_npz(path, arrays):
    """np.savez_compressed with the zip dates fixed: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asarray(arrays[k]), allow_pickle=False)


if __name__ == "__main__":
    assert ref_lib.status() == "ok", "oracle/_ref/ is not built: make -C oracle ref"
    for f, d in record().items():
        np.savez_compressed(os.path.join(HERE, f), **d)
        print("%s: %d arrays, %d bytes" % (f, len(d), os.path.getsize(os.path.join(HERE, f))))
    d = record_frames(verbose=True)
    write_npz(os.path.join(HERE, FRAMES), d)
    size = os.path.getsize(os.path.join(HERE, FRAMES))
    print("%s: %d arrays, %d bytes" % (FRAMES, len(d), size))
    assert size <= os.path.getsize(os.path.join(HERE, "frames.npz")), "reference_frames.npz is larger than frames.npz"
    # Asked of every case: its walk calls scatter more often than it starts camera rays.  Asserted last, so that the file above is
    # written and can be looked at.  At the frame sizes the cases have, this does NOT hold on 11 of the 16: much of a small frame is sky,
    # and in binary16 most camera rays miss everything (b * b overflows from create_world's far camera).  Scatter calls per camera ray:
    #     n22 0.85 (7799 / 9216)   n500 and its progressive case 0.99 (6338 / 6405)   n5 0.86 (13200 / 15360)
    #     n22 fp16 0.19 tree (1740 / 9216), 0.19 list (1777)   n500 fp16 0.35 tree (2242 / 6405), 0.37 list (2354)
    # against n10000 1.67, n2000 1.22, the reference as shipped 1.69 and n1000 2.08, where it holds.  Neither the cases nor this
    # condition are changed here: the run ends on this assertion until one of the two is decided anew.
    assert not thin, "no more scatter calls than camera rays in: " + ", ".join(thin)
