"""ctypes binding of the libraries that `make -C oracle ref` builds from the REFERENCE's own headers (oracle/ref_capi.cpp, oracle/_ref/).

Test infrastructure only.  The libraries exist where the reference's sources were at build time; on a clean checkout without them
`status()` says so and the live comparisons skip — the recorded fixtures under tests/golden/ (make_reference_golden.py) still hold."""
import ctypes as C
import os
import re

import numpy as np

from oracle_lib import ORACLE_DIR

REF_DIR = os.path.join(ORACLE_DIR, "_ref")
SPLS = (3, 4, 30, 32, 40, 64)
_LIBS = {}


def source_dir():
    """where the reference's sources are expected: $REF, else the default of oracle/Makefile"""
    if os.environ.get("REF"):
        return os.environ["REF"]
    m = re.search(r"^REF \?= *(\S+)", open(os.path.join(ORACLE_DIR, "Makefile")).read(), re.M)
    return m.group(1)


def lib_path(fp16, spl):
    return os.path.join(REF_DIR, "libref_%s_spl%d.so" % ("fp16" if fp16 else "fp32", spl))


def status():
    """'ok', 'absent' (neither libraries nor sources: nothing to compare with) or 'unbuilt' (sources without all libraries: an error)"""
    have = [os.path.exists(lib_path(f, s)) for f in (False, True) for s in SPLS]
    if all(have):
        return "ok"
    if not any(have) and not os.path.isdir(REF_DIR) and not os.path.exists(os.path.join(source_dir(), "acceleration_structure.h")):
        return "absent"
    return "unbuilt"


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def lib(fp16=False, spl=30):
    key = (bool(fp16), spl)
    if key not in _LIBS:
        L = C.CDLL(lib_path(*key))
        L.ref_world_create.restype = C.c_void_p
        L.ref_world_create.argtypes = [C.c_int] + [C.c_void_p] * 3
        L.ref_world_destroy.argtypes = [C.c_void_p]
        L.ref_build_info.argtypes = [C.c_void_p]
        L.ref_build_octree.argtypes = [C.c_void_p, C.c_void_p]
        L.ref_octree_nodes.argtypes = [C.c_void_p] * 4
        L.ref_octree_leaves.argtypes = [C.c_void_p] * 3
        L.ref_trace.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.ref_scatter.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 7
        L.ref_dielectric_branch.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5
        L.ref_camera.argtypes = [C.c_void_p, C.c_void_p]
        L.ref_get_ray.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4
        L.ref_curand_init.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
        L.ref_curand_uniform.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
        info = np.zeros(4, np.int32)
        L.ref_build_info(_p(info))
        assert info.tolist() == [int(key[0]), spl, info[2], 48], info
        _LIBS[key] = L
    return _LIBS[key]


class RefWorld:
    """a world of the reference's own sphere / material objects, from the arrays OracleScene(custom=) takes"""

    def __init__(self, geom, mat, kind, fp16=False, spl=30):
        self.L, self.fp16, self.spl = lib(fp16, spl), bool(fp16), spl
        geom, mat, kind = np.ascontiguousarray(geom, np.float32), np.ascontiguousarray(mat, np.float32), np.ascontiguousarray(kind, np.int32)
        self.n = kind.size
        assert geom.shape == (self.n, 4) and mat.shape == (self.n, 4)
        self.h = C.c_void_p(self.L.ref_world_create(self.n, _p(geom), _p(mat), _p(kind)))
        self._info = None

    def close(self):
        if self.h:
            self.L.ref_world_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def build_octree(self):
        """buildOctree: the arrays of OracleScene.octree() plus the four counts of OracleScene.info()"""
        if self._info is None:
            out = np.zeros(4, np.int64)
            self.L.ref_build_octree(self.h, _p(out))
            self._info = dict(zip(("node_count", "leaf_count", "dropped_full", "dropped_outside"), out.tolist()))
        level, box, children = np.zeros(585, np.int32), np.zeros((585, 6), np.float32), np.zeros((585, 8), np.int32)
        self.L.ref_octree_nodes(self.h, _p(level), _p(box), _p(children))
        lc = self._info["leaf_count"]
        counts, idx = np.zeros(lc, np.int32), np.zeros((lc, self.spl), np.int32)
        self.L.ref_octree_leaves(self.h, _p(counts), _p(idx))
        return dict(level=level, box=box, children=children, counts=counts, indices=idx), dict(self._info)

    def trace(self, rays, mode):
        """mode 1: hitable_list::hit, mode 2: hitTree (build_octree first); sphere -2: a ghost slot's record"""
        if mode == 2 and self._info is None:
            self.build_octree()
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = rays.shape[0]
        hit, sph, t = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        p, nrm = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        self.L.ref_trace(self.h, n, _p(rays), mode, _p(hit), _p(sph), _p(t), _p(p), _p(nrm))
        return dict(hit=hit, sphere=sph, t=t, p=p, normal=nrm)

    def scatter(self, sphere, rays, recs, states):
        sphere = np.ascontiguousarray(sphere, np.int32)
        n = sphere.size
        rays, recs = np.ascontiguousarray(rays, np.float32).reshape(n, 6), np.ascontiguousarray(recs, np.float32).reshape(n, 7)
        st = np.array(states, np.uint32).reshape(n, 12)
        ret, att, out = np.zeros(n, np.int32), np.zeros((n, 3), np.float32), np.zeros((n, 6), np.float32)
        self.L.ref_scatter(self.h, n, _p(sphere), _p(rays), _p(recs), _p(st), _p(ret), _p(att), _p(out))
        return ret, att, out, st

    def dielectric_branch(self, sphere, rays, recs, scattered):
        """witness bits per dielectric bounce: 1 the ray leaves the sphere, 2 refract() succeeded, 4 the reflected direction was taken"""
        sphere = np.ascontiguousarray(sphere, np.int32)
        n = sphere.size
        out = np.zeros(n, np.int32)
        self.L.ref_dielectric_branch(self.h, n, _p(sphere), _p(np.ascontiguousarray(rays, np.float32)), _p(np.ascontiguousarray(recs, np.float32)),
                                     _p(np.ascontiguousarray(scattered, np.float32)), _p(out))
        return out


def camera(lookfrom, lookat, vup, vfov, aspect, aperture, focus_dist, fp16=False):
    args = np.array(list(lookfrom) + list(lookat) + list(vup) + [vfov, aspect, aperture, focus_dist], np.float32)
    out = np.zeros(22, np.float32)
    lib(fp16).ref_camera(_p(args), _p(out))
    return out


def get_ray(cam, s, t, states, fp16=False):
    cam, s, t = np.ascontiguousarray(cam, np.float32).ravel(), np.ascontiguousarray(s, np.float32), np.ascontiguousarray(t, np.float32)
    st = np.array(states, np.uint32).reshape(s.size, 12)
    rays = np.zeros((s.size, 6), np.float32)
    lib(fp16).ref_get_ray(_p(cam), s.size, _p(s), _p(t), _p(st), _p(rays))
    return rays, st


def curand_init(seeds, fp16=False):
    seeds = np.ascontiguousarray(seeds, np.uint64)
    st = np.zeros((seeds.size, 12), np.uint32)
    lib(fp16).ref_curand_init(seeds.size, _p(seeds), _p(st))
    return st


def curand_uniform(states, fp16=False):
    """one curand_uniform from each state: (draws, states after)"""
    st = np.array(states, np.uint32).reshape(-1, 12)
    out = np.zeros(st.shape[0], np.float32)
    lib(fp16).ref_curand_uniform(st.shape[0], _p(st), _p(out))
    return out, st
