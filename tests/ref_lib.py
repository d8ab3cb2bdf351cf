"""ctypes binding of the libraries that `make -C oracle ref` builds from the REFERENCE's own text (oracle/_ref/): libref_* from its nine
headers (oracle/ref_capi.cpp) and libmain_* from main.cu's text above `int main(` (oracle/ref_main_capi.cpp: create_world, render_init,
render, render_progressive, output_to_stream), one main library per case of MAIN_RENDER and MAIN_WORLD.

Not reached by either: main() itself and the window loop, whose <<<>>> launches do not parse as C++.

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
# the main cases of oracle/Makefile: (fp16, NUM_SPHERES, SPHERE_RADIUS as written, USE_OCTREE, SPHERES_PER_LEAF or "own": the header's)
MAIN_RENDER = tuple((f, n, "0.1", o, s) for f, n, o, s in (
    (False, 8000, True, "own"), (False, 1000, True, 30), (False, 1000, False, 30), (False, 5, True, 30), (False, 5, False, 30),
    (False, 22, True, 30), (False, 22, False, 30), (False, 500, True, 30), (False, 500, False, 30), (False, 10000, True, 32),
    (False, 2000, True, 3), (True, 22, True, 30), (True, 22, False, 30), (True, 500, True, 30), (True, 500, False, 30)))
MAIN_WORLD = ((False, 500, "0.2", True, 30), (True, 5, "0.1", True, 30), (True, 8000, "0.1", True, "own"), (True, 10000, "0.1", True, 32),
              (True, 500, "0.2", True, 30))
OWN_SPL = 30                         # acceleration_structure.h:15 as shipped; build_info reports it
_MAIN = {}


def source_dir():
    """where the reference's sources are expected: $REF, else the default of oracle/Makefile"""
    if os.environ.get("REF"):
        return os.environ["REF"]
    m = re.search(r"^REF \?= *(\S+)", open(os.path.join(ORACLE_DIR, "Makefile")).read(), re.M)
    return m.group(1)


def lib_path(fp16, spl):
    return os.path.join(REF_DIR, "libref_%s_spl%d.so" % ("fp16" if fp16 else "fp32", spl))


def main_path(case, opt=2):
    fp16, n, radius, octree, spl = case
    return os.path.join(REF_DIR, "libmain_%s_n%d_r%s_oct%d_spl%s_O%d.so" % ("fp16" if fp16 else "fp32", n, radius, int(octree), spl, opt))


def status():
    """'ok', 'absent' (neither libraries nor sources: nothing to compare with) or 'unbuilt' (sources without all libraries: an error)"""
    have = [os.path.exists(lib_path(f, s)) for f in (False, True) for s in SPLS]
    have += [os.path.exists(main_path(c)) for c in MAIN_RENDER + MAIN_WORLD] + [os.path.exists(main_path(c, 0)) for c in MAIN_RENDER]
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


def main_case(n, fp16=False, octree=True, spl=30, radius="0.1"):
    """the case of MAIN_RENDER / MAIN_WORLD with these parameters; there is exactly one"""
    got = [c for c in MAIN_RENDER + MAIN_WORLD if c[:4] == (bool(fp16), n, radius, bool(octree)) and (c[4] == spl or (c[4] == "own" and spl == OWN_SPL))]
    assert len(got) == 1, (n, fp16, octree, spl, radius, got)
    return got[0]


def main_lib(case, opt=2):
    key = (case, opt)
    if key not in _MAIN:
        L = C.CDLL(main_path(case, opt))
        L.refmain_build_info.argtypes = [C.c_void_p, C.c_void_p]
        L.refmain_create.restype = C.c_void_p
        L.refmain_create.argtypes = [C.c_int, C.c_int]
        L.refmain_destroy.argtypes = [C.c_void_p]
        L.refmain_spheres.argtypes = [C.c_void_p] * 4
        L.refmain_world_rng.argtypes = [C.c_void_p] * 2
        L.refmain_camera.argtypes = [C.c_void_p] * 2
        L.refmain_set_camera.argtypes = [C.c_void_p] * 2
        L.refmain_build_octree.argtypes = [C.c_void_p] * 2
        L.refmain_render_init.argtypes = [C.c_int] * 4 + [C.c_void_p]
        L.refmain_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.refmain_render_progressive.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.refmain_ppm.restype = C.c_int64
        L.refmain_ppm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64]
        info, radius = np.zeros(5, np.int32), np.zeros(1, np.float32)
        L.refmain_build_info(_p(info), _p(radius))
        fp16, n, r, octree, spl = case
        assert info.tolist() == [int(fp16), n, int(octree), OWN_SPL if spl == "own" else spl, 48] and radius[0] == np.float32(r), (case, info, radius)
        _MAIN[key] = L
    return _MAIN[key]


class RefMain:
    """rand_init + create_world of the reference's main.cu for an nx x ny frame, and its render kernels run pixel by pixel.
    Same method names and array shapes as OracleScene where both have the call."""

    def __init__(self, case, nx, ny, opt=2):
        self.L, self.case, self.nx, self.ny = main_lib(case, opt), case, nx, ny
        self.fp16, self.n, _, self.use_octree, _ = case
        self.h = C.c_void_p(self.L.refmain_create(nx, ny))
        self._info = None
        if self.use_octree:
            self.build_octree()

    def close(self):
        if self.h:
            self.L.refmain_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def spheres(self):
        geom, mat, kind = np.zeros((self.n, 4), np.float32), np.zeros((self.n, 4), np.float32), np.zeros(self.n, np.int32)
        self.L.refmain_spheres(self.h, _p(geom), _p(mat), _p(kind))
        return geom, mat, kind

    def world_rng(self):
        out = np.zeros(12, np.uint32)
        self.L.refmain_world_rng(self.h, _p(out))
        return out

    def camera(self):
        out = np.zeros(22, np.float32)
        self.L.refmain_camera(self.h, _p(out))
        return out

    def set_camera(self, cam):
        cam = np.ascontiguousarray(cam, np.float32).ravel()
        assert cam.size == 22
        self.L.refmain_set_camera(self.h, _p(cam))
        return self

    def build_octree(self):
        """buildOctree on create_world's list: node_count, leaf_count, dropped_full, dropped_outside"""
        if self._info is None:
            out = np.zeros(4, np.int64)
            self.L.refmain_build_octree(self.h, _p(out))
            self._info = dict(zip(("node_count", "leaf_count", "dropped_full", "dropped_outside"), out.tolist()))
        return dict(self._info)

    def render_init(self, row0=0, rows=None):
        rows = self.ny if rows is None else rows
        st = np.zeros((rows * self.nx, 12), np.uint32)
        self.L.refmain_render_init(self.nx, self.ny, row0, rows, _p(st))
        return st

    def render(self, ns, states=None, row0=0, rows=None):
        """(frame rows x nx x 3, states after, ghost rows x nx); states None: render_init's.  ghost: the pixels where the reference
        reached a slot that create_world left unwritten and has no result (ref_main_capi.cpp): they take no part in a comparison"""
        rows = self.ny if rows is None else rows
        states = self.render_init(row0, rows) if states is None else np.array(states, np.uint32).reshape(rows * self.nx, 12)
        fb, ghost = np.zeros((rows, self.nx, 3), np.float32), np.zeros((rows, self.nx), np.uint8)
        self.L.refmain_render(self.h, _p(fb), ns, row0, rows, _p(states), _p(ghost))
        return fb, states, ghost.astype(bool)

    def render_progressive(self, fb, current_sample, states, ghost):
        """one pass over the whole frame: fb (ny x nx x 3 float32), states and ghost (ny x nx uint8, as render's) are advanced in place"""
        assert fb.dtype == np.float32 and fb.shape == (self.ny, self.nx, 3) and fb.flags.c_contiguous
        assert states.dtype == np.uint32 and states.shape == (self.ny * self.nx, 12) and states.flags.c_contiguous
        assert ghost.dtype == np.uint8 and ghost.shape == (self.ny, self.nx) and ghost.flags.c_contiguous
        self.L.refmain_render_progressive(self.h, _p(fb), current_sample, 0, self.ny, _p(states), _p(ghost))
        return fb


def main_ppm(fb, fp16=False):
    """output_to_stream of the reference on an ny x nx x 3 frame, as bytes (any built main library of that precision serves)"""
    fb = np.ascontiguousarray(fb, np.float32)
    ny, nx = fb.shape[:2]
    L = main_lib(main_case(22, fp16))
    n = L.refmain_ppm(_p(fb), nx, ny, None, 0)
    buf = C.create_string_buffer(n)
    L.refmain_ppm(_p(fb), nx, ny, buf, n)
    return buf.raw[:n]
