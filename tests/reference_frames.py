"""The frame cases that hold the restated loops of main.cu (the oracle's create_world, render_init, render, render_progressive, color)
to the reference's own text, written once: tests/test_reference_main_host.py runs them live against the main libraries of
`make -C oracle ref`, golden/make_reference_golden.py records them into golden/reference_frames.npz, and
tests/test_reference_fixtures_host.py (the oracle) and tests/test_gpu_reference_frames.py (the kernels) are held to that file.

A case is create_world at N spheres of radius 0.1 for an nx x ny frame, rendered through the tree (SPHERES_PER_LEAF spl) or the
list: `render` at ns samples from render_init's states, whole or the listed rows of it, or `passes` render_progressive passes.
Binary16 cases are rendered with the oracle's camera written into the reference's (camera.h:27-35 has a host and a device branch)."""
import collections
import hashlib

import numpy as np

Case = collections.namedtuple("Case", "name n nx ny ns spl octree fp16 rows passes")


def _c(name, n, nx, ny, ns, spl, octree, fp16=False, rows=None, passes=0):
    return Case(name, n, nx, ny, ns, spl, octree, fp16, rows, passes)


CASES = [
    _c("n22_tree", 22, 64, 36, 4, 30, True), _c("n22_list", 22, 64, 36, 4, 30, False),
    _c("n500_tree", 500, 61, 35, 3, 30, True), _c("n500_list", 500, 61, 35, 3, 30, False),
    _c("n5_tree", 5, 40, 24, 16, 30, True), _c("n5_list", 5, 40, 24, 16, 30, False),                     # four large spheres: deep paths
    _c("n10000_tree", 10000, 48, 32, 2, 32, True),
    _c("n2000_spl3_tree", 2000, 40, 30, 4, 3, True),                                                     # 834 insertions dropped: full buckets
    _c("n22_tree_fp16", 22, 64, 36, 4, 30, True, fp16=True), _c("n22_list_fp16", 22, 64, 36, 4, 30, False, fp16=True),
    _c("n500_tree_fp16", 500, 61, 35, 3, 30, True, fp16=True), _c("n500_list_fp16", 500, 61, 35, 3, 30, False, fp16=True),
    _c("shipped_n8000", 8000, 1200, 800, 10, 30, True, rows=(0, 400, 799)),                               # main.cu with no line changed
    _c("n1000_tree", 1000, 1200, 800, 10, 30, True, rows=(449, 450, 451)),                               # list and tree disagree in pixel (671, 450)
    _c("n1000_list", 1000, 1200, 800, 10, 30, False, rows=(449, 450, 451)),
    _c("n500_tree_progressive", 500, 61, 35, 1, 30, True, passes=3),
]
BY_NAME = {c.name: c for c in CASES}
RENDER = [c for c in CASES if not c.passes]
PROGRESSIVE = [c for c in CASES if c.passes]
PROGRESSIVE_START = 3.0              # what the sum buffer holds before pass 1, which must assign and not add


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def rows_of(case):
    return list(range(case.ny)) if case.rows is None else list(case.rows)


def list_digest(geom, mat, kind):
    return sha(np.asarray(geom, np.float32), np.asarray(mat, np.float32), np.asarray(kind, np.int32))


def list_digest_of_world(W):
    """the same digest from an rt.World's host list (sphere_dtype records)"""
    sp = W.spheres
    return list_digest(np.concatenate([sp["center"], sp["radius"][:, None]], 1), np.concatenate([sp["albedo"], sp["param"][:, None]], 1), sp["material"])


def state_digest(states, ghost=None):
    """SHA-256 of the six state words of every pixel, in pixel order; a ghost pixel (no result in the reference) counts as six zeros"""
    st = np.array(np.asarray(states).reshape(-1, 12)[:, :6], np.uint32)
    if ghost is not None:
        st[np.asarray(ghost, bool).ravel()] = 0
    return sha(st)


def params_of(case):
    return np.array([case.n, case.nx, case.ny, case.ns, case.spl, int(case.octree), int(case.fp16), case.passes] + list(case.rows or ()), np.int64)


def oracle_scene(case):
    from oracle_lib import OracleScene
    return OracleScene(case.n, case.nx, case.ny, fp16=case.fp16, use_octree=case.octree, spl=case.spl)


def reference_scene(case, opt=2, own_camera=False):
    """the reference's create_world (+ buildOctree); in binary16 the oracle's camera is written into it unless own_camera"""
    import ref_lib
    R = ref_lib.RefMain(ref_lib.main_case(case.n, case.fp16, case.octree, case.spl), case.nx, case.ny, opt)
    if case.fp16 and not own_camera:
        R.set_camera(oracle_scene(case).camera())
    return R


def run(side, case):
    """the case on an OracleScene or a RefMain: dict(frame, states, ghost).  render: frame [rows, nx, 3], states [rows * nx, 12];
    progressive: frame [passes, ny, nx, 3] (the sum after each pass), states after the last pass.  ghost [rows, nx] bool."""
    is_ref = hasattr(side, "set_camera")
    if case.passes:
        fb = np.full((case.ny, case.nx, 3), PROGRESSIVE_START, np.float32)
        st, ghost, sums = side.render_init(), np.zeros((case.ny, case.nx), np.uint8), []
        for k in range(1, case.passes + 1):
            if is_ref:
                side.render_progressive(fb, k, st, ghost)
            else:
                side.render_progressive(fb, k, st, nthreads=8)
            sums.append(fb.copy())
        return dict(frame=np.stack(sums), states=st, ghost=ghost.astype(bool))
    frames, states, ghosts = [], [], []
    for row0, rows in ([(0, case.ny)] if case.rows is None else [(r, 1) for r in case.rows]):
        out = side.render(case.ns, row0=row0, rows=rows) if is_ref else side.render(case.ns, row0=row0, rows=rows, nthreads=8)
        frames.append(out[0]); states.append(out[1]); ghosts.append(out[2] if is_ref else np.zeros(out[0].shape[:2], bool))
    return dict(frame=np.concatenate(frames), states=np.concatenate(states), ghost=np.concatenate(ghosts))


def oracle_content(case):
    """a check on a case's inputs: (camera rays, calls of material::scatter by kind) of the oracle's walk through it"""
    S = oracle_scene(case)
    tot = collections.Counter()
    for r in ([None] if case.rows is None else case.rows):
        tot.update(S.count_scatters(case.ns * max(case.passes, 1), *(() if r is None else (r, 1))))
    return len(rows_of(case)) * case.nx * case.ns * max(case.passes, 1), dict(tot)
