"""The oracle's restated loops of main.cu (rt_oracle.hpp: create_world, render_init, render, render_progressive, color, and
orc_ppm) against a CPU build of main.cu's OWN text above `int main(` (`make -C oracle ref`: oracle/ref_main_capi.cpp over a generated
copy in which only NUM_SPHERES, SPHERE_RADIUS and the presence of USE_OCTREE differ, one library per case).  Not marked gpu.

Every comparison is bit equality; a NaN compares as "NaN where the reference has NaN" (bitcmp.same_nan_as_ref).  The reference's
kernels are run one pixel per call (blockDim (1, 1, 1), blockIdx (i, j)).  The frame cases are those of tests/reference_frames.py.

Two things are not the reference's to give, and are handled as tests/test_reference_pins_host.py handles them:
  * camera::camera in USE_FP16 (camera.h:27-35 branches on __CUDA_ARCH__; the oracle follows the device branch): the fields that
    differ are pinned below, and binary16 frames are rendered with the oracle's 22 floats written into the reference's camera.
  * a pixel in which the reference reaches a slot that create_world left unwritten: color() (main.cu:59) calls through its null
    mat_ptr there.  The driver reports such pixels (ghost); they take no part in the comparison and are counted: none in binary32,
    under 1 % of a binary16 frame.

The live tests skip only where neither oracle/_ref/ nor the reference's sources exist (a clean checkout elsewhere: the fixtures of
tests/test_reference_fixtures_host.py stand in); sources without libraries are a failure."""
import os
import re

import numpy as np
import pytest

import oracle_lib
import ref_lib
import reference_frames as rf
from bitcmp import f32_bits, same_nan_as_ref


@pytest.fixture(scope="module", autouse=True)
def built():
    s = ref_lib.status()
    if s == "absent":
        pytest.skip("neither oracle/_ref/ nor the reference's sources are here")
    assert s == "ok", "the reference's sources are here but oracle/_ref/ is incomplete: run `make -C oracle ref` (__graft_entry__.build() does)"


_runs = {}


def both(case):
    """(the reference's run, the oracle's run) of a frame case, computed once per module"""
    if case.name not in _runs:
        _runs[case.name] = (rf.run(rf.reference_scene(case), case), rf.run(rf.oracle_scene(case), case))
    return _runs[case.name]


def test_the_makefile_builds_the_cases_listed_here():
    mk = open(os.path.join(oracle_lib.ORACLE_DIR, "Makefile")).read()

    def listed(var):
        words = re.search(r"^%s = ((?:.*\\\n)*.*)$" % var, mk, re.M).group(1).replace("\\\n", " ").split()
        return [(p == "fp16", int(n), r, o == "1", s if s == "own" else int(s)) for p, n, r, o, s in (w.split(":") for w in words)]

    assert listed("MAIN_RENDER") == list(ref_lib.MAIN_RENDER) and listed("MAIN_WORLD") == list(ref_lib.MAIN_WORLD)
    for c in rf.CASES:
        assert ref_lib.main_case(c.n, c.fp16, c.octree, c.spl) in ref_lib.MAIN_RENDER, c.name


# ---------------------------------------------------------------------------------------------------- create_world
# the floats of camera.h:51-56 that camera::camera computes from half_height: lower_left_corner 3-5, horizontal 6-8, vertical 9-11
FROM_HALF_HEIGHT = set(range(3, 12))
# binary16, host branch (tan) against device branch (hsin / hcos): the floats that differ, per frame shape.  vertical always does;
# whether a lower_left_corner or horizontal component does depends on how aspect * half_height rounds.
FP16_CAMERA_DIFFERS = {(1200, 800): [4, 9, 10, 11], (64, 36): [3, 4, 5, 6, 8, 9, 10, 11], (61, 35): [4, 5, 6, 8, 9, 10, 11], (16, 8): [4, 6, 9, 10, 11]}


@pytest.mark.parametrize("fp16", [False, True])
@pytest.mark.parametrize("n,radius", [(5, "0.1"), (22, "0.1"), (500, "0.1"), (8000, "0.1"), (10000, "0.1"), (500, "0.2")])
def test_create_world(n, radius, fp16):
    """the list (every slot: centre, radius, material kind, albedo, fuzz / index), the RNG state afterwards and the camera"""
    nx, ny = 1200, 800
    case = ref_lib.main_case(n, fp16, True, {8000: 30, 10000: 32}.get(n, 30), radius)
    R = ref_lib.RefMain(case, nx, ny)
    S = oracle_lib.OracleScene(n, nx, ny, radius=float(radius), fp16=fp16)
    for a, b, what in zip(R.spheres(), S.spheres(), ("geom", "mat", "kind")):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what
    kind = R.spheres()[2]
    assert set(kind.tolist()) <= {-1, 0, 1, 2} and kind[:4].tolist() == [0, 2, 0, 1]
    assert n != 22 or (kind == -1).sum() == 2                    # (sqrt(18) truncates to 4: 4 + 16 slots written, two left as they were)
    assert np.array_equal(R.world_rng(), S.world_rng()) and R.world_rng()[:6].any() and not R.world_rng()[6:].any()
    differ = np.flatnonzero(f32_bits(R.camera()) != f32_bits(S.camera())).tolist()
    assert differ == (FP16_CAMERA_DIFFERS[nx, ny] if fp16 else [])


@pytest.mark.parametrize("nx,ny", sorted(FP16_CAMERA_DIFFERS))
def test_the_binary16_host_camera_differs_only_in_what_half_height_feeds(nx, ny):
    R = ref_lib.RefMain(ref_lib.main_case(22, True), nx, ny)
    a, b = R.camera(), oracle_lib.OracleScene(22, nx, ny, fp16=True).camera()
    differ = np.flatnonzero(f32_bits(a) != f32_bits(b)).tolist()
    assert differ == FP16_CAMERA_DIFFERS[nx, ny] and set(differ) <= FROM_HALF_HEIGHT and {9, 10, 11} <= set(differ)
    # origin, u, v, w and lens_radius do not depend on half_height: equal.  And the overwrite writes what it is given
    assert np.array_equal(f32_bits(R.set_camera(b).camera()), f32_bits(b))


# ---------------------------------------------------------------------------------------------------- render_init
@pytest.mark.parametrize("fp16", [False, True])
def test_render_init(fp16):
    nx, ny = 61, 35
    R = ref_lib.RefMain(ref_lib.main_case(500, fp16), nx, ny)
    st = R.render_init()
    assert st.shape == (nx * ny, 12) and np.array_equal(st, oracle_lib.OracleScene(500, nx, ny, fp16=fp16).render_init())
    assert not st[:, 6:].any() and len({tuple(r) for r in st[:, :6]}) == nx * ny
    assert np.array_equal(R.render_init(7, 3), st[7 * nx:10 * nx])


# ---------------------------------------------------------------------------------------------------- render
@pytest.mark.parametrize("case", rf.RENDER, ids=lambda c: c.name)
def test_render(case):
    """whole frames (the listed rows of the 1200 x 800 ones) and the RNG states afterwards"""
    ref, orc = both(case)
    g = ref["ghost"]
    assert ref["frame"].shape == (len(rf.rows_of(case)), case.nx, 3) and ref["states"].shape == (g.size, 12)
    assert g.sum() * 100 < g.size and (case.fp16 or not g.any())
    print("%s: %d pixels, %d ghost pixels, %d NaN pixels" % (case.name, g.size, g.sum(), np.isnan(ref["frame"]).any(-1).sum()))
    assert same_nan_as_ref(orc["frame"][~g], ref["frame"][~g])
    assert np.array_equal(orc["states"][~g.ravel()], ref["states"][~g.ravel()])
    assert (ref["states"] != rf.oracle_scene(case).render_init(rf.rows_of(case)[0], 1)[0]).any()


def test_the_reference_as_shipped_is_the_generated_copy_with_no_line_changed():
    src = os.path.join(ref_lib.source_dir(), "main.cu")
    if not os.path.exists(src):
        pytest.skip("the libraries are here, the reference's sources are not")
    head = open(src).read().split("\nint main(")[0] + "\n"
    assert open(os.path.join(ref_lib.REF_DIR, "gen", "main_n8000_r0.1_oct1", "main_body.inc")).read() == head
    assert ref_lib.main_case(8000)[4] == "own"


def test_list_and_tree_disagree_where_they_are_known_to():
    """N = 1000, 1200 x 800 x 10: pixel (671, 450) and no other of rows 449 to 451, in the reference's own two paths"""
    (t, _), (l, _) = both(rf.BY_NAME["n1000_tree"]), both(rf.BY_NAME["n1000_list"])
    differ = np.argwhere((f32_bits(t["frame"]) != f32_bits(l["frame"])).any(-1))
    assert differ.tolist() == [[1, 671]]


def test_binary16_frames_need_the_device_branch_camera():
    """the same case with the reference's own host-built camera gives another frame: the overwrite matters"""
    case = rf.BY_NAME["n500_tree_fp16"]
    own = rf.run(rf.reference_scene(case, own_camera=True), case)
    ref, _ = both(case)
    assert ((f32_bits(own["frame"]) != f32_bits(ref["frame"])).any(-1)).sum() > case.nx * case.ny // 20


# ---------------------------------------------------------------------------------------------------- render_progressive
@pytest.mark.parametrize("case", rf.PROGRESSIVE, ids=lambda c: c.name)
def test_render_progressive(case):
    """the sum buffer after each pass on continuing states; pass 1 assigns over what the buffer held"""
    ref, orc = both(case)
    assert ref["frame"].shape == (case.passes, case.ny, case.nx, 3) and not ref["ghost"].any()
    for k in range(case.passes):
        assert same_nan_as_ref(orc["frame"][k], ref["frame"][k]), "pass %d" % (k + 1)
    assert np.array_equal(orc["states"], ref["states"])
    assert (ref["frame"][0] <= 1.0).all() and (ref["frame"][1] != ref["frame"][0]).any()          # (a sample is at most 1: 3.0 was overwritten)
    # three passes draw what render(3) draws: the same states afterwards
    same = rf.BY_NAME["n500_tree"]
    assert (same.n, same.nx, same.ny, same.ns, same.spl) == (case.n, case.nx, case.ny, case.passes, case.spl)
    assert np.array_equal(ref["states"], both(same)[0]["states"])


# ---------------------------------------------------------------------------------------------------- output_to_stream
@pytest.mark.parametrize("name", ["n22_tree", "n500_tree_fp16"])
def test_output_to_stream(name):
    case = rf.BY_NAME[name]
    frame = both(case)[0]["frame"]
    assert not np.isnan(frame).any()
    got = ref_lib.main_ppm(frame, case.fp16)
    assert got == oracle_lib.ppm_bytes(frame) and got.startswith(b"P3\n%d %d\n255\n" % (case.nx, case.ny)) and got.count(b"\n") == 3 + case.nx * case.ny
