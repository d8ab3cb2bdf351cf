"""rt_sequence (dd2360-raytracing_amd/host/sequence.cpp) without a GPU: the program is built, it refuses bad arguments before it
touches a device, and its motion rule (host/rt_sequence_motion.hpp), evaluated by a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/host/sequence_motion_check.cpp), gives the bits of the numpy model (tests/sequence_model.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import sequence_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dd2360-raytracing_amd")
EXE = os.path.join(PKG, "rt_sequence")
SAN = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
       "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
F = np.float32


def test_the_program_is_built(rt):
    assert os.path.isfile(EXE) and os.access(EXE, os.X_OK), "rt_sequence is missing: __graft_entry__.build() builds it (make all)"


REFUSED = [(["colour=1"], "colour"), (["frames=0"], "frames"), (["min_spp=4", "max_spp=9", "batch=4"], "batch"),
           (["budget=1", "rounds=0"], "rounds"), (["gamma=-1"], "gamma"), (["rect_radius=3"], "rect_radius"),
           (["mode=progressive", "passes=0"], "passes"), (["mode=foo"], "mode"), (["nx=4x"], "nx"), (["frames"], "frames"),
           (["fp16=1"], "fp16")]


@pytest.mark.parametrize("tokens,key", REFUSED, ids=[" ".join(t) for t, _ in REFUSED])
def test_bad_arguments_are_refused_before_any_device_work(rt, tmp_path, tokens, key):
    """exit code 99 and a message that names the key; rt_device_check has not run (its own failure would name it, and the first
    line the program prints once the arguments are accepted is absent)"""
    p = subprocess.run([EXE] + tokens, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert p.returncode == 99, (p.returncode, p.stderr)
    assert re.match(r"rt_sequence: %s: " % re.escape(key), p.stderr), p.stderr
    assert "rt_device_check" not in p.stderr and "spheres of radius" not in p.stderr and len(p.stderr.splitlines()) == 1
    assert os.listdir(tmp_path) == []


def run_motion_check(tmp_path):
    exe = str(tmp_path / "sequence_motion_check")
    p = subprocess.run(["g++"] + SAN + ["-I", os.path.join(PKG, "host"), "-o", exe, os.path.join(ROOT, "tests", "host", "sequence_motion_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    assert "sequence_motion_check: ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]
    return [line.split() for line in p.stdout.splitlines()]


def as_floats(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(F)


def test_the_motion_rule_matches_the_model_bit_for_bit(tmp_path):
    lines = run_motion_check(tmp_path)
    move_step, cam_dx, cam_dz = as_floats(next(l for l in lines if l[0] == "step")[1:])
    slots = [l for l in lines if l[0] == "in"]
    material = np.array([int(l[2]) for l in slots])
    base = np.stack([as_floats(l[3:]) for l in slots])
    n = len(slots)
    # the list holds what the rule has to survive
    assert (material == -1).any() and (base[:, 3] == 1).any() and (base[:, 3] == 1000).any() and np.isnan(base[:, :3]).any()
    assert ((base[:, :3] == 0) & np.signbit(base[:, :3])).any()
    dirs = {}
    for me in (1, 3, 0):
        got = np.array([int(l[3]) for l in lines if l[0] == "dir" and int(l[1]) == me])
        want = sm.mask(material, base[:, 3], me)
        assert len(got) == n and np.array_equal(got, want), me
        dirs[me] = want
    assert (dirs[0] == -1).all() and set(dirs[1]) == {-1, 0, 1, 2, 3} and set(dirs[3]) == {-1, 0, 1, 2, 3}
    assert (dirs[1][(material == -1) | (base[:, 3] >= 0.5)] == -1).all()       # ghosts, the ground, the unit sphere: never
    for me in (1, 3, 0):
        for f in (0, 1, 3, 1000):
            got = np.stack([as_floats(l[4:]) for l in lines if l[0] == "geom" and int(l[1]) == me and int(l[2]) == f])
            want = sm.geometry(base, dirs[me], f, move_step)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (me, f)
            still = dirs[me] == -1
            assert np.array_equal(got[still].view(np.uint32), base[still].view(np.uint32))
            if f == 0:
                assert np.array_equal(got.view(np.uint32), base.view(np.uint32))            # frame 0 sets nothing: -0 stays -0
            elif me:
                assert not np.array_equal(got.view(np.uint32), base.view(np.uint32))
    for f in (0, 1, 3, 1000):
        got = as_floats(next(l for l in lines if l[0] == "lookfrom" and int(l[1]) == f)[2:])
        assert np.array_equal(got.view(np.uint32), sm.lookfrom(f, cam_dx, cam_dz).view(np.uint32)), f


def test_frame_0_stands_where_create_world_stands(rt):
    """the camera of frame f is rt_camera_init at lookfrom(f) with create_world's other arguments: at f = 0 that is the created
    camera, bit for bit, at the sizes the GPU tests use"""
    for nx, ny in ((64, 40), (67, 41), (1200, 800)):
        W = rt.World(22, nx, ny)
        try:
            assert np.array_equal(sm.camera(rt, 0, nx, ny, 0.05, -0.03).view(np.uint8), W.camera.view(np.uint8)), (nx, ny)
            assert not np.array_equal(sm.camera(rt, 1, nx, ny, 0.05, -0.03).view(np.uint8), W.camera.view(np.uint8))
        finally:
            W.close()


def test_the_header_includes_nothing_of_the_library():
    src = open(os.path.join(PKG, "host", "rt_sequence_motion.hpp")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", src) == []
    make = open(os.path.join(PKG, "Makefile")).read()
    assert re.search(r"^all:.*\brt_sequence\b", make, re.M) and re.search(r"^\trm -rf .*\brt_sequence\b", make, re.M)
    assert "rt_sequence" in open(os.path.join(ROOT, ".gitignore")).read().split()
