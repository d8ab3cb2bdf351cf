"""rt_sequence's key `upscale` without a GPU: the rule (dd2360-raytracing_amd/host/rt_sequence_upscale.hpp), evaluated by a stand-alone
program under AddressSanitizer + UndefinedBehaviorSanitizer (tests/host/upscale_rule_check.cpp) on crafted 5x3 and 1x1 frames for
s = 2, 3 and 4, gives the bits of the numpy model (tests/upscale_model.py), and the crafted frames reach every branch of the rule; the
program refuses a bad `upscale` before it touches a device; the header includes nothing."""
import os
import re
import subprocess

import numpy as np
import pytest

import upscale_model as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dd2360-raytracing_amd")
EXE = os.path.join(PKG, "rt_sequence")
HEADER = os.path.join(PKG, "host", "rt_sequence_upscale.hpp")
# the flags of tests/test_sequence_host.py
SAN = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
       "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
F = np.float32


def as_floats(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(F)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """{(nx, ny, s): (c, sphere, sphere_high, got frame, got taps)} from one run of the check program"""
    exe = str(tmp_path_factory.mktemp("upscale") / "upscale_rule_check")
    p = subprocess.run(["g++"] + SAN + ["-I", os.path.join(PKG, "host"), "-o", exe, os.path.join(ROOT, "tests", "host", "upscale_rule_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    assert "upscale_rule_check: ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]
    out, key = {}, None
    for l in (line.split() for line in p.stdout.splitlines()):
        if l[0] == "case":
            nx, ny, s = key = tuple(int(w) for w in l[1:])
            out[key] = (np.zeros((ny, nx, 3), F), np.zeros((ny, nx), np.int32), np.zeros((s * ny, s * nx), np.int32),
                        np.zeros((s * ny, s * nx, 3), F), np.full((s * ny, s * nx), -1))
        elif l[0] == "low":
            c, sphere = out[key][:2]
            c[int(l[2]), int(l[1])], sphere[int(l[2]), int(l[1])] = as_floats(l[4:]), int(l[3])
        elif l[0] == "high":
            _, _, high, frame, taps = out[key]
            I, J = int(l[1]), int(l[2])
            high[J, I], taps[J, I], frame[J, I] = int(l[3]), int(l[4]), as_floats(l[5:])
    assert sorted(out) == sorted((nx, ny, s) for nx, ny in ((5, 3), (1, 1)) for s in (2, 3, 4))
    return out


def test_the_rule_matches_the_model_bit_for_bit(cases):
    for key, (c, sphere, high, got, got_taps) in cases.items():
        want, taps = um.upscale(c, sphere, high, key[2])
        assert np.array_equal(got_taps, taps), key
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), key


def test_the_crafted_frames_reach_every_branch(cases):
    """counted on the model alone (the test above holds the program to it)"""
    for (nx, ny, s), (c, sphere, high, _, _) in cases.items():
        frame, taps, sw = um.upscale(c, sphere, high, s, weights=True)
        i0, _ = um.axis(s * nx, s)
        j0, _ = um.axis(s * ny, s)
        assert i0.min() == -1 and i0.max() == nx - 1 and j0.min() == -1 and j0.max() == ny - 1        # taps off every border
        assert (taps == 0).any()                                                                      # the fallback
        copied = c[(np.arange(s * ny) // s)[:, None], (np.arange(s * nx) // s)[None, :]]
        fell = ~(sw > 0)
        assert np.array_equal(frame[fell].view(np.uint32), copied[fell].view(np.uint32))              # ... copies: the bits
        assert ((copied[fell] == 0) & np.signbit(copied[fell])).any()                                 # ... -0 among them
        if (nx, ny) == (1, 1):
            assert taps.max() == 1
            continue
        assert (taps == 4).any() and ((taps >= 1) & (taps <= 3)).any()
        assert ((taps > 0) & (sw == 0)).any() == (s == 3)                                             # only zero-weight taps accepted
        sky = (high == -1) & (taps > 0)
        assert sky.any() and (sphere == -1).any()                                                     # sky against sky
        assert np.isnan(c).any() and np.isposinf(c).any() and ((c == 0) & np.signbit(c)).any()
        assert (fell & np.isnan(frame).any(axis=2) & np.isnan(copied).any(axis=2)).any()              # a fallback onto a NaN pixel
        assert np.isposinf(frame).any()                                                               # nothing is clamped
        # a skipped tap adds nothing: where NaN and +inf pixels are the only neighbours left out, the result is finite
        assert np.isfinite(frame[(taps >= 1) & (taps <= 3) & (sw > 0)]).any()


def test_where_a_high_pixel_lies():
    """the issue's statements about the axis, in numpy float32, for s = 2, 3, 4 and widths 1..1200"""
    for s in (2, 3, 4):
        for nx in (1, 2, 3, 5, 21, 33, 64, 600, 1199, 1200):
            i0, ax = um.axis(s * nx, s)
            own = np.arange(s * nx) // s
            assert i0.min() == -1 and i0.max() == nx - 1 and (ax >= 0).all() and (ax < 1).all()
            assert ((own == i0) | (own == i0 + 1)).all()
            assert not (ax == F(0.5)).any()
            heavier = np.where(ax > F(0.5), i0 + 1, i0)
            assert (heavier == own).all()
            assert (ax == 0).any() == (s == 3)
            if s == 3:
                assert (ax[1::3] == 0).all()


REFUSED = [["upscale=0"], ["upscale=5"], ["upscale=2x"], ["nx=1073741824", "upscale=4"], ["nx=32768", "ny=32768", "upscale=2"],
           ["mode=progressive", "levels=0", "upscale=2"]]


@pytest.mark.parametrize("tokens", REFUSED, ids=[" ".join(t) for t in REFUSED])
def test_a_bad_upscale_is_refused_before_any_device_work(rt, tmp_path, tokens):
    """exit code 99 and one line that names the key; rt_device_check has not run and no file is written"""
    p = subprocess.run([EXE] + tokens, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert p.returncode == 99, (p.returncode, p.stderr)
    assert p.stderr.startswith("rt_sequence: upscale: "), p.stderr
    assert "rt_device_check" not in p.stderr and "spheres of radius" not in p.stderr and len(p.stderr.splitlines()) == 1
    assert os.listdir(tmp_path) == []


def test_the_header_includes_nothing_and_is_a_prerequisite():
    src = open(HEADER).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", src) == []
    make = open(os.path.join(PKG, "Makefile")).read()
    assert re.search(r"^rt_sequence:.*\bhost/rt_sequence_upscale\.hpp\b", make, re.M)
    program = open(os.path.join(PKG, "host", "sequence.cpp")).read()
    assert '#include "rt_sequence_upscale.hpp"' in program and "rt_seq_upscale_pixel(" in program
