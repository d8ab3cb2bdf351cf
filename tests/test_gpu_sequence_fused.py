"""rt_sequence adaptive=rounds | fused (-m gpu): the two runs of the program write the same frame files, byte for byte.  The arguments
are those of case 1 of tests/test_gpu_sequence.py (N = 500, SPHERES_PER_LEAF 30, 64x40, 4..8 samples, moving spheres and camera, a
budget, one filter level) with rel_error = 0.1, so that the stop rule decides something."""
import os
import subprocess

import pytest

import sequence_model as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dd2360-raytracing_amd", "rt_sequence")
CASE = dict(n=500, spl=30, nx=64, ny=40, min_spp=4, max_spp=8, batch=4, rel_error=0.1, frames=4, move_every=3, cam_dx=0.05, cam_dz=-0.03,
            budget=2, rounds=2, tol=0.2, levels=1)


def run_program(where, **keys):
    assert os.access(EXE, os.X_OK), "rt_sequence is missing: __graft_entry__.build() builds it (make all)"
    os.makedirs(where)
    p = subprocess.run([EXE] + sm.args(**keys), cwd=where, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    return {name: open(os.path.join(where, name), "rb").read() for name in sorted(os.listdir(where))}, p.stderr


def test_fused_writes_the_frames_of_the_rounds(rt, cuda, tmp_path):
    rounds, err_r = run_program(tmp_path / "rounds", adaptive="rounds", **CASE)
    fused, err_f = run_program(tmp_path / "fused", adaptive="fused", **CASE)
    default, _ = run_program(tmp_path / "default", **CASE)
    assert sorted(rounds) == ["frame_%04d.ppm" % k for k in range(4)]
    assert fused == rounds and default == rounds
    assert len(set(rounds.values())) == 4
    # the stop rule decided something: with some pixels at min_spp and some at max_spp, a frame's mean count lies strictly between
    # min_spp + budget and max_spp + budget (the spend adds `budget` samples a pixel on average) — and both runs print the same means
    means = [l for l in err_r.splitlines() if "mean samples per pixel" in l]
    assert len(means) == 4 and means == [l for l in err_f.splitlines() if "mean samples per pixel" in l]
    for l in means:
        v = float(l.split("mean samples per pixel:")[1].split()[0])
        print(l)
        assert 4 + 2 < v < 8 + 2, l
