"""rt_sequence tree=rebuild (-m gpu): frame 0 builds the tree, every later frame calls rt_octree_rebuild_gpu on the same handle, and the
frames the program writes are byte for byte those of tree=build (which tests/test_gpu_sequence.py holds to the replay through the
binding).  Each run is a child process under its own time limit."""
import os
import subprocess

import pytest

import sequence_model as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dd2360-raytracing_amd", "rt_sequence")
KEYS = dict(n=500, nx=64, ny=40, frames=4, move_every=7, cam_dx=0.01)


def run(tmp_path, **keys):
    assert os.access(EXE, os.X_OK), "rt_sequence is missing: __graft_entry__.build() builds it (make all)"
    return subprocess.run([EXE] + sm.args(**keys), cwd=tmp_path, capture_output=True, text=True, timeout=120)


def test_rebuilt_trees_give_the_frames_of_built_trees(rt, cuda, tmp_path):
    for prefix, extra in (("a_", {}), ("b_", dict(tree="rebuild"))):
        p = run(tmp_path, out=str(tmp_path / prefix), **dict(KEYS, **extra))
        assert p.returncode == 0, (prefix, p.returncode, p.stderr[-3000:])
    names = sorted(os.listdir(tmp_path))
    assert names == ["%s%04d.ppm" % (prefix, f) for prefix in ("a_", "b_") for f in range(4)]
    frames = {name: open(tmp_path / name, "rb").read() for name in names}
    for f in range(4):
        assert frames["a_%04d.ppm" % f] == frames["b_%04d.ppm" % f], f
    assert len({frames["a_%04d.ppm" % f] for f in range(4)}) == 4            # the animation moves: four different frames


def test_an_unknown_tree_value_is_refused_before_the_device_is_touched(rt, cuda, tmp_path):
    p = run(tmp_path, tree="bogus", **KEYS)
    assert p.returncode == 99, (p.returncode, p.stderr)
    assert p.stderr.startswith("rt_sequence: tree: ") and len(p.stderr.splitlines()) == 1 and "spheres of radius" not in p.stderr
    assert os.listdir(tmp_path) == []
