"""GPU tests of rt_sequence (-m gpu): every frame the program writes equals, byte for byte, the frame of the same loop replayed through
the existing wrappers of rt_amd.py (tests/sequence_model.py: the same calls in the same order with the same parameters, the geometry
and the camera from the numpy model of the motion rule).  N = 500, SPHERES_PER_LEAF 30, 64x40 (and 67x41 for edge tiles), 4..8 samples
a pixel.  Each case is one run of the program, and then the replay; a run that does not exit with 0 fails the test there."""
import os
import subprocess

import pytest

import sequence_model as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dd2360-raytracing_amd", "rt_sequence")
SHAPE = dict(n=500, spl=30, nx=64, ny=40, min_spp=4, max_spp=8, batch=4)
CASE1 = dict(SHAPE, frames=4, move_every=3, cam_dx=0.05, cam_dz=-0.03, budget=2, rounds=2, tol=0.2, levels=1)


def run_program(tmp_path, **keys):
    assert os.access(EXE, os.X_OK), "rt_sequence is missing: __graft_entry__.build() builds it (make all)"
    p = subprocess.run([EXE] + sm.args(**keys), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    return p


def written(tmp_path):
    return {name: open(os.path.join(tmp_path, name), "rb").read() for name in sorted(os.listdir(tmp_path))}


def assert_frames(tmp_path, want, prefix="frame_"):
    got = written(tmp_path)
    assert sorted(got) == ["%s%04d.ppm" % (prefix, k) for k in sorted(want)]
    for k in sorted(want):
        assert got["%s%04d.ppm" % (prefix, k)] == want[k], k


def test_moving_spheres_moving_camera_budget_and_filter(rt, cuda, tmp_path):
    """case 1.  The precondition is asserted on the replay alone: in the last frame at least a tenth of the non-empty pixels hold more
    effective samples than the frame itself took — the history is in use, so a swapped ping-pong buffer cannot go unseen.
    Measured on an MI355X at 64x40 with tol=0.2: 0.815 of 1803 non-empty pixels."""
    p = run_program(tmp_path, **CASE1)
    frames, hist, spp = sm.replay_animation(rt, cuda, **CASE1)
    neff = hist[4 * 64 * 40:]
    filled = neff > 0
    share = float((neff[filled] > spp[filled]).mean())
    print("share of non-empty pixels with neff above the frame's own samples: %.3f (%d non-empty)" % (share, int(filled.sum())))
    assert filled.sum() > 0 and share >= 0.1, share
    assert_frames(tmp_path, dict(enumerate(frames)))
    assert len(set(frames)) == 4
    assert [l for l in p.stderr.splitlines() if "mean samples per pixel" in l][-1].startswith("frame 3: ")


def test_edge_tiles_unrectified_unfiltered(rt, cuda, tmp_path):
    """case 2: 67x41 (edge tiles in both directions), gamma=0 (the unrectified rule), no budget, levels=0 (the frame shown is fb)"""
    keys = dict(CASE1, nx=67, ny=41, gamma=0, budget=0, levels=0)
    run_program(tmp_path, **keys)
    frames, _, _ = sm.replay_animation(rt, cuda, **keys)
    assert_frames(tmp_path, dict(enumerate(frames)))


def test_static_scene_still_camera(rt, cuda, tmp_path):
    """case 3: nothing moves, the tree is kept; frame 2 differs from frame 0, so the history and the continuing RNG states are in use"""
    keys = dict(SHAPE, frames=3)
    run_program(tmp_path, **keys)
    frames, _, _ = sm.replay_animation(rt, cuda, **keys)
    assert_frames(tmp_path, dict(enumerate(frames)))
    assert frames[2] != frames[0]


@pytest.mark.parametrize("levels", [2, 0])
def test_progressive_passes(rt, cuda, tmp_path, levels):
    """the reference viewer's loop: passes 2, 4 and 6 are shown — rt_render_progressive, rt_denoise (SUM) and rt_frame_levels, or with
    levels=0 rt_frame_levels of fb in SUM mode"""
    keys = dict(n=500, spl=30, nx=64, ny=40, passes=6, every=2, levels=levels)
    run_program(tmp_path, mode="progressive", **keys)
    shown = sm.replay_progressive(rt, cuda, **keys)
    assert sorted(shown) == [2, 4, 6]
    assert_frames(tmp_path, shown, "pass_")
    assert len(set(shown.values())) == 3


def test_timing_table(rt, cuda, tmp_path):
    """timing=1 out=none: no file, one line a stage and the wall-time line"""
    p = run_program(tmp_path, **dict(SHAPE, frames=3, move_every=3, budget=1, timing=1, out="none"))
    assert os.listdir(tmp_path) == []
    lines = [l for l in p.stderr.splitlines() if l.startswith("timing: ")]
    for stage in ("animate + setters", "tree rebuild", "guides", "begin", "spend", "accumulate", "filter", "levels + copy", "wall per frame"):
        mine = [l for l in lines if l.startswith("timing: " + stage + " ")]
        assert len(mine) == 1 and " mean " in mine[0] and " max " in mine[0], (stage, p.stderr)
        assert float(mine[0].split(" mean ")[1].split()[0]) >= 0
