"""GPU tests of rt_sequence's key `upscale` (-m gpu): every frame the program writes at the shown size equals, byte for byte, the frame of
the same loop replayed through the existing wrappers of rt_amd.py (tests/sequence_model.py) with the upscaling done by the numpy model
(tests/upscale_model.py: its Recorder takes the shown low frame and the low guides at the moment each frame is quantised, traces
rt_render_guides at the shown size, applies the rule and quantises with rt_frame_levels at the shown size).  N = 500, SPHERES_PER_LEAF 30,
4..8 samples a pixel.  Each case is one run of the program, and then the replay.

The conditions that keep a case from passing vacuously are asserted on the replay's tap counts alone, in every compared frame: pixels
with all four taps accepted and pixels with one to three exist, and the frame differs from the low levels enlarged by pixel repetition.
The count of pixels that accept nothing (the fallback; tests/test_upscale_host.py reaches that branch for certain) is printed."""
import os
import subprocess

import pytest

import sequence_model as sm
import upscale_model as um

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dd2360-raytracing_amd", "rt_sequence")
SHAPE = dict(n=500, spl=30, min_spp=4, max_spp=8, batch=4)
MOTION = dict(move_every=3, cam_dx=0.05, cam_dz=-0.03, tol=0.2)


def run_program(tmp_path, **keys):
    assert os.access(EXE, os.X_OK), "rt_sequence is missing: __graft_entry__.build() builds it (make all)"
    p = subprocess.run([EXE] + sm.args(**keys), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    return p


def assert_shown(tmp_path, rec, low, names, nx, ny):
    """the files are the recorder's frames; each frame is a real reconstruction"""
    s = rec.s
    assert sorted(os.listdir(tmp_path)) == names and len(rec.shown) == len(names) == len(low)
    for name, want, taps, small in zip(names, rec.shown, rec.taps, low):
        four, some, none = int((taps == 4).sum()), int(((taps >= 1) & (taps <= 3)).sum()), int((taps == 0).sum())
        print("%s: %d pixels accept four taps, %d one to three, %d none (fallback)" % (name, four, some, none))
        assert taps.shape == (s * ny, s * nx) and four > 0 and some > 0
        assert want.startswith(b"P6\n%d %d\n255\n" % (s * nx, s * ny)) and want != um.nearest(small, nx, ny, s)
        assert open(os.path.join(tmp_path, name), "rb").read() == want, name


def test_moving_scene_budget_and_filter_twofold(rt, cuda, tmp_path):
    """case (a): 33x21 shown at 66x42, the motion, budget and filter of test_gpu_sequence's case 1, 3 frames.
    Measured on an MI355X, pixels of 2772 that accept four taps / one to three / none:
    frame 0: 1573 / 1066 / 133, frame 1: 1574 / 1063 / 135, frame 2: 1541 / 1104 / 127."""
    keys = dict(SHAPE, **MOTION, nx=33, ny=21, frames=3, budget=2, rounds=2, levels=1)
    p = run_program(tmp_path, upscale=2, **keys)
    rec = um.Recorder(rt, cuda, 2)
    low, _, _ = sm.replay_animation(rec, cuda, **keys)
    assert_shown(tmp_path, rec, low, ["frame_%04d.ppm" % f for f in range(3)], 33, 21)
    assert len(set(rec.shown)) == 3
    said = [l for l in p.stderr.splitlines() if "mean samples per pixel" in l]
    assert len(said) == 3 and all("per low pixel, 33x21" in l for l in said)


def test_unrectified_unfiltered_threefold(rt, cuda, tmp_path):
    """case (b): 22x14 shown at 66x42, gamma=0 and levels=0 (the frame that is upscaled is fb itself), 2 frames; s = 3 has columns and
    rows of weight exactly 0.
    Measured on an MI355X, pixels of 2772 that accept four taps / one to three / none: frame 0: 1170 / 1405 / 197, frame 1: 1170 / 1408 / 194."""
    keys = dict(SHAPE, **MOTION, nx=22, ny=14, frames=2, gamma=0, levels=0)
    run_program(tmp_path, upscale=3, **keys)
    rec = um.Recorder(rt, cuda, 3)
    low, _, _ = sm.replay_animation(rec, cuda, **keys)
    assert_shown(tmp_path, rec, low, ["frame_%04d.ppm" % f for f in range(2)], 22, 14)


def test_upscale_1_is_the_program_without_the_key(rt, cuda, tmp_path):
    """the same files and the same report, timing table's stage names included (no `upscale` line)"""
    keys = dict(SHAPE, **MOTION, nx=33, ny=21, frames=2, budget=1)
    runs = []
    for name, extra in (("with", dict(upscale=1)), ("without", {})):
        d = tmp_path / name
        d.mkdir()
        p = run_program(d, **keys, **extra)
        runs.append(({f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}, p.stderr))
    assert runs[0][0] == runs[1][0] and sorted(runs[0][0]) == ["frame_0000.ppm", "frame_0001.ppm"]
    assert runs[0][1] == runs[1][1] and "upscale" not in runs[0][1] and "low pixel" not in runs[0][1]
    p = run_program(tmp_path, **dict(keys, upscale=1, timing=1, out="none"))
    assert not [l for l in p.stderr.splitlines() if l.startswith("timing: upscale")]
    p = run_program(tmp_path, **dict(keys, upscale=2, timing=1, out="none"))
    lines = [l for l in p.stderr.splitlines() if l.startswith("timing: ")]
    assert len([l for l in lines if l.startswith("timing: upscale ")]) == 1 and len([l for l in lines if l.startswith("timing: guides ")]) == 1


def test_progressive_fourfold(rt, cuda, tmp_path):
    """case (c): the progressive viewer, 33x21 shown at 132x84, passes 2 and 4 shown; the high guides are traced once.
    Measured on an MI355X, pixels of 11088 that accept four taps / one to three / none: both passes 6324 / 4264 / 500."""
    keys = dict(n=500, spl=30, nx=33, ny=21, passes=4, every=2)
    run_program(tmp_path, mode="progressive", upscale=4, **keys)
    rec = um.Recorder(rt, cuda, 4)
    low = sm.replay_progressive(rec, cuda, **keys)
    assert sorted(low) == [2, 4]
    assert_shown(tmp_path, rec, [low[2], low[4]], ["pass_0002.ppm", "pass_0004.ppm"], 33, 21)
    assert rec.shown[0] != rec.shown[1]
