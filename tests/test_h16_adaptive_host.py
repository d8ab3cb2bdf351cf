"""tests/h16_adaptive_model.py — the numpy model the GPU tests of rt_render_adaptive_h16 compare with — pinned to the CPU oracle, without
a GPU.  Two binary16 worlds at 64x40: 10 000 spheres with an octree at SPHERES_PER_LEAF 32, and 500 spheres on the list path.  The
per-sample colours are the oracle's one-sample render_progressive passes.  At rel_error = 0 and at min = max = k the model's frame and
the RNG states are OracleScene.render(k)'s, bit for bit (the scale and the square root of a pixel's end); and the model's count map at
the targets the GPU tests sweep is mixed — at least three distinct counts, early stops and capped pixels — which is the condition those
tests rest on."""
import numpy as np
import pytest

import h16_adaptive_model as M
from oracle_lib import OracleScene

NX, NY = 64, 40
LO, HI, STEP, FLOOR = 4, 24, 4, 0.02
WORLDS = {"tree": dict(n=10000, use_octree=True, spl=32, rel=0.2), "list": dict(n=500, use_octree=False, spl=30, rel=0.1)}


@pytest.fixture(scope="module", params=list(WORLDS))
def world(request):
    """(name, scene, samples [HI, pixels, 3] float32, RNG states after every pass [HI, pixels, 12])"""
    w = WORLDS[request.param]
    sc = OracleScene(w["n"], NX, NY, fp16=True, use_octree=w["use_octree"], spl=w["spl"])
    st = sc.render_init()
    cols, states = [], []
    for _ in range(HI):
        fb = np.zeros((NY, NX, 3), np.float32)                # a fresh fb every pass: current_sample = 1 stores the sample
        sc.render_progressive(fb, 1, st, nthreads=8)
        cols.append(fb.reshape(-1, 3).copy())
        states.append(st.copy())
    yield request.param, sc, np.stack(cols), np.stack(states)
    sc.close()


@pytest.mark.parametrize("k", [4, 8, 24])
def test_a_pixel_that_ends_after_k_samples_is_renders_pixel(world, k):
    name, sc, samples, states = world
    ref, ref_st = sc.render(k, nthreads=8)
    ref = ref.reshape(-1, 3)
    assert np.array_equal(ref.astype(np.float16).astype(np.float32), ref)            # the oracle's frame: images of binary16 values
    for params in ((k, k, 1, 0.0), (k, k, STEP, 0.3), (LO, k, STEP, 0.0)):           # no checkpoint; none either; rel_error = 0 runs to the cap
        lo, hi, step, rel = params
        got = M.run(samples, rel, FLOOR, lo, step, hi)
        assert (got["spp"] == k).all(), params
        assert np.array_equal(M.bits16(got["fb"]), M.bits16(ref)), (name, params)
        assert np.array_equal(states[got["spp"] - 1, np.arange(NX * NY)], ref_st), (name, params)
    # the state's images: the binary16 sums, whose end colour is the frame
    assert np.array_equal(M.bits16(M.end_colour(got["S"].astype(np.float16), k)), M.bits16(ref))


def test_the_swept_targets_give_mixed_frames(world):
    name, sc, samples, states = world
    ok = M.mixed_targets(samples, LO, STEP, HI, FLOOR)
    rel = WORLDS[name]["rel"]
    spp = M.run(samples, rel, FLOOR, LO, STEP, HI)["spp"]
    counts = dict(zip(*(a.tolist() for a in np.unique(spp, return_counts=True))))
    print(name, "mixed at", ok, "; rel_error", rel, "counts", counts)
    assert rel in ok and M.mixed(spp, HI)
    assert len(ok) >= 2
    assert ((spp > LO) & (spp < HI)).sum() >= NX * NY // 20            # the intermediate checkpoints stop a fair share of the frame
    assert set(counts) <= set(range(LO, HI + 1, STEP))
    # a tighter target never stops a pixel earlier
    tight = M.run(samples, ok[-1], FLOOR, LO, STEP, HI)["spp"]
    loose = M.run(samples, ok[0], FLOOR, LO, STEP, HI)["spp"]
    assert (tight >= loose).all() and (tight > loose).any()


def test_the_statistics_are_binary32_and_the_colour_binary16(world):
    """the sums the rule reads are not the colour sum's: a frame where some pixel's binary16 colour sum differs from the binary32 sum of
    the same samples, while SL is the exact binary32 running sum"""
    name, sc, samples, states = world
    got = M.run(samples, 0.0, FLOOR, HI, 1, HI)
    s32 = np.zeros((NX * NY, 3), np.float32)
    sl = np.zeros(NX * NY, np.float32)
    for k in range(HI):
        s32 = s32 + samples[k]
        sl = sl + ((samples[k][:, 0] + samples[k][:, 1]) + samples[k][:, 2])
    assert (got["S"] != s32).any()
    assert np.array_equal(got["S"].astype(np.float16).astype(np.float32), got["S"])
    assert np.array_equal(got["SL"].view(np.uint32), sl.view(np.uint32))
