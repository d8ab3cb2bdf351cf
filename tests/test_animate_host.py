"""CPU tests of the animation entry points (not gpu): the camera of a world that is never uploaded, the new symbols in header, library
and binding, and the numpy model of rt_temporal_accumulate_moving (tests/temporal_moving_model.py) on its hand-worked cases."""
import ctypes as C

import numpy as np
import pytest

import abi_header
import temporal_moving_model as tmm

NEW = ("rt_world_set_camera", "rt_world_camera", "rt_world_set_geometry", "rt_world_get_geometry", "rt_temporal_accumulate_moving")


@pytest.mark.parametrize("precision", ["FP32", "FP16"])
def test_camera_round_trip_without_a_device(rt, precision):
    prec = getattr(rt, precision)
    W = rt.World(22, 43, 21, precision=prec)
    first = W.camera.copy()
    assert np.array_equal(W.get_camera().view(np.uint8), first.view(np.uint8))
    cam = rt.camera_init((3.0, 4.0, -5.0), (0.5, 0.25, 0.0), (0, 1, 0), 40.0, 43 / 21, 0.05, 7.0, precision=prec)
    assert not np.array_equal(cam.view(np.uint8), first.view(np.uint8))
    assert W.set_camera(cam) is W
    assert np.array_equal(W.get_camera().view(np.uint8), cam.view(np.uint8))
    assert np.array_equal(W.camera.view(np.uint8), cam.view(np.uint8))
    # the bytes, whatever they are: NaN payloads and negative zeros come back as they went in
    odd = np.zeros(1, rt.camera_dtype)
    odd.view(np.uint32)[:] = np.arange(22, dtype=np.uint32) * 0x01010101 + 0x7fc00001
    W.set_camera(odd)
    assert np.array_equal(W.get_camera().view(np.uint8), odd.view(np.uint8))
    L = rt.lib()
    out = np.zeros(1, rt.camera_dtype)
    assert L.rt_world_set_camera(None, cam.ctypes.data_as(C.c_void_p)) == -1
    assert L.rt_world_set_camera(W.h, None) == -1
    assert L.rt_world_camera(None, out.ctypes.data_as(C.c_void_p)) == -1
    assert L.rt_world_camera(W.h, None) == -1
    assert np.array_equal(W.get_camera().view(np.uint8), odd.view(np.uint8))        # a refused call changes nothing
    # the geometry calls and the moving accumulate refuse NULL before they touch a device
    assert L.rt_world_set_geometry(None, None, None) == -1 and L.rt_world_set_geometry(W.h, None, None) == -1
    assert L.rt_world_set_geometry(W.h, C.c_void_p(8), None) == -1                  # not 16-byte aligned
    assert L.rt_world_get_geometry(None, None, None) == -1 and L.rt_world_get_geometry(W.h, None, None) == -1
    assert L.rt_temporal_accumulate_moving(None, None, None, None, None, None, None, None, 4, 4, C.byref(rt.temporal_params()), None) == -1
    W.close()


def test_header_library_and_binding_name_the_new_symbols(rt):
    abi_header.check_bound(rt, NEW)
    assert all(abi_header.PROTOTYPES[name][0] is C.c_int for name in NEW)
    assert len(rt.SYMBOLS["rt_temporal_accumulate_moving"][1]) == 12 and len(rt.SYMBOLS["rt_world_set_geometry"][1]) == 3
    for name in ("set_camera", "get_camera", "set_geometry", "get_geometry"):
        assert callable(getattr(rt.World, name)), name
    assert callable(rt.temporal_accumulate_moving)
    assert rt.lib().rt_abi_version() == 6 and abi_header.DEFINES["RT_ABI_VERSION"] == 6


def test_the_moving_model_on_its_hand_worked_cases():
    tmm.self_check()


def test_moving_model_on_random_buffers_keeps_both_identities():
    """fabricated 9x7 buffers, 12 spheres of which a third moved and a third changed radius: nothing moved is the static model's bytes,
    and on the pixels that kept their radius the moving model is the static model on patched guides"""
    tm = tmm.tm
    rng = np.random.default_rng(5)
    nx, ny = 9, 7
    n = nx * ny
    cam = tm.simple_camera()
    j, i = np.divmod(np.arange(n), nx)
    pts = np.stack([-1 + 2 * (i + 0.5) / nx, -1 + 2 * (j + 0.5) / ny, -np.ones(n)], 1) * rng.uniform(1.5, 2.5, n)[:, None]
    prev, state = tm.simple_frame(nx, ny, pts)
    prev["sphere"] = rng.integers(0, 12, n)
    hits = prev.copy()
    hits["sphere"][rng.choice(n, 3, replace=False)] = [-1, 12, 1 << 20]
    g0 = rng.uniform(-1, 1, (12, 4)).astype(np.float32)
    g1 = g0.copy()
    g1[1::3, :3] += np.float32(0.3)
    g1[2::3, 3] *= np.float32(1.25)
    hist = tm.make_history(rng.uniform(0, 1, (n, 4)).astype(np.float32), rng.choice(np.array([0, 4, 8], np.float32), n))
    kind = np.zeros(12, np.int32)
    args = dict(kind=kind, nx=nx, ny=ny, max_history=32, reuse_specular=0, position_tolerance=1.0, normal_min_dot=0.9)
    assert np.array_equal(tmm.accumulate_moving(hist, hits, prev, cam, g0, g0, state, **args), tm.accumulate(hist, hits, prev, cam, state, **args))
    c = {}
    got = tmm.accumulate_moving(hist, hits, prev, cam, g1, g0, state, counts=c, **args)
    ref = tm.accumulate(hist, tmm.patched_guides(hits, g1, g0), prev, cam, state, **args)
    keep = ~c["resized_mask"]
    gx, gn = tm.history_parts(got, n)
    rx, rn = tm.history_parts(ref, n)
    assert keep.sum() > n // 2 and np.array_equal(gx[keep], rx[keep]) and np.array_equal(gn[keep], rn[keep])
    assert c["resized_not_asked"] > 0 and c["moved_asked"] > 0
    first = tm.history_parts(tm.accumulate(None, hits, None, None, state, **args), n)
    assert np.array_equal(gx[~keep], first[0][~keep]) and np.array_equal(gn[~keep], first[1][~keep])
