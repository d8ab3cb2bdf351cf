"""walk_pool's thin rounds (-m gpu): calls of the pooled walk that at most 16 walkers entered form their columns one lane per
(walker, column) and deal the entries out through 64 slots; more than 64 entries go to the generic loop.

Every result is compared bit for bit with the CPU oracle's hit records or frame rows ("NaN where the oracle has NaN").
  * rt_trace_rays puts 64 consecutive rays into a wave: batches of 1 .. 65 rays put 1 .. 16, 17, 63, 64 and 1 walkers into the
    last wave, to either side of the 16; batches of 256 in which only every fifth ray can walk (the rest start above the spheres
    and point at the sky) put 12 or 13 walkers into each of four full waves;
  * tests/grid_threshold_worlds.py's `coop` world (radius 0.35) holds more than 16 entries in every column the rays cross, about 50
    in a ray's first four ranges: sixteen parallel rays overflow the 64 slots.  The model's cell starts show that on the CPU, from
    ranges NARROWER than the kernel's (so the kernel's four columns hold at least as many);
  * rays that leave the spheres' slab inside their first column, and rays that cross more than four columns, forward and backward
    along x and along z;
  * a 64 x 32 frame at 16 spp, whole and as progressive passes, and the pilot's per-tile counts (W.work, W.cols) of that frame, which
    equal the values recorded before the thin rounds existed (tests/golden/thin_rounds_tile_costs.npz)."""
import functools
import os

import numpy as np
import pytest

import grid_threshold_worlds as gw
import material_edge_worlds as mw
import reference_cases as rc
from bitcmp import same_nan_as_ref
from gpu_frames import render_frame, states_of
from oracle_lib import OracleScene
from tree_compare import assert_records, traced

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "thin_rounds_tile_costs.npz")
BATCHES = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65)
SCENES = {"tree": (10000, True, 32), "list": (500, False, 30)}
NX, NY, NS = 64, 32, 16
AXES = [(0, 1.0), (0, -1.0), (2, 1.0), (2, -1.0)]
AXIS_IDS = ["+x", "-x", "+z", "-z"]


def axis_rays(rng, k, axis, sign, short, ext=8.0):
    """k rays from inside the field, y in the spheres' slab.  short: all but vertical, down - the line leaves the slab (and meets the
    ground) within a twentieth of a unit along its major axis; else all but level: it crosses the field, tens of columns"""
    o = rng.uniform([-ext, 0.3, -ext], [ext, 0.9, ext], (k, 3))
    d = np.empty((k, 3))
    other = 2 - axis
    d[:, axis] = sign * (0.05 if short else 1.0)
    d[:, other] = rng.uniform(-0.6, 0.6, k) * (0.05 if short else 1.0)
    d[:, 1] = -1.0 if short else rng.uniform(-0.03, 0.03, k)
    return np.ascontiguousarray(np.concatenate([o, d], 1), F)


def scene_rays(n, seed):
    """walking rays of every kind: scene-like ones (origins in the field, towards points near the ground), then along both axes, both
    ways, short and long"""
    rng = np.random.default_rng(seed)
    o, d = gw._scene_rays(rng, n // 2)
    parts = [np.concatenate([o, d], 1).astype(F)]
    k = (n - n // 2) // 8
    for axis, sign in AXES:
        for short in (True, False):
            parts.append(axis_rays(rng, k, axis, sign, short))
    rays = np.concatenate(parts)
    return np.ascontiguousarray(rays[rng.permutation(len(rays))], F)


def sky_rays(rng, k):
    """fast-path rays that cannot walk: from above the spheres, upwards"""
    o = rng.uniform([-8.0, 3.0, -8.0], [8.0, 5.0, 8.0], (k, 3))
    d = rng.normal(size=(k, 3))
    d[:, 1] = np.abs(d[:, 1]) + 0.2
    return np.concatenate([o, d], 1).astype(F)


@functools.lru_cache(None)
def scene_case(name):
    """(rays, the oracle's records) of a create_world scene, computed once and never written to: 512 walking rays for the batches, then
    256 of which every fifth walks"""
    n, tree, spl = SCENES[name]
    walkers = scene_rays(512, 9100 + n)
    rng = np.random.default_rng(9200 + n)
    mixed = sky_rays(rng, 256)
    mixed[::5] = scene_rays(64, 9300 + n)[:52]
    rays = np.ascontiguousarray(np.concatenate([walkers, mixed]), F)
    ref = rc.trace(OracleScene(n, 1200, 800, use_octree=tree, spl=spl), rays, 2 if tree else 1)
    for a in [rays] + list(ref.values()):
        a.setflags(write=False)
    return rays, ref


def scene_world(rt, name):
    n, tree, spl = SCENES[name]
    W = rt.World(n, 1200, 800)
    O = rt.Octree(W, spl) if tree else None
    if O is not None:
        O.set_traversal(rt.TRAVERSAL_FAST)
    else:
        assert W.list_accel_info()["enabled"]
        W.set_list_traversal(rt.TRAVERSAL_FAST)
    return W, O


def cut(ref, a, b):
    return {k: v[a:b] for k, v in ref.items()}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_batches_either_side_of_sixteen_walkers(rt, cuda, name):
    W, O = scene_world(rt, name)
    assert rt.render_kernel_name(W, O, 0) == ("k_render<true,0,4>" if name == "tree" else "k_render<true,0,5>")
    rays, ref = scene_case(name)
    assert ref["hit"][:512].sum() > 300
    at = 0
    for n in BATCHES:
        assert_records(traced(rt, cuda, W, O, rays[at:at + n]), cut(ref, at, at + n), (name, n))
        at += n
    assert at <= 512


@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_fifth_ray_walks(rt, cuda, name):
    W, O = scene_world(rt, name)
    rays, ref = scene_case(name)
    got = traced(rt, cuda, W, O, rays[512:])
    assert_records(got, cut(ref, 512, 768), name)
    walk = np.zeros(256, bool); walk[::5] = True
    assert not ref["hit"][512:][~walk].any() and ref["hit"][512:][walk].sum() > 30


# ---------------------------------------------------------------------------------------------------- more than 64 entries
COOP = ("switches", "coop", "tree", 64)


@functools.lru_cache(None)
def coop_model():
    sp, cam = gw.world(COOP[0], COOP[1])
    return sp, cam, gw.model(sp, "tree", gw.stored_by_oracle(sp, cam, COOP[3]))


def columns_lower_bound(m, cs, rays):
    """per ray a LOWER bound of the entries in the ranges of its first four columns: the kernel's expressions in float64 with the query
    grown by the largest inflated radius only (the kernel adds slack to it) and a bin dropped at either end of every range.  The rays
    start at the middle of a column, level enough to stay in the slab for more than four columns."""
    G, Gf, h, g0 = m["G"], m["G"] * gw.FINE, m["h"], m["g0"]
    q = float(m["Rp"][~m["is_large"]].max()) / h
    out = []
    for r in np.asarray(rays, np.float64):
        xmajor = abs(r[3]) >= abs(r[5])
        om, on, dm, dn = (r[0], r[2], r[3], r[5]) if xmajor else (r[2], r[0], r[5], r[3])
        om_c, on_c, slope, step = (om - g0) / h, (on - g0) / h, dn / dm, (1 if dm > 0 else -1)
        i0, total = int(np.floor(om_c)), 0
        for c in range(4):
            i = i0 + c * step
            assert 0 <= i < G
            assert int(cs[(0 if xmajor else G * Gf + 1) + (i + 1) * Gf]) - int(cs[(0 if xmajor else G * Gf + 1) + i * Gf]) > 16      # the whole column
            u0 = on_c + (i - om_c) * slope
            u1 = u0 + slope
            k0 = int(max((min(u0, u1) - q) * gw.FINE, 0.0)) + 1
            k1 = int(min((max(u0, u1) + q) * gw.FINE, Gf - 0.5)) - 1
            base = (0 if xmajor else G * Gf + 1) + i * Gf
            total += max(0, int(cs[base + k1 + 1]) - int(cs[base + k0]))
        out.append(total)
    return np.array(out)


def parallel_rays(m, axis, sign, short):
    """sixteen parallel rays from the middles of columns of the model's grid, side by side along the minor axis"""
    h, g0 = m["h"], m["g0"]
    col = int(np.floor((-3.0 * sign - g0) / h))
    o = np.zeros((16, 3))
    o[:, axis] = g0 + (col + 0.5) * h
    o[:, 2 - axis] = np.linspace(-6.0, 6.0, 16)
    o[:, 1] = 0.5
    d = np.zeros((16, 3))
    d[:, axis] = sign * (0.05 if short else 1.0)
    d[:, 2 - axis] = 0.31 * (0.05 if short else 1.0)
    d[:, 1] = -1.0 if short else -0.01
    return np.ascontiguousarray(np.concatenate([o, d], 1), F)


@functools.lru_cache(None)
def coop_case():
    sp, cam, m = coop_model()
    sets = {}
    for (axis, sign), tag in zip(AXES, AXIS_IDS):
        long_, short = parallel_rays(m, axis, sign, False), parallel_rays(m, axis, sign, True)
        sets[tag] = dict(long=long_, short=short, mixed=np.ascontiguousarray(np.concatenate([long_[::2], short[1::2]]), F))
    S = gw.oracle(sp, cam, True, COOP[3])
    out = {}
    for tag, fam in sets.items():
        for kind, rays in fam.items():
            ref = S.trace(rays, mode=2)
            for a in [rays] + list(ref.values()):
                a.setflags(write=False)
            out[tag, kind] = (rays, ref)
    return out


@pytest.mark.parametrize("tag", AXIS_IDS)
def test_sixteen_parallel_rays_overflow_the_slots(rt, cuda, tag):
    sp, cam, m = coop_model()
    cs = gw.cell_starts(m)
    W = mw.gpu_world(rt, sp, cam, gw.NX, gw.NY)
    O = rt.Octree(W, COOP[3])
    assert rt.render_kernel_name(W, O, 0) == "k_render<true,0,4>"
    assert np.array_equal(O.upload().device_array(5).view(np.int32), cs)
    case = coop_case()
    rays, ref = case[tag, "long"]
    assert gw.fast_path(rays)["fast"].all()
    per_ray = columns_lower_bound(m, cs, rays)
    assert per_ray.sum() > 64, per_ray                                       # the sixteen walkers' first round overflows the slots
    hits = 0
    for kind in ("long", "short", "mixed"):
        rays, ref = case[tag, kind]
        assert len(rays) == 16
        assert_records(traced(rt, cuda, W, O, rays), ref, (tag, kind))
        hits += int(ref["hit"].sum())
    assert hits >= 32


# ---------------------------------------------------------------------------------------------------- frames and tile costs
@functools.lru_cache(None)
def oracle_frames():
    S = OracleScene(10000, NX, NY, use_octree=True, spl=32)
    whole, whole_st = S.render(NS, nthreads=8)
    st = S.render_init()
    acc = np.zeros((NY, NX, 3), F)
    passes = {}
    for k in range(1, NS + 1):
        S.render_progressive(acc, k, st, nthreads=8)
        if k in (1, 2, NS):
            passes[k] = (acc.copy(), st.copy())
    return whole, whole_st, passes


def test_frame_whole_and_progressive(rt, cuda):
    torch = cuda
    W = rt.World(10000, NX, NY)
    O = rt.Octree(W, 32)
    whole, whole_st, passes = oracle_frames()
    fb, st = render_frame(rt, torch, W, O, NX, NY, NS)
    assert same_nan_as_ref(fb.cpu().numpy().reshape(NY, NX, 3), whole)
    assert np.array_equal(states_of(st)[:, :6], whole_st[:, :6])
    st = rt.alloc_rand_state(NX, NY); fb = rt.alloc_fb(NX, NY)
    rt.render_init(NX, NY, st)
    for k in range(1, NS + 1):
        rt.render_progressive(fb, NX, NY, k, W, st, O)
        if k in passes:
            torch.cuda.synchronize()
            assert same_nan_as_ref(fb.cpu().numpy().reshape(NY, NX, 3), passes[k][0]), k
            assert np.array_equal(states_of(st)[:, :6], passes[k][1][:, :6]), k


@pytest.mark.parametrize("name", sorted(SCENES))
def test_tile_costs_equal_the_recorded_ones(rt, cuda, name):
    """rt_split_balanced's per-tile bounces, pooled entries (W.work) and columns (W.cols) of the 64 x 32 frame"""
    n, tree, spl = SCENES[name]
    W = rt.World(n, NX, NY)
    O = rt.Octree(W, spl) if tree else None
    starts, b, t, c = rt.split_balanced(W, O, NX, NY, 2, counts=True)
    want = np.load(GOLDEN)
    assert t.sum() > 0 and c.sum() > 0
    assert np.array_equal(b, want[name + "_bounces"])
    assert np.array_equal(t, want[name + "_tests"])
    assert np.array_equal(c, want[name + "_cols"])
    assert np.array_equal(np.array(starts, np.int64), want[name + "_starts"])
