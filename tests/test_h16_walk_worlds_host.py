"""The worlds and rays of tests/h16_walk_worlds.py on the CPU (not gpu): every input sits where its name says, shown by the numpy model
of the binary16 walk and by the oracle alone - never by the kernel - and the model can be trusted: its own record equals the oracle's
binary16 hitTree for every ray of every case, and the oracle's equals the reference build's where oracle/_ref/ is present.
tests/test_gpu_h16_walk.py then runs the same cases through closest_tree (csrc/rt_kernels_fp16.hip).  Every figure is printed before
it is asserted.  These are conditions on the inputs: where one does not hold, the world is changed, not the condition."""
import numpy as np
import pytest

import h16_walk_worlds as hw
import ref_lib
import reference_cases as rc
from bitcmp import f32_bits, same_nan_as_ref

ULP = 2.0 ** -20                                   # of binary16 at real_t(0.001f) = 1049 / 2^20


def hbits(a):
    return np.asarray(a, np.float32).astype(np.float16).view(np.uint16)


# ---------------------------------------------------------------------------------------------------- the model, the oracle, the reference
@pytest.mark.parametrize("world,rayset", hw.CASES, ids=hw.IDS)
def test_model_record_is_the_oracles(rt, world, rayset):
    rays, m, ref = hw.host_case(rt, world, rayset)
    hit = ref["sphere"] >= 0
    print(world, rayset, "%d rays, %d hits; per-wave maxima: tasks %d big %d small %d pairs %d positives %d" % (
        len(rays), hit.sum(), m["wave_tasks"].max(), m["wave_big"].max(), m["wave_small"].max(), m["wave_pairs"].max(), m["wave_positives"].max()))
    assert np.array_equal(ref["hit"] != 0, hit)
    assert np.array_equal(m["sphere"], ref["sphere"])
    assert np.array_equal(f32_bits(m["t"][hit]), f32_bits(ref["t"][hit]))


@pytest.mark.parametrize("world,rayset", hw.CASES, ids=hw.IDS)
def test_oracle_records_are_the_reference_builds(rt, world, rayset):
    s = ref_lib.status()
    if s == "absent":
        pytest.skip("neither oracle/_ref/ nor the reference's sources are here")
    assert s == "ok", "the reference's sources are here but oracle/_ref/ is incomplete: run `make -C oracle ref`"
    tree, sp, S, info = hw.host_side(rt, world)
    rays, m, ref = hw.host_case(rt, world, rayset)
    geom, mat, kind = S.spheres()
    R = ref_lib.RefWorld(geom, mat, kind, fp16=True, spl=hw.CREATED_SPL if world == "created" else hw.SPL)
    rtree, rinfo = R.build_octree()
    assert rinfo["node_count"] == info["node_count"] and rinfo["leaf_count"] == info["leaf_count"]
    got = rc.trace(R, rays, 2)
    live = got["sphere"] != -2                                      # (a ghost slot's record: the reference has no result there)
    print(world, rayset, "%d ghost records" % (~live).sum())
    assert live.sum() >= 0.99 * len(rays)
    assert np.array_equal(got["hit"][live], ref["hit"][live]) and np.array_equal(got["sphere"][live], ref["sphere"][live])
    for f in ("t", "p", "normal"):
        assert same_nan_as_ref(got[f][live], ref[f][live]), f


# ---------------------------------------------------------------------------------------------------- leaf_sizes
def test_leaf_sizes_member_counts_and_classes(rt):
    tree, sp, _, info = hw.host_side(rt, "leaf_sizes")
    l3 = np.flatnonzero(tree.level == 3)
    got = {hw.cell_of(tree, p): len(tree.members[p]) for p in l3}
    print("leaf_sizes: cells", got, "pairs", tree.pairs[l3].tolist())
    assert got == {cell: size for size, cell in hw.LEAF_CELLS.items()}
    assert info["dropped_full"] == 0 and info["dropped_outside"] == 0 and info["flat_entries"] == 78
    by_size = {len(tree.members[p]): int(tree.pairs[p]) for p in l3}
    assert by_size == {1: 1, 2: 1, 13: 7, 14: 7, 15: 8, 16: 8, 17: 9}
    assert {s: p >= hw.K_SMALL_PAIRS for s, p in by_size.items()} == {1: False, 2: False, 13: False, 14: False, 15: True, 16: True, 17: True}
    # the odd cell of 17 is the last node of the pre-order: its pairs end the pair array, the last of them half NaN, and a pass of
    # K_PP pairs that starts anywhere in it reads past the array's end
    last = l3[-1]
    assert last == len(tree.level) - 1 and hw.cell_of(tree, last) == hw.LEAF_CELLS[17] and len(tree.members[last]) % 2 == 1
    assert hw.preorder_key(hw.LEAF_CELLS[17]) == max(hw.preorder_key(c) for c in hw.LEAF_CELLS.values())
    assert tree.first[last] + tree.pairs[last] == tree.n_pairs == 41 and tree.pairs[last] < hw.K_PP


@pytest.mark.parametrize("size", list(hw.LEAF_CELLS))
def test_leaf_sizes_aimed_rays_reach_first_last_and_pad_neighbour(rt, size):
    tree, sp, _, _ = hw.host_side(rt, "leaf_sizes")
    rays, m, ref = hw.host_case(rt, "leaf_sizes", "aimed%d" % size)
    pos = hw.node_at(tree, hw.LEAF_CELLS[size])
    members = tree.members[pos]
    assert (rays[:, 1] > 2.0).all() and len(rays) % 64 == 0                  # from outside the box
    assert m["visited"][pos].all()                                           # every lane of every wave visits the cell
    hit = set(ref["sphere"].tolist())
    print("leaf_sizes aimed%d: members %s, %d of them are some ray's record" % (size, members.tolist(), len(hit & set(members.tolist()))))
    assert members[0] in hit and members[-1] in hit                          # (odd cells: the last member shares its pair with the NaN half)
    assert set(members.tolist()) <= hit
    # every wave: `size` class and pair count as the cell's
    big = tree.pairs[pos] >= hw.K_SMALL_PAIRS
    assert (m["wave_big"] == (64 if big else 0)).all() and (m["wave_small"] == (0 if big else 64)).all()
    assert (m["wave_pairs"] == 64 * ((size + 1) // 2)).all()


def test_leaf_sizes_mixed_waves_split_their_segments(rt):
    """aimed_mix: big segments of 8, 8 and 9 pairs and small ones in one wave's pools.  The big pool's pairs are dealt out in spans of
    C = ceil(pairs / 64) < 8 pairs, so every big segment is shared by several lanes, spans begin inside segments, and 9 is no multiple
    of C: passes end at segment ends with pairs to spare"""
    tree, sp, _, _ = hw.host_side(rt, "leaf_sizes")
    rays, m, ref = hw.host_case(rt, "leaf_sizes", "aimed_mix")
    big = (tree.level == 3) & (tree.pairs >= hw.K_SMALL_PAIRS)
    big_pairs = (m["visited"][big] * tree.pairs[big][:, None]).sum(axis=0).reshape(-1, 64).sum(axis=1)
    C = -(-big_pairs // 64)
    print("leaf_sizes aimed_mix: per wave big %s small %s, big pairs %s, C %s" % (m["wave_big"].tolist(), m["wave_small"].tolist(), big_pairs.tolist(), C.tolist()))
    assert (m["wave_big"] >= 16).all() and (m["wave_small"] >= 16).all() and (m["wave_big"] + m["wave_small"] == 64).all()
    assert ((C > 1) & (C < 8)).all() and (9 % C != 0).all() and (big_pairs % 64 != 0).all()
    assert (ref["sphere"] > 0).all() and len(set(ref["sphere"].tolist())) == 78           # every sphere of the world is some lane's record


# ---------------------------------------------------------------------------------------------------- twins
@pytest.mark.parametrize("kind", ["pair", "two_pairs", "two_cells", "ground"])
def test_twins_tie_and_the_earlier_visited_wins(rt, kind):
    tree, sp, _, _ = hw.host_side(rt, "twins")
    rays, m, ref = hw.host_case(rt, "twins", kind)
    first, second = hw.TWIN_SLOTS[kind]
    assert sp["center"][first].tobytes() == sp["center"][second].tobytes() and sp["radius"][first] == sp["radius"][second]
    assert sp["material"][first] != sp["material"][second]
    ties = 0
    for i in range(len(rays)):
        if ref["sphere"][i] < 0:
            continue
        o = hw.offers_of(m, i)
        tb = f32_bits(ref["t"][i])
        at_best = o["sphere"][f32_bits(o["t"]) == tb].astype(np.int64).tolist()
        if kind == "ground":
            if f32_bits(m["ground_t"][i]) == tb and second in at_best:
                ties += 1
                assert ref["sphere"][i] == 0                                 # slot 0 wins a tie with anything in the tree
        elif first in at_best and second in at_best:
            ties += 1
            assert at_best[0] == first and ref["sphere"][i] == first        # the earlier-visited sphere
            if kind == "two_cells":
                assert at_best.count(first) == 2 and at_best.count(second) == 2     # both twins in both cells
    print("twins %s: %d of %d rays end in a tie between slots %d and %d" % (kind, ties, len(rays), first, second))
    assert ties >= 64
    # the layout the arrangement is named for
    if kind == "pair":
        pos = hw.node_at(tree, hw.TWIN_CELLS["pair"])
        assert tree.members[pos].tolist() == [first, second]                                 # the two halves of one pair
    elif kind == "two_pairs":
        pos = hw.node_at(tree, hw.TWIN_CELLS["two_pairs"])
        mem = tree.members[pos].tolist()
        assert mem.index(first) // 2 != mem.index(second) // 2                               # two pairs of one cell
    elif kind == "two_cells":
        a, b = (hw.node_at(tree, c) for c in hw.TWIN_CELLS["two_cells"])
        assert a < b and tree.members[a].tolist() == tree.members[b].tolist() == [first, second]
    else:
        cells = [hw.cell_of(tree, p) for p in np.flatnonzero(tree.level == 3) if second in tree.members[p]]
        assert len(cells) == 64 and all(c[1] == 0 for c in cells)                            # the ground's twin fills the bottom layer


# ---------------------------------------------------------------------------------------------------- stack
def test_stack_fills_the_candidate_queue_inside_a_pass(rt):
    """Every aimed wave: all 64 rays visit the stack's cell and every one of its 16 entries has a positive discriminant for every ray.

    Why this drains the queue inside push_pass.  The stack's cell (8 pairs) is the only big segment a ray can pool (the cell below holds
    5 pairs: small), so a wave's big pool holds 64 segments of 8 pairs: 512 pairs, C = ceil(512 / 64) = 8 <= kPP.  Lane w takes pairs
    [8 w, 8 w + 8), exactly one segment whatever order the atomics filed them in, in ONE pass, and that pass holds 16 positive halves.
    push_pass hands out one record per lane and turn: all 64 lanes take part in the first three turns, the queue holds 0, 64, 128
    records before them, and the third finds qn + n = 128 + 64 > kCand = 128 - the drain inside push_pass, which the `qn >= 64` drain
    after a pass cannot replace.  Three positive halves in every lane's first pass are sufficient; there are sixteen."""
    tree, sp, _, _ = hw.host_side(rt, "stack")
    rays, m, ref = hw.host_case(rt, "stack", "aimed")
    pos, below = hw.node_at(tree, hw.STACK_CELL), hw.node_at(tree, (hw.STACK_CELL[0], hw.STACK_CELL[1] - 1, hw.STACK_CELL[2]))
    l3 = np.flatnonzero(tree.level == 3)
    print("stack: cells", {hw.cell_of(tree, p): len(tree.members[p]) for p in l3}, "wave positives", m["wave_positives"].tolist())
    assert sorted(l3.tolist()) == sorted([pos, below]) and len(tree.members[pos]) == 16 and len(tree.members[below]) == 9
    assert tree.pairs[pos] == 8 == hw.K_SMALL_PAIRS and tree.pairs[below] < hw.K_SMALL_PAIRS
    assert (rays[:, 1] > 2.0).all() and m["visited"][pos].all()
    f = m["offers_unique"]
    in_stack = f["node"] == pos
    per_ray = np.bincount(f["ray"][in_stack].astype(np.int64), minlength=m["unique_of"].max() + 1)[m["unique_of"]]
    assert (per_ray == 16).all()                                              # every entry, every ray
    assert (m["wave_big"] == 64).all() and (per_ray.reshape(-1, 64).sum(axis=1) >= 64 * 16).all()
    assert 64 * tree.pairs[pos] // 64 <= hw.K_PP and 3 * 64 > hw.K_CAND and (per_ray >= 3).all()
    # (the origins, 9/64 to 0.16 from the centre, lie inside the shells of radius >= 10/64 or 11/64: the record is a shell around them)
    assert np.isin(ref["sphere"], tree.members[pos]).all() and len(set(ref["sphere"].tolist())) >= 2


def test_stack_from_inside_records_only_the_stacks_cell_holds(rt):
    """stack/inside: the same 16 positives per ray and cell, but the record is a shell of radius < 1/8, which the cell below does not
    hold a second copy of: a candidate of the stack's cell lost at a drain cannot be made up for"""
    tree, sp, _, _ = hw.host_side(rt, "stack")
    rays, m, ref = hw.host_case(rt, "stack", "inside")
    pos, below = hw.node_at(tree, hw.STACK_CELL), hw.node_at(tree, (hw.STACK_CELL[0], hw.STACK_CELL[1] - 1, hw.STACK_CELL[2]))
    f = m["offers_unique"]
    per_ray = np.bincount(f["ray"][f["node"] == pos].astype(np.int64), minlength=m["unique_of"].max() + 1)[m["unique_of"]]
    print("stack inside: records %s" % sorted(set(ref["sphere"].tolist())))
    assert m["visited"][pos].all() and (per_ray == 16).all()
    assert (ref["sphere"] > 0).all() and not np.isin(ref["sphere"], tree.members[below]).any() and len(set(ref["sphere"].tolist())) >= 2
    assert {int(s) % 2 for s in ref["sphere"]} == {0, 1}                       # entries of both halves of a pair


# ---------------------------------------------------------------------------------------------------- tmin
def test_tmin_roots_sit_at_below_and_above_t_min(rt):
    rays, m, ref = hw.host_case(rt, "tmin", "surface")
    f = m["offers_unique"]
    tmin = np.float16(hw.T_MIN)
    assert float(tmin) == 1049 * ULP
    t1, t2, t = f["t1"].astype(np.float16), f["t2"].astype(np.float16), f["t"]
    roots = set(hbits(t1).tolist()) | set(hbits(t2).tolist())
    at, below, above = (int(hbits(np.float32(k * ULP))) for k in (1049, 1048, 1050))
    near_rejected_far_accepted = ~(t1 > tmin) & (t2 > tmin)
    both_rejected = ~(t1 > tmin) & ~(t2 > tmin)
    accepted_above = (f32_bits(t) == f32_bits(np.float32(1050 * ULP))).sum()
    print("tmin: %d positive discriminants; roots at t_min %s, one ulp below %s, above %s; near rejected and far accepted %d, both rejected %d, "
          "offers one ulp above t_min %d" % (len(t), at in roots, below in roots, above in roots, near_rejected_far_accepted.sum(), both_rejected.sum(), accepted_above))
    assert at in roots and below in roots and above in roots
    assert near_rejected_far_accepted.sum() >= 10 and both_rejected.sum() >= 10 and accepted_above >= 1
    assert np.array_equal(t[near_rejected_far_accepted], t2[near_rejected_far_accepted].astype(np.float32)) and np.isinf(t[both_rejected]).all()
    # unit directions, origins ON a sphere: |o - c| = r exactly for the sphere each ray was built on (axis points)
    assert set(np.abs(rays[:, 3:]).sum(axis=1).tolist()) == {1.0}
    assert (ref["sphere"] >= 0).sum() >= 50 and (ref["sphere"] < 0).sum() >= 50


# ---------------------------------------------------------------------------------------------------- on_planes
@pytest.mark.parametrize("world", ["leaf_sizes", "created"])
def test_on_planes_rays_have_nan_parameters_and_both_verdicts(rt, world):
    rays, m, ref = hw.host_case(rt, world, "on_planes")
    d = rays[:, 3:]
    zeros = (d == 0).sum(axis=1)
    print("on_planes/%s: NaN parameters per ray %d .. %d; nodes with a NaN parameter that pass %d, that fail %d; -0 components %d; hits %d" % (
        world, m["nan_params"].min(), m["nan_params"].max(), m["nan_node_pass"].sum(), m["nan_node_fail"].sum(), (np.signbit(d) & (d == 0)).sum(),
        (ref["sphere"] >= 0).sum()))
    assert (m["nan_params"] >= 1).all() and set(zeros.tolist()) == {1, 2}
    assert m["nan_params"].max() >= 2                                         # two zero components, both axes on planes
    assert (np.signbit(d) & (d == 0)).sum() >= 100 and (~np.signbit(d) & (d == 0)).sum() >= 100
    assert m["nan_node_pass"].sum() >= 100 and m["nan_node_fail"].sum() >= 100


# ---------------------------------------------------------------------------------------------------- flood
def test_flood_overflows_every_pool(rt):
    """Sums above a capacity make an overflow certain whatever the order of the atomics: waves whose rays pass more than kTask level-2
    nodes, more than kBig big and more than kSmall small level-3 nodes - among the full waves and among the mixed ones.  (This is the
    proof the docstring of test_fp16_rays_that_pass_every_node_of_the_tree argues.)"""
    rays, m, ref = hw.host_case(rt, "created", "flood")
    nfull = hw.FLOOD_FULL_WAVES
    nmixed = 2 * len(hw.FLOOD_MIXED)
    assert len(rays) == 64 * (nfull + nmixed + 2 * len(hw.FLOOD_WITH_HITTERS))
    for name, sl in (("full", slice(0, nfull)), ("mixed", slice(nfull, nfull + nmixed)), ("mixed with hitters", slice(nfull + nmixed, None))):
        t, b, s = m["wave_tasks"][sl], m["wave_big"][sl], m["wave_small"][sl]
        print("flood %s waves: tasks up to %d (%d waves > %d), big up to %d (%d > %d), small up to %d (%d > %d)" % (
            name, t.max(), (t > hw.K_TASK).sum(), hw.K_TASK, b.max(), (b > hw.K_BIG).sum(), hw.K_BIG, s.max(), (s > hw.K_SMALL).sum(), hw.K_SMALL))
        assert (t > hw.K_TASK).any() and (b > hw.K_BIG).any() and (s > hw.K_SMALL).any()
    # the mixed waves: 1, 16, 63, 64 rays that pass every node, the others none
    every = m["visited"].all(axis=0).reshape(-1, 64).sum(axis=1)[nfull:]
    none = (~m["visited"].any(axis=0)).reshape(-1, 64).sum(axis=1)[nfull:nfull + nmixed]
    assert every.tolist() == [c for c in hw.FLOOD_MIXED + hw.FLOOD_WITH_HITTERS for _ in range(2)] and (every[:nmixed] + none == 64).all()
    # a ray of the flood offers nothing (NaN discriminants): in the last waves the OTHER lanes hit, through segments that compete for the
    # same full pools - in each of these waves a lane other than the flood's has a record in the tree
    hits = (ref["sphere"] > 0).reshape(-1, 64).sum(axis=1)
    print("flood: hits per wave with hitters %s; hits of all other waves %d" % (hits[nfull + nmixed:].tolist(), hits[:nfull + nmixed].sum()))
    assert (hits[nfull + nmixed:] >= 1).all() and hits[nfull + nmixed:].sum() >= 16
