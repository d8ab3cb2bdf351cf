"""CPU test of what the frame-shaped entry points refuse, and in which order (not gpu): one table of calls with placeholder
pointers over rt_render, rt_render_progressive, rt_render_adaptive, _part, _begin, _refine, _spend, _spend_filtered, their _on forms,
rt_adaptive_budget_select, _select_filtered and rt_split_balanced.  Every case holds at least one fault that the library refuses before
its first HIP call, so nothing here starts the HIP runtime; cases with two faults pin which refusal comes first.

The expected values are literals: the table was run against the commit before the entry points were moved onto one call frame
(b3de719), and EXPECTED is what that library returned.  The library has to keep returning exactly this."""
import ctypes as C
import types

import pytest

FAKE = C.c_void_p(0x1000)          # 16-byte aligned, never dereferenced: every call below refuses before it touches a buffer
ODD = C.c_void_p(0x1008)           # guides must be 16-byte aligned
NX, NY = 64, 40                    # 8 x 5 tiles
HUGE = (65536, 65537)              # 2^32 + 65536 pixels: above the 32-bit ids of the active lists (nothing is allocated for it)


def env(rt):
    E = types.SimpleNamespace()
    E.w = rt.World(500, NX, NY)
    E.w16 = rt.World(500, NX, NY, precision=rt.FP16)
    E.wc = rt.World(500, NX, NY).set_arith(rt.ARITH_CONTRACT)
    E.o = rt.Octree(E.w, 30)                       # built on the host: no device work until it is rendered with
    E.o16 = rt.Octree(E.w16, 30)
    E.A = rt.Adaptive(4, 32, 4, 0.05, 0.01)
    E.A2 = rt.Adaptive(4, 64, 4, 0.02, 0.01)       # refines A
    E.Abad = rt.Adaptive(1, 5, 4, 0.05, 0.01)
    E.B = rt.Budget(4096, 2, 4, 64, 0.01)
    E.Bbad = rt.Budget(4096, 0, 4, 64, 0.01)
    E.F = rt.denoise_var_params()
    E.Fbad = rt.denoise_var_params(levels=0)
    P = rt.Partition
    E.parts = dict(whole=P(0, 1, 0, 0), empty=P(1, 2, 0, 0),      # 40 tiles are one run of RT_PART_RUN: part 1 of 2 has none
                   bad=P(2, 2, 0, 0), beyond=P(0, 1, 0, 41), back=P(0, 1, 5, 5))
    return E


# the arguments of each function, in its order, from one record of named slots; an _on form puts the context in front
def _p(x):
    return C.byref(x) if x is not None else None


ARGS = {
    "rt_render": lambda a: (a.fb, a.nx, a.ny, a.ns, a.world, a.rs, a.oct, a.part, None),
    "rt_render_progressive": lambda a: (a.fb, a.nx, a.ny, a.ns, a.world, a.rs, a.oct, a.part, None),
    "rt_render_adaptive": lambda a: (a.fb, a.nx, a.ny, _p(a.P), a.world, a.rs, a.oct, a.spp, None),
    "rt_render_adaptive_part": lambda a: (a.fb, a.nx, a.ny, _p(a.P), a.world, a.rs, a.oct, a.spp, a.part, None),
    "rt_render_adaptive_begin": lambda a: (a.fb, a.nx, a.ny, _p(a.P), a.world, a.rs, a.oct, a.spp, a.state, a.part, None),
    "rt_render_adaptive_refine": lambda a: (a.fb, a.nx, a.ny, _p(a.P), _p(a.to), a.world, a.rs, a.oct, a.spp, a.state, a.part, None),
    "rt_render_adaptive_spend": lambda a: (a.fb, a.nx, a.ny, _p(a.B), a.world, a.rs, a.oct, a.spp, a.state, a.part, a.picked, None),
    "rt_render_adaptive_spend_filtered": lambda a: (a.fb, a.nx, a.ny, _p(a.B), _p(a.F), a.hits, a.world, a.rs, a.oct, a.spp, a.state, a.picked, None),
    "rt_adaptive_budget_select": lambda a: (a.ctx, a.state, a.nx, a.ny, a.part, _p(a.B), a.picks, a.list, a.count, None),
    "rt_adaptive_budget_select_filtered": lambda a: (a.ctx, a.state, a.hits, a.nx, a.ny, _p(a.B), _p(a.F), a.picks, a.list, a.count, a.keys, None),
    "rt_split_balanced": lambda a: (a.ctx, a.world, a.oct, a.nx, a.ny, a.nparts, a.starts, None, None, None, None),
}
HAS_PART = {"rt_render", "rt_render_progressive", "rt_render_adaptive_part", "rt_render_adaptive_begin", "rt_render_adaptive_refine",
            "rt_render_adaptive_spend", "rt_adaptive_budget_select"}
ADAPTIVE = ["rt_render_adaptive", "rt_render_adaptive_part", "rt_render_adaptive_begin", "rt_render_adaptive_refine", "rt_render_adaptive_spend",
            "rt_render_adaptive_spend_filtered"]
NEEDS_STATE = ["rt_render_adaptive_begin", "rt_render_adaptive_refine", "rt_render_adaptive_spend", "rt_render_adaptive_spend_filtered"]
RENDER = ["rt_render", "rt_render_progressive"]
FRAME = RENDER + ADAPTIVE


def _cases():
    """(function, faults): `faults` overrides slots of a record that is otherwise valid.  A slot that names a world, tree, parameter
    block or partition holds its key in env()."""
    out = []

    def add(fns, **faults):
        for fn in fns:
            if "part" in faults and fn not in HAS_PART:
                continue
            out.append((fn, faults))
            if fn in FRAME:
                out.append((fn + "_on", faults))

    # ---- one fault each
    add(FRAME, world=None)
    add(FRAME, nx=0)
    add(FRAME, ny=-3)
    add(FRAME, part="bad")
    add(FRAME, part="beyond")                       # tile_end beyond the frame
    add(FRAME, part="back")                         # tile_end == tile_begin != 0
    add(FRAME, fb=None)
    add(FRAME, rs=None)
    add(FRAME, oct="o16")                           # a tree of the other precision
    add(RENDER, ns=0)
    add(RENDER, fb=None, part="empty")              # a part without tiles returns 0 before the pointers are looked at
    add(RENDER, oct="o16", part="empty")            # ... but rt_render checks the tree's precision first
    add(RENDER, world="w16", oct="o")
    add(ADAPTIVE[:3], P="Abad")
    add(ADAPTIVE[:3], P=None)
    add(["rt_render_adaptive_refine"], P="Abad")
    add(["rt_render_adaptive_refine"], to="A", P="A2")          # `to` does not refine `from`
    add(["rt_render_adaptive_refine"], to=None)
    add(ADAPTIVE[4:], B="Bbad")
    add(ADAPTIVE[4:], B=None)
    add(NEEDS_STATE, state=None)
    add(ADAPTIVE, world="w16")                      # binary16 with everything else valid
    add(ADAPTIVE, world="wc")                       # a contracted world
    add(ADAPTIVE, nx=HUGE[0], ny=HUGE[1])           # npx above 2^32 - 1
    add(ADAPTIVE, spp=None, picked=None, world="w16")           # the optional outputs are optional
    # ---- two faults: which refusal wins
    add(ADAPTIVE, fb=None, part="empty")
    add(ADAPTIVE, oct="o16", part="empty")
    add(ADAPTIVE, world="w16", part="empty")
    add(ADAPTIVE, world=None, part="empty")
    add(ADAPTIVE, nx=HUGE[0], ny=HUGE[1], world="w16")
    add(ADAPTIVE, nx=HUGE[0], ny=HUGE[1], fb=None)
    add(ADAPTIVE, world="w16", fb=None)
    add(ADAPTIVE, world="w16", rs=None)
    add(ADAPTIVE, world="w16", oct="o")             # precision match before RT_ENOTSUP
    add(ADAPTIVE, world="wc", oct="o16")
    add(ADAPTIVE, world="wc", fb=None)
    add(NEEDS_STATE, world="w16", state=None)       # a binary16 world plus a NULL state
    add(NEEDS_STATE, world="wc", state=None)
    add(NEEDS_STATE, state=None, part="empty")
    add(ADAPTIVE[:3], P="Abad", world="w16")
    add(ADAPTIVE[:3], P="Abad", part="empty")
    add(["rt_render_adaptive_refine"], to="A", P="A2", world="w16")
    add(ADAPTIVE[4:], B="Bbad", world="w16")
    add(ADAPTIVE[4:], B="Bbad", part="empty")
    flt = ["rt_render_adaptive_spend_filtered"]
    add(flt, F="Fbad")
    add(flt, F=None)
    add(flt, hits=None)
    add(flt, hits=ODD)
    add(flt, B="Bbad", F="Fbad")                    # bad rt_budget plus bad filter
    add(flt, F="Fbad", world="w16")
    add(flt, F="Fbad", fb=None)
    add(flt, hits=None, world="w16")
    add(flt, hits=ODD, world="wc")
    add(flt, hits=None, state=None)
    add(flt, hits=ODD, oct="o16")
    add(flt, F="Fbad", nx=HUGE[0], ny=HUGE[1])
    # ---- the selections (the context is a placeholder: everything is refused before it is looked at)
    sel, self_ = ["rt_adaptive_budget_select"], ["rt_adaptive_budget_select_filtered"]
    for fn in (sel, self_):
        add(fn, ctx=None)
        add(fn, B="Bbad")
        add(fn, B=None)
        add(fn, picks=-1)
        add(fn, picks=1 << 32)
        add(fn, nx=0)
        add(fn, state=None)
        add(fn, list=None)
        add(fn, count=None)
        add(fn, nx=HUGE[0], ny=HUGE[1])
        add(fn, ctx=None, state=None)
    add(sel, part="bad")
    add(sel, part="beyond")
    add(sel, state=None, part="empty")
    add(sel, list=None, count=None, part="empty")
    add(sel, B="Bbad", part="empty")
    add(sel, picks=-1, part="empty")
    add(sel, nx=HUGE[0], ny=HUGE[1], state=None)
    add(self_, F="Fbad")
    add(self_, F=None)
    add(self_, hits=None)
    add(self_, hits=ODD)
    add(self_, B="Bbad", F="Fbad")
    add(self_, F="Fbad", state=None)
    add(self_, F="Fbad", hits=ODD)
    add(self_, keys=None, hits=None)
    # ---- rt_split_balanced
    sp = ["rt_split_balanced"]
    add(sp, world=None)
    add(sp, starts=None)
    add(sp, nx=0)
    add(sp, nparts=0)
    add(sp, nparts=65)
    add(sp, oct="o16")
    add(sp, world="w16", oct="o")
    add(sp, nx=8, ny=8, nparts=2)                   # fewer tiles than parts
    add(sp, nx=8, ny=8, nparts=2, oct="o16")
    add(sp, nparts=41)
    add(sp, ctx=None, world=None)
    return out


def case_id(fn, faults):
    return fn + "[" + ",".join("%s=%s" % (k, v.value if isinstance(v, C.c_void_p) else v) for k, v in faults.items()) + "]"


def run_case(rt, E, fn, faults):
    a = types.SimpleNamespace(ctx=FAKE, fb=FAKE, nx=NX, ny=NY, ns=4, P="A", to="A2", world="w", rs=FAKE, oct="o", spp=FAKE, state=FAKE,
                              part="whole", B="B", F="F", hits=FAKE, picked=FAKE, picks=100, list=FAKE, count=FAKE, keys=FAKE, starts=FAKE, nparts=4)
    assert faults, "a case without a fault would start the HIP runtime"
    a.__dict__.update(faults)
    if "oct" not in faults and a.world == "w16":
        a.oct = "o16"                              # (a valid record pairs a world with a tree of its precision)
    for slot in ("P", "to", "B", "F"):
        setattr(a, slot, getattr(E, getattr(a, slot)) if getattr(a, slot) is not None else None)
    for slot in ("world", "oct"):
        setattr(a, slot, getattr(E, getattr(a, slot)).h if getattr(a, slot) is not None else None)
    a.part = E.parts[a.part]
    on = fn.endswith("_on")
    args = ARGS[fn[:-3] if on else fn](a)
    return getattr(rt.lib(), fn)(*(((a.ctx,) if on else ()) + args))


CASES = _cases()
RT_EINVAL, RT_ENOTSUP = -1, -4

# what b3de719 returned for every case (generated there, kept as literals)
EXPECTED = {
    'rt_render[world=None]': -1,
    'rt_render_on[world=None]': -1,
    'rt_render_progressive[world=None]': -1,
    'rt_render_progressive_on[world=None]': -1,
    'rt_render_adaptive[world=None]': -1,
    'rt_render_adaptive_on[world=None]': -1,
    'rt_render_adaptive_part[world=None]': -1,
    'rt_render_adaptive_part_on[world=None]': -1,
    'rt_render_adaptive_begin[world=None]': -1,
    'rt_render_adaptive_begin_on[world=None]': -1,
    'rt_render_adaptive_refine[world=None]': -1,
    'rt_render_adaptive_refine_on[world=None]': -1,
    'rt_render_adaptive_spend[world=None]': -1,
    'rt_render_adaptive_spend_on[world=None]': -1,
    'rt_render_adaptive_spend_filtered[world=None]': -1,
    'rt_render_adaptive_spend_filtered_on[world=None]': -1,
    'rt_render[nx=0]': -1,
    'rt_render_on[nx=0]': -1,
    'rt_render_progressive[nx=0]': -1,
    'rt_render_progressive_on[nx=0]': -1,
    'rt_render_adaptive[nx=0]': -1,
    'rt_render_adaptive_on[nx=0]': -1,
    'rt_render_adaptive_part[nx=0]': -1,
    'rt_render_adaptive_part_on[nx=0]': -1,
    'rt_render_adaptive_begin[nx=0]': -1,
    'rt_render_adaptive_begin_on[nx=0]': -1,
    'rt_render_adaptive_refine[nx=0]': -1,
    'rt_render_adaptive_refine_on[nx=0]': -1,
    'rt_render_adaptive_spend[nx=0]': -1,
    'rt_render_adaptive_spend_on[nx=0]': -1,
    'rt_render_adaptive_spend_filtered[nx=0]': -1,
    'rt_render_adaptive_spend_filtered_on[nx=0]': -1,
    'rt_render[ny=-3]': -1,
    'rt_render_on[ny=-3]': -1,
    'rt_render_progressive[ny=-3]': -1,
    'rt_render_progressive_on[ny=-3]': -1,
    'rt_render_adaptive[ny=-3]': -1,
    'rt_render_adaptive_on[ny=-3]': -1,
    'rt_render_adaptive_part[ny=-3]': -1,
    'rt_render_adaptive_part_on[ny=-3]': -1,
    'rt_render_adaptive_begin[ny=-3]': -1,
    'rt_render_adaptive_begin_on[ny=-3]': -1,
    'rt_render_adaptive_refine[ny=-3]': -1,
    'rt_render_adaptive_refine_on[ny=-3]': -1,
    'rt_render_adaptive_spend[ny=-3]': -1,
    'rt_render_adaptive_spend_on[ny=-3]': -1,
    'rt_render_adaptive_spend_filtered[ny=-3]': -1,
    'rt_render_adaptive_spend_filtered_on[ny=-3]': -1,
    'rt_render[part=bad]': -1,
    'rt_render_on[part=bad]': -1,
    'rt_render_progressive[part=bad]': -1,
    'rt_render_progressive_on[part=bad]': -1,
    'rt_render_adaptive_part[part=bad]': -1,
    'rt_render_adaptive_part_on[part=bad]': -1,
    'rt_render_adaptive_begin[part=bad]': -1,
    'rt_render_adaptive_begin_on[part=bad]': -1,
    'rt_render_adaptive_refine[part=bad]': -1,
    'rt_render_adaptive_refine_on[part=bad]': -1,
    'rt_render_adaptive_spend[part=bad]': -1,
    'rt_render_adaptive_spend_on[part=bad]': -1,
    'rt_render[part=beyond]': -1,
    'rt_render_on[part=beyond]': -1,
    'rt_render_progressive[part=beyond]': -1,
    'rt_render_progressive_on[part=beyond]': -1,
    'rt_render_adaptive_part[part=beyond]': -1,
    'rt_render_adaptive_part_on[part=beyond]': -1,
    'rt_render_adaptive_begin[part=beyond]': -1,
    'rt_render_adaptive_begin_on[part=beyond]': -1,
    'rt_render_adaptive_refine[part=beyond]': -1,
    'rt_render_adaptive_refine_on[part=beyond]': -1,
    'rt_render_adaptive_spend[part=beyond]': -1,
    'rt_render_adaptive_spend_on[part=beyond]': -1,
    'rt_render[part=back]': -1,
    'rt_render_on[part=back]': -1,
    'rt_render_progressive[part=back]': -1,
    'rt_render_progressive_on[part=back]': -1,
    'rt_render_adaptive_part[part=back]': -1,
    'rt_render_adaptive_part_on[part=back]': -1,
    'rt_render_adaptive_begin[part=back]': -1,
    'rt_render_adaptive_begin_on[part=back]': -1,
    'rt_render_adaptive_refine[part=back]': -1,
    'rt_render_adaptive_refine_on[part=back]': -1,
    'rt_render_adaptive_spend[part=back]': -1,
    'rt_render_adaptive_spend_on[part=back]': -1,
    'rt_render[fb=None]': -1,
    'rt_render_on[fb=None]': -1,
    'rt_render_progressive[fb=None]': -1,
    'rt_render_progressive_on[fb=None]': -1,
    'rt_render_adaptive[fb=None]': -1,
    'rt_render_adaptive_on[fb=None]': -1,
    'rt_render_adaptive_part[fb=None]': -1,
    'rt_render_adaptive_part_on[fb=None]': -1,
    'rt_render_adaptive_begin[fb=None]': -1,
    'rt_render_adaptive_begin_on[fb=None]': -1,
    'rt_render_adaptive_refine[fb=None]': -1,
    'rt_render_adaptive_refine_on[fb=None]': -1,
    'rt_render_adaptive_spend[fb=None]': -1,
    'rt_render_adaptive_spend_on[fb=None]': -1,
    'rt_render_adaptive_spend_filtered[fb=None]': -1,
    'rt_render_adaptive_spend_filtered_on[fb=None]': -1,
    'rt_render[rs=None]': -1,
    'rt_render_on[rs=None]': -1,
    'rt_render_progressive[rs=None]': -1,
    'rt_render_progressive_on[rs=None]': -1,
    'rt_render_adaptive[rs=None]': -1,
    'rt_render_adaptive_on[rs=None]': -1,
    'rt_render_adaptive_part[rs=None]': -1,
    'rt_render_adaptive_part_on[rs=None]': -1,
    'rt_render_adaptive_begin[rs=None]': -1,
    'rt_render_adaptive_begin_on[rs=None]': -1,
    'rt_render_adaptive_refine[rs=None]': -1,
    'rt_render_adaptive_refine_on[rs=None]': -1,
    'rt_render_adaptive_spend[rs=None]': -1,
    'rt_render_adaptive_spend_on[rs=None]': -1,
    'rt_render_adaptive_spend_filtered[rs=None]': -1,
    'rt_render_adaptive_spend_filtered_on[rs=None]': -1,
    'rt_render[oct=o16]': -1,
    'rt_render_on[oct=o16]': -1,
    'rt_render_progressive[oct=o16]': -1,
    'rt_render_progressive_on[oct=o16]': -1,
    'rt_render_adaptive[oct=o16]': -1,
    'rt_render_adaptive_on[oct=o16]': -1,
    'rt_render_adaptive_part[oct=o16]': -1,
    'rt_render_adaptive_part_on[oct=o16]': -1,
    'rt_render_adaptive_begin[oct=o16]': -1,
    'rt_render_adaptive_begin_on[oct=o16]': -1,
    'rt_render_adaptive_refine[oct=o16]': -1,
    'rt_render_adaptive_refine_on[oct=o16]': -1,
    'rt_render_adaptive_spend[oct=o16]': -1,
    'rt_render_adaptive_spend_on[oct=o16]': -1,
    'rt_render_adaptive_spend_filtered[oct=o16]': -1,
    'rt_render_adaptive_spend_filtered_on[oct=o16]': -1,
    'rt_render[ns=0]': -1,
    'rt_render_on[ns=0]': -1,
    'rt_render_progressive[ns=0]': -1,
    'rt_render_progressive_on[ns=0]': -1,
    'rt_render[fb=None,part=empty]': 0,
    'rt_render_on[fb=None,part=empty]': 0,
    'rt_render_progressive[fb=None,part=empty]': 0,
    'rt_render_progressive_on[fb=None,part=empty]': 0,
    'rt_render[oct=o16,part=empty]': -1,
    'rt_render_on[oct=o16,part=empty]': -1,
    'rt_render_progressive[oct=o16,part=empty]': -1,
    'rt_render_progressive_on[oct=o16,part=empty]': -1,
    'rt_render[world=w16,oct=o]': -1,
    'rt_render_on[world=w16,oct=o]': -1,
    'rt_render_progressive[world=w16,oct=o]': -1,
    'rt_render_progressive_on[world=w16,oct=o]': -1,
    'rt_render_adaptive[P=Abad]': -1,
    'rt_render_adaptive_on[P=Abad]': -1,
    'rt_render_adaptive_part[P=Abad]': -1,
    'rt_render_adaptive_part_on[P=Abad]': -1,
    'rt_render_adaptive_begin[P=Abad]': -1,
    'rt_render_adaptive_begin_on[P=Abad]': -1,
    'rt_render_adaptive[P=None]': -1,
    'rt_render_adaptive_on[P=None]': -1,
    'rt_render_adaptive_part[P=None]': -1,
    'rt_render_adaptive_part_on[P=None]': -1,
    'rt_render_adaptive_begin[P=None]': -1,
    'rt_render_adaptive_begin_on[P=None]': -1,
    'rt_render_adaptive_refine[P=Abad]': -1,
    'rt_render_adaptive_refine_on[P=Abad]': -1,
    'rt_render_adaptive_refine[to=A,P=A2]': -1,
    'rt_render_adaptive_refine_on[to=A,P=A2]': -1,
    'rt_render_adaptive_refine[to=None]': -1,
    'rt_render_adaptive_refine_on[to=None]': -1,
    'rt_render_adaptive_spend[B=Bbad]': -1,
    'rt_render_adaptive_spend_on[B=Bbad]': -1,
    'rt_render_adaptive_spend_filtered[B=Bbad]': -1,
    'rt_render_adaptive_spend_filtered_on[B=Bbad]': -1,
    'rt_render_adaptive_spend[B=None]': -1,
    'rt_render_adaptive_spend_on[B=None]': -1,
    'rt_render_adaptive_spend_filtered[B=None]': -1,
    'rt_render_adaptive_spend_filtered_on[B=None]': -1,
    'rt_render_adaptive_begin[state=None]': -1,
    'rt_render_adaptive_begin_on[state=None]': -1,
    'rt_render_adaptive_refine[state=None]': -1,
    'rt_render_adaptive_refine_on[state=None]': -1,
    'rt_render_adaptive_spend[state=None]': -1,
    'rt_render_adaptive_spend_on[state=None]': -1,
    'rt_render_adaptive_spend_filtered[state=None]': -1,
    'rt_render_adaptive_spend_filtered_on[state=None]': -1,
    'rt_render_adaptive[world=w16]': -4,
    'rt_render_adaptive_on[world=w16]': -4,
    'rt_render_adaptive_part[world=w16]': -4,
    'rt_render_adaptive_part_on[world=w16]': -4,
    'rt_render_adaptive_begin[world=w16]': -4,
    'rt_render_adaptive_begin_on[world=w16]': -4,
    'rt_render_adaptive_refine[world=w16]': -4,
    'rt_render_adaptive_refine_on[world=w16]': -4,
    'rt_render_adaptive_spend[world=w16]': -4,
    'rt_render_adaptive_spend_on[world=w16]': -4,
    'rt_render_adaptive_spend_filtered[world=w16]': -4,
    'rt_render_adaptive_spend_filtered_on[world=w16]': -4,
    'rt_render_adaptive[world=wc]': -4,
    'rt_render_adaptive_on[world=wc]': -4,
    'rt_render_adaptive_part[world=wc]': -4,
    'rt_render_adaptive_part_on[world=wc]': -4,
    'rt_render_adaptive_begin[world=wc]': -4,
    'rt_render_adaptive_begin_on[world=wc]': -4,
    'rt_render_adaptive_refine[world=wc]': -4,
    'rt_render_adaptive_refine_on[world=wc]': -4,
    'rt_render_adaptive_spend[world=wc]': -4,
    'rt_render_adaptive_spend_on[world=wc]': -4,
    'rt_render_adaptive_spend_filtered[world=wc]': -4,
    'rt_render_adaptive_spend_filtered_on[world=wc]': -4,
    'rt_render_adaptive[nx=65536,ny=65537]': -1,
    'rt_render_adaptive_on[nx=65536,ny=65537]': -1,
    'rt_render_adaptive_part[nx=65536,ny=65537]': -1,
    'rt_render_adaptive_part_on[nx=65536,ny=65537]': -1,
    'rt_render_adaptive_begin[nx=65536,ny=65537]': -1,
    'rt_render_adaptive_begin_on[nx=65536,ny=65537]': -1,
    'rt_render_adaptive_refine[nx=65536,ny=65537]': -1,
    'rt_render_adaptive_refine_on[nx=65536,ny=65537]': -1,
    'rt_render_adaptive_spend[nx=65536,ny=65537]': -1,
    'rt_render_adaptive_spend_on[nx=65536,ny=65537]': -1,
    'rt_render_adaptive_spend_filtered[nx=65536,ny=65537]': -1,
    'rt_render_adaptive_spend_filtered_on[nx=65536,ny=65537]': -1,
    'rt_render_adaptive[spp=None,picked=None,world=w16]': -4,
    'rt_render_adaptive_on[spp=None,picked=None,world=w16]': -4,
    'rt_render_adaptive_part[spp=None,picked=None,world=w16]': -4,
    'rt_render_adaptive_part_on[spp=None,picked=None,world=w16]': -4,
    'rt_render_adaptive_begin[spp=None,picked=None,world=w16]': -4,
    'rt_render_adaptive_begin_on[spp=None,picked=None,world=w16]': -4,
    'rt_render_adaptive_refine[spp=None,picked=None,world=w16]': -4,
    'rt_render_adaptive_refine_on[spp=None,picked=None,world=w16]': -4,
    'rt_render_adaptive_spend[spp=None,picked=None,world=w16]': -4,
    'rt_render_adaptive_spend_on[spp=None,picked=None,world=w16]': -4,
    'rt_render_adaptive_spend_filtered[spp=None,picked=None,world=w16]': -4,
    'rt_render_adaptive_spend_filtered_on[spp=None,picked=None,world=w16]': -4,
    'rt_render_adaptive_part[fb=None,part=empty]': 0,
    'rt_render_adaptive_part_on[fb=None,part=empty]': 0,
    'rt_render_adaptive_begin[fb=None,part=empty]': 0,
    'rt_render_adaptive_begin_on[fb=None,part=empty]': 0,
    'rt_render_adaptive_refine[fb=None,part=empty]': 0,
    'rt_render_adaptive_refine_on[fb=None,part=empty]': 0,
    'rt_render_adaptive_spend[fb=None,part=empty]': 0,
    'rt_render_adaptive_spend_on[fb=None,part=empty]': 0,
    'rt_render_adaptive_part[oct=o16,part=empty]': 0,
    'rt_render_adaptive_part_on[oct=o16,part=empty]': 0,
    'rt_render_adaptive_begin[oct=o16,part=empty]': 0,
    'rt_render_adaptive_begin_on[oct=o16,part=empty]': 0,
    'rt_render_adaptive_refine[oct=o16,part=empty]': 0,
    'rt_render_adaptive_refine_on[oct=o16,part=empty]': 0,
    'rt_render_adaptive_spend[oct=o16,part=empty]': 0,
    'rt_render_adaptive_spend_on[oct=o16,part=empty]': 0,
    'rt_render_adaptive_part[world=w16,part=empty]': 0,
    'rt_render_adaptive_part_on[world=w16,part=empty]': 0,
    'rt_render_adaptive_begin[world=w16,part=empty]': 0,
    'rt_render_adaptive_begin_on[world=w16,part=empty]': 0,
    'rt_render_adaptive_refine[world=w16,part=empty]': 0,
    'rt_render_adaptive_refine_on[world=w16,part=empty]': 0,
    'rt_render_adaptive_spend[world=w16,part=empty]': 0,
    'rt_render_adaptive_spend_on[world=w16,part=empty]': 0,
    'rt_render_adaptive_part[world=None,part=empty]': -1,
    'rt_render_adaptive_part_on[world=None,part=empty]': -1,
    'rt_render_adaptive_begin[world=None,part=empty]': -1,
    'rt_render_adaptive_begin_on[world=None,part=empty]': -1,
    'rt_render_adaptive_refine[world=None,part=empty]': -1,
    'rt_render_adaptive_refine_on[world=None,part=empty]': -1,
    'rt_render_adaptive_spend[world=None,part=empty]': -1,
    'rt_render_adaptive_spend_on[world=None,part=empty]': -1,
    'rt_render_adaptive[nx=65536,ny=65537,world=w16]': -1,
    'rt_render_adaptive_on[nx=65536,ny=65537,world=w16]': -1,
    'rt_render_adaptive_part[nx=65536,ny=65537,world=w16]': -1,
    'rt_render_adaptive_part_on[nx=65536,ny=65537,world=w16]': -1,
    'rt_render_adaptive_begin[nx=65536,ny=65537,world=w16]': -1,
    'rt_render_adaptive_begin_on[nx=65536,ny=65537,world=w16]': -1,
    'rt_render_adaptive_refine[nx=65536,ny=65537,world=w16]': -1,
    'rt_render_adaptive_refine_on[nx=65536,ny=65537,world=w16]': -1,
    'rt_render_adaptive_spend[nx=65536,ny=65537,world=w16]': -1,
    'rt_render_adaptive_spend_on[nx=65536,ny=65537,world=w16]': -1,
    'rt_render_adaptive_spend_filtered[nx=65536,ny=65537,world=w16]': -1,
    'rt_render_adaptive_spend_filtered_on[nx=65536,ny=65537,world=w16]': -1,
    'rt_render_adaptive[nx=65536,ny=65537,fb=None]': -1,
    'rt_render_adaptive_on[nx=65536,ny=65537,fb=None]': -1,
    'rt_render_adaptive_part[nx=65536,ny=65537,fb=None]': -1,
    'rt_render_adaptive_part_on[nx=65536,ny=65537,fb=None]': -1,
    'rt_render_adaptive_begin[nx=65536,ny=65537,fb=None]': -1,
    'rt_render_adaptive_begin_on[nx=65536,ny=65537,fb=None]': -1,
    'rt_render_adaptive_refine[nx=65536,ny=65537,fb=None]': -1,
    'rt_render_adaptive_refine_on[nx=65536,ny=65537,fb=None]': -1,
    'rt_render_adaptive_spend[nx=65536,ny=65537,fb=None]': -1,
    'rt_render_adaptive_spend_on[nx=65536,ny=65537,fb=None]': -1,
    'rt_render_adaptive_spend_filtered[nx=65536,ny=65537,fb=None]': -1,
    'rt_render_adaptive_spend_filtered_on[nx=65536,ny=65537,fb=None]': -1,
    'rt_render_adaptive[world=w16,fb=None]': -1,
    'rt_render_adaptive_on[world=w16,fb=None]': -1,
    'rt_render_adaptive_part[world=w16,fb=None]': -1,
    'rt_render_adaptive_part_on[world=w16,fb=None]': -1,
    'rt_render_adaptive_begin[world=w16,fb=None]': -1,
    'rt_render_adaptive_begin_on[world=w16,fb=None]': -1,
    'rt_render_adaptive_refine[world=w16,fb=None]': -1,
    'rt_render_adaptive_refine_on[world=w16,fb=None]': -1,
    'rt_render_adaptive_spend[world=w16,fb=None]': -1,
    'rt_render_adaptive_spend_on[world=w16,fb=None]': -1,
    'rt_render_adaptive_spend_filtered[world=w16,fb=None]': -1,
    'rt_render_adaptive_spend_filtered_on[world=w16,fb=None]': -1,
    'rt_render_adaptive[world=w16,rs=None]': -1,
    'rt_render_adaptive_on[world=w16,rs=None]': -1,
    'rt_render_adaptive_part[world=w16,rs=None]': -1,
    'rt_render_adaptive_part_on[world=w16,rs=None]': -1,
    'rt_render_adaptive_begin[world=w16,rs=None]': -1,
    'rt_render_adaptive_begin_on[world=w16,rs=None]': -1,
    'rt_render_adaptive_refine[world=w16,rs=None]': -1,
    'rt_render_adaptive_refine_on[world=w16,rs=None]': -1,
    'rt_render_adaptive_spend[world=w16,rs=None]': -1,
    'rt_render_adaptive_spend_on[world=w16,rs=None]': -1,
    'rt_render_adaptive_spend_filtered[world=w16,rs=None]': -1,
    'rt_render_adaptive_spend_filtered_on[world=w16,rs=None]': -1,
    'rt_render_adaptive[world=w16,oct=o]': -1,
    'rt_render_adaptive_on[world=w16,oct=o]': -1,
    'rt_render_adaptive_part[world=w16,oct=o]': -1,
    'rt_render_adaptive_part_on[world=w16,oct=o]': -1,
    'rt_render_adaptive_begin[world=w16,oct=o]': -1,
    'rt_render_adaptive_begin_on[world=w16,oct=o]': -1,
    'rt_render_adaptive_refine[world=w16,oct=o]': -1,
    'rt_render_adaptive_refine_on[world=w16,oct=o]': -1,
    'rt_render_adaptive_spend[world=w16,oct=o]': -1,
    'rt_render_adaptive_spend_on[world=w16,oct=o]': -1,
    'rt_render_adaptive_spend_filtered[world=w16,oct=o]': -1,
    'rt_render_adaptive_spend_filtered_on[world=w16,oct=o]': -1,
    'rt_render_adaptive[world=wc,oct=o16]': -1,
    'rt_render_adaptive_on[world=wc,oct=o16]': -1,
    'rt_render_adaptive_part[world=wc,oct=o16]': -1,
    'rt_render_adaptive_part_on[world=wc,oct=o16]': -1,
    'rt_render_adaptive_begin[world=wc,oct=o16]': -1,
    'rt_render_adaptive_begin_on[world=wc,oct=o16]': -1,
    'rt_render_adaptive_refine[world=wc,oct=o16]': -1,
    'rt_render_adaptive_refine_on[world=wc,oct=o16]': -1,
    'rt_render_adaptive_spend[world=wc,oct=o16]': -1,
    'rt_render_adaptive_spend_on[world=wc,oct=o16]': -1,
    'rt_render_adaptive_spend_filtered[world=wc,oct=o16]': -1,
    'rt_render_adaptive_spend_filtered_on[world=wc,oct=o16]': -1,
    'rt_render_adaptive[world=wc,fb=None]': -1,
    'rt_render_adaptive_on[world=wc,fb=None]': -1,
    'rt_render_adaptive_part[world=wc,fb=None]': -1,
    'rt_render_adaptive_part_on[world=wc,fb=None]': -1,
    'rt_render_adaptive_begin[world=wc,fb=None]': -1,
    'rt_render_adaptive_begin_on[world=wc,fb=None]': -1,
    'rt_render_adaptive_refine[world=wc,fb=None]': -1,
    'rt_render_adaptive_refine_on[world=wc,fb=None]': -1,
    'rt_render_adaptive_spend[world=wc,fb=None]': -1,
    'rt_render_adaptive_spend_on[world=wc,fb=None]': -1,
    'rt_render_adaptive_spend_filtered[world=wc,fb=None]': -1,
    'rt_render_adaptive_spend_filtered_on[world=wc,fb=None]': -1,
    'rt_render_adaptive_begin[world=w16,state=None]': -1,
    'rt_render_adaptive_begin_on[world=w16,state=None]': -1,
    'rt_render_adaptive_refine[world=w16,state=None]': -1,
    'rt_render_adaptive_refine_on[world=w16,state=None]': -1,
    'rt_render_adaptive_spend[world=w16,state=None]': -1,
    'rt_render_adaptive_spend_on[world=w16,state=None]': -1,
    'rt_render_adaptive_spend_filtered[world=w16,state=None]': -1,
    'rt_render_adaptive_spend_filtered_on[world=w16,state=None]': -1,
    'rt_render_adaptive_begin[world=wc,state=None]': -1,
    'rt_render_adaptive_begin_on[world=wc,state=None]': -1,
    'rt_render_adaptive_refine[world=wc,state=None]': -1,
    'rt_render_adaptive_refine_on[world=wc,state=None]': -1,
    'rt_render_adaptive_spend[world=wc,state=None]': -1,
    'rt_render_adaptive_spend_on[world=wc,state=None]': -1,
    'rt_render_adaptive_spend_filtered[world=wc,state=None]': -1,
    'rt_render_adaptive_spend_filtered_on[world=wc,state=None]': -1,
    'rt_render_adaptive_begin[state=None,part=empty]': 0,
    'rt_render_adaptive_begin_on[state=None,part=empty]': 0,
    'rt_render_adaptive_refine[state=None,part=empty]': 0,
    'rt_render_adaptive_refine_on[state=None,part=empty]': 0,
    'rt_render_adaptive_spend[state=None,part=empty]': 0,
    'rt_render_adaptive_spend_on[state=None,part=empty]': 0,
    'rt_render_adaptive[P=Abad,world=w16]': -1,
    'rt_render_adaptive_on[P=Abad,world=w16]': -1,
    'rt_render_adaptive_part[P=Abad,world=w16]': -1,
    'rt_render_adaptive_part_on[P=Abad,world=w16]': -1,
    'rt_render_adaptive_begin[P=Abad,world=w16]': -1,
    'rt_render_adaptive_begin_on[P=Abad,world=w16]': -1,
    'rt_render_adaptive_part[P=Abad,part=empty]': -1,
    'rt_render_adaptive_part_on[P=Abad,part=empty]': -1,
    'rt_render_adaptive_begin[P=Abad,part=empty]': -1,
    'rt_render_adaptive_begin_on[P=Abad,part=empty]': -1,
    'rt_render_adaptive_refine[to=A,P=A2,world=w16]': -1,
    'rt_render_adaptive_refine_on[to=A,P=A2,world=w16]': -1,
    'rt_render_adaptive_spend[B=Bbad,world=w16]': -1,
    'rt_render_adaptive_spend_on[B=Bbad,world=w16]': -1,
    'rt_render_adaptive_spend_filtered[B=Bbad,world=w16]': -1,
    'rt_render_adaptive_spend_filtered_on[B=Bbad,world=w16]': -1,
    'rt_render_adaptive_spend[B=Bbad,part=empty]': -1,
    'rt_render_adaptive_spend_on[B=Bbad,part=empty]': -1,
    'rt_render_adaptive_spend_filtered[F=Fbad]': -1,
    'rt_render_adaptive_spend_filtered_on[F=Fbad]': -1,
    'rt_render_adaptive_spend_filtered[F=None]': -1,
    'rt_render_adaptive_spend_filtered_on[F=None]': -1,
    'rt_render_adaptive_spend_filtered[hits=None]': -1,
    'rt_render_adaptive_spend_filtered_on[hits=None]': -1,
    'rt_render_adaptive_spend_filtered[hits=4104]': -1,
    'rt_render_adaptive_spend_filtered_on[hits=4104]': -1,
    'rt_render_adaptive_spend_filtered[B=Bbad,F=Fbad]': -1,
    'rt_render_adaptive_spend_filtered_on[B=Bbad,F=Fbad]': -1,
    'rt_render_adaptive_spend_filtered[F=Fbad,world=w16]': -1,
    'rt_render_adaptive_spend_filtered_on[F=Fbad,world=w16]': -1,
    'rt_render_adaptive_spend_filtered[F=Fbad,fb=None]': -1,
    'rt_render_adaptive_spend_filtered_on[F=Fbad,fb=None]': -1,
    'rt_render_adaptive_spend_filtered[hits=None,world=w16]': -1,
    'rt_render_adaptive_spend_filtered_on[hits=None,world=w16]': -1,
    'rt_render_adaptive_spend_filtered[hits=4104,world=wc]': -1,
    'rt_render_adaptive_spend_filtered_on[hits=4104,world=wc]': -1,
    'rt_render_adaptive_spend_filtered[hits=None,state=None]': -1,
    'rt_render_adaptive_spend_filtered_on[hits=None,state=None]': -1,
    'rt_render_adaptive_spend_filtered[hits=4104,oct=o16]': -1,
    'rt_render_adaptive_spend_filtered_on[hits=4104,oct=o16]': -1,
    'rt_render_adaptive_spend_filtered[F=Fbad,nx=65536,ny=65537]': -1,
    'rt_render_adaptive_spend_filtered_on[F=Fbad,nx=65536,ny=65537]': -1,
    'rt_adaptive_budget_select[ctx=None]': -1,
    'rt_adaptive_budget_select[B=Bbad]': -1,
    'rt_adaptive_budget_select[B=None]': -1,
    'rt_adaptive_budget_select[picks=-1]': -1,
    'rt_adaptive_budget_select[picks=4294967296]': -1,
    'rt_adaptive_budget_select[nx=0]': -1,
    'rt_adaptive_budget_select[state=None]': -1,
    'rt_adaptive_budget_select[list=None]': -1,
    'rt_adaptive_budget_select[count=None]': -1,
    'rt_adaptive_budget_select[nx=65536,ny=65537]': -1,
    'rt_adaptive_budget_select[ctx=None,state=None]': -1,
    'rt_adaptive_budget_select_filtered[ctx=None]': -1,
    'rt_adaptive_budget_select_filtered[B=Bbad]': -1,
    'rt_adaptive_budget_select_filtered[B=None]': -1,
    'rt_adaptive_budget_select_filtered[picks=-1]': -1,
    'rt_adaptive_budget_select_filtered[picks=4294967296]': -1,
    'rt_adaptive_budget_select_filtered[nx=0]': -1,
    'rt_adaptive_budget_select_filtered[state=None]': -1,
    'rt_adaptive_budget_select_filtered[list=None]': -1,
    'rt_adaptive_budget_select_filtered[count=None]': -1,
    'rt_adaptive_budget_select_filtered[nx=65536,ny=65537]': -1,
    'rt_adaptive_budget_select_filtered[ctx=None,state=None]': -1,
    'rt_adaptive_budget_select[part=bad]': -1,
    'rt_adaptive_budget_select[part=beyond]': -1,
    'rt_adaptive_budget_select[state=None,part=empty]': 0,
    'rt_adaptive_budget_select[list=None,count=None,part=empty]': 0,
    'rt_adaptive_budget_select[B=Bbad,part=empty]': -1,
    'rt_adaptive_budget_select[picks=-1,part=empty]': -1,
    'rt_adaptive_budget_select[nx=65536,ny=65537,state=None]': -1,
    'rt_adaptive_budget_select_filtered[F=Fbad]': -1,
    'rt_adaptive_budget_select_filtered[F=None]': -1,
    'rt_adaptive_budget_select_filtered[hits=None]': -1,
    'rt_adaptive_budget_select_filtered[hits=4104]': -1,
    'rt_adaptive_budget_select_filtered[B=Bbad,F=Fbad]': -1,
    'rt_adaptive_budget_select_filtered[F=Fbad,state=None]': -1,
    'rt_adaptive_budget_select_filtered[F=Fbad,hits=4104]': -1,
    'rt_adaptive_budget_select_filtered[keys=None,hits=None]': -1,
    'rt_split_balanced[world=None]': -1,
    'rt_split_balanced[starts=None]': -1,
    'rt_split_balanced[nx=0]': -1,
    'rt_split_balanced[nparts=0]': -1,
    'rt_split_balanced[nparts=65]': -1,
    'rt_split_balanced[oct=o16]': -1,
    'rt_split_balanced[world=w16,oct=o]': -1,
    'rt_split_balanced[nx=8,ny=8,nparts=2]': -1,
    'rt_split_balanced[nx=8,ny=8,nparts=2,oct=o16]': -1,
    'rt_split_balanced[nparts=41]': -1,
    'rt_split_balanced[ctx=None,world=None]': -1,
}


@pytest.fixture(scope="module")
def E(rt):
    return env(rt)


def test_the_table_is_complete():
    ids = [case_id(fn, f) for fn, f in CASES]
    assert len(set(ids)) == len(ids) and set(ids) == set(EXPECTED)
    assert set(EXPECTED.values()) <= {0, RT_EINVAL, RT_ENOTSUP}
    # 0 only ever for a part without tiles: no case gets past the refusals
    assert all("part=empty" in k for k, v in EXPECTED.items() if v == 0)
    for name in list(ARGS) + [f + "_on" for f in FRAME]:
        assert any(fn == name for fn, _ in CASES), name


@pytest.mark.parametrize("fn,faults", CASES, ids=[case_id(fn, f) for fn, f in CASES])
def test_refusal(rt, E, fn, faults):
    assert run_case(rt, E, fn, faults) == EXPECTED[case_id(fn, faults)]


def test_a_null_context_is_refused_by_every_on_form(rt, E):
    for fn in FRAME:
        assert run_case(rt, E, fn + "_on", dict(ctx=None)) == RT_EINVAL
        assert run_case(rt, E, fn + "_on", dict(ctx=None, part="empty") if fn in HAS_PART else dict(ctx=None, world="w16")) == RT_EINVAL
