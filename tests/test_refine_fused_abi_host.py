"""include/rt_amd_refine_fused.h - the declarations of the refinement in one render launch, which rt_amd.h includes last - against the
binding, without a GPU, by the rules tests/test_fused_abi_host.py applies to rt_amd_fused.h: every prototype of the file is bound in
rt_amd.SYMBOLS_REFINE_FUSED with the header's types and exported by the library, nothing else is in that table, RT_ABI_VERSION stays 6,
and a C and a C++ program see the declarations from rt_amd.h alone and from the new header alone.  Then the refusals that come before
any device work, on a world created on the host and placeholder pointers: rt_render_adaptive_refine_fused answers every case as
rt_render_adaptive_refine does - the pairs are the BAD and GOOD tables of tests/test_adaptive_refine_host.py, read from that file."""
import ast
import ctypes as C
import os
import re
import subprocess

import pytest

import abi_header

INCLUDE = os.path.dirname(abi_header.HEADER)
HEADER = os.path.join(INCLUDE, "rt_amd_refine_fused.h")
NAMES = {"rt_render_adaptive_refine_fused", "rt_render_adaptive_refine_fused_on"}
FAKE = C.c_void_p(0x1000)          # never dereferenced: the calls below refuse before they touch a buffer
NX, NY = 64, 40                    # 8 x 5 = 40 tiles
WHOLE = (0, 1, 0, 0)
EINVAL, ENOTSUP = -1, -4


def pair_tables():
    """BAD and GOOD as tests/test_adaptive_refine_host.py assigns them (a test module is nobody's library: its two assignments are
    evaluated here, nothing of it is imported)"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_adaptive_refine_host.py")
    out = {}
    for node in ast.parse(open(path).read(), path).body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and getattr(node.targets[0], "id", None) in ("BAD", "GOOD"):
            out[node.targets[0].id] = eval(compile(ast.Expression(node.value), path, "eval"), {"dict": dict, "float": float})
    return out["BAD"], out["GOOD"]


BAD, GOOD = pair_tables()


def params(rt, **kw):
    p = dict(min_spp=4, max_spp=32, batch=4, rel_error=0.2, floor=0.01)
    p.update(kw)
    return rt.Adaptive(**p)


def both(rt, world, frm, to, part=WHOLE, on=False, state=FAKE, ctx=FAKE):
    """the codes of rt_render_adaptive_refine and rt_render_adaptive_refine_fused for one set of arguments"""
    L = rt.lib()
    a = C.byref(frm) if frm is not None else None
    b = C.byref(to) if to is not None else None
    tail = (FAKE, NX, NY, a, b, world.h, FAKE, None, None, state, rt.Partition(*part), None)
    if on:
        return L.rt_render_adaptive_refine_on(ctx, *tail), L.rt_render_adaptive_refine_fused_on(ctx, *tail)
    return L.rt_render_adaptive_refine(*tail), L.rt_render_adaptive_refine_fused(*tail)


@pytest.fixture(scope="module")
def world(rt):
    W = rt.World(500, NX, NY)
    yield W
    W.close()


@pytest.fixture(scope="module")
def w16(rt):
    W = rt.World(500, NX, NY, precision=rt.FP16)
    yield W
    W.close()


def test_the_header_is_bound_whole(rt):
    own = open(HEADER).read()
    main = re.sub(r"#ifdef __cplusplus\s*\}\s*#endif", " ", open(abi_header.HEADER).read())
    prototypes, names = abi_header.parse(main + "\n" + own)[:2]
    added = set(prototypes) - set(abi_header.PROTOTYPES)
    assert added == NAMES == set(rt.SYMBOLS_REFINE_FUSED)
    assert set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", own, flags=re.S))) == NAMES, "a declaration was lost"
    assert not set(rt.SYMBOLS_REFINE_FUSED) & (set(rt.SYMBOLS) | set(rt.SYMBOLS_REBUILD) | set(rt.SYMBOLS_FUSED))
    L = rt.lib()
    assert L.rt_abi_version() == 6 == abi_header.DEFINES["RT_ABI_VERSION"]          # these are additions: the version stays
    for name in NAMES:
        assert tuple(rt.SYMBOLS_REFINE_FUSED[name]) == prototypes[name], "%s: binding %s, header %s" % (name, rt.SYMBOLS_REFINE_FUSED[name], prototypes[name])
        assert hasattr(L, name), "librt_amd.so does not export %s" % name
        fn = getattr(L, name)
        assert fn.restype is prototypes[name][0] and list(fn.argtypes) == prototypes[name][1]
    # the call takes rt_render_adaptive_refine's arguments, in its order (the contract is stated against it)
    for stem in ("", "_on"):
        assert names["rt_render_adaptive_refine_fused" + stem] == abi_header.PARAM_NAMES["rt_render_adaptive_refine" + stem]
        assert prototypes["rt_render_adaptive_refine_fused" + stem] == abi_header.PROTOTYPES["rt_render_adaptive_refine" + stem]


def test_rt_amd_h_brings_the_declarations_along(tmp_path):
    """in C and in C++, from rt_amd.h alone and from rt_amd_refine_fused.h alone, in either order"""
    text = open(abi_header.HEADER).read()
    assert re.search(r'^#include "rt_amd_refine_fused.h"', text, re.M)
    assert text.index('#include "rt_amd_fused.h"') < text.index('#include "rt_amd_refine_fused.h"')
    use = ("int use(void* fb, const rt_adaptive* p, const rt_adaptive* q, const rt_world* w, rt_rand_state* s, rt_render_ctx* c, void* state, rt_partition part) {\n"
           "    return rt_render_adaptive_refine_fused(fb, 8, 8, p, q, w, s, 0, 0, state, part, 0)\n"
           "           + rt_render_adaptive_refine_fused_on(c, fb, 8, 8, p, q, w, s, 0, 0, state, part, 0); }\n")
    for k, first in enumerate((['rt_amd.h'], ['rt_amd_refine_fused.h'], ['rt_amd_refine_fused.h', 'rt_amd.h'], ['rt_amd.h', 'rt_amd_refine_fused.h'],
                               ['rt_amd_fused.h', 'rt_amd_refine_fused.h'])):
        for compiler, ext in (("gcc", "c"), ("g++", "cpp")):
            src = tmp_path / ("use%d.%s" % (k, ext))
            src.write_text("".join('#include "%s"\n' % h for h in first) + use)
            p = subprocess.run([compiler, "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True, timeout=120)
            assert p.returncode == 0, (first, compiler, p.stderr[-2000:])


def test_the_tables_are_the_refine_tests_tables():
    assert len(BAD) == 11 and len(GOOD) == 8 and "rel_raised" in BAD and "tighter" in GOOD


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("name", list(BAD))
def test_pairs_that_do_not_refine_are_refused(rt, world, w16, name, on):
    frm, to = BAD[name]
    assert both(rt, world, params(rt, **frm), params(rt, **to), on=on) == (EINVAL, EINVAL)
    assert both(rt, w16, params(rt, **frm), params(rt, **to), on=on) == (EINVAL, EINVAL)          # before the precision is looked at


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("name", list(GOOD))
def test_pairs_that_refine_pass_the_checks(rt, w16, name, on):
    """a binary16 world answers RT_ENOTSUP, not RT_EINVAL: the pair passed the rule"""
    frm, to = GOOD[name]
    assert both(rt, w16, params(rt, **frm), params(rt, **to), on=on) == (ENOTSUP, ENOTSUP)


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("part", [(0, 1, 0, 0), (0, 3, 0, 0), (1, 2, 20, 40)], ids=["whole", "runs", "range"])
def test_contracted_worlds_are_not_supported(rt, part, on):
    wc = rt.World(500, NX, NY)
    wc.set_arith(rt.ARITH_CONTRACT)
    assert both(rt, wc, params(rt), params(rt, rel_error=0.1), part, on) == (ENOTSUP, ENOTSUP)
    wc.close()


@pytest.mark.parametrize("on", [False, True])
def test_missing_state_and_arguments_are_refused(rt, world, on):
    p, q = params(rt), params(rt, rel_error=0.1)
    assert both(rt, world, p, q, on=on, state=None) == (EINVAL, EINVAL)
    assert both(rt, world, None, q, on=on) == (EINVAL, EINVAL)
    assert both(rt, world, p, None, on=on) == (EINVAL, EINVAL)
    assert both(rt, world, p, q, part=(2, 2, 0, 0), on=on) == (EINVAL, EINVAL)                    # invalid partition
    assert both(rt, world, p, q, part=(0, 2, 30, 41), on=on) == (EINVAL, EINVAL)                  # a range past the frame's 40 tiles


def test_the_on_form_needs_a_context(rt, world):
    assert both(rt, world, params(rt), params(rt, rel_error=0.1), on=True, ctx=None) == (EINVAL, EINVAL)


def test_part_without_tiles_is_a_no_op(rt):
    """more parts than tiles: a part that owns none returns 0 before it looks at a buffer (8x8 frame: one tile)"""
    L = rt.lib()
    W = rt.World(22, 8, 8)
    p, q = params(rt), params(rt, rel_error=0.1)
    tail = (None, 8, 8, C.byref(p), C.byref(q), W.h, None, None, None, None, rt.Partition(2, 3), None)
    assert L.rt_render_adaptive_refine(*tail) == 0 and L.rt_render_adaptive_refine_fused(*tail) == 0
    assert L.rt_render_adaptive_refine_on(FAKE, *tail) == 0 and L.rt_render_adaptive_refine_fused_on(FAKE, *tail) == 0
    W.close()
