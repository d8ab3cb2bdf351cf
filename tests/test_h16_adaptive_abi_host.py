"""include/rt_amd_h16_adaptive.h - adaptive sampling of binary16 worlds, the header rt_amd.h includes last - against the binding, without
a GPU, by the rules tests/test_fused_abi_host.py applies to rt_amd_fused.h: every prototype of the file is bound in
rt_amd.SYMBOLS_H16_ADAPTIVE with the header's types and exported by the library, nothing else is in that table, the table shares no name
with the other four, RT_ABI_VERSION stays 6, a C and a C++ program see the declarations from rt_amd.h alone and from the new header
alone, and the argument lists are those of the fused call.  Then the refusals that come before any device work, in the header's
order, on worlds created on the host and placeholder pointers."""
import ctypes as C
import os
import re
import subprocess

import pytest

import abi_header

INCLUDE = os.path.dirname(abi_header.HEADER)
HEADER = os.path.join(INCLUDE, "rt_amd_h16_adaptive.h")
NAMES = {"rt_render_adaptive_h16", "rt_render_adaptive_h16_on"}
FAKE = C.c_void_p(0x1000)          # never dereferenced: the calls below refuse before they touch a buffer
NX, NY = 64, 40                    # 8 x 5 = 40 tiles
WHOLE = (0, 1, 0, 0)
EINVAL, ENOTSUP = -1, -4


def params(rt, **kw):
    p = dict(min_spp=4, max_spp=32, batch=4, rel_error=0.2, floor=0.01)
    p.update(kw)
    return rt.Adaptive(**p)


def first(rt, world, p, part=WHOLE, on=False, ctx=FAKE, fb=FAKE, st=FAKE, octree=None, nx=NX, ny=NY):
    """the code of rt_render_adaptive_h16(_on)"""
    L = rt.lib()
    tail = (fb, nx, ny, C.byref(p) if p is not None else None, world.h if world is not None else None, st, octree, None, None, rt.Partition(*part), None)
    return L.rt_render_adaptive_h16_on(ctx, *tail) if on else L.rt_render_adaptive_h16(*tail)


@pytest.fixture(scope="module")
def w32(rt):
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
    assert added == NAMES == set(rt.SYMBOLS_H16_ADAPTIVE)
    assert set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", own, flags=re.S))) == NAMES, "a declaration was lost"
    others = set(rt.SYMBOLS) | set(rt.SYMBOLS_REBUILD) | set(rt.SYMBOLS_FUSED) | set(rt.SYMBOLS_REFINE_FUSED)
    assert not set(rt.SYMBOLS_H16_ADAPTIVE) & others
    L = rt.lib()
    assert L.rt_abi_version() == 6 == abi_header.DEFINES["RT_ABI_VERSION"]          # these are additions: the version stays
    for name in NAMES:
        assert tuple(rt.SYMBOLS_H16_ADAPTIVE[name]) == prototypes[name], "%s: binding %s, header %s" % (name, rt.SYMBOLS_H16_ADAPTIVE[name], prototypes[name])
        assert hasattr(L, name), "librt_amd.so does not export %s" % name
        fn = getattr(L, name)
        assert fn.restype is prototypes[name][0] and list(fn.argtypes) == prototypes[name][1]
    # the call takes the fused call's arguments, in their order
    for mine, theirs, header in (("rt_render_adaptive_h16", "rt_render_adaptive_fused", "rt_amd_fused.h"),):
        f_protos, f_names = abi_header.parse(main + "\n" + open(os.path.join(INCLUDE, header)).read())[:2]
        for stem in ("", "_on"):
            assert names[mine + stem] == f_names[theirs + stem]
            assert prototypes[mine + stem] == f_protos[theirs + stem]


def test_rt_amd_h_brings_the_declarations_along(tmp_path):
    """in C and in C++, from rt_amd.h alone and from rt_amd_h16_adaptive.h alone, in either order"""
    text = open(abi_header.HEADER).read()
    assert re.search(r'^#include "rt_amd_h16_adaptive.h"', text, re.M)
    assert text.index('#include "rt_amd_refine_fused.h"') < text.index('#include "rt_amd_h16_adaptive.h"')
    use = ("int use(void* fb, const rt_adaptive* p, const rt_world* w, rt_rand_state* s, rt_render_ctx* c, void* state, rt_partition part) {\n"
           "    return rt_render_adaptive_h16(fb, 8, 8, p, w, s, 0, 0, state, part, 0) + rt_render_adaptive_h16_on(c, fb, 8, 8, p, w, s, 0, 0, state, part, 0); }\n")
    for k, first_ in enumerate((['rt_amd.h'], ['rt_amd_h16_adaptive.h'], ['rt_amd_h16_adaptive.h', 'rt_amd.h'], ['rt_amd.h', 'rt_amd_h16_adaptive.h'],
                                ['rt_amd_refine_fused.h', 'rt_amd_h16_adaptive.h'])):
        for compiler, ext in (("gcc", "c"), ("g++", "cpp")):
            src = tmp_path / ("use%d.%s" % (k, ext))
            src.write_text("".join('#include "%s"\n' % h for h in first_) + use)
            p = subprocess.run([compiler, "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True, timeout=120)
            assert p.returncode == 0, (first_, compiler, p.stderr[-2000:])


def test_the_binding_has_the_calls(rt):
    assert callable(rt.render_adaptive_h16) and callable(rt.RenderCtx.render_adaptive_h16)


# ---- the refusals, in the header's order ------------------------------------------------------------------------------------
BAD_PARAMS = [dict(max_spp=18), dict(min_spp=0, max_spp=16), dict(batch=0), dict(rel_error=-0.1), dict(floor=-1.0), dict(min_spp=1, max_spp=5),
              dict(max_spp=2), dict(rel_error=float("nan"))]


@pytest.mark.parametrize("on", [False, True])
def test_1_parameters_sizes_and_partitions(rt, w16, w32, on):
    """RT_EINVAL, on a binary16 world and — before the precision is looked at — on a binary32 one"""
    for W in (w16, w32):
        for kw in BAD_PARAMS:
            assert first(rt, W, params(rt, **kw), on=on) == EINVAL, kw
        assert first(rt, W, None, on=on) == EINVAL
        ok = params(rt)
        for kw in (dict(nx=0), dict(ny=-3), dict(part=(2, 2, 0, 0)), dict(part=(0, 0, 0, 0)), dict(part=(0, 2, 30, 41)), dict(part=(0, 1, 5, 3)),
                   dict(nx=1 << 17, ny=1 << 17)):                                 # the last: 2^34 elements, more than 2^32 - 1
            assert first(rt, W, ok, on=on, **kw) == EINVAL, kw
    assert first(rt, None, params(rt), on=on) == EINVAL


def test_2_a_part_without_tiles_is_a_no_op(rt):
    """more parts than tiles: 0 before a buffer or the precision is looked at (8x8 frame: one tile), on either kind of world"""
    for prec in (rt.FP16, rt.FP32):
        W = rt.World(22, 8, 8, precision=prec)
        kw = dict(part=(2, 3, 0, 0), fb=None, st=None, nx=8, ny=8)
        for on in (False, True):
            assert first(rt, W, params(rt), on=on, **kw) == 0
        W.close()


@pytest.mark.parametrize("on", [False, True])
def test_3_null_pointers_and_a_tree_of_the_other_precision(rt, w16, w32, on):
    p = params(rt)
    for W in (w16, w32):                                                           # a binary32 world too: before RT_ENOTSUP
        assert first(rt, W, p, on=on, fb=None) == EINVAL and first(rt, W, p, on=on, st=None) == EINVAL
    t32, t16 = rt.Octree(w32, 30), rt.Octree(w16, 30)                              # built on the host, never uploaded
    assert first(rt, w16, p, on=on, octree=t32.h) == EINVAL
    assert first(rt, w32, p, on=on, octree=t16.h) == EINVAL
    assert first(rt, w32, p, on=on, octree=t32.h) == ENOTSUP                        # a matching tree passes on to the precision
    t32.close()
    t16.close()


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("part", [(0, 1, 0, 0), (0, 3, 0, 0), (1, 2, 20, 40)], ids=["whole", "runs", "range"])
def test_4_worlds_that_are_not_binary16_are_not_supported(rt, w32, part, on):
    p = params(rt)
    assert first(rt, w32, p, part, on) == ENOTSUP
    wc = rt.World(500, NX, NY)
    wc.set_arith(rt.ARITH_CONTRACT)
    assert first(rt, wc, p, part, on) == ENOTSUP
    wc.close()


def test_6_the_on_forms_need_a_context(rt, w16, w32):
    for W in (w16, w32):
        assert first(rt, W, params(rt), on=True, ctx=None) == EINVAL


def test_the_existing_calls_still_refuse_binary16(rt, w16):
    """nothing that existed changes its answer for a binary16 world"""
    L = rt.lib()
    p, q = params(rt), params(rt, rel_error=0.1)
    part = rt.Partition(*WHOLE)
    assert L.rt_render_adaptive_fused(FAKE, NX, NY, C.byref(p), w16.h, FAKE, None, None, None, part, None) == ENOTSUP
    assert L.rt_render_adaptive_begin(FAKE, NX, NY, C.byref(p), w16.h, FAKE, None, None, FAKE, part, None) == ENOTSUP
    assert L.rt_render_adaptive_refine_fused(FAKE, NX, NY, C.byref(p), C.byref(q), w16.h, FAKE, None, None, FAKE, part, None) == ENOTSUP
    assert L.rt_render_adaptive_part(FAKE, NX, NY, C.byref(p), w16.h, FAKE, None, None, part, None) == ENOTSUP


def test_kernel_names(rt, w16, w32):
    """rt_render_kernel_name on a binary16 world names the kernel of the call; mode 4 stays binary32's (no device is touched)"""
    t16 = rt.Octree(w16, 30)
    for mode in (0, 1, 3):
        assert rt.render_kernel_name(w16, t16, mode) == "k_render_h<true,%d>" % mode
        assert rt.render_kernel_name(w16, None, mode) == "k_render_h<false,%d>" % mode
    buf = C.create_string_buffer(64)
    assert rt.lib().rt_render_kernel_name(w16.h, None, 2, buf, 64) == EINVAL
    assert rt.lib().rt_render_kernel_name(w16.h, None, 4, buf, 64) == ENOTSUP and rt.lib().rt_render_kernel_name(w16.h, t16.h, 4, buf, 64) == ENOTSUP
    assert rt.render_kernel_name(w32, None, 3).startswith("k_render<") and rt.render_kernel_name(w32, None, 4).startswith("k_render<")
    t16.close()
