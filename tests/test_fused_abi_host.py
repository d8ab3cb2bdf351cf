"""include/rt_amd_fused.h - the declarations of the fused adaptive frame, which rt_amd.h includes at its end - against the binding,
without a GPU, by the rules tests/test_rebuild_abi_host.py applies to rt_amd_rebuild.h (tests/abi_header.py reads the files): every
prototype of the file is bound in rt_amd.SYMBOLS_FUSED with the header's types and exported by the library, nothing else is in that
table, RT_ABI_VERSION stays 6, a C and a C++ program that include rt_amd.h alone see the declarations, and rt_sequence refuses an
unknown value of its key `adaptive` before it touches a device."""
import os
import re
import subprocess

import abi_header

INCLUDE = os.path.dirname(abi_header.HEADER)
FUSED_HEADER = os.path.join(INCLUDE, "rt_amd_fused.h")
NAMES = {"rt_render_adaptive_fused", "rt_render_adaptive_fused_on", "rt_multi_set_adaptive_fused"}
EXE = os.path.join(os.path.dirname(INCLUDE), "dd2360-raytracing_amd", "rt_sequence")


def test_the_fused_header_is_bound_whole(rt):
    own = open(FUSED_HEADER).read()
    # the handles' typedefs are rt_amd.h's: the two files are read as the one text a compiler sees (one extern "C" block around both)
    main = re.sub(r"#ifdef __cplusplus\s*\}\s*#endif", " ", open(abi_header.HEADER).read())
    prototypes = abi_header.parse(main + "\n" + own)[0]
    added = set(prototypes) - set(abi_header.PROTOTYPES)
    assert added == NAMES == set(rt.SYMBOLS_FUSED)
    assert set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", own, flags=re.S))) == NAMES, "a declaration was lost"
    assert not set(rt.SYMBOLS_FUSED) & (set(rt.SYMBOLS) | set(rt.SYMBOLS_REBUILD))
    L = rt.lib()
    assert L.rt_abi_version() == 6 == abi_header.DEFINES["RT_ABI_VERSION"]          # these are additions: the version stays
    for name in NAMES:
        assert tuple(rt.SYMBOLS_FUSED[name]) == prototypes[name], "%s: binding %s, header %s" % (name, rt.SYMBOLS_FUSED[name], prototypes[name])
        assert hasattr(L, name), "librt_amd.so does not export %s" % name
        fn = getattr(L, name)
        assert fn.restype is prototypes[name][0] and list(fn.argtypes) == prototypes[name][1]
    # the fused call takes rt_render_adaptive_begin's arguments, in its order (the contract is stated against begin)
    for stem in ("", "_on"):
        assert abi_header.parse(main + "\n" + own)[1]["rt_render_adaptive_fused" + stem] == abi_header.PARAM_NAMES["rt_render_adaptive_begin" + stem]
        assert prototypes["rt_render_adaptive_fused" + stem] == abi_header.PROTOTYPES["rt_render_adaptive_begin" + stem]


def test_the_multi_switch_refuses_without_a_device(rt):
    """RT_EINVAL for a NULL handle, whatever the value (the accepted values need a handle: tests/test_gpu_multi_fused.py)"""
    for on in (0, 1, 2, -1):
        assert rt.lib().rt_multi_set_adaptive_fused(None, on) == -1


def test_rt_amd_h_brings_the_declarations_along(tmp_path):
    """in C and in C++, from rt_amd.h alone and from rt_amd_fused.h alone, in either order"""
    assert re.search(r'^#include "rt_amd_fused.h"', open(abi_header.HEADER).read(), re.M)
    use = ("int use(void* fb, const rt_adaptive* p, const rt_world* w, rt_rand_state* s, rt_render_ctx* c, rt_multi* m, rt_partition part) {\n"
           "    return rt_render_adaptive_fused(fb, 8, 8, p, w, s, 0, 0, 0, part, 0) + rt_render_adaptive_fused_on(c, fb, 8, 8, p, w, s, 0, 0, 0, part, 0)\n"
           "           + rt_multi_set_adaptive_fused(m, 1); }\n")
    for k, first in enumerate((['rt_amd.h'], ['rt_amd_fused.h'], ['rt_amd_fused.h', 'rt_amd.h'], ['rt_amd.h', 'rt_amd_fused.h'],
                               ['rt_amd_rebuild.h', 'rt_amd_fused.h'])):
        for compiler, ext in (("gcc", "c"), ("g++", "cpp")):
            src = tmp_path / ("use%d.%s" % (k, ext))
            src.write_text("".join('#include "%s"\n' % h for h in first) + use)
            p = subprocess.run([compiler, "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)], capture_output=True, text=True, timeout=120)
            assert p.returncode == 0, (first, compiler, p.stderr[-2000:])


def test_rt_sequence_refuses_an_unknown_adaptive_before_any_device_work(rt, tmp_path):
    """exit code 99 and one line that names the key and its two values; nothing of the device's appears, nothing is written"""
    for tokens, why in ((["adaptive=foo"], "neither rounds nor fused"), (["adaptive="], "neither rounds nor fused"),
                        (["mode=progressive", "adaptive=fused"], "no adaptive frame")):
        p = subprocess.run([EXE] + tokens, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert p.returncode == 99, (tokens, p.returncode, p.stderr)
        assert re.match(r"rt_sequence: adaptive: ", p.stderr) and why in p.stderr, p.stderr
        assert "rt_device_check" not in p.stderr and "spheres of radius" not in p.stderr and len(p.stderr.splitlines()) == 1
        assert os.listdir(tmp_path) == []
