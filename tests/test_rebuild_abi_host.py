"""include/rt_amd_rebuild.h - the declarations rt_amd.h includes at its end - against the binding, without a GPU, by the rules
tests/test_host_and_abi.py applies to rt_amd.h itself (tests/abi_header.py reads both): every prototype of the file is bound in
rt_amd.SYMBOLS_REBUILD with the header's types and exported by the library, nothing else is in that table, and a C and a C++ program
that include rt_amd.h alone see the declarations."""
import os
import re
import subprocess

import abi_header

REBUILD_HEADER = os.path.join(os.path.dirname(abi_header.HEADER), "rt_amd_rebuild.h")
NAMES = {"rt_octree_rebuild_gpu", "rt_octree_rebuild_info"}


def test_the_rebuild_header_is_bound_whole(rt):
    own = open(REBUILD_HEADER).read()
    # the handles' typedefs are rt_amd.h's: the two files are read as the one text a compiler sees (one extern "C" block around both)
    main = re.sub(r"#ifdef __cplusplus\s*\}\s*#endif", " ", open(abi_header.HEADER).read())
    prototypes = abi_header.parse(main + "\n" + own)[0]
    added = set(prototypes) - set(abi_header.PROTOTYPES)
    assert added == NAMES == set(rt.SYMBOLS_REBUILD)
    assert set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", own, flags=re.S))) == NAMES, "a declaration was lost"
    assert not set(rt.SYMBOLS_REBUILD) & set(rt.SYMBOLS)
    L = rt.lib()
    for name in NAMES:
        assert tuple(rt.SYMBOLS_REBUILD[name]) == prototypes[name], "%s: binding %s, header %s" % (name, rt.SYMBOLS_REBUILD[name], prototypes[name])
        assert hasattr(L, name), "librt_amd.so does not export %s" % name
        fn = getattr(L, name)
        assert fn.restype is prototypes[name][0] and list(fn.argtypes) == prototypes[name][1]


def test_rt_amd_h_brings_the_declarations_along(tmp_path):
    """in C and in C++, from rt_amd.h alone and from rt_amd_rebuild.h alone, in either order"""
    assert re.search(r'^#include "rt_amd_rebuild.h"', open(abi_header.HEADER).read(), re.M)
    use = "int use(rt_octree* t, const rt_world* w) { uint64_t a, b, c; return rt_octree_rebuild_gpu(t, w, 0) + rt_octree_rebuild_info(t, &a, &b, &c); }\n"
    for k, first in enumerate((['rt_amd.h'], ['rt_amd_rebuild.h'], ['rt_amd_rebuild.h', 'rt_amd.h'], ['rt_amd.h', 'rt_amd_rebuild.h'])):
        for compiler, ext in (("gcc", "c"), ("g++", "cpp")):
            src = tmp_path / ("use%d.%s" % (k, ext))
            src.write_text("".join('#include "%s"\n' % h for h in first) + use)
            p = subprocess.run([compiler, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(abi_header.HEADER), str(src)],
                               capture_output=True, text=True, timeout=120)
            assert p.returncode == 0, (first, compiler, p.stderr[-2000:])
