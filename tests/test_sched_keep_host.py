"""The kept schedule's decision logic (csrc/rt_sched_keep.h: plain host C++, no HIP) as a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer on the CPU (tests/host/sched_keep_check.cpp): keys that differ in one field at a time, every way a record
is dropped or bypassed (a miss drops it before the pass is launched, a regrown or freed workspace, a stream capture and the context's
life after it, the RT_SCHED_CACHE switch), and that a failed pass leaves no valid record.  Also: the header stays free of HIP, and the
library's two reuse counters are declared, exported and bound."""
import ctypes as C
import os
import re
import subprocess

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dd2360-raytracing_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_decision_logic_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sched_keep_check")
    p = subprocess.run(["g++"] + SAN + ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "host", "sched_keep_check.cpp")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    assert "sched_keep_host: ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]


def test_the_header_includes_no_hip():
    # (rt_variant.h: the walk variants' names, which the feedback gate asks; itself plain C++ that includes nothing)
    for name, includes in (("rt_sched_keep.h", ["cstdint", "rt_variant.h"]), ("rt_variant.h", [])):
        src = open(os.path.join(CSRC, name)).read()
        assert re.findall(r"#include\s*[<\"]([^>\"]+)", src) == includes, name
        assert "__device__" not in src and "__global__" not in src and "hipStream" not in src, name


def test_reuse_counters_are_declared_exported_and_bound(rt):
    assert abi_header.DEFINES["RT_ABI_VERSION"] == 6 and rt.lib().rt_abi_version() == 6
    for name, handle in (("rt_render_ctx_schedule_reuse", "rt_render_ctx*"), ("rt_world_render_schedule_reuse", "rt_world*")):
        assert abi_header.PARAM_C_TYPES[name] == [handle, "uint64_t*", "uint64_t*"] and abi_header.PARAM_NAMES[name][1:] == ["reused", "computed"], name
        assert abi_header.PROTOTYPES[name][0] is C.c_int
        abi_header.check_bound(rt, [name])
    W = rt.World(22, 64, 40)
    try:
        assert W.schedule_reuse() == (0, 0)                  # host counters: no device needed
        assert rt.lib().rt_world_render_schedule_reuse(W.h, None, None) == -1 and rt.lib().rt_render_ctx_schedule_reuse(None, None, None) == -1
    finally:
        W.close()
    assert "RT_SCHED_CACHE" in open(os.path.join(CSRC, "rt_tuning.h")).read()
