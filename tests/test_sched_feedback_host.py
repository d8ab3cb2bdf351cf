"""The measured pass's decision (csrc/rt_sched_keep.h "Feedback": plain host C++, no HIP) as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer on the CPU (tests/host/sched_feedback_check.cpp): the gate, record / rebuild / reuse,
one rebuild per record, every way the counts end (another key, a regrown or freed workspace, a capture, the two switches), a
recording launch whose render kernel failed, and that a failed rebuild leaves no valid record.  Also: the new entry points are
declared, exported and bound, and the knobs are in rt_tuning.h."""
import ctypes as C
import os
import subprocess

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dd2360-raytracing_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_refinement_decision_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sched_feedback_check")
    p = subprocess.run(["g++"] + SAN + ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "host", "sched_feedback_check.cpp")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    assert "sched_feedback_host: ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]


def test_feedback_entry_points_are_declared_exported_and_bound(rt):
    assert abi_header.DEFINES["RT_FEEDBACK_WORDS"] == 4 and len(rt.FEEDBACK_FIELDS) == 4
    for stem, handle in (("rt_render_ctx", "rt_render_ctx*"), ("rt_world_render", "rt_world*")):
        for name, types, names in ((stem + "_schedule_feedback", ["uint64_t*", "uint32_t*", "int"], ["refined", "out", "n"]),
                                   (stem + "_schedule_counts", ["uint16_t*", "int64_t"], ["out", "n"])):
            assert abi_header.PARAM_C_TYPES[name] == [handle] + types and abi_header.PARAM_NAMES[name][1:] == names, name
            assert abi_header.PROTOTYPES[name][0] is C.c_int
            abi_header.check_bound(rt, [name])
    W = rt.World(22, 64, 40)
    try:
        f = W.schedule_feedback()                            # host state: no device needed before any launch
        assert (f["refined"], f["has_counts"], f["rebuilt"], f["max_count"], f["solo_cap"]) == (0, 0, 0, 0, 0)
        assert rt.lib().rt_world_render_schedule_feedback(W.h, None, None, 0) == -1 and rt.lib().rt_render_ctx_schedule_feedback(None, None, None, 0) == -1
        assert rt.lib().rt_world_render_schedule_counts(W.h, None, 0) == -1
    finally:
        W.close()
    tuning = open(os.path.join(CSRC, "rt_tuning.h")).read()
    for knob in ("RT_SCHED_FEEDBACK", "RT_FEEDBACK_MIN_NS", "RT_FB_SOLO_FRAC", "RT_FB_SOLO_CAP_DEN"):
        assert "#define %s " % knob in tuning, knob
