"""The layout of the test tree itself (CPU only, no GPU, no library): test modules are nobody's library, the helpers that were
unified are written once, and tools/kernel_trace.py reads a trace as the study tools expect."""
import ast
import functools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS, TOOLS = os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")

# the helpers that have one home (tests/bitcmp.py, gpu_frames.py, adaptive_frames.py, world_cases.py, temporal_paths.py, tree_compare.py,
# reference_cases.py); the comparison and view names that were retired must not come back as a second definition either
ONE_HOME = ["f32_bits", "raw_bits", "same_nan_as_ref", "same_any_nan", "assert_same_snapshots", "u32",
            "render_frame", "frame_rows", "frame_image", "states_of", "gpu_render", "whole_frame", "gpu_frame",
            "state_parts", "make_state", "part_tile", "part_layout", "inside_frame", "layout_inside", "Scene", "check_exact", "model_pick",
            "check_round", "check_round_filtered", "check_round_temporal", "stop_rule_model", "progressive_samples", "adaptive_frame",
            "random_world", "random_rays", "lattice_rays", "orbit_camera", "half_bits", "f32_to_half_bits",
            "Path", "Animation", "compare_empty", "world_of"]


@functools.lru_cache(None)
def parsed(d):
    """[(path from the root, module tree)] of every .py below d, parsed once for all tests"""
    out = []
    for base, _, files in os.walk(d):
        for f in sorted(files):
            if f.endswith(".py"):
                path = os.path.join(base, f)
                with open(path) as fi:
                    out.append((os.path.relpath(path, ROOT), ast.parse(fi.read(), path)))
    return out


def sources(*dirs):
    return [x for d in dirs for x in parsed(d)]


def statements(tree):
    """every statement of a module, nested ones included (an import is a statement: expressions need no visit)"""
    stack = [tree]
    while stack:
        node = stack.pop()
        yield node
        for field in ("body", "orelse", "finalbody", "handlers", "cases"):
            stack.extend(x for x in getattr(node, field, ()) if isinstance(x, ast.AST))


def test_no_module_imports_a_test_module():
    bad = []
    for path, tree in sources(TESTS, TOOLS):
        for node in statements(tree):                            # (imports inside functions included)
            names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            bad += ["%s:%d imports %s" % (path, node.lineno, n) for n in names if n.split(".")[-1].startswith("test_")]
    assert not bad, bad


def test_unified_helpers_are_defined_once():
    where = {}
    for path, tree in sources(TESTS):
        for node in tree.body:                                   # module level: a method or a nested function of that name is not a helper
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in ONE_HOME:
                where.setdefault(node.name, []).append(path)
    twice = {name: paths for name, paths in where.items() if len(paths) > 1}
    assert not twice, twice
    for name in ("state_parts", "make_state", "random_world", "random_rays", "lattice_rays", "orbit_camera", "f32_bits", "raw_bits",
                 "same_nan_as_ref", "same_any_nan", "assert_same_snapshots", "render_frame", "frame_rows", "frame_image"):
        assert len(where.get(name, [])) == 1, name               # (and the list names things that exist)


def test_bit_views_and_comparisons_mean_what_their_names_say():
    """tests/bitcmp.py on hand-written arrays.  The suites that use the comparisons only ever show them equal frames, so what they
    REJECT is stated here: a number where the reference has a NaN, a NaN where it has a number, another shape, one differing bit."""
    import numpy as np
    import bitcmp
    nan, nan2 = np.float32(np.nan), np.array([0x7FC0DEAD], np.uint32).view(np.float32)[0]
    ref = np.array([[1.0, nan], [-0.0, 3.0]], np.float32)
    got = ref.copy()
    got[0, 1] = nan2                                             # another payload: still "NaN where the reference has NaN"
    assert bitcmp.same_nan_as_ref(got, ref) and bitcmp.same_any_nan(got, ref)
    assert not bitcmp.same_nan_as_ref(np.array([[1.0, 2.0], [-0.0, 3.0]], np.float32), ref)       # a number where the reference has NaN
    assert not bitcmp.same_nan_as_ref(got.reshape(4), ref)                                        # the shape is part of it
    assert not bitcmp.same_nan_as_ref(np.array([[1.0, nan], [0.0, 3.0]], np.float32), ref)        # -0.0 and 0.0 differ in a bit
    extra = ref.copy()
    extra[1, 1] = nan
    assert not bitcmp.same_nan_as_ref(extra, ref) and not bitcmp.same_any_nan(extra, ref)         # a NaN where the reference has a number
    # the two views: an integer array is converted by VALUE in one and keeps its own pattern in the other
    k = np.array([1, 2], np.int32)
    assert bitcmp.f32_bits(k).tolist() == [0x3F800000, 0x40000000] and bitcmp.raw_bits(k).tolist() == [1, 2]
    x = np.array([1.0, -2.0], np.float32)
    assert np.array_equal(bitcmp.f32_bits(x), bitcmp.raw_bits(x)) and bitcmp.f32_bits([1.0]).dtype == np.uint32
    assert bitcmp.f32_bits(np.array([1.0], np.float64)).tolist() == [0x3F800000]
    # snapshot dicts: the failure names the key
    a, b = dict(fb=np.zeros(3), spp=np.arange(3)), dict(fb=np.zeros(3), spp=np.array([0, 1, 3]))
    bitcmp.assert_same_snapshots(a, dict(a))
    with pytest.raises(AssertionError, match="spp"):
        bitcmp.assert_same_snapshots(a, b, "part 0")


TRACE = """"Kind","Agent_Id","Queue_Id","Kernel_Id","Kernel_Name","Correlation_Id","Start_Timestamp","End_Timestamp"
"KERNEL_DISPATCH",1,1,7,"void rt::k_denoise_var_level<true, 1>(float4 const*, float4*)",4,4000,4900
"KERNEL_DISPATCH",1,1,3,"void rt::k_temporal_accumulate(rt::TemporalArgs)",1,1000,1250
"KERNEL_DISPATCH",1,1,7,"_ZN2rt19k_denoise_var_levelILb1ELi1EEEvPK6float4PS1_",6,6000,6700
"KERNEL_DISPATCH",1,1,8,"void rt::k_denoise_var_level<true, 2>(float4 const*, float4*)",3,3000,3100
"KERNEL_DISPATCH",1,1,7,"rt::k_denoise_var_level<true,1>(float4 const*, float4*)",5,5000,5500
"KERNEL_DISPATCH",1,1,9,"void rt::k_denoise_var_level<false, 1>(float4 const*, float4*)",2,2000,2003
"KERNEL_DISPATCH",1,1,3,"void rt::k_temporal_accumulate(rt::TemporalArgs)",7,7000,7125
"""


def test_kernel_trace_reader(tmp_path):
    sys.path.insert(0, TOOLS)
    try:
        import kernel_trace
    finally:
        sys.path.remove(TOOLS)
    d = tmp_path / "run" / "host" / "123"
    d.mkdir(parents=True)
    (d / "123_kernel_trace.csv").write_text(TRACE)
    ev = kernel_trace.read_trace(str(tmp_path))
    # start order, whatever the order of the rows; durations in us
    assert [us for _, us in ev] == [0.25, 0.003, 0.1, 0.9, 0.5, 0.7, 0.125]
    assert [kernel_trace.short_name(n) for n, _ in ev][:3] == ["k_temporal_accumulate", "k_denoise_var_level<false, 1>", "k_denoise_var_level<true, 2>"]
    # one instantiation under its three spellings, and nothing else: not <true, 2>, not <false, 1>
    assert kernel_trace.durations(ev, "k_denoise_var_level", True, 1) == [0.9, 0.5, 0.7]
    assert kernel_trace.durations(ev, "k_denoise_var_level", True, 2) == [0.1]
    assert kernel_trace.durations(ev, "k_denoise_var_level", False, 1) == [0.003]
    assert kernel_trace.durations(ev, "k_temporal_accumulate") == [0.25, 0.125]         # by name alone: the unrelated kernel
    assert kernel_trace.durations(ev, "k_denoise_var_level") == [0.003, 0.1, 0.9, 0.5, 0.7]
    assert not kernel_trace.is_instance(ev[0][0], "k_denoise_var_level", True, 1)
    with pytest.raises(IndexError):
        kernel_trace.read_trace(str(tmp_path / "run" / "nothing_here"))
