"""Exhaustive GPU check that the single-rounding sampling forms of csrc/rt_sampling.h give the reference's bits (the package
Makefile's `all` target, which __graft_entry__.build() runs, builds tools/micro/exact_forms from the kernels' own header)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_fused_sampling_forms_equal_the_two_rounding_forms_for_all_draws(cuda):
    """rng_uniform forms (float)X * 2^-32 + 2^-33 and the rejection loops 2x - 1 with one fused multiply-add each (the product is
    exact: tests/test_sampling_forms_host.py).  tools/micro/exact_forms compares both against the reference's two-step forms for all
    2^32 values of X — and 2x - 1 on every value the draw can return — as bit patterns; exit code 0 = no value differs."""
    exe = os.path.join(ROOT, "tools", "micro", "exact_forms")
    assert os.access(exe, os.X_OK), "tools/micro/exact_forms is missing: __graft_entry__.build() builds it (make all)"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all 2^32 draws: 0 uniform values differ" in p.stdout and ", 0 values of 2x-1 differ" in p.stdout, p.stdout
    assert "u in [0x1p-33, 0x1p+0]" in p.stdout, p.stdout
