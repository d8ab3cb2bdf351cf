"""CPU test (not gpu): the render kernel refuses, at compile time, a slot interleave that does not divide 64.

k_tile_order starts the queue's sorted tail on a multiple of 64 tiles; k_render decodes the tiles' own slots in blocks of kIl tiles
(RT_INTERLEAVE / RT_INTERLEAVE_DENSE / RT_INTERLEAVE_SOLO).  A block that straddled the tail start would leave some pixels unrendered
and render others twice, so a `-D` override such as RT_INTERLEAVE=48 (tools/mkvariant.sh) must not build.  Each case is one
`hipcc -fsyntax-only` of csrc/rt_kernels.hip with the Makefile's flags for that translation unit."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dd2360-raytracing_amd")
MESSAGE = "must divide 64 (the tail starts on a multiple of 64 tiles)"


def makefile_var(name):
    """a variable of the package's Makefile, as make expands it"""
    out = subprocess.run(["make", "-s", "-C", PKG, "--no-print-directory", "--eval", "print-var: ; @echo $(%s)" % name, "print-var"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True, timeout=60)
    return out.stdout.decode().strip()


def syntax_check(*defines):
    hipcc = makefile_var("HIPCC")
    assert os.path.exists(hipcc) or shutil.which(hipcc), "hipcc not found: %s" % hipcc
    # build/rt_kernels.o's recipe: $(HIPFLAGS) -fno-slp-vectorize -DRT_SPLIT_LIST
    cmd = [hipcc] + makefile_var("HIPFLAGS").split() + ["-fno-slp-vectorize", "-DRT_SPLIT_LIST"] + ["-D%s" % d for d in defines]
    cmd += ["-fsyntax-only", os.path.join(PKG, "csrc", "rt_kernels.hip")]
    p = subprocess.run(cmd, cwd=PKG, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    return p.returncode, p.stdout.decode() + p.stderr.decode()


def test_default_interleave_compiles():
    assert "--offload-arch=gfx950" in makefile_var("HIPFLAGS").split()
    rc, out = syntax_check()
    assert rc == 0, out[-3000:]


@pytest.mark.parametrize("knob", ["RT_INTERLEAVE", "RT_INTERLEAVE_DENSE", "RT_INTERLEAVE_SOLO"])
def test_interleave_that_does_not_divide_64_is_refused(knob):
    rc, out = syntax_check("%s=48" % knob)
    assert rc != 0, "a build with %s=48 compiled" % knob
    assert MESSAGE in out, out[-3000:]
    rc, out = syntax_check("%s=32" % knob)                      # a divisor of 64 still builds
    assert rc == 0, out[-3000:]
