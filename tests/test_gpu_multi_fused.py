"""rt_multi_render_adaptive after rt_multi_set_adaptive_fused(1) on the one GPU of the test box (-m gpu): N ranks as N fresh child
processes on GPU 0 (tests/multi_fused_worker.py, the custom-gather form: RCCL refuses two ranks on one device).  Every rank renders
its part with rt_render_adaptive_fused_on; rank 0 compares the assembled frame and count map, bit for bit, with the single-process
rt_render_adaptive.  At most 3 GPU processes at once."""
import os
import re
import subprocess
import sys

import pytest

from rank_runner import free_port

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "multi_fused_worker.py")


def run_fused_ranks(world, *args, timeout=300):
    """multi_fused_worker.py RANK WORLD PORT ARGS... for every rank at once, as rank_runner.run_ranks starts multi_worker.py: every
    child under the timeout, killed on failure; every rank must exit 0.  Returns rank 0's stdout."""
    tail = [str(v) for v in (world, free_port()) + args]
    procs = [subprocess.Popen([sys.executable, WORKER, str(r)] + tail, stdout=subprocess.PIPE, stderr=subprocess.PIPE) for r in range(world)]
    outs = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=timeout)
            outs.append((p.returncode, o.decode(), e.decode()))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for rc, o, e in outs:
        assert rc == 0, (rc, o[-2000:], e[-2000:])
    return outs[0][1]


@pytest.mark.parametrize("world,nx,ny,n,spl,lo,hi,step,rel", [
    (2, 203, 117, 10000, 32, 4, 32, 4, 0.1),     # ragged frame: 26 x 15 tiles, 7 runs — part 0 holds 4, part 1 holds 3 (the last of 6 tiles)
    (3, 64, 40, 500, 30, 4, 12, 4, 0.1),         # 40 tiles, less than one run: ranks 1 and 2 hold nothing and still make both gather calls
])
def test_multi_fused_child_processes_on_one_gpu(rt, cuda, world, nx, ny, n, spl, lo, hi, step, rel):
    out = run_fused_ranks(world, nx, ny, n, spl, lo, hi, step, rel, 0.02)
    m = re.search(r"fused frame and counts EQUAL the single-process frame \(counts \[(.*)\]\)", out)
    assert m, out
    assert len(m.group(1).split(",")) >= 2, m.group(1)          # a mixed frame: the count map says something
