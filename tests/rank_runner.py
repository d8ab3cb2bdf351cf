"""The ranks of an rt_multi job as fresh child processes on GPU 0 (tests/multi_worker.py), written once for the tests that start
them.  No GPU is needed to import this file."""
import os
import socket
import subprocess
import sys

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "multi_worker.py")


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def run_ranks(mode, world, *args, timeout=300):
    """multi_worker.py MODE RANK WORLD PORT ARGS... for every rank at once; every rank must exit 0.  Returns rank 0's stdout."""
    tail = [str(v) for v in (world, free_port()) + args]
    procs = [subprocess.Popen([sys.executable, WORKER, mode, str(r)] + tail, stdout=subprocess.PIPE, stderr=subprocess.PIPE) for r in range(world)]
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
