"""Host time of a call through the binding, one rt_amd.py against another (no GPU, no library): every symbol is a stand-in that returns
0, torch's current stream a constant, buffers objects with a data_ptr().  timeit, best of 9 x 20000 calls, microseconds.

    python tools/binding_call_cost.py <a copy of the earlier rt_amd.py> dd2360-raytracing_amd/rt_amd.py

The figures of profiles/r21/binding_calls.txt are this script's.  A call costs 1-4 us and the best of 9 still moves by a microsecond
from run to run on a machine that does anything else: it bounds the cost, it does not resolve differences below that."""
import ctypes as C
import importlib.util
import sys
import timeit


class Lib:
    def __getattr__(self, name):
        setattr(self, name, lambda *a: 0)
        return getattr(self, name)


class Buf:
    def __init__(self, address):
        self.data_ptr = lambda: address


def cases(path, tag):
    spec = importlib.util.spec_from_file_location("rt_amd_" + tag, path)
    rt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rt)
    rt._LIB, rt._stream = Lib(), (lambda: C.c_void_p(0x5EED))
    W, ctx = rt.World(22, 16, 8), rt.RenderCtx()
    W.h, ctx.h = C.c_void_p(0xA100), C.c_void_p(0xC100)
    fb, st, state, hits = Buf(0x1000), Buf(0x1040), Buf(0x1080), Buf(0x10C0)
    Bd, T, TI = rt.Budget(1000, 2, 4, 64, 0.01), rt.temporal_params(), rt.temporal_inputs(hits)
    return {"render": lambda: rt.render(fb, 16, 8, 4, W, st),
            "RenderCtx.render": lambda: ctx.render(fb, 16, 8, 4, W, st),
            "render_adaptive_spend_temporal": lambda: rt.render_adaptive_spend_temporal(fb, 16, 8, Bd, TI, T, W, st, state)}, (W, ctx)


if __name__ == "__main__":
    before, keep_b = cases(sys.argv[1], "before")
    after, keep_a = cases(sys.argv[2], "after")
    print("%-34s %8s %8s %8s" % ("wrapper", "before", "after", "added"))
    for name in before:
        b, a = (min(timeit.repeat(f, number=20000, repeat=9)) / 20000 * 1e6 for f in (before[name], after[name]))
        print("%-34s %8.3f %8.3f %+8.3f" % (name, b, a, a - b))
    for obj in keep_b + keep_a:
        obj.h = None            # stand-in handles: nothing to free
