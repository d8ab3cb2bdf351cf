"""What the GPU tests of rt_render_adaptive_h16 share: ONE Frame of sentinel-filled binary16
buffers (adaptive_frames.Frame for fb of 3 x binary16 per element), the GPU's own one-sample passes as the model's per-sample colours,
and the checks against tests/h16_adaptive_model.py.  Every comparison is bit equality.  torch is the caller's (the cuda fixture):
importing this needs no GPU."""
import numpy as np

import h16_adaptive_model as M
from adaptive_frames import SENTINEL, STATE_FILL, inside_frame, part_layout, part_tuple, state_parts
from bitcmp import raw_bits

SENTINEL16 = 0x7EAD                # a binary16 NaN pattern nothing renders
FLOOR = 0.02
LO, HI, STEP = 4, 24, 4


class Frame:
    """the buffers of one part of a binary16 frame: fb pre-filled with SENTINEL16, d_spp with SENTINEL, RNG states from
    rt_render_init(part), a state of STATE_FILL bytes.  With a context every call goes through it, on `stream`."""

    def __init__(self, rt, torch, nx, ny, part, ctx=None, stream=None):
        self.rt, self.torch, self.nx, self.ny, self.part, self.ctx, self.stream = rt, torch, nx, ny, part, ctx, stream
        n = self.n = rt.part_pixels(nx, ny, part)
        self.fb = torch.full((n * 3,), SENTINEL16, dtype=torch.int16, device="cuda").view(torch.float16)
        self.spp = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
        self.st = rt.alloc_rand_state(nx, ny, part)
        rt.render_init(nx, ny, self.st, part)
        self.state = torch.full((n * rt.ADAPTIVE_STATE_BYTES,), STATE_FILL, dtype=torch.uint8, device="cuda")
        self.inside = inside_frame(nx, ny, part_tuple(part), n)
        torch.cuda.synchronize()

    def _call(self, name, *args):
        if self.ctx is not None:
            getattr(self.ctx, name)(*args, stream=self.stream)
        else:
            getattr(self.rt, name)(*args)

    def first(self, W, O, P, state=True, spp=True):
        """rt_render_adaptive_h16"""
        self._call("render_adaptive_h16", self.fb, self.nx, self.ny, self.rt.Adaptive(*P), W, self.st, self.state if state else None, O,
                   self.spp if spp else None, self.part)
        return self

    def snap(self):
        self.torch.cuda.synchronize()
        return dict(fb=self.fb.view(self.torch.int16).cpu().numpy().view(np.uint16).reshape(-1, 3), spp=self.spp.cpu().numpy(),
                    st=self.st.cpu().numpy().view(np.uint32).reshape(-1, 12), state=self.state.cpu().numpy().copy())


def progressive_samples16(rt, torch, W, O, nx, ny, count):
    """per-sample colours [count, pixels, 3] (float32 images of the binary16 values) and the RNG state after every pass
    [count, pixels, 12], from one-sample rt_render_progressive passes, current_sample = 1 into a fresh binary16 fb each"""
    st = rt.alloc_rand_state(nx, ny)
    rt.render_init(nx, ny, st)
    cols, states = [], []
    for _ in range(count):
        fb = rt.alloc_fb(nx, ny, precision=rt.FP16)
        rt.render_progressive(fb, nx, ny, 1, W, st, O)
        cols.append(fb)
        states.append(st.clone())
    torch.cuda.synchronize()
    return (np.stack([c.cpu().numpy().astype(np.float32).reshape(-1, 3) for c in cols]),
            np.stack([s.cpu().numpy().view(np.uint32).reshape(-1, 12) for s in states]))


def render16(rt, torch, W, O, nx, ny, ns, part=None):
    """(fb [n, 3] uint16, RNG states [n, 12]) of rt_render(ns) of a binary16 world on fresh buffers"""
    part = part or rt.WHOLE
    st = rt.alloc_rand_state(nx, ny, part)
    fb = rt.alloc_fb(nx, ny, part, rt.FP16)
    rt.render_init(nx, ny, st, part)
    rt.render(fb, nx, ny, ns, W, st, O, part)
    torch.cuda.synchronize()
    return fb.view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1, 3), st.cpu().numpy().view(np.uint32).reshape(-1, 12)


class Scene16:
    """a binary16 world (and tree: spl None = the list, gpu: rt_build_octree_gpu) for one frame size, with the GPU's own per-sample
    colours and the sweep's mixed targets, each computed once"""

    def __init__(self, rt, torch, n, spl, nx, ny, gpu=False, count=HI):
        self.rt, self.torch, self.nx, self.ny = rt, torch, nx, ny
        self.W = rt.World(n, nx, ny, precision=rt.FP16)
        self.O = rt.Octree(self.W, spl, gpu=gpu) if spl else None
        self.samples, self.states = progressive_samples16(rt, torch, self.W, self.O, nx, ny, count)
        self.targets = M.mixed_targets(self.samples, LO, STEP, HI, FLOOR)          # from the loosest down
        self._k = {}

    def at_k(self, k, part=None):
        """rt_render(ns = k) on fresh buffers of the part"""
        key = (int(k), part_tuple(part) if part is not None else None)
        if key not in self._k:
            self._k[key] = render16(self.rt, self.torch, self.W, self.O, self.nx, self.ny, int(k), part)
        return self._k[key]

    def close(self):
        if self.O is not None:
            self.O.close()
        self.W.close()


def check_model(sc, snap, P):
    """a whole-frame snapshot against the model of the rule on the scene's samples: counts, colours, RNG states and the state's record"""
    lo, hi, step, rel, floor = P
    m = M.run(sc.samples, rel, floor, lo, step, hi)
    n = m["spp"].size
    assert np.array_equal(snap["spp"], m["spp"])
    assert np.array_equal(snap["fb"], M.bits16(m["fb"]))
    assert np.array_equal(snap["st"], sc.states[m["spp"] - 1, np.arange(n)])
    S, SL, Q, k = state_parts(snap["state"], n)
    assert np.array_equal(k, m["spp"])
    assert np.array_equal(raw_bits(S), raw_bits(m["S"])) and np.array_equal(raw_bits(SL), raw_bits(m["SL"])) and np.array_equal(raw_bits(Q), raw_bits(m["Q"]))
    return m


def check_padding(F, snap):
    """the padding of a part's edge tiles keeps the sentinels, the state's fill and rt_render_init's RNG bytes"""
    out = ~F.inside
    init = Frame(F.rt, F.torch, F.nx, F.ny, F.part).snap()
    assert (snap["fb"][out] == SENTINEL16).all() and (snap["spp"][out] == SENTINEL).all()
    assert np.array_equal(snap["st"][out], init["st"][out])
    for a in state_parts(snap["state"], F.n):
        assert (raw_bits(a[out]) == 0xA5A5A5A5).all()
    return out


def check_part_of_whole(F, snap, whole):
    """every in-frame element of a part's snapshot holds the whole frame's pixel: fb, d_spp, RNG state and the state's record"""
    pix, inside = part_layout(F.nx, F.ny, part_tuple(F.part), F.n)
    p = pix[inside]
    for key in ("fb", "spp", "st"):
        assert np.array_equal(snap[key][inside], whole[key][p]), key
    for a, b in zip(state_parts(snap["state"], F.n), state_parts(whole["state"], F.nx * F.ny)):
        assert np.array_equal(raw_bits(a[inside]), raw_bits(b[p]))
