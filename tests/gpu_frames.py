"""rt_render_init + rt_render of a part or the whole frame on fresh buffers, written once, and readers for the shapes the tests
compare.  torch is the caller's (the cuda fixture), so importing this file needs no GPU."""
import numpy as np


def render_frame(rt, torch, W, O, nx, ny, ns, part=None, precision=None):
    """the device fb and RNG states of one rt_render; part None: the whole frame, precision None: binary32"""
    part = part or rt.WHOLE
    st = rt.alloc_rand_state(nx, ny, part)
    fb = rt.alloc_fb(nx, ny, part, rt.FP32 if precision is None else precision)
    rt.render_init(nx, ny, st, part)
    rt.render(fb, nx, ny, ns, W, st, O, part)
    torch.cuda.synchronize()
    return fb, st


def states_of(st):
    """the RNG states read back: [n, 12] uint32"""
    return st.cpu().numpy().view(np.uint32).reshape(-1, 12)


def frame_rows(fb, st):
    """(pixels [n, 3] in fb's float type, RNG states [n, 12] uint32) on the host"""
    return fb.cpu().numpy().reshape(-1, 3), states_of(st)


def frame_image(fb, nx, ny):
    """the whole frame on the host: [ny, nx, 3]"""
    return fb.cpu().numpy().reshape(ny, nx, 3)
