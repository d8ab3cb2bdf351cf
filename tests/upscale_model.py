"""Model of rt_sequence's key `upscale` (dd2360-raytracing_amd/host/rt_sequence_upscale.hpp), in two halves.

The rule in numpy float32, one rounding per operation, sums in tap order: axis() and upscale().  A tap that is skipped adds nothing
(not even a zero); a pixel without an accepted weight is COPIED from low pixel (I // s, J // s), so -0 and NaN survive.

The program's loop with the key set: Recorder wraps rt_amd.py for sequence_model.replay_animation / replay_progressive.  It passes every
call on; at the moment a frame is quantised it takes the shown low frame and the low guides the replay just used, traces
rt_render_guides at the shown size on the same world and tree, applies upscale() and quantises the result with rt_frame_levels at the
shown size — what the program does with its kernel k_upscale."""
import numpy as np

import sequence_model as sm

F = np.float32


def axis(n_high, s):
    """per high coordinate: the first of its two low taps and the weight of the second"""
    f = (np.arange(n_high).astype(F) + F(0.5)) / F(s) - F(0.5)
    i0 = np.floor(f)
    return i0.astype(np.int64), (f - i0).astype(F)


def upscale(c, sphere, sphere_high, s, weights=False):
    """c: the low gamma frame [ny, nx, 3] float32; sphere: its guides' sphere ids [ny, nx]; sphere_high: the shown frame's
    [s*ny, s*nx].  Returns (the shown frame [s*ny, s*nx, 3] float32, the number of accepted taps per shown pixel) and, with
    weights=True, the sum of the accepted weights as well"""
    c = np.ascontiguousarray(c, F)
    ny, nx = sphere.shape
    NY, NX = s * ny, s * nx
    assert c.shape == (ny, nx, 3) and sphere_high.shape == (NY, NX)
    i0, ax = axis(NX, s)
    j0, ay = axis(NY, s)
    sw = np.zeros((NY, NX), F)
    y = np.zeros((NY, NX, 3), F)
    taps = np.zeros((NY, NX), np.int64)
    with np.errstate(all="ignore"):
        for b in (0, 1):
            for a in (0, 1):
                i, j = i0 + a, j0 + b
                inside = ((j >= 0) & (j < ny))[:, None] & ((i >= 0) & (i < nx))[None, :]
                jj, ii = np.clip(j, 0, ny - 1)[:, None], np.clip(i, 0, nx - 1)[None, :]
                cq = c[jj, ii]
                ok = inside & (sphere[jj, ii] == sphere_high) & np.isfinite(cq).all(axis=2)
                w = ((ax if a else F(1) - ax)[None, :] * (ay if b else F(1) - ay)[:, None]).astype(F)
                x = cq * cq
                sw = np.where(ok, sw + w, sw)
                y = np.where(ok[:, :, None], y + w[:, :, None] * x, y)
                taps += ok
        blended = np.sqrt(y / sw[:, :, None])
    assert sw.dtype == F and y.dtype == F and blended.dtype == F
    fallback = c[(np.arange(NY) // s)[:, None], (np.arange(NX) // s)[None, :]]
    frame = np.where((sw > 0)[:, :, None], blended, fallback)
    return (frame, taps, sw) if weights else (frame, taps)


def nearest(p6_low, nx, ny, s):
    """the P6 bytes of a low frame enlarged s-fold by pixel repetition"""
    head = b"P6\n%d %d\n255\n" % (nx, ny)
    assert p6_low.startswith(head)
    px = np.frombuffer(p6_low[len(head):], np.uint8).reshape(ny, nx, 3)
    return b"P6\n%d %d\n255\n" % (s * nx, s * ny) + px.repeat(s, axis=0).repeat(s, axis=1).tobytes()


class Recorder:
    """rt_amd.py with two calls observed.  shown: the P6 bytes of every quantised frame at the shown size; taps: the accepted-tap
    counts of the same frames."""

    def __init__(self, rt, torch, s):
        self._rt, self._torch, self.s = rt, torch, s
        self.shown, self.taps = [], []
        self._guides = None

    def __getattr__(self, name):
        return getattr(self._rt, name)

    def render_guides(self, world, octree, nx, ny, d_hits):
        self._rt.render_guides(world, octree, nx, ny, d_hits)
        self._guides = (world, octree, nx, ny, d_hits)

    def frame_levels(self, d_out, fb, nx, ny, params, **kw):
        rt, torch, s = self._rt, self._torch, self.s
        world, octree, gx, gy, d_hits = self._guides
        assert (gx, gy) == (nx, ny) and params.input == rt.DENOISE_INPUT_GAMMA
        NX, NY = s * nx, s * ny
        d_high = rt.alloc_guides(NX, NY)
        rt.render_guides(world, octree, NX, NY, d_high)
        torch.cuda.synchronize()
        low = d_hits.cpu().numpy().view(rt.hit_record_dtype)["sphere"].reshape(ny, nx)
        high = d_high.cpu().numpy().view(rt.hit_record_dtype)["sphere"].reshape(NY, NX)
        frame, taps = upscale(fb.cpu().numpy().reshape(ny, nx, 3), low, high, s)
        d_levels = torch.zeros(rt.frame_levels_bytes(NX, NY), dtype=torch.uint8, device="cuda")
        rt.frame_levels(d_levels, torch.from_numpy(np.ascontiguousarray(frame, F).reshape(-1)).cuda(), NX, NY, params)
        torch.cuda.synchronize()
        self.shown.append(sm.p6(NX, NY, d_levels))
        self.taps.append(taps)
        rt.frame_levels(d_out, fb, nx, ny, params, **kw)                     # the low levels too: what the replay itself returns
