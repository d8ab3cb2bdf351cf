"""Frame sequences for the temporal tests: Path (a world per camera position, the spheres stand) with its chains of histories on the
GPU and in the model, and Animation (ONE world whose spheres move).  No fixtures here; torch is the caller's."""
import numpy as np

import temporal_model as tm
from world_cases import orbit_camera

PATHS = dict(static=0.0, orbit=1.0, jump=60.0)          # the camera paths of tests/test_gpu_temporal.py: degrees per frame
STEP = np.float32(0.5)             # what a moved sphere of an Animation travels in x per frame


class Path:
    """frames of one world on a camera path: frame f is rendered by a world of its own (same spheres, camera f) with the RNG states carried
    on; each leaves its state, gamma frame and guides on the device and on the host"""

    def __init__(self, rt, torch, n_spheres, spl, nx, ny, degs, adapt):
        self.rt, self.torch, self.nx, self.ny = rt, torch, nx, ny
        base = rt.World(n_spheres, nx, ny)
        self.kind = base.spheres["material"].astype(np.int32)
        st = rt.alloc_rand_state(nx, ny)
        rt.render_init(nx, ny, st)
        self.worlds, self.trees, self.frames = {}, {}, []
        for f, deg in enumerate(degs):
            if deg not in self.worlds:
                cam = orbit_camera(rt, deg, nx, ny)
                if deg == 0.0:
                    assert np.array_equal(cam.view(np.uint8), base.camera.view(np.uint8))
                self.worlds[deg] = rt.World(n_spheres, nx, ny, spheres=base.spheres, camera=cam)
                self.trees[deg] = rt.Octree(self.worlds[deg], spl)
            W, O = self.worlds[deg], self.trees[deg]
            fb, state, d_hits = rt.alloc_fb(nx, ny), rt.alloc_adaptive_state(nx, ny), rt.alloc_guides(nx, ny)
            rt.render_adaptive_begin(fb, nx, ny, rt.Adaptive(*adapt[f % len(adapt)]), W, st, state, O)
            rt.render_guides(W, O, nx, ny, d_hits)
            torch.cuda.synchronize()
            self.frames.append(dict(W=W, O=O, cam=W.camera.copy(), fb=fb, state=state, d_hits=d_hits, h_state=state.cpu().numpy(),
                                    hits=d_hits.cpu().numpy().view(rt.hit_record_dtype)))
        base.close()

    def close(self):
        for O in self.trees.values():
            O.close()
        for W in self.worlds.values():
            W.close()


def gpu_chain(rt, torch, P, p, upto=None):
    """the histories of the path's frames on the GPU, each fed with the last: device tensors"""
    out = []
    for f, fr in enumerate(P.frames[:upto]):
        h = rt.alloc_temporal_history(P.nx, P.ny)
        h.fill_(7.0)                                                             # every pixel must be written
        prev = P.frames[f - 1] if f else None
        rt.temporal_accumulate(h, out[-1] if f else None, fr["d_hits"], prev["d_hits"] if f else None, prev["cam"] if f else None, fr["state"],
                               fr["W"], P.nx, P.ny, p)
        out.append(h)
    torch.cuda.synchronize()
    return out


def model_chain(P, p, upto=None):
    """the same chain in the model, each fed with the model's last, and the counts of every frame"""
    out, counts = [], []
    for f, fr in enumerate(P.frames[:upto]):
        prev = P.frames[f - 1] if f else None
        c = {}
        out.append(tm.accumulate(out[-1] if f else None, fr["hits"], prev["hits"] if f else None, prev["cam"] if f else None, fr["h_state"], P.kind,
                                 P.nx, P.ny, p.max_history, p.reuse_specular, p.position_tolerance, p.normal_min_dot, counts=c))
        counts.append(c)
    return out, counts


def motion_sets(spheres, every=7):
    """the small spheres that move (every `every`-th) and, disjoint from them for every > 3, those that change radius"""
    small = np.flatnonzero((spheres["material"] != -1) & (spheres["radius"] < 0.5) & (np.arange(len(spheres)) > 0))
    return small[::every], small[3::7]


class Animation:
    """frames of ONE world: before frame f > 0 the geometry is read back (what the next accumulate takes as d_geom_prev), the moved set
    is translated and the second set resized, the camera is set and the tree is built again on the device; every frame leaves its
    state, gamma frame, guides, camera and geometry on the device and on the host"""

    def __init__(self, rt, torch, n_spheres, spl, nx, ny, degs, adapt, resize=True, every=7):
        self.rt, self.torch, self.nx, self.ny, self.spl = rt, torch, nx, ny, spl
        self.W = W = rt.World(n_spheres, nx, ny)
        self.kind = W.spheres["material"].astype(np.int32)
        self.moved, self.resized = motion_sets(W.spheres, every)
        assert len(self.moved) >= 1 and not (resize and set(self.moved) & set(self.resized))
        st = rt.alloc_rand_state(nx, ny)
        rt.render_init(nx, ny, st)
        self.frames, self.tree = [], None
        for f, deg in enumerate(degs):
            if f:
                nxt = W.get_geometry()
                nxt[torch.from_numpy(self.moved).cuda(), 0] += float(STEP)
                if resize:
                    nxt[torch.from_numpy(self.resized).cuda(), 3] *= 1.25
                W.set_geometry(nxt)
                W.set_camera(orbit_camera(rt, deg, nx, ny))
            self.rebuild()
            fb, state, d_hits = rt.alloc_fb(nx, ny), rt.alloc_adaptive_state(nx, ny), rt.alloc_guides(nx, ny)
            rt.render_adaptive_begin(fb, nx, ny, rt.Adaptive(*adapt), W, st, state, self.tree)
            rt.render_guides(W, self.tree, nx, ny, d_hits)
            d_geom = W.get_geometry()
            torch.cuda.synchronize()
            self.frames.append(dict(cam=W.get_camera(), fb=fb, state=state, d_hits=d_hits, d_geom=d_geom, h_state=state.cpu().numpy(),
                                    hits=d_hits.cpu().numpy().view(rt.hit_record_dtype), geom=d_geom.cpu().numpy()))

    def rebuild(self):
        if self.tree is not None:
            self.tree.close()
        self.tree = self.rt.Octree(self.W, self.spl, gpu=True)

    def at(self, f):
        """the world with the geometry and camera of frame f again (the moving accumulate reads this frame's geometry from the world)"""
        self.W.set_geometry(self.frames[f]["d_geom"])
        self.W.set_camera(self.frames[f]["cam"])
        return self.frames[f]

    def close(self):
        if self.tree is not None:
            self.tree.close()
        self.W.close()
