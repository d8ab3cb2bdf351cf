"""Model of rt_sequence (dd2360-raytracing_amd/host/sequence.cpp), in two halves.

The motion rule of host/rt_sequence_motion.hpp in numpy float32, one rounding per operation: mask(), geometry(), lookfrom().  A
field the rule does not change is copied, never multiplied by 0 or 1, so -0 and NaN survive; frame 0 sets nothing.

The loop itself, replayed through the existing wrappers of rt_amd.py: replay_animation() and replay_progressive() make the calls of
the program in its order with its parameters — DEFAULTS restates the program's defaults, and args() turns the same dictionary into
the program's key=value tokens — and return the P6 bytes of every frame the program writes."""
import numpy as np

F = np.float32

DEFAULTS = dict(n=500, nx=64, ny=40, spl=30, radius=0.1, frames=4, min_spp=4, max_spp=8, batch=4, rel_error=0.0, floor=0.0,
                budget=0, rounds=1, budget_max_spp=0, move_every=0, move_step=0.02, cam_dx=0.0, cam_dz=0.0,
                max_history=32, tol=0.03, min_dot=0.9, reuse_specular=0, rect_radius=1, rect_min_count=4, gamma=1.5,
                levels=1, sigma_variance=4.0, passes=10, every=1)


def args(**kw):
    """the program's tokens for these keys (the others keep the program's defaults)"""
    return ["%s=%s" % (k, v) for k, v in kw.items()]


# ---- the motion rule -------------------------------------------------------------------------------------------------------------
def mask(material, radius, move_every):
    """dir[i]: (i / move_every) & 3 for every move_every-th slot that is filled and holds a small sphere, else -1"""
    material, radius = np.asarray(material), np.asarray(radius, F)
    i = np.arange(len(material))
    if move_every <= 0:
        return np.full(len(material), -1, np.int8)
    moves = (i % move_every == 0) & (material != -1) & (radius < F(0.5))
    return np.where(moves, (i // move_every) & 3, -1).astype(np.int8)


def geometry(base, dirs, f, move_step):
    """frame f's (cx, cy, cz, radius) records from the created list's: x + t, z + t, x - t or z - t with t = (float)f * move_step"""
    base = np.ascontiguousarray(base, F)
    g = base.copy()
    if f == 0:
        return g
    t = F(f) * F(move_step)
    with np.errstate(invalid="ignore"):
        for d, (col, sign) in enumerate(((0, 1), (2, 1), (0, -1), (2, -1))):
            m = dirs == d
            g[m, col] = base[m, col] + t if sign > 0 else base[m, col] - t
    return g


def lookfrom(f, cam_dx, cam_dz):
    return np.array([F(13) + F(f) * F(cam_dx), F(2), F(3) + F(f) * F(cam_dz)], F)


def camera(rt, f, nx, ny, cam_dx, cam_dz):
    """create_world's camera from frame f's place"""
    return rt.camera_init(lookfrom(f, cam_dx, cam_dz), (0, 0, 0), (0, 1, 0), 30.0, float(F(nx) / F(ny)), 0.1, 10.0)


# ---- the loop --------------------------------------------------------------------------------------------------------------------
def p6(nx, ny, levels):
    return b"P6\n%d %d\n255\n" % (nx, ny) + levels.cpu().numpy().tobytes()


def replay_animation(rt, torch, **kw):
    """the animation loop of the program; returns (the P6 bytes of every frame, the last history as float32 [5 * pixels], the last
    frame's sample counts)"""
    o = dict(DEFAULTS, **kw)
    n, nx, ny = o["n"], o["nx"], o["ny"]
    spheres_move, camera_moves = o["move_every"] > 0, F(o["cam_dx"]) != 0 or F(o["cam_dz"]) != 0
    W = rt.World(n, nx, ny, sphere_radius=o["radius"]).upload()
    base = np.ascontiguousarray(np.concatenate([W.spheres["center"], W.spheres["radius"][:, None]], 1), F)
    dirs = mask(W.spheres["material"], W.spheres["radius"], o["move_every"])
    adaptive = rt.Adaptive(o["min_spp"], o["max_spp"], o["batch"], o["rel_error"], o["floor"])
    cap = o["budget_max_spp"] or o["max_spp"] + o["rounds"] * o["batch"]
    budget = rt.Budget(o["budget"] * nx * ny, o["rounds"], o["batch"], cap, o["floor"])
    temporal = rt.temporal_params(max_history=o["max_history"], reuse_specular=o["reuse_specular"], position_tolerance=o["tol"],
                                  normal_min_dot=o["min_dot"])
    rectify = rt.temporal_rectify(radius=o["rect_radius"], min_count=o["rect_min_count"], gamma=o["gamma"])
    filt = rt.denoise_var_params(levels=o["levels"], sigma_variance=o["sigma_variance"])
    lp = rt.LevelsParams(rt.DENOISE_INPUT_GAMMA, 1, rt.LEVELS_RGB8, 1)

    fb = rt.alloc_fb(nx, ny)
    show = rt.alloc_fb(nx, ny) if o["levels"] > 0 else fb
    st, state, work = rt.alloc_rand_state(nx, ny), rt.alloc_adaptive_state(nx, ny), rt.alloc_denoise_work(nx, ny)
    spp = torch.zeros(nx * ny, dtype=torch.int32, device="cuda")
    levels = torch.zeros(rt.frame_levels_bytes(nx, ny), dtype=torch.uint8, device="cuda")
    hist = [rt.alloc_temporal_history(nx, ny), rt.alloc_temporal_history(nx, ny)]
    hits = [rt.alloc_guides(nx, ny), rt.alloc_guides(nx, ny)]
    geom = [torch.from_numpy(base).cuda(), None]
    created = W.camera.copy()
    cams = [created, created]
    rt.render_init(nx, ny, st)                                               # once: the states continue from frame to frame
    tree, frames = None, []
    for f in range(o["frames"]):
        c, l = f & 1, (f & 1) ^ 1
        cams[c] = camera(rt, f, nx, ny, o["cam_dx"], o["cam_dz"]) if f > 0 and camera_moves else created
        if f > 0 and spheres_move:
            geom[c] = torch.from_numpy(geometry(base, dirs, f, o["move_step"])).cuda()
            W.set_geometry(geom[c])
        if f > 0 and camera_moves:
            W.set_camera(cams[c])
        if f == 0 or spheres_move:
            torch.cuda.synchronize()
            if tree is not None:
                tree.close()
            tree = rt.Octree(W, o["spl"], gpu=True)
        rt.render_guides(W, tree, nx, ny, hits[c])
        rt.render_adaptive_begin(fb, nx, ny, adaptive, W, st, state, tree, spp)
        if o["budget"] > 0:
            inputs = rt.temporal_inputs(hits[c], hist[l] if f else None, hits[l], cams[l])
            rt.render_adaptive_spend_temporal(fb, nx, ny, budget, inputs, temporal, W, st, state, tree, spp)
        rt.temporal_accumulate_rectified(hist[c], hist[l] if f else None, hits[c], hits[l], cams[l], state, W, nx, ny, temporal, rectify,
                                         d_geom_prev=geom[l] if f and spheres_move else None)
        if o["levels"] > 0:
            rt.denoise_history(show, fb, nx, ny, hits[c], hist[c], filt, work)
        rt.frame_levels(levels, show, nx, ny, lp)
        torch.cuda.synchronize()
        frames.append(p6(nx, ny, levels))
    last = (o["frames"] - 1) & 1
    out = frames, hist[last].cpu().numpy(), spp.cpu().numpy()
    tree.close()
    W.close()
    return out


def replay_progressive(rt, torch, **kw):
    """the progressive loop of the program; returns {pass: its P6 bytes} for the passes the program shows"""
    o = dict(DEFAULTS, **kw)
    n, nx, ny = o["n"], o["nx"], o["ny"]
    W = rt.World(n, nx, ny, sphere_radius=o["radius"]).upload()
    tree = rt.Octree(W, o["spl"], gpu=True)
    fb = rt.alloc_fb(nx, ny)
    show = rt.alloc_fb(nx, ny) if o["levels"] > 0 else fb
    st, work, hits = rt.alloc_rand_state(nx, ny), rt.alloc_denoise_work(nx, ny), rt.alloc_guides(nx, ny)
    levels = torch.zeros(rt.frame_levels_bytes(nx, ny), dtype=torch.uint8, device="cuda")
    rt.render_init(nx, ny, st)
    rt.render_guides(W, tree, nx, ny, hits)
    shown = {}
    for s in range(1, o["passes"] + 1):
        rt.render_progressive(fb, nx, ny, s, W, st, tree)
        if s % o["every"] != 0 and s != o["passes"]:
            continue
        if o["levels"] > 0:
            rt.denoise(show, fb, nx, ny, hits, rt.denoise_params(rt.DENOISE_INPUT_SUM, s, levels=o["levels"]), work)
            lp = rt.LevelsParams(rt.DENOISE_INPUT_GAMMA, s, rt.LEVELS_RGB8, 1)
        else:
            lp = rt.LevelsParams(rt.DENOISE_INPUT_SUM, s, rt.LEVELS_RGB8, 1)
        rt.frame_levels(levels, show, nx, ny, lp)
        torch.cuda.synchronize()
        shown[s] = p6(nx, ny, levels)
    tree.close()
    W.close()
    return shown
