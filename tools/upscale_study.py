"""Quality at equal time of rt_sequence's key `upscale`: is a frame rendered at half the size and rebuilt at the shown size better
than the frame the same time buys at the shown size?  Drives the program only (dd2360-raytracing_amd/rt_sequence) and compares the P6
files it writes with tools/image_metrics.py.

For a static scene and a moving one (move_every=7 cam_dx=0.05), and k = 4 and 16 samples a pixel, at the shown size 1200x800:
  (i)   native, min_spp = max_spp = k;
  (ii)  600x400 upscale=2 with the sample count, among the --candidates multiples of k (rounded), whose wall time a frame is closest to (i)'s;
  (iii) 600x400 upscale=2 at the same k.
Each is compared, in the last frame of the run, against the native frame of the same scene frame at 1024 samples a pixel, unfiltered,
unrectified and without history (levels=0 gamma=0 max_history=0).  The wall time is the program's own (timing=1: frames 1.., frame 0
left out).  RMSE is over the 8-bit RGB levels; PSNR and SSIM are the grey metrics of tools/image_metrics.py.

  python tools/upscale_study.py [--frames 8] [--n 10000] [--spl 32] [--ref-spp 1024] [--candidates 1,1.25,1.5,1.75,2,2.5,3,4]"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import image_metrics as im  # noqa: E402

EXE = os.path.join(ROOT, "dd2360-raytracing_amd", "rt_sequence")


def run(workdir, prefix, **keys):
    """one run of the program; returns (its wall time a frame in ms, the path of its last frame)"""
    tokens = ["%s=%s" % kv for kv in keys.items()] + ["timing=1", "out=" + prefix]
    p = subprocess.run([EXE] + tokens, cwd=workdir, capture_output=True, text=True, timeout=1200)
    if p.returncode != 0:
        sys.exit("rt_sequence %s: exit code %d\n%s" % (" ".join(tokens), p.returncode, p.stderr[-2000:]))
    wall = float(re.search(r"^timing: wall per frame\s+mean\s+([0-9.]+) ms", p.stderr, re.M).group(1))
    return wall, os.path.join(workdir, "%s%04d.ppm" % (prefix, keys["frames"] - 1))


def read_p6(path):
    data = open(path, "rb").read()
    m = re.match(rb"P6\n(\d+) (\d+)\n255\n", data)
    nx, ny = int(m.group(1)), int(m.group(2))
    return np.frombuffer(data[m.end():], np.uint8).reshape(ny, nx, 3).astype(np.int64)


def metrics(path, ref):
    a = read_p6(path)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    ga, gb = im.gray8(a), im.gray8(ref)
    return float(np.sqrt(((a - ref) ** 2).mean())), im.psnr(ga, gb), im.ssim(ga, gb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--spl", type=int, default=32)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--candidates", default="1,1.25,1.5,1.75,2,2.5,3,4")
    a = ap.parse_args()
    multiples = [float(x) for x in a.candidates.split(",")]
    scenes = [("static", {}), ("moving", dict(move_every=7, cam_dx=0.05))]
    base = dict(n=a.n, spl=a.spl, frames=a.frames)
    print("shown 1200x800, n=%d spl=%d, frame %d of %d compared against native %d spp (levels=0 gamma=0 max_history=0)"
          % (a.n, a.spl, a.frames - 1, a.frames, a.ref_spp))
    print("%-7s %3s  %-26s %5s %9s %8s %8s %7s" % ("scene", "k", "arm", "spp", "wall ms", "RMSE", "PSNR dB", "SSIM"))
    with tempfile.TemporaryDirectory() as tmp:
        for scene, motion in scenes:
            _, ref_path = run(tmp, "ref_", nx=1200, ny=800, min_spp=a.ref_spp, max_spp=a.ref_spp, levels=0, gamma=0, max_history=0, **base, **motion)
            ref = read_p6(ref_path)
            for k in (4, 16):
                rows = []
                wall_i, path = run(tmp, "i_", nx=1200, ny=800, min_spp=k, max_spp=k, **base, **motion)
                rows.append(("(i) native", k, wall_i, path))
                tried = {}
                for spp in sorted({max(2, int(round(m * k))) for m in multiples}):
                    tried[spp] = run(tmp, "c%d_" % spp, nx=600, ny=400, upscale=2, min_spp=spp, max_spp=spp, **base, **motion)
                print("#   600x400 upscale=2, wall ms by spp: " + "  ".join("%d: %.3f" % (spp, tried[spp][0]) for spp in sorted(tried)))
                best = min(tried, key=lambda spp: abs(tried[spp][0] - wall_i))
                rows.append(("(ii) 600x400 x2, equal time", best) + tried[best])
                rows.append(("(iii) 600x400 x2, equal k", k) + tried[k] if k in tried else ("(iii) 600x400 x2, equal k", k) + run(
                    tmp, "iii_", nx=600, ny=400, upscale=2, min_spp=k, max_spp=k, **base, **motion))
                for arm, spp, wall, path in rows:
                    rmse, psnr, ssim = metrics(path, ref)
                    print("%-7s %3d  %-26s %5d %9.3f %8.3f %8.3f %7.4f" % (scene, k, arm, spp, wall, rmse, psnr, ssim))
                sys.stdout.flush()


if __name__ == "__main__":
    main()
