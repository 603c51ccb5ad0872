"""Forward + backward time of the drop-in rasterizer's argument forms at the headline's Gaussian count (default 5.8 M,
1920x1080), in one process, alternating, after warm-up, with device events:

  a  colors_precomp + scales/rotations       (the form ContextGS renders with)
  b  torch SH evaluation -> colors_precomp    (what a caller had to do without the SH form)
  c  shs (degree 3, 16 coefficients)          (SH evaluated in the preprocess kernels)
  d  cov3D_precomp + colors_precomp

Prints one table (median / min per form, ms) and, with --out, also writes it to that file.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script (e.g. --iters 3 --warmup 1).

  python tools/sh_raster_micro.py [--P 5800000] [--iters 10] [--warmup 3] [--out FILE]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=5_800_000)
    ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--H", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sh_raster_micro: needs the GPU")
    from contextgs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from contextgs_amd.synth import look_at_camera, random_gaussians
    from raster_harness import cov6_torch, sh_eval_torch

    P, W, H, D, M = a.P, a.W, a.H, 3, 16
    cam = look_at_camera((0.4, -2.2, 0.6), (0, 0, 0), W, H, fovx_deg=60.0)
    g = random_gaussians(P, seed=0, extent=1.0, scale_lo=0.0015, scale_hi=0.008)
    rng = np.random.default_rng(1)
    sh = rng.normal(0.0, 0.2, size=(P, M, 3)).astype(np.float32)
    c = cam.to_torch("cuda")
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2),
                                       torch.tensor((0.1, 0.2, 0.3), device="cuda"), 1.0, c.world_view_transform,
                                       c.full_proj_transform, D, c.camera_center, False, False)
    rast = GaussianRasterizer(rs)
    leaf = lambda v: torch.tensor(v, device="cuda", requires_grad=True)
    t = {k: leaf(v) for k, v in g.items()}
    shs = leaf(sh)
    with torch.no_grad():
        cov6 = cov6_torch(t["scales"], t["rotations"], 1.0)
    cov6.requires_grad_(True)
    m2 = torch.zeros(P, 3, device="cuda", requires_grad=True)
    w = torch.tensor(np.random.default_rng(2).normal(size=(3, H, W)).astype(np.float32), device="cuda")
    campos = rs.campos.float()

    def step(form):
        kw = dict(means3D=t["means3D"], means2D=m2, opacities=t["opacities"])
        if form == "a":
            kw.update(colors_precomp=t["colors"], scales=t["scales"], rotations=t["rotations"])
        elif form == "b":
            kw.update(colors_precomp=sh_eval_torch(shs, t["means3D"], campos, D), scales=t["scales"], rotations=t["rotations"])
        elif form == "c":
            kw.update(shs=shs, scales=t["scales"], rotations=t["rotations"])
        else:
            kw.update(colors_precomp=t["colors"], cov3D_precomp=cov6)
        color, radii = rast(**kw)
        (color * w).sum().backward()
        return radii

    forms = ("a", "b", "c", "d")
    for _ in range(a.warmup):
        for f in forms:
            step(f)
    torch.cuda.synchronize()
    times = {f: [] for f in forms}
    for _ in range(a.iters):
        for f in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            radii = step(f)
            e1.record()
            torch.cuda.synchronize()
            times[f].append(e0.elapsed_time(e1))
    vis = int((radii > 0).sum())
    names = {"a": "colors_precomp + scales/rotations", "b": "torch SH eval -> colors_precomp", "c": "shs (D=3, M=16)",
             "d": "cov3D_precomp + colors_precomp"}
    lines = [f"# tools/sh_raster_micro.py: P={P}, {W}x{H}, visible {vis}, forward+backward per call, device events, "
             f"{a.iters} alternating rounds after {a.warmup} warm-up rounds",
             f"{'form':<40s} {'median ms':>10s} {'min ms':>10s}"]
    for f in forms:
        v = sorted(times[f])
        lines.append(f"({f}) {names[f]:<36s} {v[len(v) // 2]:10.3f} {v[0]:10.3f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
