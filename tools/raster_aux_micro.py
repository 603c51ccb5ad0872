"""Cost of the rasterizer's depth / inverse-depth / alpha maps (csrc/raster_aux.hip) at the headline's Gaussian count (default
5.8 M, 1920x1080), in one process, alternating, after warm-up, with device events:

  a  colour forward + backward                                   (return_aux=False)
  b  the same with return_aux=True and a loss on colour only     (maps computed, no map gradient: the colour backward alone)
  c  return_aux=True, loss on colour + depth + alpha             (colour and map backward)
  d  forward only, without aux
  e  forward only, with aux

b - a is the aux forward, c - b the aux backward plus the dL/dz chain.  Prints one table (median / min per case, ms) and, with
--out, also writes it to that file.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script
(e.g. --iters 3 --warmup 1).

  python tools/raster_aux_micro.py [--P 5800000] [--iters 10] [--warmup 3] [--out FILE]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
        raise SystemExit("raster_aux_micro: needs the GPU")
    from contextgs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from contextgs_amd.synth import look_at_camera, random_gaussians

    P, W, H = a.P, a.W, a.H
    cam = look_at_camera((0.4, -2.2, 0.6), (0, 0, 0), W, H, fovx_deg=60.0)
    g = random_gaussians(P, seed=0, extent=1.0, scale_lo=0.0015, scale_hi=0.008)
    c = cam.to_torch("cuda")
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2),
                                       torch.tensor((0.1, 0.2, 0.3), device="cuda"), 1.0, c.world_view_transform,
                                       c.full_proj_transform, 1, c.camera_center, False, False)
    rast = GaussianRasterizer(rs)
    t = {k: torch.tensor(v, device="cuda", requires_grad=True) for k, v in g.items()}
    m2 = torch.zeros(P, 3, device="cuda", requires_grad=True)
    rng = np.random.default_rng(2)
    w = torch.tensor(rng.normal(size=(3, H, W)).astype(np.float32), device="cuda")
    wd = torch.tensor(rng.normal(size=(1, H, W)).astype(np.float32), device="cuda")
    wa = torch.tensor(rng.normal(size=(1, H, W)).astype(np.float32), device="cuda")
    kw = dict(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], colors_precomp=t["colors"], scales=t["scales"],
              rotations=t["rotations"])

    def step(case):
        if case in ("d", "e"):
            with torch.no_grad():
                return rast(**kw, return_aux=case == "e")[1]
        if case == "a":
            color, radii = rast(**kw)
            (color * w).sum().backward()
            return radii
        color, radii, aux = rast(**kw, return_aux=True)
        loss = (color * w).sum()
        if case == "c":
            loss = loss + (aux["depth"] * wd).sum() + (aux["alpha"] * wa).sum()
        loss.backward()
        return radii

    cases = ("a", "b", "c", "d", "e")
    for _ in range(a.warmup):
        for f in cases:
            step(f)
    torch.cuda.synchronize()
    times = {f: [] for f in cases}
    for _ in range(a.iters):
        for f in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            radii = step(f)
            e1.record()
            torch.cuda.synchronize()
            times[f].append(e0.elapsed_time(e1))
    vis = int((radii > 0).sum())
    names = {"a": "colour fwd + bwd", "b": "aux fwd, colour loss, bwd", "c": "aux fwd, colour+depth+alpha, bwd",
             "d": "forward only", "e": "forward only, return_aux"}
    lines = [f"# tools/raster_aux_micro.py: P={P}, {W}x{H}, visible {vis}, device events, "
             f"{a.iters} alternating rounds after {a.warmup} warm-up rounds",
             f"{'case':<40s} {'median ms':>10s} {'min ms':>10s}"]
    med = {}
    for f in cases:
        v = sorted(times[f])
        med[f] = v[len(v) // 2]
        lines.append(f"({f}) {names[f]:<36s} {med[f]:10.3f} {v[0]:10.3f}")
    lines.append(f"aux forward (e - d) {med['e'] - med['d']:.3f} ms, (b - a) {med['b'] - med['a']:.3f} ms; "
                 f"aux backward + dz chain (c - b) {med['c'] - med['b']:.3f} ms")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
