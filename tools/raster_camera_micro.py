"""The camera-gradient kernel (csrc/raster_camera.hip) next to the preprocess backward of the same call, at the headline's
Gaussian count (default 5.8 M, 1920x1080; the scene of tools/raster_aa_micro.py).  Forward + backward per call with the three
camera tensors requiring a gradient, antialiasing off and on, in form (a) colors_precomp + scales/rotations and form (d) shs
(degree 3) + cov3D_precomp.  The kernels' own times come from a `rocprofv3 --kernel-trace --stats` run of this script (no counters):
raster_camera_bwd_kernel<...> against preprocess_bwd_kernel / preprocess_bwd_form_kernel.  --no-camera: the same calls with plain
camera tensors (kernel names and launch counts of a backward without camera gradients).

  python tools/raster_camera_micro.py [--P 5800000] [--iters 3] [--warmup 1] [--no-camera]
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
    ap.add_argument("--no-camera", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("raster_camera_micro: needs the GPU")
    from contextgs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from contextgs_amd.synth import look_at_camera, random_gaussians

    P, W, H = a.P, a.W, a.H
    cam = look_at_camera((0.4, -2.2, 0.6), (0, 0, 0), W, H, fovx_deg=60.0)
    g = random_gaussians(P, seed=0, extent=1.0, scale_lo=0.0015, scale_hi=0.008)
    c = cam.to_torch("cuda")
    if not a.no_camera:
        for k in ("world_view_transform", "full_proj_transform", "camera_center"):
            setattr(c, k, getattr(c, k).clone().requires_grad_(True))
    rast = {aa: GaussianRasterizer(GaussianRasterizationSettings(
        H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), torch.tensor((0.1, 0.2, 0.3), device="cuda"), 1.0,
        c.world_view_transform, c.full_proj_transform, 3, c.camera_center, False, False, aa)) for aa in (False, True)}
    t = {k: torch.tensor(v, device="cuda", requires_grad=True) for k, v in g.items()}
    rng = np.random.default_rng(2)
    t["shs"] = torch.tensor(rng.normal(0.0, 0.25, size=(P, 16, 3)).astype(np.float32), device="cuda", requires_grad=True)
    m2 = torch.zeros(P, 3, device="cuda", requires_grad=True)
    w = torch.tensor(rng.normal(size=(3, H, W)).astype(np.float32), device="cuda")

    def cov6():
        q = t["rotations"].detach()
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
        L = R * t["scales"].detach()[:, None, :]
        S = L @ L.transpose(1, 2)
        return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).contiguous()

    c6 = cov6().requires_grad_(True)

    def step(form, aa):
        if form == "a":
            kw = dict(colors_precomp=t["colors"], scales=t["scales"], rotations=t["rotations"])
        else:
            kw = dict(shs=t["shs"], cov3D_precomp=c6)
        color, radii = rast[aa](means3D=t["means3D"], means2D=m2, opacities=t["opacities"], **kw)
        (color * w).sum().backward()
        return radii

    cases = [(f, aa) for f in ("a", "d") for aa in (False, True)]
    for _ in range(a.warmup):
        for f, aa in cases:
            step(f, aa)
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(a.iters):
        for f, aa in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            radii = step(f, aa)
            e1.record()
            torch.cuda.synchronize()
            times[(f, aa)].append(e0.elapsed_time(e1))
    vis = int((radii > 0).sum())
    names = {"a": "(a) colors_precomp + scales/rotations", "d": "(d) shs deg 3 + cov3D_precomp"}
    mode = "plain camera tensors" if a.no_camera else "camera gradients"
    lines = [f"# tools/raster_camera_micro.py ({mode}): P={P}, {W}x{H}, visible {vis}, forward + backward per call, device events, "
             f"{a.iters} alternating rounds after {a.warmup} warm-up rounds",
             f"{'form':<40s} {'AA':>4s} {'median ms':>10s} {'min ms':>10s}"]
    med = {}
    for f, aa in cases:
        v = sorted(times[(f, aa)])
        med[(f, aa)] = v[len(v) // 2]
        lines.append(f"{names[f]:<40s} {'on' if aa else 'off':>4s} {med[(f, aa)]:10.3f} {v[0]:10.3f}")
    for f in ("a", "d"):
        lines.append(f"{names[f]}: AA on - off = {med[(f, True)] - med[(f, False)]:+.3f} ms per call")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
