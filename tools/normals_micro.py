"""Cost of the normal-map kernels (csrc/normal_maps.hip) at the bench view, 1920x1080 and 5.8 M Gaussians, alternating in one
run, device events after a warm-up:
  normal_consistency forward + backward  vs  the same loss composed in torch from ATen ops (pad, slices, cross, norm, sum)
  depth_normals forward + backward       vs  the torch composition
  gaussian_normals forward + backward alone
next to the bytes each pair must move and the share of HBM bandwidth (6.29 TB/s) that makes.  The comparison partner is the
torch composition of the same run, never an earlier number.  Usage: python tools/normals_micro.py [P] [iters] -> stdout (kept as
profiles/normal_maps.txt).  GPU box."""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from contextgs_amd.normals import depth_normals, gaussian_normals, normal_consistency
from contextgs_amd.rasterizer import GaussianRasterizationSettings
from contextgs_amd.synth import look_at_camera

P = int(sys.argv[1]) if len(sys.argv) > 1 else 5_800_000
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 30
H, W = 1080, 1920
HBM = 6.29e12
dev = "cuda"
cam = look_at_camera((0.4, -2.2, 0.6), (0, 0, 0), W, H, fovx_deg=60.0).to_torch(dev)
tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
rs = GaussianRasterizationSettings(H, W, tx, ty, torch.zeros(3, device=dev), 1.0, cam.world_view_transform,
                                   cam.full_proj_transform, 1, cam.camera_center, False, False)
g = torch.Generator(device=dev).manual_seed(0)
v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                      indexing="ij")
depth = (2.0 + 0.0004 * u - 0.0003 * v + 0.01 * torch.rand(H, W, device=dev, generator=g))[None].requires_grad_()
normals = torch.randn(3, H, W, device=dev, generator=g).requires_grad_()
weight = torch.rand(1, H, W, device=dev, generator=g)
gE = torch.randn(1, H, W, device=dev, generator=g)
gN = torch.randn(3, H, W, device=dev, generator=g)
means = torch.randn(P, 3, device=dev, generator=g)
scales = torch.rand(P, 3, device=dev, generator=g) + 0.01
rots = torch.randn(P, 4, device=dev, generator=g).requires_grad_()
gP = torch.randn(P, 3, device=dev, generator=g)
fx, fy = W / (2 * tx), H / (2 * ty)


def torch_depth_normals(d):
    p = torch.cat([d * (u - W / 2) / fx, d * (v - H / 2) / fy, d], 0)[None]
    p = F.pad(p, (1, 1, 1, 1), "replicate")
    d0 = p[:, :, 2:, 1:-1] - p[:, :, :-2, 1:-1]
    d1 = p[:, :, 1:-1, 2:] - p[:, :, 1:-1, :-2]
    n = torch.cross(d0, d1, dim=1)
    return (-n / torch.norm(n, dim=1, keepdim=True))[0]


def clear():
    depth.grad = normals.grad = rots.grad = None


def fused_loss():
    clear()
    normal_consistency(normals, depth, rs, weight=weight).backward(gE)


def torch_loss():
    clear()
    (1 - weight * (normals * torch_depth_normals(depth)).sum(0, keepdim=True)).backward(gE)


def fused_normals():
    clear()
    depth_normals(depth, rs).backward(gN)


def torch_normals():
    clear()
    torch_depth_normals(depth).backward(gN)


def per_gaussian():
    clear()
    gaussian_normals(means, scales, rots, rs).backward(gP)


PLANE = H * W * 4
CASES = [("normal_consistency fwd + bwd (fused)", fused_loss, 16 * PLANE),
         ("normal_consistency fwd + bwd (torch composition)", torch_loss, None),
         ("depth_normals fwd + bwd (fused)", fused_normals, 9 * PLANE),
         ("depth_normals fwd + bwd (torch composition)", torch_normals, None),
         (f"gaussian_normals fwd + bwd, P = {P}", per_gaussian, 120 * P)]
for _, fn, _ in CASES:
    for _ in range(3):
        fn()
torch.cuda.synchronize()
total = {name: 0.0 for name, _, _ in CASES}
for _ in range(ITERS):              # alternating: every case sees the same clocks
    for name, fn, _ in CASES:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        total[name] += a.elapsed_time(b)
fused_loss()
e1 = normal_consistency(normals, depth, rs, weight=weight).detach()
e2 = (1 - weight * (normals * torch_depth_normals(depth)).sum(0, keepdim=True)).detach()
print(f"# {W}x{H}, {ITERS} alternating iterations, device events; max |fused - torch| of E: {float((e1 - e2).abs().max()):.2e}")
for name, _, nbytes in CASES:
    us = total[name] / ITERS * 1e3
    tail = f"  must move {nbytes / 1e6:.1f} MB = {nbytes / (us * 1e-6) / HBM * 100:.1f} % of {HBM / 1e12:.2f} TB/s" if nbytes else ""
    print(f"{name}: {us:.1f} us{tail}")
