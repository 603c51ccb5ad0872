"""A camera with a trainable pose for render() (contextgs_amd/renderer.py).

`TrainableCamera(camera)` wraps a camera of the reference's kind (scene/cameras.py: `world_view_transform` V0 and
`full_proj_transform` PM0 in the row-vector convention, point' = [p, 1] @ M, plus `camera_center`) and exposes the fields
render() reads as functions of ONE 6-vector `xi` = (rotation vector w, translation tau), zeros = the wrapped camera:

  exp(xi) = [[R(w)^T, 0], [tau, 1]]      R(w) = exp([w]_x) (Rodrigues): a view-space point t moves to R t + tau
  world_view_transform = V = V0 exp(xi)
  full_proj_transform  = V P             P = inv(V0) PM0, the camera's projection, fixed
  camera_center        = inv(V)[3, :3]   = ([-tau R, 1] inv(V0))[:3]

so the three tensors stay consistent, and the gradients the rasterizer returns for each of them (rasterizer.py) add up in
`xi.grad` through autograd.  Torch only: 4x4 algebra is plumbing, evaluated in float64 and handed out as float32.  Every read
of a field evaluates the algebra anew (a few dozen tiny launches): nothing is cached, so that every render() owns its graph.
"""
from __future__ import annotations

import torch
import torch.nn as nn


def so3_exp(w: torch.Tensor) -> torch.Tensor:
    """R = exp([w]_x) [3,3] of a rotation vector w [3] (Rodrigues), differentiable everywhere: below |w|^2 = 1e-8 the two
    coefficients are their Taylor series (error < 1e-28), so no sqrt(0) enters the graph."""
    t2 = (w * w).sum()
    small = t2 < 1e-8
    t2s = torch.where(small, torch.ones_like(t2), t2)
    th = t2s.sqrt()
    a = torch.where(small, 1.0 - t2 / 6.0 + t2 * t2 / 120.0, th.sin() / th)
    half = (0.5 * th).sin()
    b = torch.where(small, 0.5 - t2 / 24.0 + t2 * t2 / 720.0, 2.0 * half * half / t2s)
    z = torch.zeros_like(t2)
    K = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
    return torch.eye(3, dtype=w.dtype, device=w.device) + a * K + b * (K @ K)


def se3_exp(xi: torch.Tensor) -> torch.Tensor:
    """exp(xi) [4,4] of the module docstring, row-vector convention: [[R(w)^T, 0], [tau, 1]] for xi = (w, tau)."""
    R = so3_exp(xi[:3])
    top = torch.cat([R.transpose(0, 1), torch.zeros(3, 1, dtype=xi.dtype, device=xi.device)], dim=1)
    bottom = torch.cat([xi[3:], torch.ones(1, dtype=xi.dtype, device=xi.device)]).unsqueeze(0)
    return torch.cat([top, bottom], dim=0)


def pose_tensors(xi: torch.Tensor, V0: torch.Tensor, P: torch.Tensor, V0_inv: torch.Tensor, PM0: torch.Tensor,
                 c0: torch.Tensor):
    """(V, PM, camera_center) of the module docstring in the dtype of V0 (float64 in TrainableCamera).  PM and the centre are
    formed as the wrapped camera's own PM0 / c0 plus the change, PM0 + (V - V0) P and c0 - (tau R) inv(V0)[:3, :3]: at
    xi = 0 all three tensors are the wrapped camera's bit for bit (PM0 is V0 P only up to the rounding it was stored with)."""
    x = xi.to(V0.dtype)
    V = V0 @ se3_exp(x)
    R = so3_exp(x[:3])
    return V, PM0 + (V - V0) @ P, c0 - (x[3:] @ R) @ V0_inv[:3, :3]      # inv(exp(xi))[3] = [-tau R, 1]


class TrainableCamera(nn.Module):
    """See the module docstring.  `xi` is the only parameter; every other attribute (uid, image_name, original_image, ...)
    reads through to the wrapped camera."""

    def __init__(self, camera, dtype=torch.float32):
        super().__init__()
        object.__setattr__(self, "_camera", camera)
        V0 = camera.world_view_transform.detach()
        dev = V0.device
        V0 = V0.double().cpu()
        PM0 = camera.full_proj_transform.detach().double().cpu()
        V0_inv = torch.linalg.inv(V0)
        self.register_buffer("V0", V0.to(dev), persistent=False)
        self.register_buffer("P", (V0_inv @ PM0).to(dev), persistent=False)
        self.register_buffer("V0_inv", V0_inv.to(dev), persistent=False)
        self.register_buffer("PM0", PM0.to(dev), persistent=False)
        self.register_buffer("c0", camera.camera_center.detach().double().to(dev), persistent=False)
        self.xi = nn.Parameter(torch.zeros(6, dtype=dtype, device=dev))
        self.image_height, self.image_width = int(camera.image_height), int(camera.image_width)
        self.FoVx, self.FoVy = camera.FoVx, camera.FoVy

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(self.__dict__["_camera"], name)

    def pose(self):
        """(world_view_transform, full_proj_transform, camera_center) from one evaluation, float32."""
        return tuple(t.float() for t in pose_tensors(self.xi, self.V0, self.P, self.V0_inv, self.PM0, self.c0))

    # (each field evaluates only its own part of pose_tensors: render() reads them one at a time)
    @property
    def world_view_transform(self) -> torch.Tensor:
        return (self.V0 @ se3_exp(self.xi.to(self.V0.dtype))).float()

    @property
    def full_proj_transform(self) -> torch.Tensor:
        return (self.PM0 + (self.V0 @ se3_exp(self.xi.to(self.V0.dtype)) - self.V0) @ self.P).float()

    @property
    def camera_center(self) -> torch.Tensor:
        x = self.xi.to(self.V0.dtype)
        return (self.c0 - (x[3:] @ so3_exp(x[:3])) @ self.V0_inv[:3, :3]).float()

    @torch.no_grad()
    def pose_delta(self):
        """(rotation angle in radians, translation norm) of exp(xi): the distance from the wrapped camera's pose."""
        return float(self.xi[:3].norm()), float(self.xi[3:].norm())
