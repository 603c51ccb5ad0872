"""Normal maps and the normal-consistency regulariser of 2DGS / GOF / RaDe-GS / PGSR (csrc/normal_maps.hip; include/cgs.h has
the definitions and the gradients spelled out).  Three autograd functions over the C-ABI, no CPU path:

  gaussian_normals(means3D, scales, rotations, raster_settings) -> [P,3]
      per Gaussian: the axis of its smallest scale (ties: the lowest index), column k of R(q / |q|), in camera space
      (n_w @ viewmatrix[:3,:3]) and turned so that n . t >= 0 with t the view-space mean.  The gradient reaches `rotations`
      only (through the normalisation too): scales only pick k, means3D only picks the sign, the camera is a constant.
  depth_normals(depth, raster_settings, eps=0.0) -> [3,H,W]
      the reference's depthImgToPosCam_Batched + computeNormalsFromPosCam_Batched (utils/visualize_utils.py) with
      fx = W / (2 tanfovx), fy = H / (2 tanfovy), principal point (W/2, H/2), integer pixel coordinates:
      p = (d (u - W/2) / fx, d (v - H/2) / fy, d), edges replicated, d0 = p(v+1,u) - p(v-1,u), d1 = p(v,u+1) - p(v,u-1),
      n = d0 x d1, N = -n / (|n| + eps).  Where |n| = 0 (undrawn regions, an image one pixel wide or high) N = 0 and the
      gradient through the norm is 0, never NaN.  eps=1e-5 reproduces the reference, whose constant is meant for pictures:
      at 1920 px and depth 2, |n| is about 6e-6 and every normal comes out 0.37 long.  The default 0 gives unit normals.
  normal_consistency(normals, depth, raster_settings, weight=None, eps=0.0) -> [1,H,W]
      E = 1 - m sum_c normals_c N_c with N = depth_normals(depth) computed inside the kernel and never stored, m the optional
      `weight` map [1,H,W] (not differentiated; 2DGS passes alpha.detach()).  One launch forward, one backward, which writes
      dL/dnormals and dL/ddepth (only the one that is asked for when the other input is detached).

All three work in CAMERA space, the view space of `viewmatrix` in the row-vector convention (t = [x y z 1] @ viewmatrix, x
right, y down, z forward), and all normals point AWAY from the camera: a fronto-parallel plane gives (0, 0, +1), as the
reference's computeNormalsFromPosCam_Batched does.  This is the opposite of 2DGS's convention (towards the camera); what
matters for the regulariser is that the blended Gaussian normals and the depth normals agree, and they do (tests/
test_normals_gpu.py has a tilted plane of randomly flipped Gaussians).  The depth gradients are gathers (each pixel sums the
stencils that read it, in a fixed order), so every backward here is free of float atomics and bit-reproducible.

`GaussianRasterizer.forward(..., return_normals=True)` renders sum_i w_i gaussian_normals_i as `extras["normals"]`
(contextgs_amd/rasterizer.py); the training snippet is in INTEGRATION.md."""
from __future__ import annotations

import torch

from . import _lib
from .rasterizer import _Cfg, _f32c


class _GaussianNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, scales, rotations, raster_settings):
        _lib.require_device(means3D, scales, rotations)
        means3D, scales, rotations = (_f32c(t.detach()) for t in (means3D, scales, rotations))
        P = means3D.shape[0]
        cfg = _Cfg(raster_settings)
        out = torch.empty(P, 3, dtype=torch.float32, device=means3D.device)
        _lib.check(_lib.lib().cgs_gaussian_normals_fwd(cfg.ref, P, _lib.ptr(means3D), _lib.ptr(scales), _lib.ptr(rotations),
                                                       _lib.ptr(out), _lib.current_stream()), "cgs_gaussian_normals_fwd")
        ctx.cfg = cfg
        ctx.save_for_backward(means3D, scales, rotations)
        return out

    @staticmethod
    def backward(ctx, g):
        means3D, scales, rotations = ctx.saved_tensors
        P = means3D.shape[0]
        d_rot = torch.empty(P, 4, dtype=torch.float32, device=means3D.device)      # every row is written
        _lib.check(_lib.lib().cgs_gaussian_normals_bwd(ctx.cfg.ref, P, _lib.ptr(means3D), _lib.ptr(scales), _lib.ptr(rotations),
                                                       _lib.ptr(_f32c(g)), _lib.ptr(d_rot), _lib.current_stream()),
                   "cgs_gaussian_normals_bwd")
        return None, None, d_rot, None


def gaussian_normals(means3D, scales, rotations, raster_settings):
    """[P,3] camera-space unit normals of the Gaussians, pointing away from the camera (module docstring).  P = 0 is fine."""
    P = means3D.shape[0]
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise ValueError(f"means3D must be [P, 3], got {tuple(means3D.shape)}")
    if tuple(scales.shape) != (P, 3):
        raise ValueError(f"scales must be [P, 3] = [{P}, 3], got {tuple(scales.shape)}")
    if tuple(rotations.shape) != (P, 4):
        raise ValueError(f"rotations must be [P, 4] = [{P}, 4], got {tuple(rotations.shape)}")
    return _GaussianNormals.apply(means3D, scales, rotations, raster_settings)


def _view_args(depth, raster_settings, eps):
    """(H, W, tanfovx, tanfovy, eps) of the per-pixel entry points, checked against `depth` [1,H,W] or [H,W]."""
    H, W = int(raster_settings.image_height), int(raster_settings.image_width)
    if tuple(depth.shape) not in ((1, H, W), (H, W)):
        raise ValueError(f"depth must be [1, H, W] or [H, W] with H, W = {H}, {W} of raster_settings, got {tuple(depth.shape)}")
    eps = float(eps)
    if not 0.0 <= eps < float("inf"):
        raise ValueError(f"eps must be >= 0 and finite, got {eps}")
    return H, W, float(raster_settings.tanfovx), float(raster_settings.tanfovy), eps


class _DepthNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, view):
        _lib.require_device(depth)
        depth = _f32c(depth.detach())
        out = torch.empty(3, view[0], view[1], dtype=torch.float32, device=depth.device)
        _lib.check(_lib.lib().cgs_depth_normals_fwd(*view, _lib.ptr(depth), _lib.ptr(out), _lib.current_stream()),
                   "cgs_depth_normals_fwd")
        ctx.view = view
        ctx.save_for_backward(depth)
        return out

    @staticmethod
    def backward(ctx, g):
        depth, = ctx.saved_tensors
        d_depth = torch.empty_like(depth)       # every pixel is written
        _lib.check(_lib.lib().cgs_depth_normals_bwd(*ctx.view, _lib.ptr(depth), _lib.ptr(_f32c(g)), _lib.ptr(d_depth),
                                                    _lib.current_stream()), "cgs_depth_normals_bwd")
        return d_depth, None


def depth_normals(depth, raster_settings, eps=0.0):
    """[3,H,W] camera-space normals of the surface `depth` ([1,H,W] or [H,W]) describes, pointing away from the camera; unit
    length with eps=0, the reference's visualisation with eps=1e-5 (module docstring)."""
    return _DepthNormals.apply(depth, _view_args(depth, raster_settings, eps))


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normals, depth, weight, view):
        _lib.require_device(normals, depth, weight)
        normals, depth = _f32c(normals.detach()), _f32c(depth.detach())
        weight = _f32c(weight.detach()) if weight is not None else None
        out = torch.empty(1, view[0], view[1], dtype=torch.float32, device=depth.device)
        _lib.check(_lib.lib().cgs_normal_consistency_fwd(*view, _lib.ptr(normals), _lib.ptr(depth), _lib.ptr(weight),
                                                         _lib.ptr(out), _lib.current_stream()), "cgs_normal_consistency_fwd")
        ctx.view = view
        ctx.save_for_backward(normals, depth, weight)
        return out

    @staticmethod
    def backward(ctx, g):
        normals, depth, weight = ctx.saved_tensors
        need_n, need_d = ctx.needs_input_grad[:2]
        if not (need_n or need_d):
            return None, None, None, None
        # every pixel of an output that is asked for is written; the other is not computed
        d_normals = torch.empty_like(normals) if need_n else None
        d_depth = torch.empty_like(depth) if need_d else None
        _lib.check(_lib.lib().cgs_normal_consistency_bwd(*ctx.view, _lib.ptr(normals), _lib.ptr(depth), _lib.ptr(weight),
                                                         _lib.ptr(_f32c(g)), _lib.ptr(d_normals), _lib.ptr(d_depth),
                                                         _lib.current_stream()), "cgs_normal_consistency_bwd")
        return d_normals, d_depth, None, None


def normal_consistency(normals, depth, raster_settings, weight=None, eps=0.0):
    """[1,H,W]: E = 1 - weight * <normals, depth_normals(depth, eps)>, fused (module docstring).  `normals` [3,H,W] is usually
    the rasterizer's `extras["normals"]`, `depth` the expected depth depth / alpha or the median depth; `weight` [1,H,W] or
    [H,W] is not differentiated."""
    view = _view_args(depth, raster_settings, eps)
    H, W = view[:2]
    if tuple(normals.shape) != (3, H, W):
        raise ValueError(f"normals must be [3, H, W] = [3, {H}, {W}], got {tuple(normals.shape)}")
    if weight is not None and tuple(weight.shape) not in ((1, H, W), (H, W)):
        raise ValueError(f"weight must be [1, H, W] or [H, W] with H, W = {H}, {W}, got {tuple(weight.shape)}")
    return _NormalConsistency.apply(normals, depth, weight, view)
