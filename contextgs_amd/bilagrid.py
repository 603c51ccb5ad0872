"""Per-view bilateral grids: the strong form of appearance compensation (Bilateral Guided Radiance Field Processing; gsplat's
`bilagrid`), next to the global per-view affine map of contextgs_amd/exposure.py.

Each training image owns a small 3-D grid G [12, L, Gh, Gw] of 3x4 affine colour maps (channel 4 i + j = A[i][j]), indexed by the
pixel's position and the render's own luminance and sliced per pixel.  For pixel (y, x) of a [3,H,W] image with colour (r, g, b):

  gx = (x + 0.5) / W (Gw - 1),  gy = (y + 0.5) / H (Gh - 1),  z = 0.299 r + 0.587 g + 0.114 b,  gz = clamp(z (L - 1), 0, L - 1)
  per axis of n nodes: i0 = clamp(floor(g), 0, n - 1), i1 = min(i0 + 1, n - 1), f = g - i0, weights 1 - f on i0 and f on i1
  A = sum over the 8 corners of wz wy wx G[:, zi, yi, xi];   out_i = sum_j A[i][j] rgb_j + A[i][3]

which is `grid_sample(mode='bilinear', align_corners=True, padding_mode='border')` of the grid followed by the affine map.  The
guidance is the image itself, so d image has a second term through gz, zero where the guidance is clamped.  The slice, d image and
d grid are fused HIP kernels (csrc/bilagrid.hip); d grid uses no float atomics and is bit-reproducible.  The total-variation term
`tv_loss()` = (1/N) sum over views and axes of (sum of squared forward differences) / (their number per view) keeps the grids smooth.

  grids = BilateralGrid(len(train_cameras)).cuda()
  grid_opt = torch.optim.Adam(grids.parameters(), lr=2e-3, eps=1e-15)    # its own optimizer, or one more group of the scene's
  image = render(...)["render"]
  image = grids(image, cam.uid)                                         # between render() and the loss
  loss, l1, ssim = training_image_loss(image, gt, 0.2)
  (loss + 10.0 * grids.tv_loss()).backward(); grid_opt.step()

Only the used view's slab of `grids.grad` receives a non-zero gradient from the slice (a dense [N, 12, L, Gh, Gw] gradient: 98 KB
per view at the default size); the TV term touches every view.  Evaluate without the grids.  Device tensors only: no CPU fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib


def _f32c(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


def _on_device(who, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{who}: tensor on {t.device}; the bilateral grid runs on the HIP device only, there is no CPU fallback")
    _lib.require_device(*tensors)


class _Slice(torch.autograd.Function):
    """out = slice(grid, image) as one node: one launch forward; backward one launch for d image, two for d grid."""

    @staticmethod
    def forward(ctx, grid, image):
        _on_device("bilagrid_slice", grid, image)
        g, x = _f32c(grid), _f32c(image)
        _, Lz, Gh, Gw = g.shape
        _, H, W = x.shape
        out = torch.empty_like(x)
        _lib.check(_lib.lib().cgs_bilagrid_slice_fwd(_lib.ptr(g), Lz, Gh, Gw, _lib.ptr(x), H, W, _lib.ptr(out), _lib.current_stream()),
                   "cgs_bilagrid_slice_fwd")
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(g, x)
        ctx.like = (grid.dtype, image.dtype)
        return out.to(image.dtype)

    @staticmethod
    def backward(ctx, dout):
        g, x = ctx.saved_tensors
        _, Lz, Gh, Gw = g.shape
        _, H, W = x.shape
        L = _lib.lib()
        need_g, need_x = ctx.needs_input_grad
        d = _f32c(dout)
        dimg = torch.empty_like(x) if need_x else None
        dgrid = scratch = None
        nbytes = 0
        if need_g:
            dgrid = torch.empty_like(g)
            nbytes = int(L.cgs_bilagrid_bwd_scratch_bytes(Lz, Gh, Gw, H, W))
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=g.device)
        _lib.check(L.cgs_bilagrid_slice_bwd(_lib.ptr(g), Lz, Gh, Gw, _lib.ptr(x), _lib.ptr(d), H, W, _lib.ptr(dimg), _lib.ptr(dgrid),
                                            _lib.ptr(scratch), nbytes, _lib.current_stream()), "cgs_bilagrid_slice_bwd")
        return (None if dgrid is None else dgrid.to(ctx.like[0])), (None if dimg is None else dimg.to(ctx.like[1]))


class _TV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        _on_device("bilagrid tv_loss", grids)
        g = _f32c(grids)
        N, _, Lz, Gh, Gw = g.shape
        L = _lib.lib()
        out = torch.empty(1, dtype=torch.float32, device=g.device)
        scratch = torch.empty(int(L.cgs_bilagrid_tv_scratch_bytes(N, Lz, Gh, Gw)), dtype=torch.uint8, device=g.device)
        _lib.check(L.cgs_bilagrid_tv_fwd(_lib.ptr(g), N, Lz, Gh, Gw, _lib.ptr(out), _lib.ptr(scratch), _lib.current_stream()),
                   "cgs_bilagrid_tv_fwd")
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(g)
        ctx.like = grids.dtype
        return out.reshape(())

    @staticmethod
    def backward(ctx, gout):
        (g,) = ctx.saved_tensors
        N, _, Lz, Gh, Gw = g.shape
        d = torch.empty_like(g)
        _lib.check(_lib.lib().cgs_bilagrid_tv_bwd(_lib.ptr(g), N, Lz, Gh, Gw, _lib.ptr(gout.float().reshape(1).contiguous()), _lib.ptr(d),
                                                  _lib.current_stream()), "cgs_bilagrid_tv_bwd")
        return d.to(ctx.like)


def _check_grid(who, grid, rank):
    shape = "[12, L, Gh, Gw]" if rank == 4 else "[N, 12, L, Gh, Gw]"
    if not isinstance(grid, torch.Tensor) or grid.dim() != rank or grid.shape[rank - 4] != 12 or not grid.is_floating_point() \
            or min(grid.shape) < 1:
        raise ValueError(f"{who}: the grid must be a float {shape} tensor, got "
                         f"{tuple(grid.shape) if isinstance(grid, torch.Tensor) else type(grid).__name__}")


def _check_image(who, image, grid):
    if not isinstance(image, torch.Tensor) or image.dim() != 3 or not image.is_floating_point() or min(image.shape) < 1:
        raise ValueError(f"{who}: the image must be a float [3, H, W] tensor, got "
                         f"{tuple(image.shape) if isinstance(image, torch.Tensor) else type(image).__name__}")
    if image.shape[0] != 3:
        raise ValueError(f"{who}: a bilateral grid needs a three-channel image, got C = {image.shape[0]}")
    if image.device != grid.device:
        raise ValueError(f"{who}: image on {image.device}, grid on {grid.device}")


def bilagrid_slice(grid: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
    """The [3,H,W] image sliced through one view's grid [12, L, Gh, Gw] (module docstring), as one autograd node.  Either input may
    require grad; with neither, the call is one launch and keeps nothing.  Other float types and layouts are converted to
    contiguous float32 first; the gradients come back in the inputs' own types."""
    _check_grid("bilagrid_slice", grid, 4)
    _check_image("bilagrid_slice", image, grid)
    return _Slice.apply(grid, image)


def bilagrid_tv(grids: torch.Tensor) -> torch.Tensor:
    """The total-variation scalar of grids [N, 12, L, Gh, Gw] (module docstring), one autograd node."""
    _check_grid("bilagrid_tv", grids, 5)
    return _TV.apply(grids)


class BilateralGrid(nn.Module):
    """See the module docstring.  `grids` [n_views, 12, grid_w, grid_y, grid_x] (luminance, y, x nodes) is the only parameter,
    initialised to the identity map: channels 0, 5 and 10 are 1, the rest 0."""

    def __init__(self, n_views: int, grid_x: int = 16, grid_y: int = 16, grid_w: int = 8, device=None):
        super().__init__()
        if n_views < 1 or grid_x < 1 or grid_y < 1 or grid_w < 1:
            raise ValueError("BilateralGrid needs at least one view and one node per axis")
        eye = torch.eye(3, 4, dtype=torch.float32, device=device).reshape(1, 12, 1, 1, 1)
        self.grids = nn.Parameter(eye.repeat(n_views, 1, grid_w, grid_y, grid_x))

    def forward(self, image: torch.Tensor, i: int) -> torch.Tensor:
        """The image of view i through its grid, [3,H,W], through autograd (to the image and to `grids[i]`)."""
        n = self.grids.shape[0]
        if not isinstance(i, int) or isinstance(i, bool) or not 0 <= i < n:
            raise IndexError(f"BilateralGrid: view index {i!r} outside [0, {n})")
        _check_image("BilateralGrid", image, self.grids)
        return bilagrid_slice(self.grids[i], image)

    def tv_loss(self) -> torch.Tensor:
        return bilagrid_tv(self.grids)
