"""Depth regularisation against a monocular prior: aligned L1 / L2 and Pearson-correlation depth losses, fused HIP kernels
(csrc/depth_prior.hip; the definition is in include/cgs.h above cgs_depth_prior_fwd).

  x     the rendered map, [H,W] or [1,H,W]: typically `extras["invdepth"]` of `render(..., return_aux=True)`.  Differentiated.
  y     the prior (a monocular network's inverse depth), same shape.  Never differentiated.
  mask  optional [H,W] or [1,H,W].  Float values >= 0 are weights m; `bool` / `uint8` are read as bytes by the kernels (m = 1 where
        the byte is not 0), with no conversion launch.  Never differentiated.

A pixel of m = 0 is selected out, not multiplied out: its x and y may be NaN or +-Inf (sky in the prior, zero alpha in the render);
every result stays finite and that pixel's gradient is exactly +0.  With n = H W and the moments over the other pixels

  M = sum m, Sx = sum m x, Sy = sum m y, Sxx, Syy, Sxy;   Vx = M Sxx - Sx^2, Vy = M Syy - Sy^2, C = M Sxy - Sx Sy

(these differences cancel: the moments are accumulated in fp64, where a product of two fp32 inputs is exact):

  depth_prior_loss   r = x - (a y + b);  L = sum m |r| / N (kind="l1") or sum m r^2 / N ("l2");  N = M (mean_over="mask") or
                     n ("image": upstream 3DGS's `.mean()` over all pixels).  (a, b) is `affine=(a, b)` (floats, or 1-element
                     device tensors that may require grad: a learned per-view alignment), or `align="lstsq"`: a = C / Vy,
                     b = (Sx - a Sy) / M solved on the device (Vy <= 1e-12 M Syy: a = 0, b = Sx / M), constants of the backward —
                     for "l2" that is also the exact total derivative, since the normal equations make dL/da = dL/db = 0.
                     Neither given: a = 1, b = 0.  dL/dx_p = g m_p w(r_p) / N, w = sign(r) (sign(0) = 0) or 2 r;
                     dL/da = -(g / N) sum m w(r) y, dL/db = -(g / N) sum m w(r).  M = 0: L = 0 and every gradient is 0.
  pearson_depth_loss 1 - rho, rho = C / sqrt(Vx Vy); dL/dx_p = -g m_p [(M y_p - Sy) / sqrt(Vx Vy) - rho (M x_p - Sx) / Vx];
                     Vx <= 1e-12 M Sxx or Vy <= 1e-12 M Syy or M = 0: L = 1, gradient 0.
  scale_shift        the least-squares (a, b) as two float32 0-d device tensors, not differentiable (evaluation with aligned depth).

Direction.  The prior is always mapped into the RENDER's units (target = a y + b), as upstream 3DGS does with the per-image scale
and offset of its depth-params file (`-d`, `depth_l1_weight`).  MiDaS / MonoSDF align the other way (render -> prior, a x + b
against y).  Here the fitted side must be the one without a gradient: (a, b) then depend on x only through the normal equations,
which is what lets the backward treat them as constants, and the loss is measured in the units the scene is optimised in, so its
weight does not change with the prior's arbitrary scale.  The scale-free, symmetric alternative is the Pearson loss.

Launches (counted by tools/depth_prior_micro.py): forward 2 for "l2", Pearson and scale_shift, 2 for "l1" with a given affine,
4 for "l1" with align="lstsq"; backward 1, plus 2 when a or b wants a gradient.  Every sum is per-workgroup partials added by one
workgroup in index order: no float atomics, so values, (a, b), rho and every gradient are bit-reproducible from call to call and do
not depend on the 16-byte alignment of the planes.  The coefficients the backward needs stay on the device in fp64; no call
synchronises with the host or reads a count back.  The nodes are differentiable once: a second derivative through the loss
raises instead of treating d x as a constant.  Device tensors only: no CPU fallback.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib

_KINDS = {"l1": 0, "l2": 1}
_PEARSON = 2
_MEANS = {"mask": 0, "image": 1}
_MASK_NONE, _MASK_FLOAT, _MASK_BYTE = 0, 1, 2
_COEF_BYTES = 64


def _f32c(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


def _refuse_grad(ctx, who):
    for i, name in ((1, "`y` (the prior)"), (2, "`mask`")):
        if ctx.needs_input_grad[i]:
            raise NotImplementedError(f"{who}: {name} requires grad, but the fused loss differentiates `x` (the rendered map) "
                                      "only; detach it, or pass the map to optimise first")


def _check_planes(who, x, y, mask):
    """(H, W) of the planes; ValueError for anything a kernel could not take, before a device is touched."""
    for name, t in (("x", x), ("y", y)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError(f"{who}: {name} must be a float [H,W] or [1,H,W] tensor, got "
                             f"{(tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[0] != 1) or min(x.shape) < 1:
        raise ValueError(f"{who}: x must be [H,W] or [1,H,W] with H, W >= 1, got {tuple(x.shape)}")
    if y.shape != x.shape:
        raise ValueError(f"{who}: shape mismatch: x {tuple(x.shape)}, y {tuple(y.shape)}")
    H, W = x.shape[-2:]
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or not (mask.is_floating_point() or mask.dtype in (torch.bool, torch.uint8)):
            raise ValueError(f"{who}: the mask must be a float, bool or uint8 tensor, got "
                             f"{mask.dtype if isinstance(mask, torch.Tensor) else type(mask).__name__}")
        if tuple(mask.shape) not in ((H, W), (1, H, W)):
            raise ValueError(f"{who}: shape mismatch: x {tuple(x.shape)}, mask {tuple(mask.shape)}")
    return H, W


def _on_device(who, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{who}: tensor on {t.device}; the depth-prior losses run on the HIP device only, there is no CPU fallback")
    _lib.require_device(*tensors)


def _mask_arg(mask):
    """(tensor the kernel reads, mask type): bytes are passed as they are."""
    if mask is None:
        return None, _MASK_NONE
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8), _MASK_BYTE
    if mask.dtype == torch.uint8:
        return mask.contiguous(), _MASK_BYTE
    return _f32c(mask), _MASK_FLOAT


def _scratch(L, H, W, device):
    nbytes = int(L.cgs_depth_prior_scratch_bytes(H, W))
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device), nbytes


def _g32(gout):
    return gout if gout.dtype == torch.float32 else gout.float()       # (one element: contiguous in any shape)


def _keep(ctx, x, xs, ys, m, coef, mask_type):
    """What the backward needs: the tensors by reference (they keep the planes alive), their addresses, the input's shape and type."""
    ctx.save_for_backward(xs, ys, m, coef)
    ctx.ptrs = (xs.data_ptr(), ys.data_ptr(), None if m is None else m.data_ptr(), mask_type, x.shape[-2], x.shape[-1])
    ctx.coef_ptr = coef.data_ptr()
    ctx.like = (x.shape, x.dtype, x.device)


def _backward(ctx, gout, kind, need_x, need_ab):
    """(dx or None, dab [2] or None): one launch for dx, two for d (a, b); the graph's buffers, the upstream gradient, the library
    and the stream are looked up once for both."""
    ctx.saved_tensors                                                   # (raises once the graph's buffers have been freed)
    g32 = _g32(gout)                                                    # (kept until the launches are queued)
    g = g32.data_ptr()
    L, st = _lib.lib(), _lib.current_stream()
    shape, dtype, device = ctx.like
    dx = dab = None
    if need_x:
        dx = torch.empty(shape, dtype=torch.float32, device=device)
        rc = L.cgs_depth_prior_bwd(*ctx.ptrs, kind, ctx.coef_ptr, g, dx.data_ptr(), st)
        if rc:
            _lib.check(rc, "cgs_depth_prior_bwd")
        if dtype != torch.float32:
            dx = dx.to(dtype)
    if need_ab:
        dab = torch.empty(2, dtype=torch.float32, device=device)
        scratch, nbytes = _scratch(L, ctx.ptrs[4], ctx.ptrs[5], device)
        _lib.check(L.cgs_depth_prior_dab(*ctx.ptrs, kind, ctx.coef_ptr, g, dab.data_ptr(), scratch.data_ptr(), nbytes, st),
                   "cgs_depth_prior_dab")
    return dx, dab


class _DepthPrior(torch.autograd.Function):
    """L1 / L2 against a y + b as one node.  a_t / b_t: 1-element device tensors or None (then the float a_f / b_f)."""

    @staticmethod
    def forward(ctx, x, y, mask, a_t, b_t, kind, lstsq, mean_over, a_f, b_f):
        _refuse_grad(ctx, "depth_prior_loss")
        _on_device("depth_prior_loss", x, y, mask, a_t, b_t)
        H, W = x.shape[-2:]
        xs, ys = _f32c(x), _f32c(y)
        m, mask_type = _mask_arg(mask)
        a32 = None if a_t is None else _f32c(a_t.detach()).reshape(1)
        b32 = None if b_t is None else _f32c(b_t.detach()).reshape(1)
        L = _lib.lib()
        out = torch.empty((), dtype=torch.float32, device=x.device)
        coef = torch.empty(_COEF_BYTES // 8, dtype=torch.float64, device=x.device)
        scratch, nbytes = _scratch(L, H, W, x.device)
        st = _lib.current_stream()
        _lib.check(L.cgs_depth_prior_fwd(_lib.ptr(xs), _lib.ptr(ys), _lib.ptr(m), mask_type, H, W, kind, int(lstsq), mean_over, a_f, b_f,
                                         _lib.ptr(a32), _lib.ptr(b32), out.data_ptr(), _lib.ptr(coef), _lib.ptr(scratch), nbytes, st),
                   "cgs_depth_prior_fwd")
        need_a = a_t is not None and ctx.needs_input_grad[3]
        need_b = b_t is not None and ctx.needs_input_grad[4]
        if ctx.needs_input_grad[0] or need_a or need_b:
            _keep(ctx, x, xs, ys, m, coef, mask_type)
        ctx.kind = kind
        ctx.ab_like = tuple(None if t is None else (t.shape, t.dtype) for t in (a_t, b_t))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        need_x, need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        dx, dab = _backward(ctx, gout, ctx.kind, need_x, need_a or need_b)
        da = dab[0].reshape(ctx.ab_like[0][0]).to(ctx.ab_like[0][1]) if need_a else None
        db = dab[1].reshape(ctx.ab_like[1][0]).to(ctx.ab_like[1][1]) if need_b else None
        return dx, None, None, da, db, None, None, None, None, None


class _Pearson(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, mask):
        _refuse_grad(ctx, "pearson_depth_loss")
        _on_device("pearson_depth_loss", x, y, mask)
        H, W = x.shape[-2:]
        xs, ys = _f32c(x), _f32c(y)
        m, mask_type = _mask_arg(mask)
        L = _lib.lib()
        out = torch.empty((), dtype=torch.float32, device=x.device)
        coef = torch.empty(_COEF_BYTES // 8, dtype=torch.float64, device=x.device)
        scratch, nbytes = _scratch(L, H, W, x.device)
        st = _lib.current_stream()
        _lib.check(L.cgs_depth_prior_fwd(_lib.ptr(xs), _lib.ptr(ys), _lib.ptr(m), mask_type, H, W, _PEARSON, 0, 0, 0.0, 0.0, None, None,
                                         out.data_ptr(), _lib.ptr(coef), _lib.ptr(scratch), nbytes, st), "cgs_depth_prior_fwd")
        if ctx.needs_input_grad[0]:
            _keep(ctx, x, xs, ys, m, coef, mask_type)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        return _backward(ctx, gout, _PEARSON, True, False)[0], None, None


def _affine_arg(who, v, name):
    """(device tensor or None, float): a float, a CPU tensor without grad (read here, on the host) or a 1-element device tensor."""
    if isinstance(v, torch.Tensor):
        if v.numel() != 1 or not v.is_floating_point():
            raise ValueError(f"{who}: affine {name} must be a float or a 1-element float tensor, got {tuple(v.shape)} {v.dtype}")
        if v.is_cuda or v.requires_grad:
            return v, 0.0
        return None, float(v)
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(f"{who}: affine {name} must be a float or a 1-element float tensor, got {type(v).__name__}")
    return None, float(v)


def depth_prior_loss(x, y, mask=None, *, kind="l1", affine=None, align=None, mean_over="mask"):
    """sum m |x - (a y + b)| / N or sum m (x - (a y + b))^2 / N as one autograd node (module docstring).  Other float types and
    layouts of x, y and a float mask are converted to contiguous float32 first; gradients come back in the inputs' own types."""
    who = "depth_prior_loss"
    if kind not in _KINDS:
        raise ValueError(f"{who}: kind must be 'l1' or 'l2', got {kind!r}")
    if mean_over not in _MEANS:
        raise ValueError(f"{who}: mean_over must be 'mask' or 'image', got {mean_over!r}")
    if affine is not None and align is not None:
        raise ValueError(f"{who}: give affine=(a, b) or align='lstsq', not both")
    if align not in (None, "lstsq"):
        raise ValueError(f"{who}: align must be None or 'lstsq', got {align!r}")
    a_t = b_t = None
    a_f, b_f = 1.0, 0.0
    if affine is not None:
        if not isinstance(affine, (tuple, list)) or len(affine) != 2:
            raise ValueError(f"{who}: affine must be a pair (a, b)")
        a_t, a_f = _affine_arg(who, affine[0], "a")
        b_t, b_f = _affine_arg(who, affine[1], "b")
    _check_planes(who, x, y, mask)
    return _DepthPrior.apply(x, y, mask, a_t, b_t, _KINDS[kind], align == "lstsq", _MEANS[mean_over], a_f, b_f)


def pearson_depth_loss(x, y, mask=None):
    """1 - the (weighted) Pearson correlation of x and y over the masked pixels, one autograd node (module docstring)."""
    _check_planes("pearson_depth_loss", x, y, mask)
    return _Pearson.apply(x, y, mask)


def scale_shift(x, y, mask=None):
    """The least-squares (a, b) of a y + b against x over the masked pixels: two float32 0-d device tensors, no gradient."""
    H, W = _check_planes("scale_shift", x, y, mask)
    _on_device("scale_shift", x, y, mask)
    xs, ys = _f32c(x.detach()), _f32c(y.detach())
    m, mask_type = _mask_arg(None if mask is None else mask.detach())
    L = _lib.lib()
    ab = torch.empty(2, dtype=torch.float32, device=x.device)
    scratch, nbytes = _scratch(L, H, W, x.device)
    _lib.check(L.cgs_depth_prior_scale_shift(_lib.ptr(xs), _lib.ptr(ys), _lib.ptr(m), mask_type, H, W, _lib.ptr(ab), _lib.ptr(scratch),
                                             nbytes, _lib.current_stream()), "cgs_depth_prior_scale_shift")
    return ab[0], ab[1]
