"""Drop-in for the reference's utils/loss_utils.py (`l1_loss`, `l2_loss`, `ssim`) — SURVEY section 8(f) rank 2.

`ssim` (11x11 Gaussian window, sigma 1.5, zero padding, per channel, mean; utils/loss_utils.py:33-63) and
`l1_loss` run as ONE fused HIP launch forward and one backward (csrc/loss.hip, `cgs_l1_ssim_{fwd,bwd}`) instead
of five grouped conv2d + ~15 element-wise passes each way.  `l1_ssim(image, gt)` returns both means from a
single launch; `ssim` / `l1_loss` keep the reference's signatures.  `scaling_reg` and `mask_reg` are the two
regularisers train.py:203,209 adds to the image terms, one launch each way (torch's `prod` backward reads a zero
count back on the host in the middle of every backward).  Device tensors only: there is no CPU path.
"""
from __future__ import annotations

import torch

from . import _lib


def _refuse_target_grad(ctx, who):
    if ctx.needs_input_grad[1]:
        raise NotImplementedError(f"{who}: `gt` (the second image) requires grad, but the fused loss differentiates the first image "
                                  "only; detach the target, or pass the image to optimise first")


class _L1Ssim(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, gt):
        _refuse_target_grad(ctx, "l1_ssim")
        _lib.require_device(img, gt)
        x = img if (img.dtype == torch.float32 and img.is_contiguous()) else img.float().contiguous()
        y = gt if (gt.dtype == torch.float32 and gt.is_contiguous()) else gt.float().contiguous()
        if x.shape != y.shape or x.dim() != 3:
            raise ValueError("l1_ssim expects two [C,H,W] images of the same shape")
        C, H, W = x.shape
        L = _lib.lib()
        need = ctx.needs_input_grad[0]
        maps = torch.empty(3, C, H, W, dtype=torch.float32, device=x.device) if need else None
        partials = torch.empty(int(L.cgs_l1_ssim_partials(C, H, W)), 2, dtype=torch.float32, device=x.device)
        _lib.check(L.cgs_l1_ssim_fwd(_lib.ptr(x), _lib.ptr(y), C, H, W, _lib.ptr(maps), _lib.ptr(partials),
                                     _lib.current_stream()), "cgs_l1_ssim_fwd")
        sums = partials.sum(dim=0) / float(C * H * W)
        if need:
            ctx.save_for_backward(x, y, maps)
        return sums[0], sums[1]

    @staticmethod
    def backward(ctx, g_l1, g_ssim):
        x, y, maps = ctx.saved_tensors
        C, H, W = x.shape
        z = torch.zeros((), dtype=torch.float32, device=x.device)
        g = torch.stack([z if g_l1 is None else g_l1.float().reshape(()), z if g_ssim is None else g_ssim.float().reshape(())])
        dimg = torch.empty_like(x)
        _lib.check(_lib.lib().cgs_l1_ssim_bwd(_lib.ptr(x), _lib.ptr(y), _lib.ptr(maps), _lib.ptr(g), C, H, W,
                                              _lib.ptr(dimg), _lib.current_stream()), "cgs_l1_ssim_bwd")
        return dimg, None


def l1_ssim(image: torch.Tensor, gt: torch.Tensor):
    """(mean |image - gt|, mean SSIM) of two [C,H,W] images from one fused launch."""
    if image.dim() == 4 and image.shape[0] == 1:
        image, gt = image[0], gt[0]
    return _L1Ssim.apply(image, gt)


def l1_loss(network_output, gt):                                    # utils/loss_utils.py:17-18
    if network_output.is_cuda and network_output.dim() == 3 and network_output.shape == gt.shape:
        return l1_ssim(network_output, gt)[0]
    return torch.abs(network_output - gt).mean()


def l2_loss(network_output, gt):                                    # :20-21
    return ((network_output - gt) ** 2).mean()


def ssim(img1, img2, window_size=11, size_average=True):            # :33-63
    if window_size != 11 or not size_average:
        raise NotImplementedError("the fused SSIM implements the training configuration: window 11, mean")
    return l1_ssim(img1, img2)[1]


class _TrainImageLoss(torch.autograd.Function):
    """(loss, L1, SSIM) with loss = (1 - lam) L1 + lam (1 - SSIM) as ONE node: the forward kernel, a single-workgroup finish
    launch (partials -> the three values) and one backward launch that reads the gradient of `loss` on the device — the scalar
    arithmetic around _L1Ssim cost ~14 tiny launches per training step (profiles/r06_loss.txt)."""

    @staticmethod
    def forward(ctx, img, gt, lam):
        _refuse_target_grad(ctx, "training_image_loss")
        _lib.require_device(img, gt)
        x = img if (img.dtype == torch.float32 and img.is_contiguous()) else img.float().contiguous()
        y = gt if (gt.dtype == torch.float32 and gt.is_contiguous()) else gt.float().contiguous()
        if x.shape != y.shape or x.dim() != 3:
            raise ValueError("training_image_loss expects two [C,H,W] images of the same shape")
        C, H, W = x.shape
        L = _lib.lib()
        need = ctx.needs_input_grad[0]
        maps = torch.empty(3, C, H, W, dtype=torch.float32, device=x.device) if need else None
        partials = torch.empty(int(L.cgs_l1_ssim_partials(C, H, W)), 2, dtype=torch.float32, device=x.device)
        st = _lib.current_stream()
        _lib.check(L.cgs_l1_ssim_fwd(_lib.ptr(x), _lib.ptr(y), C, H, W, _lib.ptr(maps), _lib.ptr(partials), st), "cgs_l1_ssim_fwd")
        out3 = torch.empty(3, dtype=torch.float32, device=x.device)
        _lib.check(L.cgs_l1_ssim_finish(_lib.ptr(partials), C, H, W, float(lam), _lib.ptr(out3), st), "cgs_l1_ssim_finish")
        if need:
            ctx.save_for_backward(x, y, maps)
        ctx.lam = float(lam)
        ctx.set_materialize_grads(False)
        return out3[0], out3[1], out3[2]

    @staticmethod
    def backward(ctx, g_loss, g_l1, g_ssim):
        x, y, maps = ctx.saved_tensors
        C, H, W = x.shape
        g2 = None
        if g_l1 is not None or g_ssim is not None:      # (L1 / SSIM read by the objective as well: rare — they are logged)
            z = torch.zeros((), dtype=torch.float32, device=x.device)
            g2 = torch.stack([z if g_l1 is None else g_l1.float().reshape(()), z if g_ssim is None else g_ssim.float().reshape(())])
        if g_loss is None and g2 is None:
            return None, None, None
        gl = None if g_loss is None else g_loss.float().reshape(1).contiguous()
        dimg = torch.empty_like(x)
        _lib.check(_lib.lib().cgs_l1_ssim_bwd_loss(_lib.ptr(x), _lib.ptr(y), _lib.ptr(maps), _lib.ptr(gl), _lib.ptr(g2), ctx.lam, C, H, W,
                                                   _lib.ptr(dimg), _lib.current_stream()), "cgs_l1_ssim_bwd_loss")
        return dimg, None, None


def training_image_loss(image, gt, lambda_dssim: float = 0.2):
    """((1 - lambda) L1 + lambda (1 - SSIM), L1, SSIM) of train.py:199-204 from one node (three launches per training step)."""
    if image.dim() == 4 and image.shape[0] == 1:
        image, gt = image[0], gt[0]
    if image.is_cuda and image.dim() == 3 and image.shape == gt.shape:
        return _TrainImageLoss.apply(image, gt, float(lambda_dssim))
    l1, s = l1_ssim(image, gt)
    return (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - s), l1, s


class _MeanReg(torch.autograd.Function):
    """mean over rows of prod(dim=1) ([P,3], kind 0) or mean of sigmoid (any shape, kind 1): csrc/loss.hip."""

    @staticmethod
    def forward(ctx, x, kind):
        _lib.require_device(x)
        x = x if (x.dtype == torch.float32 and x.is_contiguous() and x.data_ptr() % 16 == 0) else x.float().contiguous().clone()
        L = _lib.lib()
        n = x.shape[0] if kind == 0 else x.numel()
        fwd = L.cgs_scaling_reg_fwd if kind == 0 else L.cgs_sigmoid_mean_fwd
        partials = torch.empty(int(L.cgs_reg_partials(n)), dtype=torch.float32, device=x.device)
        _lib.check(fwd(_lib.ptr(x), n, _lib.ptr(partials), _lib.current_stream()), "cgs_reg_fwd")
        ctx.kind, ctx.n = kind, n
        ctx.save_for_backward(x)
        return partials.sum() / float(n)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        L = _lib.lib()
        bwd = L.cgs_scaling_reg_bwd if ctx.kind == 0 else L.cgs_sigmoid_mean_bwd
        d = torch.empty_like(x)
        _lib.check(bwd(_lib.ptr(x), _lib.ptr(g.float().reshape(1).contiguous()), ctx.n, _lib.ptr(d), _lib.current_stream()),
                   "cgs_reg_bwd")
        return d, None


def scaling_reg(scaling: torch.Tensor):
    """`scaling.prod(dim=1).mean()` of train.py:203 for the rendered Gaussians' scales [P,3] (render()'s "scaling")."""
    if scaling.dim() != 2 or scaling.shape[1] != 3:
        raise ValueError("scaling_reg expects [P,3]")
    if scaling.shape[0] == 0:
        return scaling.prod(dim=1).mean()           # nan, as the reference's expression on an empty view
    return _MeanReg.apply(scaling, 0)


def mask_reg(mask: torch.Tensor):
    """`torch.mean(torch.sigmoid(gaussians._mask))` of train.py:209."""
    if mask.numel() == 0:
        return torch.mean(torch.sigmoid(mask))
    return _MeanReg.apply(mask, 1)


_WSUM_SCRATCH = {}


class _WeightedImageSum(torch.autograd.Function):
    """sum(image * w) + lam * rate as ONE node and one launch each way (cgs_weighted_sum_*): the linear objective bench.py puts
    behind render() — torch's mul / sum / mul / add chain and its backward are nine launches, a dot-product node five."""

    @staticmethod
    def forward(ctx, img, w, rate, lam):
        L = _lib.lib()
        _lib.require_device(img, w)
        img_c, w_c = img.detach().float().contiguous(), w.detach().float().contiguous()
        assert img_c.numel() == w_c.numel()
        dev = img_c.device
        ws = _WSUM_SCRATCH.get(dev)
        if ws is None:
            ws = _WSUM_SCRATCH[dev] = torch.zeros(int(L.cgs_weighted_sum_scratch_bytes()), dtype=torch.uint8, device=dev)
        rate_c = None if rate is None else rate.detach().float().reshape(1).contiguous()
        out = torch.empty(1, dtype=torch.float32, device=dev)
        _lib.check(L.cgs_weighted_sum_fwd(_lib.ptr(img_c), _lib.ptr(w_c), img_c.numel(), _lib.ptr(rate_c), float(lam), _lib.ptr(ws),
                                          ws.numel(), _lib.ptr(out), _lib.current_stream()), "cgs_weighted_sum_fwd")
        ctx.save_for_backward(w_c)
        ctx.lam, ctx.img_shape, ctx.rate_shape = float(lam), img.shape, (None if rate is None else rate.shape)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        (w_c,) = ctx.saved_tensors
        L = _lib.lib()
        g = g.float().reshape(1).contiguous()
        dimg = torch.empty(ctx.img_shape, dtype=torch.float32, device=w_c.device)
        drate = torch.empty(1, dtype=torch.float32, device=w_c.device) if ctx.rate_shape is not None else None
        _lib.check(L.cgs_weighted_sum_bwd(_lib.ptr(g), _lib.ptr(w_c), w_c.numel(), ctx.lam, _lib.ptr(dimg), _lib.ptr(drate),
                                          _lib.current_stream()), "cgs_weighted_sum_bwd")
        return dimg, None, (None if drate is None else drate.reshape(ctx.rate_shape)), None


def weighted_image_sum(image, w, rate=None, lam=0.0):
    """sum(image * w) + lam * rate (rate: a one-element tensor or None) — see _WeightedImageSum."""
    return _WeightedImageSum.apply(image, w, rate, lam)
