"""Drop-in for the reference's utils/loss_utils.py (`l1_loss`, `l2_loss`, `ssim`) — SURVEY section 8(f) rank 2.

`ssim` (11x11 Gaussian window, sigma 1.5, zero padding, per channel, mean; utils/loss_utils.py:33-63) and
`l1_loss` run as ONE fused HIP launch forward and one backward (csrc/loss.hip, `cgs_l1_ssim_{fwd,bwd}`) instead
of five grouped conv2d + ~15 element-wise passes each way.  `l1_ssim(image, gt)` returns both means from a
single launch; `ssim` / `l1_loss` keep the reference's signatures.  `scaling_reg` and `mask_reg` are the two
regularisers train.py:203,209 adds to the image terms, one launch each way (torch's `prod` backward reads a zero
count back on the host in the middle of every backward).  Device tensors only: there is no CPU path.

`training_image_loss(image, gt, lambda_dssim, *, weight=None, exposure=None)` is train.py:199-204 as one node.  With both
keywords None it is the plain node: the same three launches and kernels.  Otherwise, still one node (`cgs_l1_ssim_w_*`), with
x = image, y = gt, both [C,H,W]:

  exposure  E, a float [3,4] device tensor that may require grad (needs C == 3; contextgs_amd/exposure.py holds one per view):
            the loss is computed on  x'_c(p) = sum_k x_k(p) E[k,c] + E[c,3]  — upstream 3DGS's convention,
            matmul(image.permute(1,2,0), E[:3,:3]).permute(2,0,1) + E[:3,3,None,None].  Nothing is clamped.  Without it x' = x.
  weight    w, [H,W] or [1,H,W] on the device, float32 / fp16 / bf16 / bool (converted to float32 once), shared by the channels
            (a mask, or a soft per-pixel weight).  With S = sum_p w_p:
                L1   = sum_{c,p} w_p |x'_c(p) - y_c(p)| / (C S)
                SSIM = sum_{c,p} w_p ssim_c(p) / (C S)
                loss = (1 - lambda) L1 + lambda (1 - SSIM)
            ssim_c(p) is the SSIM map of (x', y) as ever: same window, zero padding and tap order.  A window's statistics see
            every pixel, weighted or not — the weight applies to the MAP, not to the inputs — so a pixel of weight 0 within
            five pixels of a weighted one does receive an SSIM gradient, and exactly none from L1.  A weighted mean keeps the
            image term on one scale whatever the mask's area (it is added to lambda_e * bits).  Without it w = 1, S = H W.
            S == 0 returns (0, 0, 1) and exact zero gradients, decided on the device.  Negative or non-finite weights are the
            caller's error (checking would need a host read); a weight that requires grad raises NotImplementedError.
  gradients with G_c(p) = dL/dx'_c(p):  dL/dx_k(p) = sum_c E[k,c] G_c(p),  dL/dE[k,c] = sum_p x_k(p) G_c(p),
            dL/dE[c,3] = sum_p G_c(p); any of loss, L1, SSIM may have received a gradient.  Neither x' nor G is written to
            memory; the 12 sums of dE are per-workgroup partials added in a fixed order by a single-workgroup launch (no float
            atomics), so two runs are bit-identical.  Launches: forward 2, backward 1, or 2 when the exposure requires grad.
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


class _TrainImageLossWeighted(torch.autograd.Function):
    """_TrainImageLoss with a per-pixel weight and / or a per-view exposure (module docstring): still one node — the forward kernel
    and its finish (which leaves 1 / (C S) on the device), one backward launch, and the 12 sums of dE from per-tile partials by a
    single-workgroup launch when the exposure asks for a gradient.  `w` is float32 [H,W] or None, `E` float32 [3,4] or None."""

    @staticmethod
    def forward(ctx, img, gt, lam, w, E):
        _refuse_target_grad(ctx, "training_image_loss")
        _lib.require_device(img, gt, w, E)
        x = img if (img.dtype == torch.float32 and img.is_contiguous()) else img.float().contiguous()
        y = gt if (gt.dtype == torch.float32 and gt.is_contiguous()) else gt.float().contiguous()
        e = None if E is None else (E if (E.dtype == torch.float32 and E.is_contiguous()) else E.float().contiguous())
        C, H, W = x.shape
        L = _lib.lib()
        need_x, need_e = ctx.needs_input_grad[0], e is not None and ctx.needs_input_grad[4]
        maps = torch.empty(3, C, H, W, dtype=torch.float32, device=x.device) if (need_x or need_e) else None
        partials = torch.empty(int(L.cgs_l1_ssim_partials(C, H, W)), 3, dtype=torch.float32, device=x.device)
        st = _lib.current_stream()
        _lib.check(L.cgs_l1_ssim_w_fwd(_lib.ptr(x), _lib.ptr(y), _lib.ptr(w), _lib.ptr(e), C, H, W, _lib.ptr(maps), _lib.ptr(partials), st),
                   "cgs_l1_ssim_w_fwd")
        out3 = torch.empty(3, dtype=torch.float32, device=x.device)
        inv_cs = torch.empty(1, dtype=torch.float32, device=x.device)
        _lib.check(L.cgs_l1_ssim_w_finish(_lib.ptr(partials), C, H, W, float(lam), _lib.ptr(out3), _lib.ptr(inv_cs), st), "cgs_l1_ssim_w_finish")
        if maps is not None:
            ctx.save_for_backward(x, y, maps, inv_cs, w, e)
        ctx.lam, ctx.need_x, ctx.need_e = float(lam), need_x, need_e
        ctx.e_like = None if E is None else (E.shape, E.dtype)
        ctx.set_materialize_grads(False)
        return out3[0], out3[1], out3[2]

    @staticmethod
    def backward(ctx, g_loss, g_l1, g_ssim):
        x, y, maps, inv_cs, w, e = ctx.saved_tensors
        C, H, W = x.shape
        g2 = None
        if g_l1 is not None or g_ssim is not None:
            z = torch.zeros((), dtype=torch.float32, device=x.device)
            g2 = torch.stack([z if g_l1 is None else g_l1.float().reshape(()), z if g_ssim is None else g_ssim.float().reshape(())])
        if g_loss is None and g2 is None:
            return None, None, None, None, None
        gl = None if g_loss is None else g_loss.float().reshape(1).contiguous()
        L = _lib.lib()
        st = _lib.current_stream()
        dimg = torch.empty_like(x) if ctx.need_x else None
        part = torch.empty(int(L.cgs_l1_ssim_partials(1, H, W)), 12, dtype=torch.float32, device=x.device) if ctx.need_e else None
        _lib.check(L.cgs_l1_ssim_w_bwd(_lib.ptr(x), _lib.ptr(y), _lib.ptr(w), _lib.ptr(e), _lib.ptr(maps), _lib.ptr(inv_cs), _lib.ptr(gl),
                                       _lib.ptr(g2), ctx.lam, C, H, W, _lib.ptr(dimg), _lib.ptr(part), st), "cgs_l1_ssim_w_bwd")
        dE = None
        if ctx.need_e:
            dE = torch.empty(3, 4, dtype=torch.float32, device=x.device)
            _lib.check(L.cgs_l1_ssim_w_dexposure(_lib.ptr(part), H, W, _lib.ptr(dE), st), "cgs_l1_ssim_w_dexposure")
            dE = dE.reshape(ctx.e_like[0]).to(ctx.e_like[1])
        return dimg, None, None, None, dE


def _loss_weight(weight, H, W, image):
    """The float32 contiguous [H,W] form of a [H,W] / [1,H,W] weight, checked without touching the device."""
    if not isinstance(weight, torch.Tensor) or tuple(weight.shape) not in ((H, W), (1, H, W)):
        raise ValueError(f"training_image_loss: weight must be a [{H},{W}] or [1,{H},{W}] tensor, got "
                         f"{tuple(weight.shape) if isinstance(weight, torch.Tensor) else type(weight).__name__}")
    if weight.requires_grad:
        raise NotImplementedError("training_image_loss: `weight` requires grad, but the fused loss differentiates the image and the "
                                  "exposure only; detach the weight")
    if not (weight.dtype in (torch.float32, torch.float16, torch.bfloat16, torch.bool)):
        raise ValueError(f"training_image_loss: weight must be float32, float16, bfloat16 or bool, got {weight.dtype}")
    if weight.device != image.device:
        raise ValueError(f"training_image_loss: weight on {weight.device}, image on {image.device}")
    return weight.reshape(H, W).to(torch.float32).contiguous()


def _loss_exposure(exposure, C, image):
    if not isinstance(exposure, torch.Tensor) or tuple(exposure.shape) != (3, 4) or not exposure.is_floating_point():
        raise ValueError("training_image_loss: exposure must be a float [3,4] tensor (a 3x3 colour matrix and a bias column), got "
                         f"{tuple(exposure.shape) if isinstance(exposure, torch.Tensor) else type(exposure).__name__}")
    if C != 3:
        raise ValueError(f"training_image_loss: an exposure needs a three-channel image, got C = {C}")
    if exposure.device != image.device:
        raise ValueError(f"training_image_loss: exposure on {exposure.device}, image on {image.device}")
    return exposure


def training_image_loss(image, gt, lambda_dssim: float = 0.2, *, weight=None, exposure=None):
    """((1 - lambda) L1 + lambda (1 - SSIM), L1, SSIM) of train.py:199-204 from one node (three launches per training step).
    `weight` ([H,W] or [1,H,W]: a mask or a soft per-pixel weight) and `exposure` (a [3,4] affine colour transform of the render,
    which may require grad) are defined in the module docstring; without them the call is the plain node, launch for launch."""
    if image.dim() == 4 and image.shape[0] == 1:
        image, gt = image[0], gt[0]
    if weight is None and exposure is None:
        if image.is_cuda and image.dim() == 3 and image.shape == gt.shape:
            return _TrainImageLoss.apply(image, gt, float(lambda_dssim))
        l1, s = l1_ssim(image, gt)
        return (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - s), l1, s
    if image.dim() != 3 or image.shape != gt.shape:
        raise ValueError("training_image_loss expects two [C,H,W] images of the same shape")
    if image.device != gt.device:
        raise ValueError(f"training_image_loss: image on {image.device}, gt on {gt.device}")
    C, H, W = image.shape
    w = None if weight is None else _loss_weight(weight, H, W, image)
    E = None if exposure is None else _loss_exposure(exposure, C, image)
    return _TrainImageLossWeighted.apply(image, gt, float(lambda_dssim), w, E)


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
