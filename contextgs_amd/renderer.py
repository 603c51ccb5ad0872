"""Drop-in for the reference's `gaussian_renderer/__init__.py`:
`prefilter_voxel`, `generate_neural_gaussians`, `render` with the same
signatures, phase switches and return values (cited lines are that file).

What runs where: the visibility filter and the whole rasterizer are HIP
kernels (rasterizer.py); the anchor->Gaussian elementwise/compaction chain is
the fused HIP expansion (expand.hip) behind `_ExpandGaussians`; the three
anchor MLPs share their input and run as one fused fp32-MFMA launch each way
(mlp3.hip; rocprof showed the rocBLAS + element-wise version dominating the
step); the context model of the training / eval phases is context_model.py.
"""
from __future__ import annotations

import collections
import ctypes as C
import math
import os

import torch
import torch.nn.functional as F

from . import _lib, anchor_gen, ctx_ops, mlp
from .context_model import (LazyRows, begin_step, early_levels_begin, early_visible_rows, gather_unique, gather_unique_attach,
                            gather_unique_pair_attach, gather_unique_values, multi_scale_generating_visible)
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer, RasterRequest, check_deterministic

Q_FEAT, Q_SCALING, Q_OFFSETS = 1, 0.001, 0.2      # :40-42


def _c(t):
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


import threading as _threading

_OUTSTANDING = _threading.local()      # per thread and kind: the object whose *_launch owns the library's pinned count slot


def _own_slot(kind, obj):
    setattr(_OUTSTANDING, kind, obj)


def _check_slot(kind, obj):
    # The library keeps ONE pinned count slot per kind and thread (csrc: g_nz_slot, g_expand_slot): *_wait returns what the most
    # recent *_launch of the thread wrote.  An object that waits after another one of its kind was launched would read that
    # other object's count and mis-size its outputs — refuse instead.
    if getattr(_OUTSTANDING, kind, None) is not obj:
        raise RuntimeError(f"{type(obj).__name__}: another {kind} launch was issued on this thread before wait(); "
                           "launch / wait pairs of one kind must not interleave")


class VisibleList:
    """torch.nonzero(mask)[:, 0] in two halves (cgs_nonzero_launch / _wait): the kernels are enqueued at construction,
    `wait()` blocks only until the count has been copied back and returns the index tensor."""

    def __init__(self, mask):
        L = _lib.lib()
        m = mask if mask.dtype == torch.uint8 else mask.view(torch.uint8)
        self.mask = m = m.contiguous().reshape(-1)
        n = int(m.numel())
        self.idx = torch.empty(n, dtype=torch.int64, device=m.device)
        self.scratch = torch.empty(int(L.cgs_nonzero_scratch_bytes(n)), dtype=torch.uint8, device=m.device)
        self.ticket = C.c_uint64(0)      # the library refuses a wait whose ticket a later launch of the kind has replaced
        _lib.check(L.cgs_nonzero_launch(_lib.ptr(m), n, _lib.ptr(self.idx), _lib.ptr(self.scratch), self.scratch.numel(),
                                        _lib.current_stream(), C.byref(self.ticket)), "cgs_nonzero_launch")
        self._idx = None
        _own_slot("nonzero", self)

    def wait(self):
        if self._idx is not None:
            return self._idx
        _check_slot("nonzero", self)
        cnt = C.c_int64(0)
        _lib.check(_lib.lib().cgs_nonzero_wait(self.ticket, C.byref(cnt)), "cgs_nonzero_wait")
        idx = self.idx[:int(cnt.value)]
        idx._cgs_ascending = True        # row gathers by this list take the one-pass backward (cgs_scatter_rows_sorted)
        self._idx = idx
        return idx


class ExpandCount:
    """Pass A of the expansion (mask * opacity, survivor flags, their scan) enqueued WITHOUT reading the survivor count:
    `launch` returns at once, the caller may enqueue independent work (the rate model of the step), `wait` then blocks
    only until the count has arrived — the device does not drain at this read-back."""

    def __init__(self, op_raw, masks, K):
        L = _lib.lib()
        op_raw, masks = _c(op_raw.detach()), _c(masks.detach())
        _lib.require_device(op_raw, masks)
        n = int(op_raw.shape[0])
        dev = op_raw.device
        slots = n * K
        self.n, self.K = n, K
        self.neural_opacity = torch.empty(slots, 1, dtype=torch.float32, device=dev)
        self.mask_out = torch.empty(slots, dtype=torch.bool, device=dev)
        self.flags = self.mask_out        # (the survivor flags ARE the bytes of mask_out: the kernels scan and read those)
        self.pos = torch.empty(slots, dtype=torch.int32, device=dev)
        self.scratch = torch.empty(L.cgs_expand_scratch_bytes(n, K), dtype=torch.uint8, device=dev)
        self.P = None
        self.ticket = C.c_uint64(0)
        _lib.check(L.cgs_expand_count_launch(n, K, _lib.ptr(op_raw), _lib.ptr(masks), _lib.ptr(self.neural_opacity),
                                             _lib.ptr(self.mask_out), None, _lib.ptr(self.pos),
                                             _lib.ptr(self.scratch), self.scratch.numel(), _lib.current_stream(),
                                             C.byref(self.ticket)), "cgs_expand_count_launch")
        _own_slot("expand_count", self)

    def wait(self) -> int:
        if self.P is None:
            _check_slot("expand_count", self)
            cnt = C.c_int64(0)
            _lib.check(_lib.lib().cgs_expand_count_wait(self.ticket, C.byref(cnt)), "cgs_expand_count_wait")
            self.P = int(cnt.value)
        return self.P


def _expand_operands(anchor, gscaling, offsets, masks, op_raw, color_in, cov_in, K, pre):
    """The expansion's seven operands as contiguous fp32 tensors, and their count launch `pre` (launched here when None)."""
    _lib.require_device(anchor, gscaling, offsets, masks, op_raw, color_in, cov_in)
    ops = tuple(_c(t) for t in (anchor, gscaling, offsets, masks, op_raw, color_in, cov_in))
    if pre is None:
        pre = ExpandCount(ops[4], ops[3], K)
    assert pre.n == ops[0].shape[0] and pre.K == K
    return ops, pre


def _expand_backward(saved, n, K, src_row, g_xyz, g_color, g_opacity, g_scaling, g_rot, g_no, stream):
    """cgs_expand_backward on the per-Gaussian gradients (g_no may be None) -> those of the expansion's seven operands."""
    flags, pos, gscaling, offsets, op_raw, masks, cov_in = saved
    dev = gscaling.device
    e = lambda t: torch.empty_like(t)
    d_anchor = torch.empty(n, 3, dtype=torch.float32, device=dev)
    d_op, d_mask = e(op_raw), e(masks)
    if src_row is None:
        d_gs, d_off = e(gscaling), e(offsets)
    else:       # rows of the larger arrays that no visible anchor reads get a zero gradient (zero_unlisted_rows: only those
        # rows are written, not a fill of the whole arrays); when src_row names every row there is nothing to zero
        flat = torch.empty(gscaling.numel() + offsets.numel(), dtype=torch.float32, device=dev)
        d_gs, d_off = flat[:gscaling.numel()].view_as(gscaling), flat[gscaling.numel():].view_as(offsets)
        if n != gscaling.shape[0]:
            ctx_ops.zero_unlisted_rows(src_row, gscaling.shape[0], [d_gs, d_off])
    d_color = torch.empty(n, 3 * K, dtype=torch.float32, device=dev)
    d_cov = e(cov_in)
    _lib.check(_lib.lib().cgs_expand_backward(
        n, K, _lib.ptr(flags), _lib.ptr(pos), _lib.ptr(gscaling), _lib.ptr(offsets), _lib.ptr(op_raw), _lib.ptr(masks),
        _lib.ptr(cov_in), _lib.ptr(g_xyz), _lib.ptr(g_color), _lib.ptr(g_opacity), _lib.ptr(g_scaling), _lib.ptr(g_rot),
        _lib.ptr(g_no), _lib.ptr(d_anchor), _lib.ptr(d_gs), _lib.ptr(d_off), _lib.ptr(d_op), _lib.ptr(d_mask),
        _lib.ptr(d_color), _lib.ptr(d_cov), _lib.ptr(src_row), stream), "cgs_expand_backward")
    return d_anchor, d_gs, d_off, d_mask, d_op, d_color, d_cov


class _ExpandGaussians(torch.autograd.Function):
    """(anchor, grid_scaling, offsets, masks, mlp outputs) -> compacted Gaussians (:112-145)."""

    @staticmethod
    def forward(ctx, anchor, gscaling, offsets, masks, op_raw, color_in, cov_in, K, src_row=None, pre=None):
        # src_row: gscaling / offsets are the context model's full coding-order outputs and visible anchor n uses
        # their row src_row[n] (the visibility gather is done by the kernel)
        # pre: an ExpandCount already launched for (op_raw, masks) by the caller
        L = _lib.lib()
        (anchor, gscaling, offsets, masks, op_raw, color_in, cov_in), pre = _expand_operands(
            anchor, gscaling, offsets, masks, op_raw, color_in, cov_in, K, pre)
        n, dev, stream = anchor.shape[0], anchor.device, _lib.current_stream()
        ctx.set_materialize_grads(False)        # an unused output (neural_opacity in most losses) arrives as None, not as zeros
        P = pre.wait()
        neural_opacity, mask_out, flags, pos = pre.neural_opacity, pre.mask_out, pre.flags, pre.pos
        xyz, color, opacity, scaling, rot = (torch.empty(P, w, dtype=torch.float32, device=dev) for w in (3, 3, 1, 3, 4))
        _lib.check(L.cgs_expand_write(n, K, _lib.ptr(flags), _lib.ptr(pos), _lib.ptr(anchor), _lib.ptr(gscaling),
                                      _lib.ptr(offsets), _lib.ptr(neural_opacity), _lib.ptr(color_in),
                                      _lib.ptr(cov_in), _lib.ptr(xyz), _lib.ptr(color), _lib.ptr(opacity),
                                      _lib.ptr(scaling), _lib.ptr(rot), _lib.ptr(src_row), stream), "cgs_expand_write")
        ctx.K, ctx.n, ctx.src_row = K, n, src_row
        ctx.P = P                   # the substitutes of absent output gradients are sized from this, not from g_xyz
        ctx.save_for_backward(flags, pos, gscaling, offsets, op_raw, masks, cov_in)
        ctx.mark_non_differentiable(mask_out)
        return xyz, color, opacity, scaling, rot, neural_opacity, mask_out

    @staticmethod
    def backward(ctx, g_xyz, g_color, g_opacity, g_scaling, g_rot, g_no, _g_mask):
        saved, P = ctx.saved_tensors, ctx.P
        grads = [_c(g) if g is not None else torch.zeros(P, w, dtype=torch.float32, device=saved[2].device)
                 for g, w in zip((g_xyz, g_color, g_opacity, g_scaling, g_rot), (3, 3, 1, 3, 4))]
        g_no = _c(g_no) if g_no is not None else None
        return (*_expand_backward(saved, ctx.n, ctx.K, ctx.src_row, *grads, g_no, _lib.current_stream()), None, None, None)


EARLY_MLP3 = os.environ.get("CGS_EARLY_MLP3", "1") != "0"            # A/B knob: 0 = the anchor MLPs are enqueued where their node is created
FUSE_VIEW = os.environ.get("CGS_FUSE_VIEW", "1") != "0"    # tuning / A-B knob: expansion fused with the rasterizer's preprocess


class ViewFusion:
    """What render() hands to generate_neural_gaussians when the expansion may run fused with the rasterizer: the view's
    raster settings in, the rendered view out (`done`: (image, radii, screenspace_points))."""

    def __init__(self, raster_settings, retain_grad, absgrad=False, deterministic=False):
        self.raster_settings, self.retain_grad, self.done = raster_settings, retain_grad, None
        self.absgrad = bool(absgrad)       # screenspace_points is [P,4] and the backward is cgs_raster_backward_abs
        self.deterministic = bool(deterministic)       # the rasterizer's backward is cgs_raster_backward_det (3 or 4 columns)


class _ExpandRasterize(torch.autograd.Function):
    """_ExpandGaussians followed by the rasterizer (rasterizer._RasterizeGaussians) as ONE node whose forward goes from the
    expansion's slots to the rasterizer's records in one kernel (csrc/expand_raster.hip): colour and opacity never exist as
    per-Gaussian tensors and nothing the expansion writes is read back by the preprocess stage.  The backward is the two
    nodes' backward launches (cgs_raster_backward, cgs_expand_backward) with their hand-over buffers kept inside the node.
    Same device functions on the same values as the two nodes: bit-identical image, radii and scaling
    (tests/test_fused_view_gpu.py).  means2D: the view's screenspace_points (its gradient is the only thing it
    carries), created by the caller once the survivor count P is known.  absgrad: means2D is [P,4] and the rasterizer's
    backward launch is cgs_raster_backward_abs with the same arguments (rasterizer.py: the absolute sums in columns 2:4).
    deterministic: the rasterizer's backward launch is cgs_raster_backward_det with the plain form's arguments (rasterizer.py:
    no float atomics; same records and same lists as the unfused node, so the same bits)."""

    @staticmethod
    def forward(ctx, anchor, gscaling, offsets, masks, op_raw, color_in, cov_in, means2D, K, src_row, pre, raster_settings,
                absgrad=False, deterministic=False):
        from . import rasterizer as rz
        L = _lib.lib()
        (anchor, gscaling, offsets, masks, op_raw, color_in, cov_in), pre = _expand_operands(
            anchor, gscaling, offsets, masks, op_raw, color_in, cov_in, K, pre)
        n, dev, stream = anchor.shape[0], anchor.device, _lib.current_stream()
        ctx.set_materialize_grads(False)
        P = pre.wait()
        assert means2D.shape[0] == P and means2D.shape[1] == (4 if absgrad else 3)
        ctx.absgrad, ctx.deterministic = bool(absgrad), bool(deterministic)
        neural_opacity, mask_out, flags, pos = pre.neural_opacity, pre.mask_out, pre.flags, pre.pos
        cfg = rz._Cfg(raster_settings)
        H, W = cfg.c.image_height, cfg.c.image_width
        flat = torch.empty(P * 10, dtype=torch.float32, device=dev)          # scaling | xyz | rot (kept for the backward)
        scaling, xyz, rot = flat[:3 * P].view(P, 3), flat[3 * P:6 * P].view(P, 3), flat[6 * P:].view(P, 4)
        radii = torch.empty(P, dtype=torch.int32, device=dev)
        geom = rz._workspace(L.cgs_raster_geom_bytes(P), dev)
        img = rz._workspace(L.cgs_raster_img_bytes(H, W), dev)
        color = torch.empty(3, H, W, dtype=torch.float32, device=dev)
        ticket = C.c_uint64(0)
        _lib.check(L.cgs_raster_preprocess_expand_launch(
            cfg.ref, n, K, _lib.ptr(flags), _lib.ptr(pos), _lib.ptr(anchor), _lib.ptr(gscaling), _lib.ptr(offsets),
            _lib.ptr(neural_opacity), _lib.ptr(color_in), _lib.ptr(cov_in), _lib.ptr(src_row), P, _lib.ptr(scaling),
            _lib.ptr(xyz), _lib.ptr(rot), _lib.ptr(geom), geom.numel(), _lib.ptr(radii), stream, C.byref(ticket)),
            "cgs_raster_preprocess_expand_launch")
        binws, bin_R, _num_rendered = rz.bin_and_blend(cfg, P, geom, img, color, stream, ticket)
        ctx.cfg, ctx.num_rendered, ctx.K, ctx.n, ctx.src_row, ctx.P = cfg, bin_R, K, n, src_row, P
        ctx.save_for_backward(flags, pos, gscaling, offsets, op_raw, masks, cov_in, xyz, scaling, rot, radii, geom, binws, img)
        ctx.mark_non_differentiable(radii, mask_out)
        return color, radii, scaling, neural_opacity, mask_out

    @staticmethod
    def backward(ctx, g_img, _g_radii, g_scaling, g_no, _g_mask):
        from . import rasterizer as rz
        saved = ctx.saved_tensors
        xyz, scaling, rot, radii, geom, binws, img = saved[7:]
        cfg, K, n, src_row, P = ctx.cfg, ctx.K, ctx.n, ctx.src_row, ctx.P
        dev, stream = xyz.device, _lib.current_stream()
        # ---- the rasterizer's backward (rasterizer.launch_backward) into buffers that stay inside this node: the unfused
        # node's carve, at least one row allocated, and zero-filled unless the deterministic backward runs
        launch = g_img is not None and P > 0
        b = rz.carve_backward_buffers(P, 4 if ctx.absgrad else 3, dev, zero_acc=not (launch and ctx.deterministic),
                                      rows=max(P, 1))
        if launch:
            # the plain form's arguments; the colours never existed as a tensor and the backward of this form does not read
            # them (the pointer only says "colours, not SH": include/cgs.h), so the gradient buffer stands in
            rz.launch_backward(rz._KeptView(cfg, P, ctx.num_rendered, geom, binws, img),
                               (xyz, b.colors, None, None, scaling, rot, None, radii), 0, 0, rz._f32c(g_img), (None, None, None),
                               (b.means3D, b.means2D, b.colors, b.opac, None, b.scales, b.rots, None), stream, 0, ctx.absgrad,
                               ctx.deterministic)
        else:
            b.rest.zero_()
        d_scales = b.scales
        if g_scaling is not None:            # the loss reads `scaling` too (train.py:204): what autograd would have summed
            d_scales = d_scales + _c(g_scaling)
        g_no = _c(g_no) if g_no is not None else None
        return (*_expand_backward(saved[:7], n, K, src_row, b.means3D, b.colors, b.opac, d_scales, b.rots, g_no, stream),
                b.means2D, None, None, None, None, None, None)


def _anchor_mlps(pc, x):
    """mlp_opacity / mlp_color / mlp_cov on the shared [N,54] input (:112,122,126).
    The three first layers are one GEMM; outputs are identical dot products."""
    mo, mc, mv = pc.get_opacity_mlp, pc.get_color_mlp, pc.get_cov_mlp
    if mlp.anchor_mlp3_supported(mo, mc, mv):
        # the three MLPs share x: one fused launch forward, one backward (csrc/mlp3.hip)
        return mlp.anchor_mlp3(x, mo, mc, mv)
    if mlp.supported(mo) and mlp.supported(mc) and mlp.supported(mv):
        # one fused fp32-MFMA launch per MLP forward, three backward (csrc/mlp.hip): rocprof showed the
        # rocBLAS + elementwise + bias-reduction version of these skinny MLPs dominating the step
        return mlp.mlp2(x, mo), mlp.mlp2(x, mc), mlp.mlp2(x, mv)
    D = mo[0].out_features
    W1 = torch.cat([mo[0].weight, mc[0].weight, mv[0].weight], dim=0)
    b1 = torch.cat([mo[0].bias, mc[0].bias, mv[0].bias], dim=0)
    h = F.relu(F.linear(x, W1, b1))
    op_raw = torch.tanh(F.linear(h[:, :D], mo[2].weight, mo[2].bias))
    color = torch.sigmoid(F.linear(h[:, D:2 * D], mc[2].weight, mc[2].bias))
    cov = F.linear(h[:, 2 * D:], mv[2].weight, mv[2].bias)
    return op_raw, color, cov


def _generate_fused(viewpoint_camera, pc, anchor, feat, grid_scaling, grid_offsets, binary_grid_masks, K):
    """:106-145 as one autograd node over the fused kernel family (anchor_gen.py): MLP input assembly, the three anchor
    MLPs, mask, compaction and the per-Gaussian tail.  None when the shapes are not the ones the kernels are built for."""
    mo, mc, mv = pc.get_opacity_mlp, pc.get_color_mlp, pc.get_cov_mlp
    fs, fr = (feat.src, feat.idx) if isinstance(feat, LazyRows) else (feat, None)
    lazy_s, lazy_o = isinstance(grid_scaling, LazyRows), isinstance(grid_offsets, LazyRows)
    if lazy_s and lazy_o and grid_scaling.idx is grid_offsets.idx:
        gsrc, osrc, grow = grid_scaling.src, grid_offsets.src, grid_scaling.idx
    elif not lazy_s and not lazy_o:
        gsrc, osrc, grow = grid_scaling, grid_offsets, None
    else:
        return None
    if not (fs.dim() == 2 and fs.shape[1] == 50 and gsrc.dim() == 2 and gsrc.shape[1] == 6
            and anchor_gen.supported(mo, mc, mv, K, fs, fr, anchor, gsrc, osrc, grow, binary_grid_masks)):
        return None
    return anchor_gen.anchor_gen(fs, fr, anchor, viewpoint_camera.camera_center, gsrc, osrc, grow,
                                 binary_grid_masks.reshape(-1, K), mo, mc, mv)


def _generate_unfused(viewpoint_camera, pc, anchor, feat, grid_scaling, grid_offsets, binary_grid_masks, K, between=None,
                      view=None, mlp_pre=None):
    """The same stage as separate launches: fused three-MLP kernel (or torch) + the expansion kernels.
    between: called after the expansion's survivor count has been ENQUEUED and before it is read — work it launches
    (the step's rate model) runs on the device while the host waits for the count."""
    mo, mc, mv = pc.get_opacity_mlp, pc.get_color_mlp, pc.get_cov_mlp
    if (isinstance(feat, LazyRows) and feat.src.dim() == 2 and feat.src.shape[1] == 50 and feat.src.is_cuda
            and mlp.anchor_mlp3_supported(mo, mc, mv)):
        # :106-127 in one launch: the visibility gather of the context model's output, the view direction / distance
        # and the [feat, view, dist] concatenation happen inside the fused three-MLP kernel's operand load (and its
        # backward scatters straight into the source rows): no [n,54] gather / scatter / norm / div launches
        op_raw, color_in, cov_in = mlp.anchor_mlp3_rows(feat.src, feat.idx, anchor, viewpoint_camera.camera_center,
                                                        mo, mc, mv, pre=mlp_pre)
    else:
        ob_view = anchor - viewpoint_camera.camera_center                               # :106-110
        ob_dist = ob_view.norm(dim=1, keepdim=True)
        ob_view = ob_view / ob_dist
        if isinstance(feat, LazyRows):
            # the visibility gather of the context model's output and this concatenation are one launch (and one
            # scatter on the way back) instead of a gather + a cat
            cat_local_view = feat.cat_with(ob_view, ob_dist)
        else:
            cat_local_view = torch.cat([feat, ob_view, ob_dist], dim=1)
        op_raw, color_in, cov_in = _anchor_mlps(pc, cat_local_view)                      # :112-127
    src_row = None
    if isinstance(grid_scaling, LazyRows) and isinstance(grid_offsets, LazyRows) and grid_scaling.idx is grid_offsets.idx:
        # the expansion kernels read the context model's coding-order outputs through the row index themselves
        src_row, grid_scaling, grid_offsets = grid_scaling.idx, grid_scaling.src, grid_offsets.src
    else:
        grid_scaling = grid_scaling.materialize() if isinstance(grid_scaling, LazyRows) else grid_scaling
        grid_offsets = grid_offsets.materialize() if isinstance(grid_offsets, LazyRows) else grid_offsets
    masks2 = binary_grid_masks.reshape(-1, K)
    pre = None
    if op_raw.is_cuda and masks2.is_cuda:
        pre = ExpandCount(op_raw, masks2, K)
    if between is not None:
        between()
    if view is not None and _fusable_on_device(pre, anchor, grid_scaling, grid_offsets):
        # the expansion and the rasterizer as one node (csrc/expand_raster.hip); the survivor count is read here, after
        # `between` has put the rate model in the queue, so that screenspace_points can be an INPUT of the node
        P = pre.wait()
        screenspace_points = _zero_points(torch.empty(P, 0, device=anchor.device), 4 if view.absgrad else 3)
        _retain_grad(screenspace_points, view.retain_grad)
        image, radii, scaling, neural_opacity, mask = _ExpandRasterize.apply(
            anchor, grid_scaling, grid_offsets, masks2, op_raw, color_in, cov_in, screenspace_points, K, src_row, pre,
            view.raster_settings, view.absgrad, view.deterministic)
        view.done = (image, radii, screenspace_points)
        return None, None, None, scaling, None, neural_opacity, mask
    return _ExpandGaussians.apply(anchor, grid_scaling, grid_offsets, masks2, op_raw, color_in, cov_in, K, src_row, pre)


def _fusable_on_device(pre, anchor, grid_scaling, grid_offsets):
    # what _view_fusion cannot know up front: the expansion's count is in flight and its operands are on the device
    return pre is not None and anchor.is_cuda and grid_scaling.is_cuda and grid_offsets.is_cuda


_GenPlan = collections.namedtuple("_GenPlan", "phase predict_rate update_bound")


def _gen_plan(is_training, step, decoded_version):
    """What a call runs, from plain values (the one place that compares `step` with a number).  phase: "plain" (raw parameters),
    "noise" (:54-58) or "context" (:63 in training, :83 in eval); predict_rate; update_bound: update_anchor_bound() runs (:60)."""
    context = (is_training and step > 10000) or (not is_training and not decoded_version)
    phase = "context" if context else "noise" if (is_training and 3000 < step <= 10000) else "plain"
    return _GenPlan(phase, bool(is_training and context), bool(is_training and step == 10000))


class _DeferredMask:
    """The offset mask of a step that trains it on the device: `values` at once, the autograd node when node() is first called."""
    # the level plan needs the anchor mask, but the node is attached after the level loop's (ctx_ops._MaskSTEAttach: `_mask`'s
    # gradient is then final BEFORE the level kernels run in the backward); visible_values: the visible anchors' rows of `values`

    def __init__(self, param, values):
        self.param, self.values, self.visible_values, self._node = param, values, None, None

    def node(self):
        if self._node is None:
            self._node = ctx_ops.mask_ste_attach(self.param, self.values)
        return self._node


class _ViewStep:
    """One call of generate_neural_gaussians: what its stages hand to each other."""

    def __init__(self, camera, pc, plan, is_training, visible_mask, view):
        self.camera, self.pc, self.plan, self.is_training, self.visible_mask = camera, pc, plan, is_training, visible_mask
        self.view = view                            # a ViewFusion: the fused expand + raster node may be taken
        self.full_anchor = self.vis_pending = self.vis_idx = self.anchor = None     # (anchor: the visible rows of full_anchor)
        # the offset mask of all anchors (a tensor, or the node() of `mask`, the _DeferredMask) and "any offset alive" of it
        self.binary_all = self.mask_anchor_bool = self.mask = None
        # context_model.begin_step's handle, get_scaling as the early levels read it, mlp.anchor_mlp3_rows_launch's record
        self.begun = self.scaling_all = self.mlp_pre = None
        self.feat = self.grid_scaling = self.grid_offsets = self.masks = None    # the expansion's inputs (tensors or LazyRows)
        self.rate = self.chosen_rows = self.masks_chosen = None     # the deferred rate model, the mask rows it reads, those rows gathered
        self.rates = (None,) * 5                    # bit_per_param, bit_per_feat / scaling / offsets_param, bpp_per_level

    def run_rate(self):
        if self.rate is not None:
            self.rates = self.rate(self.masks_chosen)


def _begin_context(s):
    # everything of the context model that does not depend on the visible set is enqueued BEFORE the read-back of the visible
    # count: the GPU works through it while the host waits, and the context model's own count read-back finds its data there
    if s.plan.phase != "context":
        return
    pc = s.pc
    if (s.is_training and hasattr(pc, "get_mask_pair") and not pc.decoded_version and pc._mask.is_cuda and pc._mask.requires_grad
            and torch.is_grad_enabled()):
        values, s.mask_anchor_bool = ctx_ops.mask_ste_values(pc._mask)
        s.mask = _DeferredMask(pc._mask, values)
        s.binary_all = s.mask.node
    elif hasattr(pc, "get_mask_pair"):
        s.binary_all, s.mask_anchor_bool = pc.get_mask_pair()
    else:                                   # the reference's own GaussianModel
        s.binary_all = pc.get_mask
        s.mask_anchor_bool = s.binary_all.detach().sum(dim=1)[:, 0] > 0
    s.begun = begin_step(pc, s.full_anchor, s.mask_anchor_bool, s.is_training)
    if s.begun is not None and s.is_training:
        # the step's level kernels depend on nothing the host still has to read (not on the view either): 0.4 ms of device
        # work behind which the read-backs below and the small launches between them disappear (context_model._early_levels)
        s.scaling_all = pc.get_scaling
        early_levels_begin(pc, s.full_anchor, pc._hyper_latent, pc._anchor_feat, pc._offset, s.scaling_all, s.mask_anchor_bool,
                           s.begun)


def _note_touched_rows(s):
    # multi-GPU: the per-anchor gradients of this view only reach the visible anchors unless the context model runs over all
    # of them (dist.GradientSync(sparse="auto") exchanges the union of the ranks' rows instead of dense tensors)
    if s.is_training:
        from . import dist
        dist.note_touched_rows(None if s.plan.phase == "context" else s.visible_mask, int(s.vis_idx.shape[0]))


def _launch_early_mlps(s):
    # The three anchor MLPs, enqueued on the buffer the level kernels (already in the queue) are writing: their operands are
    # all known here, and the host has ~0.3 ms of node creation in front of it (hyper step, level nodes, the mask's node) during
    # which the device would finish the level kernels and idle (profiles/r06_gpu_idle_gaps.txt).  The node is created later, by
    # _generate_unfused, around this launch; if the step turns out different (the plan was rebuilt, another expansion path), the
    # launch is dropped and repeated there (mlp._M3Launch.fits).
    pc = s.pc
    mlps = (pc.get_opacity_mlp, pc.get_color_mlp, pc.get_cov_mlp)
    if not (s.begun is not None and s.is_training and EARLY_MLP3 and torch.is_grad_enabled()
            and mlp.anchor_mlp3_supported(*mlps) and pc._anchor_feat.shape[1] == 50
            and not anchor_gen.supported(*mlps, pc.n_offsets, s.full_anchor)):
        return
    early = early_visible_rows(s.begun, s.vis_idx)
    if early is not None:
        s.mlp_pre = mlp.anchor_mlp3_rows_launch(*early, s.anchor.detach(), s.camera.camera_center, *mlps)


def _gather_mask_rows(s):
    # enqueued in front of the context model's count read-back: the host falls behind the device while it waits there, and a
    # gather the device still has queued covers part of the catch-up
    if s.mask is not None:
        s.mask.visible_values = gather_unique_values(s.mask.values, s.vis_idx)
    elif s.binary_all is not None:
        s.masks = gather_unique(s.binary_all, s.vis_idx)


def _gather_raw_inputs(s):
    if s.plan.phase == "context":
        return
    pc, noise = s.pc, s.plan.phase == "noise"
    sel = lambda t: gather_unique(t, s.vis_idx)
    # raw features of the visible anchors: left as (source, rows) when nothing is added to them, so that the anchor-MLP kernel
    # gathers them itself
    feat = LazyRows(pc._anchor_feat, s.vis_idx) if (not noise and pc._anchor_feat.is_cuda) else sel(pc._anchor_feat)
    grid_offsets = sel(pc._offset)
    grid_scaling = sel(pc.get_scaling)
    s.masks = sel(pc.get_mask)
    if noise:                                                                           # :54-58
        if feat.is_cuda and grid_offsets.dim() == 3:
            # x + U(-1/2, 1/2) Q for the three tensors in ONE launch (the level kernel of the context model with a zero step-size
            # adjustment: Q = q0 (1 + tanh 0) = q0) instead of three uniform_ / mul / add chains over [n,50], [n,6], [n,30]; the
            # build's counter-based generator instead of torch's Philox stream (same distribution),
            # backward = identity
            n_vis = feat.shape[0]
            zero_adj = torch.zeros(n_vis, 3, dtype=torch.float32, device=feat.device)
            off_flat = grid_offsets.reshape(n_vis, grid_offsets.shape[1] * grid_offsets.shape[2])    # (explicit: n_vis may be 0)
            feat, grid_scaling, off2, _q = ctx_ops.noise_quant(feat, grid_scaling, off_flat, zero_adj,
                                                               (Q_FEAT, Q_SCALING, Q_OFFSETS))
            grid_offsets = off2.view(grid_offsets.shape)
        else:
            feat = feat + torch.empty_like(feat).uniform_(-0.5, 0.5) * Q_FEAT
            grid_scaling = grid_scaling + torch.empty_like(grid_scaling).uniform_(-0.5, 0.5) * Q_SCALING
            grid_offsets = grid_offsets + torch.empty_like(grid_offsets).uniform_(-0.5, 0.5) * Q_OFFSETS
    s.feat, s.grid_scaling, s.grid_offsets = feat, grid_scaling, grid_offsets


def _run_context_model(s):                                                              # :63-81 (train) / :83-101 (eval)
    if s.plan.phase != "context":
        return
    pc = s.pc
    # (get_mask_anchor, scene/gaussian_model.py:302-310, is "any offset alive" of the SAME mask values: both came from one
    # evaluation in _begin_context instead of running the sigmoid / threshold / STE chain twice)
    res = multi_scale_generating_visible(pc, s.full_anchor, pc._hyper_latent, pc._anchor_feat, pc._offset,
                                         s.scaling_all if s.scaling_all is not None else pc.get_scaling, s.binary_all,
                                         s.mask_anchor_bool, s.vis_idx, training=s.is_training,
                                         predict_bpp=s.plan.predict_rate, defer_feat=True, begun=s.begun, defer_rate=True)
    s.feat, s.grid_scaling, s.grid_offsets = res[:3]
    if s.plan.predict_rate:     # the rate model (:1657-1707) is enqueued behind the expansion's count (_expand)
        s.rate, s.chosen_rows = res[3:]


def _attach_mask(s):
    if s.mask is None:
        return
    if s.chosen_rows is not None and s.chosen_rows.is_cuda:
        # the visible rows (for the expansion) and the rate subset's rows of the mask weights through ONE node: one gradient
        # buffer instead of two and the engine's add (context_model._GatherUniquePair)
        s.masks, s.masks_chosen = gather_unique_pair_attach(s.mask.node(), s.vis_idx, s.mask.visible_values, s.chosen_rows)
    else:
        s.masks = gather_unique_attach(s.mask.node(), s.vis_idx, s.mask.visible_values)


def _expand(s):
    K = s.pc.n_offsets
    out = _generate_fused(s.camera, s.pc, s.anchor, s.feat, s.grid_scaling, s.grid_offsets, s.masks, K)
    if out is not None:
        s.run_rate()
        return out
    # the rate model goes into the queue between the expansion's count launch and the read of that count
    return _generate_unfused(s.camera, s.pc, s.anchor, s.feat, s.grid_scaling, s.grid_offsets, s.masks, K, between=s.run_rate,
                             view=s.view, mlp_pre=s.mlp_pre)


def _side_outputs(s, mask, rows, slots):
    K = s.pc.n_offsets
    if rows is not None:        # the visible anchor index once per offset, then through the expansion's selection mask
        rows.append(s.vis_idx.repeat_interleave(K)[mask.reshape(-1)])
    if slots is not None:       # a * K + k of every (visible anchor, offset), then through the same mask
        ak = s.vis_idx.to(torch.int32)[:, None] * K + torch.arange(K, dtype=torch.int32, device=s.vis_idx.device)
        slots.append(ak.reshape(-1)[mask.reshape(-1)])


def generate_neural_gaussians(viewpoint_camera, pc, visible_mask=None, is_training=False, step=0, _view=None,
                              _rows=None, _slots=None):   # :25-150
    """The stages in launch order; a stage that does not belong to the plan's phase returns at once."""
    # _rows: a list that receives, for every Gaussian produced, the row of its anchor in pc.get_anchor (render(anchor_features=))
    # _slots: likewise, int32 a * K + k for offset k of anchor a (render(contrib=))
    if visible_mask is None:
        visible_mask = torch.ones(pc.get_anchor.shape[0], dtype=torch.bool, device=pc.get_anchor.device)
    s = _ViewStep(viewpoint_camera, pc, _gen_plan(is_training, step, pc.decoded_version), is_training, visible_mask,
                  _view if is_training else None)
    # the visible-anchor list is ENQUEUED first and read after everything that does not need it (:44-50)
    s.vis_pending = VisibleList(visible_mask) if visible_mask.is_cuda else None
    s.full_anchor = pc.get_anchor       # one Quantize_anchor launch per call (the reference re-derives it ~5x)
    _begin_context(s)
    # visible rows are distinct anchors: gather by index with a sort-free scatter backward (the reference's boolean-mask
    # indexing, :44-50, backpropagates through index_put_(accumulate) = a device sort per tensor)
    s.vis_idx = s.vis_pending.wait() if s.vis_pending is not None else torch.nonzero(visible_mask)[:, 0]
    _note_touched_rows(s)
    s.anchor = gather_unique(s.full_anchor, s.vis_idx)
    _launch_early_mlps(s)
    _gather_mask_rows(s)
    _gather_raw_inputs(s)
    if s.plan.update_bound:                                                             # :60-61
        pc.update_anchor_bound()
    _run_context_model(s)
    _attach_mask(s)
    xyz, color, opacity, scaling, rot, neural_opacity, mask = _expand(s)
    _side_outputs(s, mask, _rows, _slots)
    if is_training:                                                                      # :147-150
        return (xyz, color, opacity, scaling, rot, neural_opacity, mask, s.rates[0], 16, *s.rates[1:])
    return xyz, color, opacity, scaling, rot, 0


class _ZeroPoints(torch.autograd.Function):
    """The reference's `screenspace_points` (gaussian_renderer/__init__.py:168: a zero [P,3] non-leaf tensor whose .grad
    receives the 2-D position gradients): a FRESH zero tensor per view, as in the reference — independent storage, so a caller
    that writes into one view's tensor does not touch another's — wrapped in an autograd node so that it is a non-leaf tensor
    that requires grad without the reference's `+ 0` launch.  One fill of 12 B per Gaussian per view ([P,4], 16 B, with
    render(absgrad=True))."""

    @staticmethod
    def forward(ctx, like, token, cols=3):
        return torch.zeros(int(like.shape[0]), cols, dtype=torch.float32, device=like.device)

    @staticmethod
    def backward(ctx, _g):
        return None, None, None


_GRAD_TOKEN = {}


def _zero_points(xyz, cols=3):
    tok = _GRAD_TOKEN.get(xyz.device)
    if tok is None:
        tok = _GRAD_TOKEN[xyz.device] = torch.zeros(1, device=xyz.device, requires_grad=True)
    return _ZeroPoints.apply(xyz.detach(), tok, cols)


def _retain_grad(points, wanted):
    if wanted:
        try:
            points.retain_grad()
        except Exception:
            pass


def _raster_settings(viewpoint_camera, pipe, bg_color, scaling_modifier):
    return GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5), tanfovy=math.tan(viewpoint_camera.FoVy * 0.5),
        bg=bg_color, scale_modifier=scaling_modifier, viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform, sh_degree=1, campos=viewpoint_camera.camera_center,
        prefiltered=False, debug=bool(getattr(pipe, "debug", False)),
        antialiasing=bool(getattr(pipe, "antialiasing", False)))


def _view_fusion(is_training, return_aux, return_geometry, antialiasing, cam_grad, anchor_features, contrib,
                 raster_settings=None, retain_grad=False, absgrad=False, deterministic=False, return_normals=False):
    """The ViewFusion of a view that may take the fused expand + raster node, None of one that may not (render()'s docstring)."""
    if (not is_training or return_aux or return_geometry or return_normals or antialiasing or cam_grad
            or anchor_features is not None or contrib is not None or not FUSE_VIEW or not torch.is_grad_enabled()):
        return None
    return ViewFusion(raster_settings, retain_grad, absgrad, deterministic)


_RATE_KEYS = ("bit_per_param", "bit_per_anchor_param", "bit_per_feat_param", "bit_per_scaling_param", "bit_per_offsets_param",
              "bpp_per_level")


def _training_result(image, radii, points, scaling, rest):
    """render()'s dict of a training call (:209-222); rest: what generate_neural_gaussians returns behind `rot`."""
    neural_opacity, mask, *rates = rest
    return {"render": image, "viewspace_points": points, "visibility_filter": radii > 0, "radii": radii,
            "selection_mask": mask, "neural_opacity": neural_opacity, "scaling": scaling, **dict(zip(_RATE_KEYS, rates))}


class _DetachedCamera:
    """A camera as the Gaussian generation sees it when its pose is being trained: every attribute of the wrapped camera, the
    three pose tensors detached (render()'s docstring: the anchor MLPs' input is not differentiated with respect to the camera)."""

    def __init__(self, camera):
        self._camera = camera
        self.world_view_transform = camera.world_view_transform.detach()
        self.full_proj_transform = camera.full_proj_transform.detach()
        self.camera_center = camera.camera_center.detach()

    def __getattr__(self, name):
        return getattr(self._camera, name)


def render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier=1.0, visible_mask=None, retain_grad=False,
           step=0, *, return_aux=False, anchor_features=None, contrib=None, absgrad=False, deterministic=None,
           return_geometry=False, return_normals=False):   # :155-229
    """Render the scene.  Background tensor (bg_color) must be on the GPU.

    return_aux=True: the dict also holds the rasterizer's "depth", "invdepth" and "alpha" maps ([1,H,W] each, see
    contextgs_amd/rasterizer.py).  In training mode such a call takes the unfused path (the one CGS_FUSE_VIEW=0 takes), and so
    does one with `pipe.antialiasing` set (upstream's --antialiasing, see contextgs_amd/rasterizer.py).

    anchor_features: a float tensor [N, C] over all anchors (pc.get_anchor's row order), 1 <= C <= 32.  Every neural Gaussian
    carries its anchor's row and the dict gains "features" [C,H,W], the rasterizer's blend of them over a zero background
    (rasterizer.py).  The gradient reaches `anchor_features` (zero rows for anchors that are not visible) and the geometry.
    In training mode such a call takes the unfused path, as return_aux does.

    contrib: a rasterizer.GaussianContrib of N * K rows (N anchors in pc.get_anchor's order, K = pc.n_offsets; row a * K + k is
    offset k of anchor a) that the view's per-Gaussian contribution statistics are accumulated into, or True for a fresh one.
    The dict gains "contrib" (the object), "top_id" int32 [H,W] (the slot a * K + k of the Gaussian with the largest blending
    weight at each pixel, -1 where there is none), "top_weight" [1,H,W] and "count" int32 [H,W] (rasterizer.py).  Rows of
    anchors outside `visible_mask` and of offsets the selection mask drops are not touched.  Nothing of it is differentiable.
    In training mode such a call takes the unfused path, as return_aux does.

    return_geometry=True: the dict also holds the rasterizer's "distortion" and "median_depth" maps ([1,H,W] each; the
    depth-distortion regulariser and the depth at which a ray's accumulated opacity crosses one half) and "median_id" int32
    [H,W], the index of that Gaussian among the view's neural Gaussians (the order of "radii"), -1 where there is none
    (rasterizer.py has the definitions and the gradients).  In training mode such a call takes the unfused path, as return_aux
    does.

    return_normals=True: the dict also holds "normals" [3,H,W], the rasterizer's blend of the neural Gaussians' camera-space
    normals (the axis of each one's smallest scale, turned away from the camera; rasterizer.py and normals.py have the
    definition), for normals.normal_consistency.  It takes three of the 32 feature channels, so it composes with
    `anchor_features` of at most 29 columns.  In training mode such a call takes the unfused path, as anchor_features does; not
    with a camera whose world_view_transform requires a gradient (ValueError).

    absgrad=True: "viewspace_points" is created [P,4] and its gradient holds the signed 2-D position gradient in columns 0:2,
    as without the flag, and in columns 2:4 the sums over the pixels of the ABSOLUTE per-pixel gradients of the colour image
    (AbsGS's densification statistic; contextgs_amd/rasterizer.py has the definition and what it excludes).  Training-mode
    calls stay on the fused expand + raster node; every other path hands the keyword to the rasterizer.
    densify.training_statis (GaussianModel.training_statis) accumulates ||grad[:, 2:4]|| when the gradient has four columns.

    deterministic=True (None, the default: the environment variable CGS_RASTER_DETERMINISTIC=1): the rasterizer's backward runs
    without float atomics and its gradients are bit-reproducible (contextgs_amd/rasterizer.py has the contract).  Training-mode
    calls stay on the fused expand + raster node, whose backward launch is then cgs_raster_backward_det; every other path hands
    the keyword to the rasterizer; fused and unfused give the same bits.  Not covered, ValueError before a device is touched:
    return_aux, anchor_features, contrib, return_geometry, return_normals.  The rasterizer's gradients only: other launches of a training step still sum with
    float atomics (DESIGN.md section 8 lists them).

    A camera whose `world_view_transform`, `full_proj_transform` or `camera_center` requires a gradient (a trainable pose,
    contextgs_amd/camera_pose.py) takes the unfused path too, in training and in eval mode, and the gradient reaches the three
    tensors through the rasterizer (rasterizer.py: the projection, the covariance chain, the depth of the maps).  Not
    differentiated with respect to the camera: the anchor MLPs' input (anchor - camera_center), which is evaluated on the
    detached position, and the fused expand + raster node, which such a call never takes."""
    deterministic = check_deterministic(deterministic, return_aux, anchor_features, contrib, return_geometry, return_normals)
    return_geometry, return_normals = bool(return_geometry), bool(return_normals)
    is_training = pc.get_color_mlp.training
    cam_grad = torch.is_grad_enabled() and any(
        isinstance(t, torch.Tensor) and t.requires_grad for t in (
            viewpoint_camera.world_view_transform, viewpoint_camera.full_proj_transform, viewpoint_camera.camera_center))
    gen_camera = _DetachedCamera(viewpoint_camera) if cam_grad else viewpoint_camera
    rows = [] if anchor_features is not None else None
    if anchor_features is not None and (anchor_features.dim() != 2 or anchor_features.shape[0] != pc.get_anchor.shape[0]):
        raise ValueError(f"anchor_features must be [N, C] with N = {pc.get_anchor.shape[0]} anchors, "
                         f"got {tuple(anchor_features.shape)}")
    slots = None
    if contrib is not None and contrib is not False:
        from .rasterizer import GaussianContrib
        n_rows = pc.get_anchor.shape[0] * pc.n_offsets
        if contrib is True:
            contrib = GaussianContrib.zeros(n_rows, pc.get_anchor.device)
        elif not isinstance(contrib, GaussianContrib):
            raise ValueError(f"contrib must be a GaussianContrib or True, got {type(contrib).__name__}")
        if len(contrib) != n_rows:
            raise ValueError(f"contrib has {len(contrib)} rows for {pc.get_anchor.shape[0]} anchors x {pc.n_offsets} offsets "
                             f"= {n_rows}")
        slots = []
    else:
        contrib = None
    # what the rasterizer is asked for (deterministic: resolved above, the rasterizer does not read the environment again);
    # the slot table follows once the view's Gaussians exist
    request = RasterRequest(bool(return_aux), contrib, None, bool(absgrad), deterministic, return_geometry,
                            3 if return_normals else 0)
    settings = _raster_settings(viewpoint_camera, pipe, bg_color, scaling_modifier)
    view = _view_fusion(is_training, return_aux, return_geometry, settings.antialiasing, cam_grad, anchor_features, contrib,
                        settings, retain_grad, absgrad, deterministic, return_normals)
    xyz, color, opacity, scaling, rot, *rest = generate_neural_gaussians(
        gen_camera, pc, visible_mask, is_training=is_training, step=step, _view=view, _rows=rows, _slots=slots)
    if view is not None and view.done is not None:
        # (xyz / color / opacity / rot are None: they never existed as tensors)
        return _training_result(*view.done, scaling, rest)

    screenspace_points = _zero_points(xyz, 4 if absgrad else 3)       # :168 `torch.zeros_like(xyz, requires_grad=True) + 0`
    _retain_grad(screenspace_points, retain_grad)
    rasterizer = GaussianRasterizer(settings)
    if slots is not None:
        request = request._replace(contrib_slots=slots[0])
    rendered_image, radii, *aux = rasterizer(
        means3D=xyz, means2D=screenspace_points, shs=None, colors_precomp=color, opacities=opacity, scales=scaling,
        rotations=rot, cov3D_precomp=None, **request.keywords(),
        features=anchor_features.index_select(0, rows[0]) if rows is not None else None)      # plumbing: plain torch
    if slots is not None:       # a Gaussian index means nothing outside this call: one gather to slot ids, -1 kept
        tid = aux[0]["top_id"].long()
        table = torch.cat([slots[0], slots[0].new_full((1,), -1)])      # (index -1 reads the appended -1)
        aux[0]["top_id"] = table[tid]
    if is_training:
        out = _training_result(rendered_image, radii, screenspace_points, scaling, rest)
    else:
        out = {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0,
               "radii": radii, "time_sub": rest[0]}
    if aux:     # the rasterizer returned a third value
        out.update(aux[0])
    return out


def prefilter_voxel(viewpoint_camera, pc, pipe, bg_color, scaling_modifier=1.0, override_color=None):   # :232-287
    """Anchor-level frustum/size cull: bool[N]."""
    rs = _raster_settings(viewpoint_camera, pipe, bg_color, scaling_modifier)
    with torch.no_grad():
        means3D = pc.get_anchor
        # The reference evaluates get_scaling / get_rotation on all N rows and then reads three scale columns and
        # rotation row 0 (:262-266, :283: `rotations[[0], :].repeat(N, 1)`).  Both activations are row / element-wise,
        # so applying them to exactly what is read gives the same values: exp of 3 columns, normalisation of one row.
        # (rotation row 0 changes only when the optimizer touches _rotation: normalised once per version of the parameter)
        hit = getattr(pc, "_rot0_cache", None)
        if hit is not None and hit[0] is pc._rotation and hit[1] == pc._rotation._version:
            rot0 = hit[2]
        else:
            rot0 = pc.rotation_activation(pc._rotation[:1])
            pc._rot0_cache = (pc._rotation, pc._rotation._version, rot0)
        sc = pc._scaling
        if (means3D.is_cuda and sc.is_cuda and sc.dtype == torch.float32 and sc.dim() == 2 and sc.stride(1) == 1
                and means3D.dtype == torch.float32):
            # one launch (csrc/raster_geom.hip filter_voxel_kernel): exp of the three columns and the shared rotation are
            # applied inside, the bool mask comes out directly — no exp / repeat / zero-fill / compare launches
            from .rasterizer import _Cfg
            cfg = _Cfg(rs)
            N = int(means3D.shape[0])
            m = means3D.contiguous()
            r1 = rot0.reshape(-1).float().contiguous()
            vis = torch.empty(N, dtype=torch.bool, device=m.device)
            _lib.check(_lib.lib().cgs_filter_voxel(cfg.ref, N, _lib.ptr(m), sc.data_ptr(), int(sc.stride(0)),
                                                   0 if pc.decoded_version else 1, _lib.ptr(r1), _lib.ptr(vis),
                                                   _lib.current_stream()), "cgs_filter_voxel")
            return vis
        scales3 = sc[:, :3] if pc.decoded_version else torch.exp(sc[:, :3])
        rasterizer = GaussianRasterizer(rs)
        radii_pure = rasterizer.visible_filter(means3D=means3D, scales=scales3,
                                               rotations=rot0.repeat(means3D.shape[0], 1), cov3D_precomp=None)
    return radii_pure > 0
