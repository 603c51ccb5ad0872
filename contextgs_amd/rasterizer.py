"""Drop-in for the reference's `diff_gaussian_rasterization` package.

Same Python surface as the Scaffold-GS fork the reference imports
(gaussian_renderer/__init__.py:20): `GaussianRasterizationSettings`,
`GaussianRasterizer(raster_settings)(means3D, means2D, shs, colors_precomp,
opacities, scales, rotations, cov3D_precomp) -> (color[3,H,W], radii int32[P])`
and `.visible_filter(means3D, scales, rotations, cov3D_precomp) -> radii`.
All arithmetic runs in libcgs_hip.so (hand-written gfx950 kernels) through the
C-ABI of include/cgs.h; there is no CPU implementation here.

All four argument forms of upstream are implemented: colours as `colors_precomp`
[P,3] or as spherical harmonics `shs` [P,M,3] (M <= 16, degree
`raster_settings.sh_degree` evaluated in the preprocess kernel from the direction
means3D - campos, clamped at 0), covariances from `scales` + `rotations` or as
`cov3D_precomp` [P,6] (upper triangle xx, xy, xz, yy, yz, zz, used as given:
scale_modifier does not apply).  Exactly one of each pair; anything else raises
ValueError before a device is touched.  Every form, with or without the maps and
antialiasing below, is ONE autograd node, `_RasterizeGaussians`.  Its forward is
cgs_raster_preprocess_launch_opt, the binning and the blend; for the form the
reference renders with (colors_precomp + scales/rotations,
gaussian_renderer/__init__.py:197-205) that is cgs_raster_preprocess_launch, for
the others the kernels of csrc/raster_forms.hip.  Its backward is
cgs_raster_backward_ex (cgs_raster_backward for the reference's form) when only the
colour image got a gradient and antialiasing is off, cgs_raster_backward_feat without
features (which is cgs_raster_backward_opt) when antialiasing is on or one of the maps
got a gradient.

`forward(..., return_aux=True)` returns `(color, radii, {"depth", "invdepth", "alpha"})`, float32 [1,H,W] each, in all
four forms (csrc/raster_aux.hip); without it the call runs exactly the code above.  For pixel p the
contributors i are exactly those of the colour blend (same order, same alpha = min(0.99, o exp(power)), same skip below
1/255, same stop at T (1 - alpha) < 1e-4); with w_i = alpha_i T_i and z_i the view-space depth of Gaussian i's centre:

  depth[p]    = sum_i w_i z_i
  invdepth[p] = sum_i w_i / z_i      (upstream's `invdepths`)
  alpha[p]    = 1 - T_final[p]       (= sum_i w_i)

The background contributes to none of them; expected depth is depth / alpha.  Each map is the colour blend of a
per-Gaussian scalar (z, 1/z, 1) with a zero background, and gradients flow accordingly to means3D (also directly through z),
means2D, opacities, scales, rotations and cov3D_precomp, never to shs / colors_precomp.  means2D.grad (the densification
statistic) includes the maps' share, as upstream's `invdepths` backward does.

`forward(..., features=F)` with F a float tensor [P, C], 1 <= C <= 32 (semantic or language features, normals, per-anchor
statistics), blends the rows of F exactly as the colour is blended and returns `(color, radii, extras)` with
`extras["features"]` float32 [C,H,W] (and the three maps too with return_aux=True):

  features[c, p] = sum_i w_i F[i, c]

over the same contributors and weights as above, each pixel stopping where the colour pass stopped it.  Values are blended as
given (any sign, nothing clamped) over a zero background; a caller composites one with features + (1 - alpha) bg.  It is one
more walk of the view's tile lists (csrc/raster_feat.hip, cgs_raster_render_features), not ceil(C/3) renders; without `features`
the call runs exactly the code above.  When the feature map got a gradient the backward is cgs_raster_backward_feat: gradients
reach `features`, means2D, opacities, means3D, scales / rotations or cov3D_precomp and the camera tensors that ask, never
shs / colors_precomp; when only the feature map got one, no colour blend backward runs.  dL/dfeatures is summed with float
atomics, like dL/dcolors: not bit-reproducible.  Shape errors (not 2-D, rows != P, C outside 1..32) raise ValueError before a
device is touched.

`GaussianRasterizationSettings(..., antialiasing=True)` (upstream's last field, default False) is the 2-D filter of
Mip-Splatting that 3DGS code bases turn on with `--antialiasing`.  With [[a, b], [b, c]] the projected 2-D covariance before
the fixed 0.3 px^2 dilation:

  h = sqrt(max(2.5e-5, (a c - b^2) / ((a + 0.3)(c + 0.3) - b^2)))

and every blend (colour and maps) reads opacity * h: a sub-pixel Gaussian is still widened, but its integrated alpha no
longer grows with the widening, so a view rendered below the training resolution does not come out too bright and too thick.
Conic, radii and visible_filter are those of a call without it.  Gradients: opacities get h dL/d(opacity * h), and h's own
gradient reaches means3D and scales / rotations or cov3D_precomp (not means2D, shs or colors_precomp).  All four argument
forms, with and without return_aux, pass CGS_RASTER_ANTIALIAS to cgs_raster_preprocess_launch_opt / cgs_raster_backward_feat;
with antialiasing=False exactly the code above runs.

The camera is differentiable too (csrc/raster_camera.hip, cgs_raster_camera_backward): when `raster_settings.viewmatrix`,
`.projmatrix` or `.campos` requires a gradient, the node returns dL/dviewmatrix [4,4], dL/dprojmatrix [4,4] and dL/dcampos [3]
in the tensors' logical shape (a transposed view, as scene/cameras.py builds them, receives its own layout through autograd).
The rasterizer reads the three tensors independently and each gets the gradient of exactly its uses, summed over all Gaussians
(row-vector convention, V[c][i]):

  viewmatrix V: t = [p,1] V (the Jacobian J of the projection, the depth z = t_z of the maps and of the sort) and W = V[:3,:3]
                in cov2D = J W Sigma W^T J^T (with antialiasing also h)
  projmatrix PM: the pixel mean only, (hx, hy, hw) = [p,1] PM[:, (0,1,3)], ndc = h / (hw + 1e-7)
  campos: the SH direction means3D - campos only (forms with shs; without shs it is unused and gets None)

so a caller who builds PM = V P and campos = inv(V)[3,:3] in torch gets the pose gradient from autograd
(contextgs_amd/camera_pose.py).  V[:,3] and PM[:,2] are never read: exactly 0.  Not differentiable, as for the per-Gaussian
inputs: near-plane culling, radii and tile rectangles, the alpha >= 1/255 skip, the 0.99 cap, the T < 1e-4 stop, and t_x, t_y where
the 1.3 tanfov clamp of the Jacobian is active (zero, as for means3D).  The kernel runs behind the backward above, only when one
of the three asks; a call in which none does enqueues exactly what it did before.  No float atomics: at a fixed scratch the
three gradients are bit-reproducible.

`forward(..., contrib=...)` measures the reverse direction: how much each Gaussian mattered to the view (importance pruning,
covisibility, picking).  With w_i(p) = alpha_i T_i > 0 for the contributors of pixel p, exactly those of the colour blend as
above, and 0 otherwise, the call accumulates per Gaussian i into a `GaussianContrib` (four caller-owned tensors, added into
and never zeroed by the call, so that one object collects a whole set of training views):

  weight     += sum_p w_i(p)                     (float32; LightGaussian's accumulated blending weight)
  max_weight  = max(max_weight, max_p w_i(p))    (float32, values >= 0; RadSplat's criterion)
  pixels     += #{p : w_i(p) > 0}                (int64; MonoGS's n_touched)
  top_pixels += #{p : i has the largest w at p}  (int64; Mini-Splatting's count; an exact tie goes to the front-most)

and returns `(color, radii, extras)` with `extras["contrib"]` the object, `extras["top_id"]` int32 [H,W] (the index of that
largest contributor in the call's Gaussian order, -1 where the pixel has none), `extras["top_weight"]` float32 [1,H,W] (its w,
0 where none) and `extras["count"]` int32 [H,W] (the number of contributors).  `contrib=True` allocates a zeroed object of P
rows; a `GaussianContrib` instance must have P rows.  `contrib_slots`, int32 [P], redirects Gaussian i's four updates to row
contrib_slots[i] of an object of any length >= 1 (several Gaussians may share a row; values outside [0, len) are the caller's
error and are not checked on the device); `top_id` stays a Gaussian index.  Culled Gaussians and Gaussians that contributed
nowhere leave their rows untouched.  It is one more walk of the view's tile lists (csrc/raster_contrib.hip,
cgs_raster_contrib) behind the render that was kept; it combines freely with return_aux and features, nothing of it is
differentiable and the backward neither sees nor saves anything of it; without `contrib` the call enqueues exactly what it
did before.  `weight` is summed with float atomics (not bit-reproducible); the other results are exact.  A wrong length, dtype
or a non-contiguous tensor, or contrib_slots without contrib, raises ValueError before a device is touched.

`forward(..., absgrad=True)` returns AbsGS's densification statistic (gsplat's `absgrad`) next to the signed gradient.
means2D.grad is a SIGNED sum over the pixels a Gaussian covers: a large Gaussian that straddles an over-reconstructed region
gets per-pixel pulls in opposite directions, they cancel, and the Gaussians that most need splitting score lowest.  With the
flag `means2D` must be [P,4] and its gradient holds, with L = sum_p L_p the loss on the colour image, (mx_i, my_i) Gaussian
i's pixel mean and W, H the image size:

  grad[:, 0:2] = the signed gradient exactly as without the flag (0.5 W dL/dmx_i, 0.5 H dL/dmy_i)
  grad[:, 2]   = 0.5 W sum_p |dL_p / dmx_i|          grad[:, 3] = 0.5 H sum_p |dL_p / dmy_i|

in the same convention (pixel-mean gradient x 0.5 W, x 0.5 H), summed over exactly the contributors the colour backward walks
with the same alphas: the same 1/255 skip, the same 0.99 cap, the same stop where the forward stopped the pixel, and with
antialiasing the same opacity * h.  Culled Gaussians get four exact zeros.  The absolute columns hold the COLOUR image's share
only: gradients that arrive through the depth / inverse-depth / alpha maps or the feature map keep flowing into the signed
columns and are not part of the absolute ones (their blends are separate kernels, and |a| + |b| per blend is not a quantity
anyone densifies on); a backward in which the colour image got no gradient leaves them zero.  The per-pixel terms exist only
inside the blend backward, whose ABS instance (csrc/raster_blend_rows.hip) reduces the two extra values with the others;
the backward is then cgs_raster_backward_abs in every form, with return_aux, features, contrib, antialiasing and camera
gradients as before.  Summed with float atomics like the signed gradient: not bit-reproducible.  A [P,4] means2D without the
keyword, or the keyword with any other shape, raises ValueError before a device is touched; without the flag the call enqueues
exactly what it did before.  densify.training_statis accumulates ||grad[:, 2:4]|| when it is handed a [P,4] gradient.

`forward(..., return_geometry=True)` returns the two maps people regularise and measure geometry with, `(color, radii, extras)`
with `extras["distortion"]` and `extras["median_depth"]` float32 [1,H,W] and `extras["median_id"]` int32 [H,W]
(csrc/raster_geom_maps.hip, cgs_raster_render_geom: one more walk of the view's tile lists).  For pixel p the contributors
i = 1..n are exactly those of the colour blend, front to back: the same order, the same alpha_i = min(0.99, o_i exp(power)), the
same skip below 1/255, each pixel stopping where the colour pass stopped it (n_contrib), with antialiasing the same opacity * h.
Let T_1 = 1, T_{i+1} = T_i (1 - alpha_i), w_i = alpha_i T_i, z_i the view-space depth of Gaussian i's centre (the value
`return_aux` blends), A_i = sum_{k<=i} w_k and D_i = sum_{k<=i} w_k z_k:

  distortion[p]   = 2 sum_i w_i (z_i A_{i-1} - D_{i-1})
  median_depth[p] = z_m,  m = the first contributor with T_m (1 - alpha_m) < 0.5;   0 where no contributor crosses
  median_id[p]    = index of m in the call's Gaussian order (int32), -1 where none

The distortion is Mip-NeRF 360's distortion loss as 2DGS, gsplat (`distloss`), GOF and RaDe-GS render it, defined by this running
sum as gsplat defines it; the lists are sorted by the float bits of z, so z is non-decreasing along a list and the sum equals
sum_{i,j} w_i w_j |z_i - z_j|.  It is in depth units, homogeneous of degree 1 in z, not normalised (divide by a scene scale if
you want) and the background contributes nothing.  The median depth is the depth mesh extraction and depth evaluation use: the
expected depth depth / alpha smears across occlusion edges.  Gradients of the distortion, with
e_i = 2 [z_i A_{i-1} - D_{i-1} + (D_n - D_i) - z_i (A_n - A_i)]: through the weights it is the colour blend's backward with the
per-pixel scalar "colour" e_i over a zero background, d/dalpha_i = T_i e_i - (sum_{k>i} e_k w_k) / (1 - alpha_i), reaching
means2D, opacities, means3D and scales / rotations or cov3D_precomp; directly through z, d/dz_i = 2 w_i (A_{i-1} - (A_n - A_i)),
chained to means3D through the view matrix as the maps' dL/dz; shs and colors_precomp get none.  The median depth sends
dL/dz_m += g[p] to the chosen Gaussian and nothing else (the choice is not differentiable); median_id is not differentiable.
The keyword combines with all four argument forms, antialiasing, return_aux, features, contrib, absgrad (the new share goes to
the signed columns only, as for the other maps) and camera gradients, and stays the one autograd node: the forward's sums the
backward needs (`moments` [2,H,W]) are saved and not returned, and the backward is cgs_raster_backward_geom when one of the two
maps got a gradient; when neither did, no geometry backward kernel runs and the backward is the one of a call without the
keyword.  Float atomics like the other side passes: not bit-reproducible.  Without the keyword the call enqueues exactly what it
did before.

`forward(..., return_normals=True)` returns the rendered normal map, `extras["normals"]` float32 [3,H,W]:

  normals[c, p] = sum_i w_i n_i[c]

over the colour blend's own contributors and weights and a zero background, with n_i = gaussian_normals(means3D, scales,
rotations, raster_settings)[i] (contextgs_amd/normals.py, csrc/normal_maps.hip): the axis of Gaussian i's smallest scale, from
the NORMALISED quaternion, in CAMERA space (the view space of `viewmatrix`: x right, y down, z forward) and turned AWAY from
the camera (n_i . t_i >= 0), the hemisphere of the reference's computeNormalsFromPosCam_Batched and of
normals.depth_normals, the opposite of 2DGS's convention.  The map is not normalised: its length is at most alpha; divide by
alpha for a unit-ish normal.  The three columns are appended to the feature matrix of the feature walk above and split off
its output: no second blend kernel runs.  Gradients flow as for `features` (means2D, opacities, means3D, scales, rotations
through the weights), plus gaussian_normals' own backward into `rotations`.  The keyword combines with return_aux,
return_geometry, contrib, absgrad, antialiasing, SH colours and user `features` of at most CGS_RASTER_MAX_FEATURES - 3 = 29
columns.  ValueError before a device is touched: cov3D_precomp (no axes to read), more than 29 feature columns,
deterministic=True (as for `features`), and a `viewmatrix` that requires a gradient (n_i's own dependence on the camera is not
differentiated; a silently partial camera gradient is worse than a refusal).  Without the keyword the call enqueues exactly
what it did before.  normals.normal_consistency(extras["normals"], depth, raster_settings, weight=alpha) is the regulariser.

`forward(..., deterministic=True)` makes the backward bit-reproducible.  The forward already is (no atomics in the blend, a
stable depth sort, binnings that leave the same lists); the default backward sums every Gaussian's partial gradients with float
atomics, in LDS inside a tile and in global memory across tiles, in the order of arrival.  With the flag the backward is
cgs_raster_backward_det (include/cgs.h has the contract and the slot formula): inside a tile every wave sums into a plane of its
own in a fixed order, every (Gaussian, tile) pair stores its sums to a slot of its own, and a per-Gaussian kernel adds a
Gaussian's slots in an order that depends on its tile count only.  Every gradient the node returns (means3D, means2D with 3 or
4 columns, shs / colors_precomp, opacities, scales / rotations or cov3D_precomp, the three camera tensors) is then bit-identical
from call to call for the same input bits, library build and device model, whichever binning ran, with or without pair-count
speculation, whatever else the device does; the values are the default backward's up to the order of the sums.  All four
argument forms, antialiasing, absgrad and camera gradients are covered; the forward is untouched.  NOT covered, and refused with
ValueError before a device is touched: return_aux, features, contrib, return_normals and return_geometry (the map, feature and geometry blends'
backward and GaussianContrib.weight are separate kernels that sum with float atomics).  `deterministic=None` (the default) reads the
environment variable CGS_RASTER_DETERMINISTIC (1 = on), so that a training script that never heard of the keyword can be
switched; without the flag the call enqueues exactly what it did before.  The mode costs a workspace of 48 bytes per
(Gaussian, tile) pair and time (DESIGN.md sections 4 and 7 have the numbers).
"""
from __future__ import annotations

import collections
import ctypes as C
import os
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import _lib


class _SettingsFields(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


class GaussianRasterizationSettings(_SettingsFields):
    """The reference fork's twelve fields (`_fields`, gaussian_renderer/__init__.py:179-192) plus upstream's
    `antialiasing`, its last argument (positional 13th or keyword, default False).  `antialiasing` is an attribute rather
    than a tuple field so that the twelve-field tuple the fork's code unpacks and compares stays exactly as it was;
    `_replace`, repr and pickling carry it."""
    antialiasing = False

    def __new__(cls, *args, antialiasing=False, **kw):
        if len(args) == len(_SettingsFields._fields) + 1:
            args, antialiasing = args[:-1], args[-1]
        self = super().__new__(cls, *args, **kw)
        self.antialiasing = bool(antialiasing)
        return self

    def _replace(self, **kw):
        aa = kw.pop("antialiasing", self.antialiasing)
        return type(self)(*tuple(super()._replace(**kw)), antialiasing=aa)

    def __reduce__(self):
        return type(self), tuple(self) + (self.antialiasing,)

    def __repr__(self):
        return super().__repr__()[:-1] + f", antialiasing={self.antialiasing!r})"


def _f32c(t: torch.Tensor) -> torch.Tensor:
    """float32, contiguous.  A camera's matrices arrive as transposed views (scene/cameras.py builds them with .transpose(0, 1)):
    the dense copy is made once per tensor and kept on the tensor object, keyed by its version counter (two launches per step
    otherwise)."""
    if t.dtype == torch.float32 and t.is_contiguous():
        return t
    hit = getattr(t, "_cgs_f32c", None)
    if hit is not None and hit[0] == t._version:
        return hit[1]
    r = t.detach().float().contiguous()
    try:
        t._cgs_f32c = (t._version, r)
    except Exception:
        pass
    return r


class _Cfg:
    """Owns the ctypes struct plus the device tensors it points at."""

    def __init__(self, rs: GaussianRasterizationSettings):
        self.view = _f32c(rs.viewmatrix)
        self.proj = _f32c(rs.projmatrix)
        self.bg = _f32c(rs.bg)
        self.campos = _f32c(rs.campos) if rs.campos is not None else None
        _lib.require_device(self.view, self.proj, self.bg)
        self.c = _lib.RasterCfg(
            image_height=int(rs.image_height), image_width=int(rs.image_width),
            tanfovx=float(rs.tanfovx), tanfovy=float(rs.tanfovy),
            scale_modifier=float(rs.scale_modifier), prefiltered=int(bool(rs.prefiltered)),
            debug=int(bool(rs.debug)),
            viewmatrix=_lib.ptr(self.view), projmatrix=_lib.ptr(self.proj),
            campos=_lib.ptr(self.campos), bg=_lib.ptr(self.bg))

    @property
    def ref(self):
        return C.byref(self.c)


last_call: dict = {}   # sizes / image workspace of the most recent forward (bench.py's byte accounting)

# Pair-count speculation (cgs_raster_render_spec): the binning + blend of a view are enqueued before the host has read the
# view's pair count, into a workspace whose capacity is kept per image size (1.25 x the count that last exceeded it, rounded
# up to a whole 2^20 pairs, so that the workspace keeps ONE size and the caching allocator keeps handing out the same block:
# a capacity that crept up with every new maximum cost a fresh multi-GB hipMalloc each time); the count is
# read through an event while the device renders.  A view that needs more pairs than that is rendered again with its true
# count (same buffers, same stream: nothing has consumed the first attempt).  CGS_RASTER_SPEC=0 turns it off.
SPECULATE = os.environ.get("CGS_RASTER_SPEC", "1") != "0"
_pair_capacity: dict = {}     # (H, W) -> capacity (pairs) of the speculative binning workspace


def pair_capacity_for(num_rendered: int) -> int:
    """The capacity a view with `num_rendered` pairs sets for the following views of its image size."""
    return ((num_rendered + num_rendered // 4 + 4096 + (1 << 20) - 1) >> 20) << 20


def _workspace(nbytes: int, device) -> torch.Tensor:
    # (plain caching-allocator blocks.  A pool of size-classed buffers of our own was tried in round 5 while hunting 19 ms steps
    #  at 136 M pairs — it was not the cause (a leak in ctx_ops._LevelFused was) and cost 0.3 ms of host time per step: removed)
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def bin_and_blend(cfg, P, geom, img, color, stream, ticket):
    """Everything of a view's forward behind a cgs_raster_preprocess*_launch on `geom`: the speculative binning + blend with
    the image size's pair capacity, the read of the pair count, and the re-render with the true count when the capacity did
    not hold.  Returns (binning workspace, the pair count it was carved with = the backward's `R`, the view's pair count)."""
    L = _lib.lib()
    dev = geom.device
    H, W = cfg.c.image_height, cfg.c.image_width
    R = C.c_int64(0)
    tiles = ((H + 15) // 16) * ((W + 15) // 16)
    cap = _pair_capacity.get((H, W), 0) if (SPECULATE and P > 0 and tiles <= 65536) else 0
    binws = None
    if cap:
        binws = _workspace(L.cgs_raster_bin_bytes(P, cap), dev)
        _lib.check(L.cgs_raster_render_spec(cfg.ref, P, cap, _lib.ptr(geom), geom.numel(), _lib.ptr(binws),
                                            binws.numel(), _lib.ptr(img), img.numel(), _lib.ptr(color), stream),
                   "cgs_raster_render_spec")
    resorted = C.c_int(0)        # the view was sorted again on 32-bit depth keys (a depth beyond ~13107): the speculative render is void
    _lib.check(L.cgs_raster_preprocess_wait2(ticket, C.byref(R), C.byref(resorted)), "cgs_raster_preprocess_wait")
    num_rendered = int(R.value)
    if num_rendered > _pair_capacity.get((H, W), 0):
        _pair_capacity[(H, W)] = pair_capacity_for(num_rendered)
    bin_R = cap                              # the count the binning workspace was carved with (the backward's `R`)
    if not cap or num_rendered > cap or resorted.value:
        bin_R = num_rendered
        binws = _workspace(L.cgs_raster_bin_bytes(P, num_rendered), dev)
        _lib.check(L.cgs_raster_render(cfg.ref, P, num_rendered, _lib.ptr(geom), geom.numel(), _lib.ptr(binws),
                                       binws.numel(), _lib.ptr(img), img.numel(), _lib.ptr(color), stream),
                   "cgs_raster_render")
    last_call.update(P=P, num_rendered=num_rendered, bin_R=bin_R, img_ws=img, geom_ws=geom, bin_ws=binws, cfg=cfg)
    return binws, bin_R, num_rendered


def _check_cov_form(scales, rotations, cov3D_precomp) -> None:
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
            ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise ValueError("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")


def check_forms(shs, colors_precomp, scales, rotations, cov3D_precomp, sh_degree=None) -> None:
    """Upstream's argument rules (diff_gaussian_rasterization.GaussianRasterizer.forward) plus the SH shape rules, on shapes
    only: no device is touched."""
    if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
        raise ValueError("Please provide excatly one of either SHs or precomputed colors!")
    _check_cov_form(scales, rotations, cov3D_precomp)
    if shs is not None:
        D = int(sh_degree)
        if shs.dim() != 3 or shs.shape[2] != 3:
            raise ValueError(f"shs must be [P, M, 3], got {tuple(shs.shape)}")
        if not 0 <= D <= 3:
            raise ValueError(f"sh_degree {D} outside 0..3")
        if not (D + 1) ** 2 <= shs.shape[1] <= 16:
            raise ValueError(f"sh_degree {D} needs {(D + 1) ** 2}..16 SH coefficients per Gaussian, got {shs.shape[1]}")
    if cov3D_precomp is not None and (cov3D_precomp.dim() != 2 or cov3D_precomp.shape[1] != 6):
        raise ValueError(f"cov3D_precomp must be [P, 6], got {tuple(cov3D_precomp.shape)}")


CGS_RASTER_ANTIALIAS = 1      # include/cgs.h: the option bit of the *_opt entry points
CGS_RASTER_CAMERA_MAPS = 2    # include/cgs.h, cgs_raster_camera_backward: the scratch is that of cgs_raster_backward_opt (dL/dz)
CGS_RASTER_MAX_FEATURES = 32  # include/cgs.h: channels of `features`


def check_features(features, P) -> None:
    """Shape rules of `features` [P, C], on shapes only: no device is touched."""
    if features is None:
        return
    if features.dim() != 2:
        raise ValueError(f"features must be [P, C], got {tuple(features.shape)}")
    if features.shape[0] != P:
        raise ValueError(f"features has {features.shape[0]} rows for {P} Gaussians")
    if not 1 <= features.shape[1] <= CGS_RASTER_MAX_FEATURES:
        raise ValueError(f"features has {features.shape[1]} channels, outside 1..{CGS_RASTER_MAX_FEATURES}")


def check_absgrad(means2D, absgrad, P) -> None:
    """`absgrad` and the width of means2D go together ([P,4] with it, never without), on shapes only: no device is touched."""
    shape = tuple(means2D.shape) if means2D is not None else None
    if absgrad:
        if shape != (P, 4):
            raise ValueError(f"absgrad=True needs means2D [P, 4] = [{P}, 4] (signed x, y | absolute x, y), got {shape}")
    elif shape is not None and len(shape) == 2 and shape[1] == 4:
        raise ValueError(f"means2D is {shape}: four columns are the layout of absgrad=True, which was not given")


def check_deterministic(deterministic, return_aux=False, features=None, contrib=None, return_geometry=False,
                        return_normals=False) -> bool:
    """The resolved `deterministic` flag (None: the environment variable CGS_RASTER_DETERMINISTIC, 1 = on).  With the flag on,
    the keywords whose backward or accumulation still sums with float atomics are refused; no device is touched.  With the flag
    off nothing is checked."""
    if deterministic is None:
        deterministic = os.environ.get("CGS_RASTER_DETERMINISTIC", "0") == "1"
    if not deterministic:
        return False
    for name, given in (("return_aux", bool(return_aux)), ("features", features is not None),
                        ("contrib", contrib is not None and contrib is not False)):
        if given:
            raise ValueError(f"deterministic=True does not cover {name}: the depth / alpha map blends, the feature blend and "
                             f"GaussianContrib.weight sum with float atomics (not covered: return_aux, features, contrib)")
    if return_geometry:
        raise ValueError("deterministic=True does not cover return_geometry: the distortion / median-depth blend's backward sums "
                         "with float atomics (not covered: return_aux, features, contrib, return_geometry)")
    if return_normals:
        raise ValueError("deterministic=True does not cover return_normals: the normal map is three more columns of the feature "
                         "blend, whose backward sums with float atomics (not covered: return_aux, features, contrib, "
                         "return_geometry, return_normals)")
    return True


def check_normals(return_normals, features, cov3D_precomp, viewmatrix) -> None:
    """Rules of `return_normals`, on shapes and flags only: no device is touched."""
    if not return_normals:
        return
    if cov3D_precomp is not None:
        raise ValueError("return_normals=True needs scales and rotations: a cov3D_precomp has no axes to read a normal from")
    if features is not None and features.shape[1] > CGS_RASTER_MAX_FEATURES - 3:
        raise ValueError(f"return_normals=True takes three of the {CGS_RASTER_MAX_FEATURES} feature channels: features has "
                         f"{features.shape[1]} columns, more than {CGS_RASTER_MAX_FEATURES - 3}")
    if isinstance(viewmatrix, torch.Tensor) and viewmatrix.requires_grad:
        raise ValueError("return_normals=True with a viewmatrix that requires a gradient: the normals' own dependence on the "
                         "camera is not differentiated, and a silently partial camera gradient is worse than a refusal "
                         "(pass viewmatrix.detach(), or render the normals in a second call)")


class GaussianContrib:
    """Per-Gaussian (or per-slot) contribution statistics accumulated over views: `weight`, `max_weight` float32 [n], `pixels`,
    `top_pixels` int64 [n] (module docstring), and `views`, the number of calls accumulated since the last reset."""
    FIELDS = (("weight", torch.float32), ("max_weight", torch.float32), ("pixels", torch.int64), ("top_pixels", torch.int64))

    def __init__(self, weight, max_weight, pixels, top_pixels, views=0):
        self.weight, self.max_weight, self.pixels, self.top_pixels = weight, max_weight, pixels, top_pixels
        self.views = int(views)

    @classmethod
    def zeros(cls, n, device=None):
        return cls(*(torch.zeros(int(n), dtype=dt, device=device) for _, dt in cls.FIELDS))

    def tensors(self):
        return tuple(getattr(self, name) for name, _ in self.FIELDS)

    def __len__(self):
        return int(self.weight.shape[0])

    def reset(self):
        for t in self.tensors():
            t.zero_()
        self.views = 0
        return self


def check_contrib(contrib, contrib_slots, means3D) -> None:
    """Rules of `contrib` (None, True or a GaussianContrib) / `contrib_slots`, on shapes, dtypes, strides and the tensors'
    `.device` attributes only: no device is touched."""
    P = means3D.shape[0]
    if contrib is None:
        if contrib_slots is not None:
            raise ValueError("contrib_slots given without contrib")
        return
    if contrib_slots is not None:
        if not isinstance(contrib_slots, torch.Tensor) or contrib_slots.dtype != torch.int32:
            raise ValueError(f"contrib_slots must be an int32 tensor, got {getattr(contrib_slots, 'dtype', type(contrib_slots))}")
        if contrib_slots.dim() != 1 or contrib_slots.shape[0] != P:
            raise ValueError(f"contrib_slots must be [P] = [{P}], got {tuple(contrib_slots.shape)}")
        if not contrib_slots.is_contiguous():
            raise ValueError("contrib_slots must be contiguous")
        if contrib_slots.device != means3D.device:
            raise ValueError(f"contrib_slots is on {contrib_slots.device}, means3D on {means3D.device}")
    if contrib is True:
        return
    if not isinstance(contrib, GaussianContrib):
        raise ValueError(f"contrib must be a GaussianContrib or True, got {type(contrib).__name__}")
    n = contrib.weight.shape[0] if contrib.weight.dim() == 1 else -1
    for (name, dt), t in zip(GaussianContrib.FIELDS, contrib.tensors()):
        if t.dtype != dt:
            raise ValueError(f"contrib.{name} must be {dt}, got {t.dtype}")
        if t.dim() != 1 or t.shape[0] != n:
            raise ValueError(f"contrib.{name} must be [n] like contrib.weight, got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"contrib.{name} must be contiguous")
        if t.device != means3D.device:      # (the kernel writes through raw pointers in means3D's device context)
            raise ValueError(f"contrib.{name} is on {t.device}, means3D on {means3D.device}")
    if contrib_slots is None and n != P:
        raise ValueError(f"contrib has {n} rows for {P} Gaussians (any length needs contrib_slots)")
    if contrib_slots is not None and n < 1:
        raise ValueError("contrib needs at least one row with contrib_slots")


class RasterRequest(NamedTuple):
    """What a call wants besides colour and radii (module docstring): the one non-tensor argument of _RasterizeGaussians besides
    the settings.  `contrib`: the GaussianContrib accumulated into (None: off); `normals`: how many trailing columns of the
    node's `features` are the Gaussians' normals (0 or 3)."""
    aux: bool = False
    contrib: Optional["GaussianContrib"] = None
    contrib_slots: Optional[torch.Tensor] = None
    absgrad: bool = False
    deterministic: bool = False
    geometry: bool = False
    normals: int = 0

    def flags(self) -> "RasterRequest":
        """The request without its objects (contrib: True or None), as the node keeps it for the backward."""
        return self._replace(contrib=None if self.contrib is None else True, contrib_slots=None)

    def keywords(self) -> dict:
        """The request as keywords of GaussianRasterizer.forward."""
        return dict(return_aux=self.aux, contrib=self.contrib, contrib_slots=self.contrib_slots, absgrad=self.absgrad,
                    deterministic=self.deterministic, return_geometry=self.geometry, return_normals=bool(self.normals))


AUX_MAPS = ("depth", "invdepth", "alpha")
CONTRIB_MAPS = ("top_id", "top_weight", "count")
GEOMETRY_MAPS = ("distortion", "median_depth", "median_id")
NON_DIFFERENTIABLE = frozenset(("radii", "top_id", "top_weight", "count", "median_id"))
# the inputs of _RasterizeGaussians.forward behind ctx: the backward's return, ctx.needs_input_grad by name
INPUT_NAMES = ("request", "means3D", "means2D", "shs", "colors", "opacities", "scales", "rotations", "cov3D", "raster_settings",
               "viewmatrix", "projmatrix", "campos", "features")


def output_names(request: RasterRequest, has_features: bool) -> tuple:
    """The node's outputs in order, for the forward's return, the backward's incoming gradients and the caller's extras."""
    return (("color", "radii") + (AUX_MAPS if request.aux else ()) + (CONTRIB_MAPS if request.contrib is not None else ())
            + (GEOMETRY_MAPS if request.geometry else ()) + (("features",) if has_features else ()))


def named_extras(request: RasterRequest, has_user_features: bool, out: dict) -> dict:
    """GaussianRasterizer.forward's third value from the node's outputs by name.  The one place that knows that the normals
    are the three trailing channels of the feature map."""
    extras = {}
    for k, v in out.items():
        if k == CONTRIB_MAPS[0]:
            extras["contrib"] = request.contrib
        if k not in ("color", "radii", "features"):
            extras[k] = v
    if has_user_features:
        extras["features"] = out["features"][:-request.normals] if request.normals else out["features"]
    if request.normals:
        extras["normals"] = out["features"][-request.normals:]
    return extras


class _KeptView(NamedTuple):
    """The render of a view that bin_and_blend kept: what every further walk of its lists and its backward are pointed at.
    R: the pair count the binning workspace was carved with."""
    cfg: _Cfg
    P: int
    R: int
    geom: torch.Tensor
    binws: Optional[torch.Tensor]
    img: torch.Tensor

    def args(self) -> tuple:
        """cfg, P, R and the three workspaces, pointer and bytes each: the nine leading arguments of cgs_raster_render_aux,
        _render_features, _render_geom and cgs_raster_contrib (include/cgs.h)."""
        p = _lib.ptr
        return (self.cfg.ref, self.P, self.R, p(self.geom), self.geom.numel(), p(self.binws),
                self.binws.numel() if self.binws is not None else 0, p(self.img), self.img.numel())


# the gradient buffers of a cgs_raster_backward* call, carved from two allocations (`rest` is the whole second one)
_BackwardBuffers = collections.namedtuple("_BackwardBuffers", "rest means3D means2D colors opac scales rots cov")


def carve_backward_buffers(P, m2, dev, cov_form=False, zero_acc=True, rows=None, opac_shape=None) -> _BackwardBuffers:
    """For both autograd nodes.  One allocation for what the blends accumulate atomically, dL/dcolors (read by the SH backward)
    | dL/dopacities: zero-filled, or left empty for the deterministic backward, which writes every row of both itself.  One for
    what the preprocess backward writes for EVERY Gaussian (zeros for culled ones): dL/dmeans3D | dL/dmeans2D [P, m2] |
    dL/dscales | dL/drotations, or | dL/dcov3D with `cov_form`.  rows: the rows allocated (default P)."""
    rows = P if rows is None else rows
    acc = (torch.zeros if zero_acc else torch.empty)(rows * 4, dtype=torch.float32, device=dev)
    rest = torch.empty(rows * (3 + m2 + (6 if cov_form else 7)), dtype=torch.float32, device=dev)
    at = (3 + m2) * P
    return _BackwardBuffers(
        rest, rest[:3 * P].view(P, 3), rest[3 * P:at].view(P, m2), acc[:3 * P].view(P, 3),
        acc[3 * P:4 * P].view(opac_shape or (P, 1)),
        None if cov_form else rest[at:at + 3 * P].view(P, 3), None if cov_form else rest[at + 3 * P:at + 7 * P].view(P, 4),
        rest[at:at + 6 * P].view(P, 6) if cov_form else None)


def launch_backward(view, inputs, D, M, g, maps, grads, stream, opts=0, absgrad=False, deterministic=False,
                    features=None, geometry=None):
    """The one cgs_raster_backward* call of a view, for both autograd nodes (_RasterizeGaussians, renderer._ExpandRasterize).
    view: the _KeptView; inputs: (means3D, colors, shs, opacities, scales, rotations, cov3D, radii), None for what the form does
    not have; g, maps: the upstream gradients of the colour image and of the depth / inverse-depth / alpha maps (None: no
    gradient); grads: (dL_dmeans3D,
    dL_dmeans2D [P, 4 with absgrad else 3], dL_dcolors, dL_dopacities, dL_dshs, dL_dscales, dL_drotations, dL_dcov3D), the
    caller's buffers (dL_dcolors / dL_dopacities zero-filled unless `deterministic`); features: (features, the feature map's
    gradient, dL_dfeatures zero-filled) or None; geometry: (moments, median_id, the distortion map's gradient, the median-depth
    map's gradient) when one of the two got a gradient, else None (dL_dmeans2D is then [P, 4] whatever `absgrad`).  The entry
    point: geometry -> _geom; deterministic -> _det (the colour image alone); absgrad ->
    _abs, whatever got a gradient; maps, an option bit or a feature-map gradient -> _feat (without features it is
    cgs_raster_backward_opt's); otherwise the colour image alone -> _ex (cgs_raster_backward for colours + scales / rotations).
    Returns the scratch, which cgs_raster_camera_backward reads, and the `opts` to call that with."""
    L = _lib.lib()
    p = _lib.ptr
    means3D, colors, shs, opac, scales, rots, cov, radii = inputs
    P, dev = view.P, means3D.device
    feat, g_fmap, d_feat = features if features is not None else (None, None, None)
    m2 = 4 if absgrad else 3        # columns of dL/dmeans2D
    map_ptrs = tuple(p(t) for t in maps)
    tail = (opts, p(feat), feat.shape[1] if feat is not None else 0, p(g_fmap), p(d_feat))
    # (every scratch but _ex's begins with cgs_raster_backward_opt's; _det writes its dL/dz zero)
    cam_opts = opts | CGS_RASTER_CAMERA_MAPS
    if geometry is not None:
        name, scratch_bytes = "cgs_raster_backward_geom", L.cgs_raster_bwd_abs_scratch_bytes(P)
        tail += tuple(p(t) for t in geometry)
    elif deterministic:
        name, scratch_bytes = "cgs_raster_backward_det", L.cgs_raster_bwd_abs_scratch_bytes(P)
    elif absgrad:
        name, scratch_bytes = "cgs_raster_backward_abs", L.cgs_raster_bwd_abs_scratch_bytes(P)
    elif features is not None or opts or any(t is not None for t in maps):
        name, scratch_bytes = "cgs_raster_backward_feat", L.cgs_raster_bwd_aux_scratch_bytes(P)
    else:
        name, scratch_bytes, map_ptrs, tail, cam_opts = "cgs_raster_backward_ex", L.cgs_raster_bwd_scratch_bytes(P), (), (), 0
    scratch = _workspace(scratch_bytes, dev)
    if deterministic:
        det_ws = _workspace(L.cgs_raster_bwd_det_bytes(P, view.R, m2), dev)
        tail = (opts, m2, p(det_ws), det_ws.numel())
    kept = view.args()
    _lib.check(getattr(L, name)(
        *kept[:3], p(means3D), p(colors), p(shs), D, M, p(opac), p(scales), p(rots), p(cov), p(radii), *kept[3:],
        p(g), *map_ptrs, *(p(t) for t in grads), p(scratch), scratch.numel(), stream, *tail), name)
    return scratch, cam_opts


class _RasterizeGaussians(torch.autograd.Function):
    """The one node of the drop-in: any of the four argument forms (absent inputs are None), antialiasing from
    `raster_settings.antialiasing`, and the depth / inverse-depth / alpha maps as three more outputs when `aux`.  The forward
    is cgs_raster_preprocess_launch_opt (with no option bit and neither shs nor cov3D it is cgs_raster_preprocess_launch), the
    binning and colour blend, then one walk of the final per-tile lists for the maps.  The backward is cgs_raster_backward_ex
    (cgs_raster_backward for colours + scales / rotations) when only the colour image got a gradient and antialiasing is off,
    cgs_raster_backward_feat otherwise (without features it is cgs_raster_backward_opt): it runs no colour blend backward when
    the image got none, and with antialiasing its per-Gaussian kernel turns the blends' dL/d(opacity * h) into dL/d(opacity) and
    chains h's gradient to the covariance.  With `features` [P, C] (the last input; None = none of this runs) one more walk of
    the lists gives the feature map as the last output (cgs_raster_render_features), and when that map got a gradient the same
    backward call runs the feature blend backward too.
    With `contrib` (a GaussianContrib; None = none of this runs) one more walk accumulates into it and gives the
    top_id / top_weight / count maps as three non-differentiable outputs behind the aux maps (cgs_raster_contrib).
    With `absgrad` the forward is unchanged and the backward is cgs_raster_backward_abs whatever got a gradient: means2D's
    gradient is [P,4], the signed columns and the absolute sums of the colour image's per-pixel terms (module docstring).
    With `deterministic` (never together with aux, features, contrib or geometry) the forward is unchanged and the backward is
    cgs_raster_backward_det: no float atomics, bit-reproducible gradients (module docstring).
    With `geometry` one more walk gives the distortion and median-depth maps and the non-differentiable median_id behind the
    contrib maps (cgs_raster_render_geom); its moments and median_id are saved, and when one of the two maps got a gradient the
    backward is cgs_raster_backward_geom (module docstring).
    `aux`, `contrib` (with `contrib_slots`), `absgrad`, `deterministic` and `geometry` are fields of `request`, a RasterRequest,
    of which the node keeps the flags only.  Nothing here counts positions: the outputs, and the gradients that come back for
    them, go by output_names(); the gradients returned, and ctx.needs_input_grad, by INPUT_NAMES."""

    @staticmethod
    def forward(ctx, request, means3D, means2D, shs, colors, opacities, scales, rotations, cov3D, raster_settings,
                viewmatrix, projmatrix, campos, features):
        # viewmatrix / projmatrix / campos: the settings' three camera tensors once more, as inputs of the node so that autograd
        # can hand them a gradient; the forward reads them through _Cfg as before
        L = _lib.lib()
        contrib, contrib_slots = request.contrib, request.contrib_slots
        _lib.require_device(means3D, shs, colors, opacities, scales, rotations, cov3D, features, contrib_slots,
                            *(contrib.tensors() if isinstance(contrib, GaussianContrib) else ()))
        means3D, shs, colors, opac, scales, rots, cov, feat = (
            None if t is None else _f32c(t) for t in (means3D, shs, colors, opacities, scales, rotations, cov3D, features))
        P = means3D.shape[0]
        dev = means3D.device
        cfg = _Cfg(raster_settings)
        if shs is not None:
            _lib.require_device(cfg.campos)
        D = int(raster_settings.sh_degree) if shs is not None else 0
        M = int(shs.shape[1]) if shs is not None else 0
        opts = CGS_RASTER_ANTIALIAS if getattr(raster_settings, "antialiasing", False) else 0
        H, W = cfg.c.image_height, cfg.c.image_width
        stream = _lib.current_stream()
        ctx.set_materialize_grads(False)        # no zero tensors for the gradients of `radii` and of unused outputs

        radii = torch.empty(P, dtype=torch.int32, device=dev)       # the preprocess kernel writes every entry (0 = culled)
        geom = _workspace(L.cgs_raster_geom_bytes(P), dev)
        img = _workspace(L.cgs_raster_img_bytes(H, W), dev)
        color = torch.empty(3, H, W, dtype=torch.float32, device=dev)
        ticket = C.c_uint64(0)
        _lib.check(L.cgs_raster_preprocess_launch_opt(
            cfg.ref, P, _lib.ptr(means3D), _lib.ptr(colors), _lib.ptr(shs), D, M, _lib.ptr(opac), _lib.ptr(scales),
            _lib.ptr(rots), _lib.ptr(cov), _lib.ptr(geom), geom.numel(), _lib.ptr(radii), stream, C.byref(ticket), opts),
            "cgs_raster_preprocess_launch_opt")
        binws, bin_R, _num_rendered = bin_and_blend(cfg, P, geom, img, color, stream, ticket)
        # every further walk runs behind the render bin_and_blend kept (a voided speculative render has been redone by now) and
        # writes every pixel of its maps
        kept = _KeptView(cfg, P, bin_R, geom, binws, img).args()
        new = lambda *shape, dtype=torch.float32, make=torch.empty: make(*shape, dtype=dtype, device=dev)
        out = {"color": color, "radii": radii}
        if request.aux:
            out.update((n, new(1, H, W)) for n in AUX_MAPS)
            _lib.check(L.cgs_raster_render_aux(*kept, *(_lib.ptr(out[n]) for n in AUX_MAPS), stream), "cgs_raster_render_aux")
        if contrib is not None:     # accumulates into the caller's object
            out.update(top_id=new(H, W, dtype=torch.int32), top_weight=new(1, H, W), count=new(H, W, dtype=torch.int32))
            # (P == 0: no row can be touched, and an empty slot table has no pointer to tell it from an absent one)
            accs = [_lib.ptr(t) for t in contrib.tensors()] if P > 0 else [None] * 4
            _lib.check(L.cgs_raster_contrib(*kept, _lib.ptr(contrib_slots) if P > 0 else None, len(contrib) if P > 0 else 0,
                                            *accs, *(_lib.ptr(out[n]) for n in CONTRIB_MAPS), stream), "cgs_raster_contrib")
            contrib.views += 1
        geom_saved = ()
        if request.geometry:    # (P == 0: the call enqueues nothing, the fills below stand)
            make = torch.empty if P > 0 else torch.zeros
            out.update(distortion=new(1, H, W, make=make), median_depth=new(1, H, W, make=make))
            out["median_id"] = (new(H, W, dtype=torch.int32) if P > 0
                                else torch.full((H, W), -1, dtype=torch.int32, device=dev))
            moments = new(2, H, W, make=make)
            _lib.check(L.cgs_raster_render_geom(*kept, *(_lib.ptr(out[n]) for n in GEOMETRY_MAPS), _lib.ptr(moments), stream),
                       "cgs_raster_render_geom")
            geom_saved = (moments, out["median_id"])
        if feat is not None:
            out["features"] = new(feat.shape[1], H, W)
            _lib.check(L.cgs_raster_render_features(*kept, _lib.ptr(feat), feat.shape[1], _lib.ptr(out["features"]), stream),
                       "cgs_raster_render_features")
        ctx.cfg, ctx.num_rendered, ctx.D, ctx.M, ctx.opts, ctx.request = cfg, bin_R, D, M, opts, request.flags()
        ctx.save_for_backward(means3D, shs, colors, opac, scales, rots, cov, radii, geom, binws, img, feat, *geom_saved)
        names = output_names(request, feat is not None)
        ctx.mark_non_differentiable(*(out[n] for n in names if n in NON_DIFFERENTIABLE))      # ONE call: torch keeps only the last
        return tuple(out[n] for n in names)

    @staticmethod
    def backward(ctx, *grad_outputs):
        L = _lib.lib()
        means3D, shs, colors, opac, scales, rots, cov, radii, geom, binws, img, feat, *geom_saved = ctx.saved_tensors
        req = ctx.request
        g = {k: None if t is None else _f32c(t) for k, t in zip(output_names(req, feat is not None), grad_outputs)}
        maps = [g.get(k) for k in AUX_MAPS]
        g_geom = [g.get("distortion"), g.get("median_depth")]
        with_geom = any(t is not None for t in g_geom)       # (neither map got a gradient: the backward of a call without them)
        with_feat = g.get("features") is not None
        grads = dict.fromkeys(INPUT_NAMES)
        if g["color"] is None and not with_feat and all(t is None for t in maps) and not with_geom:
            return tuple(grads.values())
        view = _KeptView(ctx.cfg, means3D.shape[0], ctx.num_rendered, geom, binws, img)
        P, dev = view.P, means3D.device
        m2 = 4 if (req.absgrad or with_geom) else 3     # columns of dL/dmeans2D (cgs_raster_backward_geom: always four)
        b = carve_backward_buffers(P, m2, dev, cov is not None, not req.deterministic, opac_shape=opac.shape)
        d_shs = torch.empty_like(shs) if shs is not None else None      # of its own: aligned as shs is (vector stores)
        d_feat = torch.zeros_like(feat) if with_feat else None          # accumulated atomically, like dL/dcolor
        stream = _lib.current_stream()
        scratch, cam_opts = launch_backward(
            view, (means3D, colors, shs, opac, scales, rots, cov, radii), ctx.D, ctx.M, g["color"], maps,
            (b.means3D, b.means2D, b.colors, b.opac, d_shs, b.scales, b.rots, b.cov), stream, ctx.opts, req.absgrad,
            req.deterministic, (feat, g["features"], d_feat) if with_feat else None,
            (*geom_saved, *g_geom) if with_geom else None)
        # the camera: only when one of its tensors asks (campos without shs is unused: None), behind the backward above while
        # its scratch and its dL_dcolors / dL_dopacities are intact
        need = dict(zip(INPUT_NAMES, ctx.needs_input_grad))
        need["campos"] = need["campos"] and shs is not None
        if need["viewmatrix"] or need["projmatrix"] or need["campos"]:
            cam = torch.empty(35, dtype=torch.float32, device=dev)
            grads.update(viewmatrix=cam[:16].view(4, 4) if need["viewmatrix"] else None,
                         projmatrix=cam[16:32].view(4, 4) if need["projmatrix"] else None,
                         campos=cam[32:] if need["campos"] else None)
            work = _workspace(L.cgs_raster_camera_bytes(P), dev)
            _lib.check(L.cgs_raster_camera_backward(
                view.cfg.ref, P, _lib.ptr(means3D), _lib.ptr(shs) if need["campos"] else None, ctx.D, ctx.M, _lib.ptr(opac),
                _lib.ptr(scales), _lib.ptr(rots), _lib.ptr(cov), _lib.ptr(radii), _lib.ptr(scratch), scratch.numel(),
                _lib.ptr(b.colors), _lib.ptr(b.opac), cam_opts, _lib.ptr(grads["viewmatrix"]), _lib.ptr(grads["projmatrix"]),
                _lib.ptr(grads["campos"]), _lib.ptr(work), work.numel(), stream), "cgs_raster_camera_backward")
        d_means2D = b.means2D
        if with_geom and not req.absgrad:       # means2D is [P, 3]: the signed columns and the zero every [P, 3] backward writes
            d_means2D = torch.nn.functional.pad(d_means2D[:, :2], (0, 1))
        grads.update(means3D=b.means3D, means2D=d_means2D, opacities=b.opac, scales=b.scales, rotations=b.rots, cov3D=b.cov,
                     features=d_feat)
        if g["color"] is not None:       # the maps and the features send no gradient to the colour inputs
            grads.update(shs=d_shs, colors=b.colors if colors is not None else None)
        return tuple(grads.values())


def _camera_inputs(rs):
    """The settings' camera tensors as inputs of the node, in their own layout (a transposed view stays one: autograd hands
    its base the transposed gradient).  A tensor that requires no gradient is passed all the same; it costs nothing."""
    return rs.viewmatrix, rs.projmatrix, rs.campos


def rasterize_gaussians(means3D, means2D, colors_precomp, opacities, scales, rotations, raster_settings):
    return _RasterizeGaussians.apply(RasterRequest(), means3D, means2D, None, colors_precomp, opacities, scales, rotations, None,
                                     raster_settings, *_camera_inputs(raster_settings), None)


def raster_stats(raster_settings: GaussianRasterizationSettings, img_ws: torch.Tensor) -> torch.Tensor:
    """[R_eff, non-empty tiles] of the last render that used `img_ws` (int64[2], device)."""
    L = _lib.lib()
    cfg = _Cfg(raster_settings)
    out = torch.zeros(2, dtype=torch.int64, device=img_ws.device)
    _lib.check(L.cgs_raster_stats(cfg.ref, _lib.ptr(img_ws), img_ws.numel(), _lib.ptr(out), _lib.current_stream()),
               "cgs_raster_stats")
    return out


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """Near-plane frustum test (the only cull the rasterizer applies)."""
        with torch.no_grad():
            rs = self.raster_settings
            ones = torch.ones_like(positions[:, :1])
            z = (torch.cat([positions, ones], dim=1) @ rs.viewmatrix)[:, 2]
            return z > 0.2

    def visible_filter(self, means3D, scales=None, rotations=None, cov3D_precomp=None):
        _check_cov_form(scales, rotations, cov3D_precomp)
        L = _lib.lib()
        _lib.require_device(means3D, scales, rotations, cov3D_precomp)
        with torch.no_grad():
            m = _f32c(means3D)
            N = m.shape[0]
            cfg = _Cfg(self.raster_settings)
            radii = torch.zeros(N, dtype=torch.int32, device=m.device)
            if cov3D_precomp is not None:
                _lib.check(L.cgs_filter_cov(cfg.ref, N, _lib.ptr(m), _lib.ptr(_f32c(cov3D_precomp)), _lib.ptr(radii),
                                            _lib.current_stream()), "cgs_filter_cov")
            else:
                _lib.check(L.cgs_filter(cfg.ref, N, _lib.ptr(m), _lib.ptr(_f32c(scales)), _lib.ptr(_f32c(rotations)),
                                        _lib.ptr(radii), _lib.current_stream()), "cgs_filter")
        return radii

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, features=None, return_aux=False, contrib=None, contrib_slots=None, absgrad=False,
                deterministic=None, return_geometry=False, return_normals=False):
        """(color [3,H,W], radii int32 [P]); with return_aux=True, features [P,C] and / or contrib a third value, the dict of
        {"depth", "invdepth", "alpha"}, float32 [1,H,W] each, {"features"}, float32 [C,H,W], and / or {"contrib", "top_id",
        "top_weight", "count"} (see the module docstring).  absgrad=True: means2D is [P,4] and its gradient's columns 2:4 are
        the sums over the pixels of the absolute per-pixel gradients of the colour image (module docstring).
        deterministic=True (None: CGS_RASTER_DETERMINISTIC=1): a bit-reproducible backward without float atomics; not with
        return_aux, features, contrib or return_geometry (module docstring).  return_geometry=True: the dict gains
        {"distortion", "median_depth"}, float32 [1,H,W], and {"median_id"}, int32 [H,W] (module docstring).
        return_normals=True: the dict gains {"normals"}, float32 [3,H,W], the blend of the Gaussians' camera-space normals
        (module docstring); scales / rotations only, not with deterministic=True or a viewmatrix that requires a gradient."""
        deterministic = check_deterministic(deterministic, return_aux, features, contrib, return_geometry, return_normals)
        check_forms(shs, colors_precomp, scales, rotations, cov3D_precomp, self.raster_settings.sh_degree)
        check_absgrad(means2D, absgrad, means3D.shape[0])
        check_features(features, means3D.shape[0])
        check_normals(return_normals, features, cov3D_precomp, self.raster_settings.viewmatrix)
        user_features = features
        if return_normals:      # three more columns of the ONE feature walk: no second blend
            from .normals import gaussian_normals      # (here, not at the top: normals.py imports _Cfg and _f32c from this module)
            nrm = gaussian_normals(means3D, scales, rotations, self.raster_settings)
            features = nrm if features is None else torch.cat([features.to(nrm.dtype), nrm], dim=1)
        if contrib is False:
            contrib = None
        check_contrib(contrib, contrib_slots, means3D)
        if contrib is True:
            contrib = GaussianContrib.zeros(means3D.shape[0], means3D.device)
        request = RasterRequest(bool(return_aux), contrib, contrib_slots, bool(absgrad), deterministic, bool(return_geometry),
                                3 if return_normals else 0)
        out = _RasterizeGaussians.apply(request, means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                        cov3D_precomp, self.raster_settings, *_camera_inputs(self.raster_settings), features)
        names = output_names(request, features is not None)
        if len(names) == 2:
            return out
        return out[0], out[1], named_extras(request, user_features is not None, dict(zip(names, out)))
