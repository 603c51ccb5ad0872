"""The rasterizer's depth / inverse-depth / alpha maps without a GPU: the C-ABI entry points exist and their argument errors
come back as CGS_ERR_ARG with a message (nothing is launched); the drop-in's `return_aux` keyword is off by default and the
argument rules still raise first; render() takes the keyword."""
import ctypes as C
import inspect
import math

import pytest
import torch

from raster_harness import fake_cfg

CGS_ERR_ARG = 1
CGS_ERR_WORKSPACE = 3

NEW_SYMBOLS = ("cgs_raster_render_aux", "cgs_raster_backward_aux", "cgs_raster_bwd_aux_scratch_bytes")
P1 = C.c_void_p(4096)      # a non-NULL stand-in: the checks only look at which pointers are given


def _render_aux(cfg, P=1, R=1, geom=P1, bin_ws=P1, img=P1, depth=P1, invdepth=P1, alpha=P1):
    from contextgs_amd import _lib
    L = _lib.lib()
    ref = C.byref(cfg) if cfg is not None else None
    rc = L.cgs_raster_render_aux(ref, P, R, geom, 1 << 30, bin_ws, 1 << 30, img, 1 << 30, depth, invdepth, alpha, None)
    return rc, L.cgs_last_error().decode()


def _backward_aux(cfg, P=1, colors=None, shs=None, D=0, M=0, scales=None, rotations=None, cov3D=None, outs=None, scratch=P1,
                  scratch_bytes=1 << 40):
    from contextgs_amd import _lib
    L = _lib.lib()
    o = dict(means3D=P1, means2D=P1, colors=P1, opac=P1, shs=None, scales=None, rots=None, cov=None)
    o.update(outs or {})
    rc = L.cgs_raster_backward_aux(C.byref(cfg), P, 0, P1, colors, shs, D, M, P1, scales, rotations, cov3D, P1, P1, 1 << 30,
                                   None, 0, P1, 1 << 30, None, None, None, None, o["means3D"], o["means2D"], o["colors"],
                                   o["opac"], o["shs"], o["scales"], o["rots"], o["cov"], scratch, scratch_bytes, None)
    return rc, L.cgs_last_error().decode()


def test_new_symbols_resolve():
    from contextgs_amd import _lib
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n) and n in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["cgs_raster_render_aux"][1]) == 13
    assert len(_lib.SIGNATURES["cgs_raster_backward_aux"][1]) == 34
    # one more float per Gaussian (dL/dz) than the colour backward's scratch
    assert L.cgs_raster_bwd_aux_scratch_bytes(1 << 20) >= L.cgs_raster_bwd_scratch_bytes(1 << 20) + 4 * (1 << 20)


def test_render_aux_argument_errors():
    assert _render_aux(None)[0] == CGS_ERR_ARG
    rc, msg = _render_aux(fake_cfg(H=0))
    assert rc == CGS_ERR_ARG and "image size" in msg
    for kw in (dict(depth=None), dict(invdepth=None), dict(alpha=None), dict(img=None), dict(geom=None), dict(bin_ws=None)):
        rc, msg = _render_aux(fake_cfg(), **kw)
        assert rc == CGS_ERR_ARG and "NULL" in msg, (kw, msg)
    rc, msg = _render_aux(fake_cfg(), P=-1)
    assert rc == CGS_ERR_ARG and "P < 0" in msg
    rc, msg = _render_aux(fake_cfg(), R=-1)
    assert rc == CGS_ERR_ARG


@pytest.mark.parametrize("kw, needle", [
    (dict(scales=P1, rotations=P1), "exactly one of either SHs or precomputed colors"),
    (dict(colors=P1, shs=P1, M=1, scales=P1, rotations=P1), "exactly one of either SHs or precomputed colors"),
    (dict(colors=P1), "scale/rotation pair or precomputed 3D covariance"),
    (dict(colors=P1, scales=P1, rotations=P1, cov3D=P1), "scale/rotation pair or precomputed 3D covariance"),
    (dict(shs=P1, D=4, M=16, cov3D=P1), "sh_degree 4 outside 0..3"),
    (dict(shs=P1, D=2, M=8, cov3D=P1), "degree 2 needs 9..16"),
    (dict(colors=P1, scales=P1, rotations=P1), "NULL input"),                         # dL_dscales / dL_drotations missing
    (dict(shs=P1, D=1, M=4, cov3D=P1, outs=dict(cov=P1)), "NULL input"),             # dL_dshs missing
    (dict(colors=P1, cov3D=P1), "NULL input"),                                       # dL_dcov3D missing
    (dict(colors=P1, scales=P1, rotations=P1, outs=dict(scales=P1, rots=P1, colors=None)), "NULL input"),
    (dict(colors=P1, scales=P1, rotations=P1, outs=dict(scales=P1, rots=P1), scratch=None), "NULL input"),
])
def test_backward_aux_argument_errors(kw, needle):
    rc, msg = _backward_aux(fake_cfg(), **kw)
    assert rc == CGS_ERR_ARG, (rc, msg)
    assert needle in msg, msg


def test_backward_aux_small_scratch_is_a_workspace_error():
    rc, msg = _backward_aux(fake_cfg(), P=1000, colors=P1, scales=P1, rotations=P1, outs=dict(scales=P1, rots=P1), scratch_bytes=16)
    assert rc == CGS_ERR_WORKSPACE and "scratch" in msg


def test_backward_aux_sh_without_campos():
    rc, msg = _backward_aux(fake_cfg(campos=False), shs=P1, D=1, M=4, scales=P1, rotations=P1,
                            outs=dict(shs=P1, scales=P1, rots=P1))
    assert rc == CGS_ERR_ARG and "campos" in msg


def _rasterizer(sh_degree=1):
    from contextgs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    eye = torch.eye(4)
    rs = GaussianRasterizationSettings(16, 16, math.tan(0.5), math.tan(0.5), torch.zeros(3), 1.0, eye, eye, sh_degree,
                                       torch.zeros(3), False, False)
    return GaussianRasterizer(rs)


def test_return_aux_defaults_to_off():
    from contextgs_amd.rasterizer import GaussianRasterizer
    p = inspect.signature(GaussianRasterizer.forward).parameters["return_aux"]
    assert p.default is False
    from contextgs_amd.dropin import diff_gaussian_rasterization as shim
    assert shim.GaussianRasterizer is GaussianRasterizer


@pytest.mark.parametrize("return_aux", [False, True])
@pytest.mark.parametrize("kw, needle", [
    (dict(scales=True, rotations=True), "SHs or precomputed colors"),
    (dict(colors_precomp=True), "scale/rotation pair"),
    (dict(colors_precomp=True, scales=True, rotations=True, cov3D_precomp=True), "scale/rotation pair"),
])
def test_form_errors_come_first(return_aux, kw, needle):
    P = 5
    shapes = dict(shs=(P, 4, 3), colors_precomp=(P, 3), scales=(P, 3), rotations=(P, 4), cov3D_precomp=(P, 6))
    args = {k: torch.zeros(shapes[k]) for k in kw}
    with pytest.raises(ValueError, match=needle):
        _rasterizer()(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.zeros(P, 1),
                      return_aux=return_aux, **args)


@pytest.mark.parametrize("form", ["plain", "shs", "cov"])
def test_return_aux_has_no_cpu_path(form):
    P = 5
    args = dict(plain=dict(colors_precomp=torch.zeros(P, 3), scales=torch.zeros(P, 3), rotations=torch.zeros(P, 4)),
                shs=dict(shs=torch.zeros(P, 4, 3), scales=torch.zeros(P, 3), rotations=torch.zeros(P, 4)),
                cov=dict(colors_precomp=torch.zeros(P, 3), cov3D_precomp=torch.zeros(P, 6)))[form]
    with pytest.raises(RuntimeError, match="no CPU path"):
        _rasterizer(1)(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.zeros(P, 1), return_aux=True,
                       **args)


def test_render_accepts_the_keyword():
    from contextgs_amd import renderer
    p = inspect.signature(renderer.render).parameters["return_aux"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
