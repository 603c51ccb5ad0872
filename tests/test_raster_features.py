"""The rasterizer's N-channel feature blend without a GPU: the C-ABI entry points exist and their argument errors come back
with their code and a message (nothing is launched); the drop-in's `features` keyword is off by default, its shape rules raise
ValueError before a device is touched in all four argument forms, and a CPU call has no path; render() takes
`anchor_features` as a keyword-only argument."""
import ctypes as C
import inspect
import math

import pytest
import torch

from raster_harness import fake_cfg

CGS_ERR_ARG = 1
CGS_ERR_WORKSPACE = 3

NEW_SYMBOLS = ("cgs_raster_render_features", "cgs_raster_backward_feat")
P1 = C.c_void_p(4096)      # a non-NULL stand-in: the checks only look at which pointers are given


def _render_features(P=1, R=1, geom=P1, bin_ws=P1, img=P1, img_bytes=1 << 30, features=P1, Cn=5, out=P1):
    from contextgs_amd import _lib
    L = _lib.lib()
    rc = L.cgs_raster_render_features(C.byref(fake_cfg()), P, R, geom, 1 << 30, bin_ws, 1 << 30, img, img_bytes, features, Cn, out,
                                      None)
    return rc, L.cgs_last_error().decode()


def _backward_feat(P=1, R=0, geom=P1, img=P1, scratch=P1, scratch_bytes=1 << 40, features=P1, Cn=5, g_map=P1, d_feat=P1):
    """colours + scales / rotations, every other pointer given"""
    from contextgs_amd import _lib
    L = _lib.lib()
    rc = L.cgs_raster_backward_feat(C.byref(fake_cfg()), P, R, P1, P1, None, 0, 0, P1, P1, P1, None, P1, geom, 1 << 30, None, 0,
                                    img, 1 << 30, None, None, None, None, P1, P1, P1, P1, None, P1, P1, None, scratch,
                                    scratch_bytes, None, 0, features, Cn, g_map, d_feat)
    return rc, L.cgs_last_error().decode()


def test_new_symbols_resolve():
    from contextgs_amd import _lib
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n) and n in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["cgs_raster_render_features"][1]) == 13
    assert len(_lib.SIGNATURES["cgs_raster_backward_feat"][1]) == len(_lib.SIGNATURES["cgs_raster_backward_opt"][1]) + 4


@pytest.mark.parametrize("Cn", [0, -1, 33, 1 << 20])
def test_channel_count_outside_1_32_is_an_argument_error(Cn):
    for rc, msg in (_render_features(Cn=Cn), _backward_feat(Cn=Cn)):
        assert rc == CGS_ERR_ARG and "outside 1..32" in msg, (rc, msg)


def test_render_features_argument_errors():
    for kw in (dict(features=None), dict(out=None)):
        rc, msg = _render_features(**kw)
        assert rc == CGS_ERR_ARG and "go together" in msg, (kw, msg)
    for kw in (dict(img=None), dict(geom=None), dict(bin_ws=None)):
        rc, msg = _render_features(**kw)
        assert rc == CGS_ERR_ARG and "NULL workspace" in msg, (kw, msg)
    rc, msg = _render_features(P=-1)
    assert rc == CGS_ERR_ARG and "P < 0" in msg
    rc, msg = _render_features(R=0, img_bytes=16)
    assert rc == CGS_ERR_WORKSPACE and "workspace too small" in msg


def test_backward_feat_argument_errors():
    for kw in (dict(features=None), dict(d_feat=None)):
        rc, msg = _backward_feat(**kw)
        assert rc == CGS_ERR_ARG and "go together" in msg, (kw, msg)
    for kw in (dict(geom=None), dict(img=None), dict(scratch=None)):
        rc, msg = _backward_feat(**kw)
        assert rc == CGS_ERR_ARG and "NULL" in msg, (kw, msg)
    rc, msg = _backward_feat(P=-1)
    assert rc == CGS_ERR_ARG and "P < 0" in msg
    rc, msg = _backward_feat(P=1000, scratch_bytes=16)
    assert rc == CGS_ERR_WORKSPACE and "scratch" in msg
    from contextgs_amd import _lib
    L = _lib.lib()        # an unknown option bit, as cgs_raster_backward_opt
    rc = L.cgs_raster_backward_feat(C.byref(fake_cfg()), 1, 0, P1, P1, None, 0, 0, P1, P1, P1, None, P1, P1, 1 << 30, None, 0, P1,
                                    1 << 30, None, None, None, None, P1, P1, P1, P1, None, P1, P1, None, P1, 1 << 40, None, 4,
                                    P1, 5, P1, P1)
    assert rc == CGS_ERR_ARG and "cgs_raster_backward_feat" in L.cgs_last_error().decode()


def _rasterizer(sh_degree=1):
    from contextgs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    eye = torch.eye(4)
    rs = GaussianRasterizationSettings(16, 16, math.tan(0.5), math.tan(0.5), torch.zeros(3), 1.0, eye, eye, sh_degree,
                                       torch.zeros(3), False, False)
    return GaussianRasterizer(rs)


def test_features_defaults_to_none():
    from contextgs_amd.rasterizer import GaussianRasterizer
    sig = inspect.signature(GaussianRasterizer.forward).parameters
    assert sig["features"].default is None and sig["return_aux"].default is False
    from contextgs_amd.dropin import diff_gaussian_rasterization as shim
    assert shim.GaussianRasterizer is GaussianRasterizer


def _form(form, P=5):
    return dict(plain=dict(colors_precomp=torch.zeros(P, 3), scales=torch.zeros(P, 3), rotations=torch.zeros(P, 4)),
                shs=dict(shs=torch.zeros(P, 4, 3), scales=torch.zeros(P, 3), rotations=torch.zeros(P, 4)),
                shs_cov=dict(shs=torch.zeros(P, 4, 3), cov3D_precomp=torch.zeros(P, 6)),
                cov=dict(colors_precomp=torch.zeros(P, 3), cov3D_precomp=torch.zeros(P, 6)))[form]


@pytest.mark.parametrize("form", ["plain", "shs", "shs_cov", "cov"])
@pytest.mark.parametrize("shape, needle", [((5,), r"must be \[P, C\]"), ((5, 2, 2), r"must be \[P, C\]"), ((4, 3), "rows for 5 Gaussians"),
                                           ((5, 0), "outside 1..32"), ((5, 33), "outside 1..32")])
def test_shape_errors_come_before_any_device(form, shape, needle):
    P = 5
    with pytest.raises(ValueError, match=needle):       # (CPU tensors: a device check would raise RuntimeError instead)
        _rasterizer()(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.zeros(P, 1),
                      features=torch.zeros(shape), **_form(form))


@pytest.mark.parametrize("form", ["plain", "shs", "shs_cov", "cov"])
def test_features_have_no_cpu_path(form):
    P = 5
    with pytest.raises(RuntimeError, match="no CPU path"):
        _rasterizer()(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.zeros(P, 1),
                      features=torch.zeros(P, 7), **_form(form))


def test_render_accepts_the_keyword():
    from contextgs_amd import renderer
    p = inspect.signature(renderer.render).parameters["anchor_features"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
