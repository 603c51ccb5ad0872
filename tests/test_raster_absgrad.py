"""The rasterizer's absolute screen-space gradients without a GPU: the three C-ABI entry points exist and the argument errors of
the two backward-side calls come back with their code and a message (nothing is launched); the drop-in's `absgrad` keyword is
off by default, its two shape rules raise ValueError before a device is touched in all four argument forms, and a CPU call has
no path; render() takes `absgrad` as a keyword-only argument; training_statis refuses a gradient that is neither [P,3] nor [P,4]."""
import ctypes as C
import inspect
import math
import types

import pytest
import torch

from raster_harness import fake_cfg

CGS_OK = 0
CGS_ERR_ARG = 1
CGS_ERR_WORKSPACE = 3

NEW_SYMBOLS = ("cgs_raster_backward_abs", "cgs_raster_bwd_abs_scratch_bytes", "cgs_densify_stats_ex")
P1 = C.c_void_p(4096)      # a non-NULL stand-in: the checks only look at which pointers are given


def _backward_abs(P=1, R=0, geom=P1, img=P1, scratch=P1, scratch_bytes=1 << 40, features=P1, Cn=5, g_map=P1, d_feat=P1, m2=P1,
                  opts=0):
    """colours + scales / rotations, every other pointer given"""
    from contextgs_amd import _lib
    L = _lib.lib()
    rc = L.cgs_raster_backward_abs(C.byref(fake_cfg()), P, R, P1, P1, None, 0, 0, P1, P1, P1, None, P1, geom, 1 << 30, None, 0, img,
                                   1 << 30, None, None, None, None, P1, m2, P1, P1, None, P1, P1, None, scratch, scratch_bytes,
                                   None, opts, features, Cn, g_map, d_feat)
    return rc, L.cgs_last_error().decode()


def _densify_ex(n_vis=1, K=10, grad=P1, stride=4, col=2):
    from contextgs_amd import _lib
    L = _lib.lib()
    rc = L.cgs_densify_stats_ex(n_vis, K, P1, P1, P1, P1, P1, grad, P1, P1, P1, P1, None, stride, col)
    return rc, L.cgs_last_error().decode()


def test_new_symbols_resolve():
    from contextgs_amd import _lib
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n) and n in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["cgs_raster_backward_abs"][1]) == len(_lib.SIGNATURES["cgs_raster_backward_feat"][1])
    assert len(_lib.SIGNATURES["cgs_densify_stats_ex"][1]) == len(_lib.SIGNATURES["cgs_densify_stats"][1]) + 2


def test_abs_scratch_appends_the_accumulator_behind_the_aux_scratch():
    from contextgs_amd import _lib
    L = _lib.lib()
    for P in (0, 1, 1000, 1 << 20):
        aux, ab = L.cgs_raster_bwd_aux_scratch_bytes(P), L.cgs_raster_bwd_abs_scratch_bytes(P)
        assert ab >= aux + 8 * P and ab % 256 == 0 and aux % 256 == 0, (P, aux, ab)


def test_backward_abs_argument_errors():
    for kw in (dict(features=None), dict(d_feat=None)):
        rc, msg = _backward_abs(**kw)
        assert rc == CGS_ERR_ARG and "go together" in msg, (kw, msg)
    for Cn in (0, 33):
        rc, msg = _backward_abs(Cn=Cn)
        assert rc == CGS_ERR_ARG and "outside 1..32" in msg, (Cn, msg)
    for kw in (dict(geom=None), dict(img=None), dict(scratch=None), dict(m2=None)):
        rc, msg = _backward_abs(**kw)
        assert rc == CGS_ERR_ARG and "NULL" in msg and "cgs_raster_backward_abs" in msg, (kw, msg)
    rc, msg = _backward_abs(P=-1)
    assert rc == CGS_ERR_ARG and "P < 0" in msg
    from contextgs_amd import _lib
    L = _lib.lib()
    # a scratch that holds cgs_raster_backward_feat's layout but not the appended accumulator
    rc, msg = _backward_abs(P=1000, scratch_bytes=L.cgs_raster_bwd_aux_scratch_bytes(1000))
    assert rc == CGS_ERR_WORKSPACE and "scratch too small" in msg and "cgs_raster_backward_abs" in msg, msg
    for opts in (4, 2, 1 << 31):      # no new option bit: what cgs_raster_backward_opt does not know is unknown here too
        rc, msg = _backward_abs(opts=opts)
        assert rc == CGS_ERR_ARG and "cgs_raster_backward_abs" in msg and "unknown option bits" in msg, (opts, msg)
    rc, msg = _backward_abs(P=0, geom=None, img=None, scratch=None, m2=None)
    assert rc == CGS_OK, msg


def test_densify_stats_ex_argument_errors():
    rc, msg = _densify_ex(K=0)
    assert rc == CGS_ERR_ARG and "bad args" in msg
    rc, msg = _densify_ex(grad=None)
    assert rc == CGS_ERR_ARG and "NULL" in msg
    for stride, col in ((4, 3), (4, -1), (1, 0), (3, 2)):
        rc, msg = _densify_ex(stride=stride, col=col)
        assert rc == CGS_ERR_ARG and "outside rows" in msg, (stride, col, msg)
    rc, msg = _densify_ex(n_vis=0, grad=None)
    assert rc == CGS_OK, msg


def _rasterizer(sh_degree=1):
    from contextgs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    eye = torch.eye(4)
    rs = GaussianRasterizationSettings(16, 16, math.tan(0.5), math.tan(0.5), torch.zeros(3), 1.0, eye, eye, sh_degree,
                                       torch.zeros(3), False, False)
    return GaussianRasterizer(rs)


def test_absgrad_defaults_to_false():
    from contextgs_amd import renderer
    from contextgs_amd.rasterizer import GaussianRasterizer
    assert inspect.signature(GaussianRasterizer.forward).parameters["absgrad"].default is False
    p = inspect.signature(renderer.render).parameters["absgrad"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY


def _form(form, P=5):
    return dict(plain=dict(colors_precomp=torch.zeros(P, 3), scales=torch.zeros(P, 3), rotations=torch.zeros(P, 4)),
                shs=dict(shs=torch.zeros(P, 4, 3), scales=torch.zeros(P, 3), rotations=torch.zeros(P, 4)),
                shs_cov=dict(shs=torch.zeros(P, 4, 3), cov3D_precomp=torch.zeros(P, 6)),
                cov=dict(colors_precomp=torch.zeros(P, 3), cov3D_precomp=torch.zeros(P, 6)))[form]


FORMS = ["plain", "shs", "shs_cov", "cov"]


@pytest.mark.parametrize("form", FORMS)
def test_four_columns_without_the_keyword_raise_before_any_device(form):
    P = 5
    with pytest.raises(ValueError, match="absgrad=True, which was not given"):       # (CPU tensors: a device check would raise RuntimeError)
        _rasterizer()(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 4), opacities=torch.zeros(P, 1), **_form(form))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", [(5, 3), (5, 2), (5, 5), (4, 4), (5,), (5, 4, 1)])
def test_the_keyword_with_another_shape_raises_before_any_device(form, shape):
    P = 5
    with pytest.raises(ValueError, match=r"needs means2D \[P, 4\]"):
        _rasterizer()(means3D=torch.zeros(P, 3), means2D=torch.zeros(shape), opacities=torch.zeros(P, 1), absgrad=True,
                      **_form(form))


@pytest.mark.parametrize("form", FORMS)
def test_absgrad_has_no_cpu_path(form):
    P = 5
    with pytest.raises(RuntimeError, match="no CPU path"):
        _rasterizer()(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 4), opacities=torch.zeros(P, 1), absgrad=True,
                      **_form(form))


@pytest.mark.parametrize("cols", [5, 2, 1])
def test_training_statis_rejects_other_widths(cols):
    from contextgs_amd import densify
    P, K = 6, 2
    pc = types.SimpleNamespace(n_offsets=K)
    vp = types.SimpleNamespace(grad=torch.zeros(P, cols))
    with pytest.raises(ValueError, match=r"\[P,3\] or, from render\(absgrad=True\), \[P,4\]"):
        densify.training_statis(pc, vp, torch.zeros(3 * K, 1), torch.ones(P, dtype=torch.bool), torch.ones(3 * K, dtype=torch.bool),
                                torch.ones(3, dtype=torch.bool))
