"""The rasterizer's SH-colour and precomputed-covariance forms without a GPU: the C-ABI entry points exist, their argument
errors come back as CGS_ERR_ARG with a message (nothing is launched), and the drop-in's argument rules raise before any
device is touched."""
import ctypes as C
import math

import pytest
import torch

from raster_harness import fake_cfg

CGS_ERR_ARG = 1

NEW_SYMBOLS = ("cgs_raster_preprocess_launch_ex", "cgs_raster_backward_ex", "cgs_filter_cov")


def _launch_ex(cfg, P=1, colors=None, shs=None, D=0, M=0, scales=None, rotations=None, cov3D=None):
    from contextgs_amd import _lib
    L = _lib.lib()
    ticket = C.c_uint64(7)
    rc = L.cgs_raster_preprocess_launch_ex(C.byref(cfg), P, None, colors, shs, D, M, None, scales, rotations, cov3D, None, 0,
                                           None, None, C.byref(ticket))
    return rc, L.cgs_last_error().decode(), ticket.value


def _backward_ex(cfg, P=1, colors=None, shs=None, D=0, M=0, scales=None, rotations=None, cov3D=None):
    from contextgs_amd import _lib
    L = _lib.lib()
    rc = L.cgs_raster_backward_ex(C.byref(cfg), P, 0, None, colors, shs, D, M, None, scales, rotations, cov3D, None, None, 0,
                                  None, 0, None, 0, None, None, None, None, None, None, None, None, None, None, 0, None)
    return rc, L.cgs_last_error().decode()


def test_new_symbols_resolve():
    from contextgs_amd import _lib
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n) and n in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["cgs_raster_preprocess_launch_ex"][1]) == 16
    assert len(_lib.SIGNATURES["cgs_raster_backward_ex"][1]) == 31


P1 = C.c_void_p(4096)      # a non-NULL stand-in: the form checks only look at which pointers are given


@pytest.mark.parametrize("call", [_launch_ex, _backward_ex])
@pytest.mark.parametrize("kw, needle", [
    (dict(scales=P1, rotations=P1), "exactly one of either SHs or precomputed colors"),                      # neither colour
    (dict(colors=P1, shs=P1, M=1, scales=P1, rotations=P1), "exactly one of either SHs or precomputed colors"),
    (dict(colors=P1), "scale/rotation pair or precomputed 3D covariance"),                                   # no covariance
    (dict(colors=P1, scales=P1, rotations=P1, cov3D=P1), "scale/rotation pair or precomputed 3D covariance"),
    (dict(colors=P1, scales=P1), "scale/rotation pair or precomputed 3D covariance"),                         # half a pair
    (dict(colors=P1, rotations=P1, cov3D=P1), "scale/rotation pair or precomputed 3D covariance"),
    (dict(shs=P1, D=4, M=16, cov3D=P1), "sh_degree 4 outside 0..3"),
    (dict(shs=P1, D=-1, M=16, cov3D=P1), "sh_degree -1 outside 0..3"),
    (dict(shs=P1, D=2, M=8, cov3D=P1), "degree 2 needs 9..16"),
    (dict(shs=P1, D=0, M=17, cov3D=P1), "17 SH coefficients"),
])
def test_argument_errors_return_err_arg(call, kw, needle):
    out = call(fake_cfg(), **kw)
    assert out[0] == CGS_ERR_ARG, out
    assert needle in out[1], out[1]


def test_sh_without_campos_is_an_argument_error():
    rc, msg, _ = _launch_ex(fake_cfg(campos=False), shs=P1, D=1, M=4, scales=P1, rotations=P1)
    assert rc == CGS_ERR_ARG and "campos" in msg
    rc, msg = _backward_ex(fake_cfg(campos=False), shs=P1, D=1, M=4, scales=P1, rotations=P1)
    assert rc == CGS_ERR_ARG and "campos" in msg


def test_launch_ex_clears_the_ticket_on_an_argument_error():
    rc, _, ticket = _launch_ex(fake_cfg(), shs=P1, D=3, M=4, cov3D=P1)
    assert rc == CGS_ERR_ARG and ticket == 0


def test_filter_cov_argument_errors():
    from contextgs_amd import _lib
    L = _lib.lib()
    assert L.cgs_filter_cov(None, 10, None, None, None, None) == CGS_ERR_ARG
    assert b"cfg" in L.cgs_last_error()
    cfg = fake_cfg()
    assert L.cgs_filter_cov(C.byref(cfg), 10, P1, None, P1, None) == CGS_ERR_ARG
    assert b"NULL" in L.cgs_last_error()
    assert L.cgs_filter_cov(C.byref(cfg), -1, P1, P1, P1, None) == CGS_ERR_ARG


def _rasterizer(sh_degree=1):
    from contextgs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    eye = torch.eye(4)
    rs = GaussianRasterizationSettings(16, 16, math.tan(0.5), math.tan(0.5), torch.zeros(3), 1.0, eye, eye, sh_degree,
                                       torch.zeros(3), False, False)
    return GaussianRasterizer(rs)


@pytest.mark.parametrize("kw, needle", [
    (dict(scales=True, rotations=True), "SHs or precomputed colors"),
    (dict(shs=True, colors_precomp=True, scales=True, rotations=True), "SHs or precomputed colors"),
    (dict(colors_precomp=True), "scale/rotation pair"),
    (dict(colors_precomp=True, scales=True), "scale/rotation pair"),
    (dict(colors_precomp=True, scales=True, rotations=True, cov3D_precomp=True), "scale/rotation pair"),
])
def test_forward_raises_on_both_or_neither_form_before_any_device(kw, needle):
    P = 5
    shapes = dict(shs=(P, 4, 3), colors_precomp=(P, 3), scales=(P, 3), rotations=(P, 4), cov3D_precomp=(P, 6))
    args = {k: torch.zeros(shapes[k]) for k in kw}
    with pytest.raises(ValueError, match=needle):
        _rasterizer()(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.zeros(P, 1), **args)


@pytest.mark.parametrize("D, shape, needle", [
    (4, (5, 16, 3), "outside 0..3"),
    (2, (5, 4, 3), "needs 9..16"),
    (0, (5, 17, 3), "needs 1..16"),
    (1, (5, 12), r"\[P, M, 3\]"),
])
def test_forward_checks_the_sh_shape_before_any_device(D, shape, needle):
    P = 5
    with pytest.raises(ValueError, match=needle):
        _rasterizer(D)(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.zeros(P, 1),
                       shs=torch.zeros(shape), cov3D_precomp=torch.zeros(P, 6))


def test_valid_new_forms_reach_the_device_check():
    """A valid shs / cov3D_precomp call on CPU tensors gets past the argument rules and stops at the device check:
    no CPU fallback."""
    P = 5
    with pytest.raises(RuntimeError, match="no CPU path"):
        _rasterizer(1)(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.zeros(P, 1),
                       shs=torch.zeros(P, 4, 3), cov3D_precomp=torch.zeros(P, 6))


def test_visible_filter_argument_rules():
    P = 5
    r = _rasterizer()
    with pytest.raises(ValueError, match="scale/rotation pair"):
        r.visible_filter(torch.zeros(P, 3))
    with pytest.raises(ValueError, match="scale/rotation pair"):
        r.visible_filter(torch.zeros(P, 3), torch.zeros(P, 3), torch.zeros(P, 4), torch.zeros(P, 6))
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.visible_filter(torch.zeros(P, 3), cov3D_precomp=torch.zeros(P, 6))
