"""The rasterizer's bit-reproducible backward without a GPU: the two C-ABI entry points exist and their argument errors come back
with their code and a message (nothing is launched); `check_deterministic` accepts the flag alone, refuses return_aux / features
/ contrib by name, is a no-op with the flag off and reads CGS_RASTER_DETERMINISTIC; the drop-in and render() take the keyword."""
import ctypes as C
import inspect

import pytest
import torch

from raster_harness import fake_cfg

CGS_OK = 0
CGS_ERR_ARG = 1
CGS_ERR_WORKSPACE = 3

NEW_SYMBOLS = ("cgs_raster_backward_det", "cgs_raster_bwd_det_bytes")
P1 = C.c_void_p(4096)      # a non-NULL stand-in: the checks only look at which pointers are given


def _backward_det(P=1, R=0, geom=P1, img=P1, scratch=P1, scratch_bytes=1 << 40, d_depth=None, d_invdepth=None, d_alpha=None,
                  opts=0, cols=3, det_ws=P1, det_bytes=1 << 40):
    """colours + scales / rotations, every other pointer given"""
    from contextgs_amd import _lib
    L = _lib.lib()
    rc = L.cgs_raster_backward_det(C.byref(fake_cfg()), P, R, P1, P1, None, 0, 0, P1, P1, P1, None, P1, geom, 1 << 30,
                                   P1 if R else None, 1 << 40 if R else 0, img, 1 << 30, None, d_depth, d_invdepth, d_alpha,
                                   P1, P1, P1, P1, None, P1, P1, None, scratch, scratch_bytes, None, opts, cols, det_ws, det_bytes)
    return rc, L.cgs_last_error().decode()


def test_new_symbols_resolve():
    from contextgs_amd import _lib
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n) and n in _lib.SIGNATURES
    # cgs_raster_backward_abs's arguments up to and including opts (four feature arguments fewer), then cols, det_ws, det_bytes
    assert len(_lib.SIGNATURES["cgs_raster_backward_det"][1]) == len(_lib.SIGNATURES["cgs_raster_backward_abs"][1]) - 4 + 3
    assert _lib.SIGNATURES["cgs_raster_backward_det"][1][:-3] == _lib.SIGNATURES["cgs_raster_backward_abs"][1][:-4]


def test_det_workspace_holds_base_and_48_bytes_per_pair():
    from contextgs_amd import _lib
    L = _lib.lib()
    for P, R in ((0, 0), (1, 0), (1000, 565), (1 << 20, 7 << 20)):
        for cols in (3, 4):
            n = L.cgs_raster_bwd_det_bytes(P, R, cols)
            assert n >= 4 * P + 48 * R and n % 256 == 0, (P, R, cols, n)
    # 64-bit sizes: 2^32 pairs are 192 GiB of slots
    assert L.cgs_raster_bwd_det_bytes(1 << 20, 1 << 32, 3) >= 48 << 32


def test_backward_det_argument_errors():
    for kw in (dict(d_depth=P1), dict(d_invdepth=P1), dict(d_alpha=P1)):
        rc, msg = _backward_det(**kw)
        assert rc == CGS_ERR_ARG and "must be NULL" in msg and "cgs_raster_backward_det" in msg, (kw, msg)
    for kw in (dict(geom=None), dict(img=None), dict(scratch=None), dict(det_ws=None)):
        rc, msg = _backward_det(**kw)
        assert rc == CGS_ERR_ARG and "NULL" in msg and "cgs_raster_backward_det" in msg, (kw, msg)
    for cols in (0, 2, 5):
        rc, msg = _backward_det(cols=cols)
        assert rc == CGS_ERR_ARG and "means2D_cols" in msg, (cols, msg)
    for opts in (4, 2, 1 << 31):
        rc, msg = _backward_det(opts=opts)
        assert rc == CGS_ERR_ARG and "unknown option bits" in msg, (opts, msg)
    rc, msg = _backward_det(P=-1)
    assert rc == CGS_ERR_ARG and "P < 0" in msg
    from contextgs_amd import _lib
    L = _lib.lib()
    rc, msg = _backward_det(P=1000, scratch_bytes=L.cgs_raster_bwd_aux_scratch_bytes(1000))
    assert rc == CGS_ERR_WORKSPACE and "scratch too small" in msg, msg
    for cols in (3, 4):
        rc, msg = _backward_det(P=1000, R=565, cols=cols, det_bytes=L.cgs_raster_bwd_det_bytes(1000, 565, cols) - 1)
        assert rc == CGS_ERR_WORKSPACE and "det_ws too small" in msg and "cgs_raster_backward_det" in msg, msg
    assert _backward_det(P=0)[0] == CGS_OK         # nothing to do, nothing enqueued


def test_check_deterministic_accepts_the_flag_alone(monkeypatch):
    from contextgs_amd.rasterizer import check_deterministic
    monkeypatch.delenv("CGS_RASTER_DETERMINISTIC", raising=False)
    assert check_deterministic(True) is True
    assert check_deterministic(True, False, None, None) is True
    assert check_deterministic(True, return_aux=False, features=None, contrib=False) is True
    assert check_deterministic(False) is False and check_deterministic(None) is False


@pytest.mark.parametrize("kw, name", [(dict(return_aux=True), "return_aux"), (dict(features=torch.zeros(3, 2)), "features"),
                                      (dict(contrib=True), "contrib")])
def test_check_deterministic_names_what_is_not_covered(monkeypatch, kw, name):
    from contextgs_amd.rasterizer import check_deterministic
    monkeypatch.delenv("CGS_RASTER_DETERMINISTIC", raising=False)
    with pytest.raises(ValueError, match=name):
        check_deterministic(True, **kw)
    assert check_deterministic(False, **kw) is False       # flag off: nothing is checked
    assert check_deterministic(None, **kw) is False
    monkeypatch.setenv("CGS_RASTER_DETERMINISTIC", "1")
    with pytest.raises(ValueError, match=name):
        check_deterministic(None, **kw)
    assert check_deterministic(False, **kw) is False       # an explicit False wins over the environment


def test_check_deterministic_reads_the_environment(monkeypatch):
    from contextgs_amd.rasterizer import check_deterministic
    monkeypatch.setenv("CGS_RASTER_DETERMINISTIC", "1")
    assert check_deterministic(None) is True and check_deterministic(False) is False
    monkeypatch.setenv("CGS_RASTER_DETERMINISTIC", "0")
    assert check_deterministic(None) is False and check_deterministic(True) is True


def test_keyword_surfaces():
    from contextgs_amd import renderer
    from contextgs_amd.rasterizer import GaussianRasterizer, RasterRequest
    assert inspect.signature(GaussianRasterizer.forward).parameters["deterministic"].default is None
    p = inspect.signature(renderer.render).parameters["deterministic"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert RasterRequest._field_defaults["deterministic"] is False
    assert inspect.signature(renderer.ViewFusion.__init__).parameters["deterministic"].default is False


def test_forward_refuses_before_a_device_is_touched():
    """CPU tensors: the ValueError of the flag's exclusions comes before any device check, with antialiasing and absgrad too."""
    import math
    from contextgs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    P = 4
    eye = torch.eye(4)
    for aa in (False, True):
        rs = GaussianRasterizationSettings(16, 16, math.tan(0.4), math.tan(0.4), torch.zeros(3), 1.0, eye, eye, 0, torch.zeros(3),
                                           False, False, antialiasing=aa)
        for absgrad in (False, True):
            args = dict(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 4 if absgrad else 3), opacities=torch.zeros(P, 1),
                        colors_precomp=torch.zeros(P, 3), scales=torch.ones(P, 3), rotations=torch.ones(P, 4), absgrad=absgrad)
            for kw, name in ((dict(return_aux=True), "return_aux"), (dict(features=torch.zeros(P, 2)), "features"),
                             (dict(contrib=True), "contrib")):
                with pytest.raises(ValueError, match=name):
                    GaussianRasterizer(rs)(deterministic=True, **args, **kw)
