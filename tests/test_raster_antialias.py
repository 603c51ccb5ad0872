"""The rasterizer's antialiasing without a GPU: the settings field, the C-ABI entry points with an options word and their
argument errors (CGS_ERR_ARG with a message, nothing launched), and the refusal of CPU tensors."""
import ctypes as C
import math

import pytest
import torch

from raster_harness import fake_cfg

CGS_ERR_ARG = 1
CGS_RASTER_ANTIALIAS = 1
P1 = C.c_void_p(4096)      # a non-NULL stand-in: the checks only look at which pointers are given


def _launch_opt(opts, P=1, colors=P1, shs=None, D=0, M=0, scales=P1, rotations=P1, cov3D=None, cfg=None):
    from contextgs_amd import _lib
    L = _lib.lib()
    ticket = C.c_uint64(7)
    rc = L.cgs_raster_preprocess_launch_opt(C.byref(cfg or fake_cfg()), P, P1, colors, shs, D, M, P1, scales, rotations, cov3D, P1,
                                            1 << 30, P1, None, C.byref(ticket), opts)
    return rc, L.cgs_last_error().decode(), ticket.value


def _backward_opt(opts, P=1, colors=P1, shs=None, D=0, M=0, scales=P1, rotations=P1, cov3D=None, opac=P1, outs=None):
    from contextgs_amd import _lib
    L = _lib.lib()
    o = dict(means3D=P1, means2D=P1, colors=P1, opac=P1, shs=None, scales=P1, rots=P1, cov=None)
    o.update(outs or {})
    rc = L.cgs_raster_backward_opt(C.byref(fake_cfg()), P, 0, P1, colors, shs, D, M, opac, scales, rotations, cov3D, P1, P1,
                                   1 << 30, None, 0, P1, 1 << 30, P1, None, None, None, o["means3D"], o["means2D"], o["colors"],
                                   o["opac"], o["shs"], o["scales"], o["rots"], o["cov"], P1, 1 << 40, None, opts)
    return rc, L.cgs_last_error().decode()


def _settings(**kw):
    from contextgs_amd.rasterizer import GaussianRasterizationSettings
    eye = torch.eye(4)
    return GaussianRasterizationSettings(16, 16, math.tan(0.5), math.tan(0.5), torch.zeros(3), 1.0, eye, eye, 1, torch.zeros(3),
                                         False, False, **kw)


def test_antialiasing_is_the_last_argument_and_off_by_default():
    from contextgs_amd.rasterizer import GaussianRasterizationSettings
    assert _settings().antialiasing is False
    assert _settings(antialiasing=True).antialiasing is True
    eye = torch.eye(4)
    rs = GaussianRasterizationSettings(16, 16, 0.5, 0.5, torch.zeros(3), 1.0, eye, eye, 1, torch.zeros(3), False, False, True)
    assert rs.antialiasing is True                                       # upstream's position: after debug
    assert rs._fields[-1] == "debug" and len(rs) == 12                  # the twelve-field tuple stays as it was
    assert rs._replace(debug=True).antialiasing is True
    assert rs._replace(antialiasing=False).antialiasing is False
    assert "antialiasing=True" in repr(rs)
    with pytest.raises(TypeError):
        GaussianRasterizationSettings(16, 16, 0.5, 0.5)


def test_new_symbols_resolve():
    from contextgs_amd import _lib
    L = _lib.lib()
    for n in ("cgs_raster_preprocess_launch_opt", "cgs_raster_backward_opt"):
        assert hasattr(L, n) and n in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["cgs_raster_preprocess_launch_opt"][1]) == \
        len(_lib.SIGNATURES["cgs_raster_preprocess_launch_ex"][1]) + 1
    assert len(_lib.SIGNATURES["cgs_raster_backward_opt"][1]) == len(_lib.SIGNATURES["cgs_raster_backward_aux"][1]) + 1


@pytest.mark.parametrize("opts", [2, 4, 0x80000000, 3, 0xFFFFFFFF])
def test_unknown_option_bits_are_refused(opts):
    rc, msg, ticket = _launch_opt(opts)
    assert rc == CGS_ERR_ARG and "unknown option bits" in msg, msg
    assert ticket == 0
    rc, msg = _backward_opt(opts)
    assert rc == CGS_ERR_ARG and "unknown option bits" in msg, msg


@pytest.mark.parametrize("opts", [0, CGS_RASTER_ANTIALIAS])
@pytest.mark.parametrize("kw, needle", [
    (dict(colors=None), "exactly one of either SHs or precomputed colors"),
    (dict(shs=P1, M=1), "exactly one of either SHs or precomputed colors"),
    (dict(scales=None, rotations=None), "scale/rotation pair or precomputed 3D covariance"),
    (dict(cov3D=P1), "scale/rotation pair or precomputed 3D covariance"),
    (dict(colors=None, shs=P1, D=4, M=16), "sh_degree 4 outside 0..3"),
    (dict(colors=None, shs=P1, D=2, M=8), "degree 2 needs 9..16"),
])
def test_bad_forms(opts, kw, needle):
    rc, msg, _ = _launch_opt(opts, **kw)
    assert rc == CGS_ERR_ARG and needle in msg, msg
    assert "cgs_raster_preprocess_launch_opt" in msg
    rc, msg = _backward_opt(opts, **kw)
    assert rc == CGS_ERR_ARG and needle in msg, msg
    assert "cgs_raster_backward_opt" in msg


@pytest.mark.parametrize("kw", [dict(opac=None), dict(outs=dict(opac=None)), dict(outs=dict(means3D=None)),
                                dict(outs=dict(scales=None)), dict(outs=dict(colors=None))])
def test_backward_null_outputs(kw):
    rc, msg = _backward_opt(CGS_RASTER_ANTIALIAS, **kw)
    assert rc == CGS_ERR_ARG and "NULL input" in msg, msg


def test_backward_without_antialiasing_does_not_need_opacities():
    # opts == 0 is cgs_raster_backward_aux, which never reads opacities: only the missing dL_dscales is reported
    rc, msg = _backward_opt(0, opac=None, outs=dict(scales=None))
    assert rc == CGS_ERR_ARG and "NULL input" in msg


def test_sh_without_campos():
    rc, msg, _ = _launch_opt(CGS_RASTER_ANTIALIAS, colors=None, shs=P1, D=1, M=4, cfg=fake_cfg(campos=False))
    assert rc == CGS_ERR_ARG and "campos" in msg


@pytest.mark.parametrize("return_aux", [False, True])
@pytest.mark.parametrize("form", ["plain", "shs", "cov"])
def test_antialiasing_has_no_cpu_path(form, return_aux):
    from contextgs_amd.rasterizer import GaussianRasterizer
    P = 5
    args = dict(plain=dict(colors_precomp=torch.zeros(P, 3), scales=torch.zeros(P, 3), rotations=torch.zeros(P, 4)),
                shs=dict(shs=torch.zeros(P, 4, 3), scales=torch.zeros(P, 3), rotations=torch.zeros(P, 4)),
                cov=dict(colors_precomp=torch.zeros(P, 3), cov3D_precomp=torch.zeros(P, 6)))[form]
    with pytest.raises(RuntimeError, match="no CPU path"):
        GaussianRasterizer(_settings(antialiasing=True))(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3),
                                                         opacities=torch.zeros(P, 1), return_aux=return_aux, **args)


def test_form_errors_come_first_with_antialiasing():
    from contextgs_amd.rasterizer import GaussianRasterizer
    with pytest.raises(ValueError, match="SHs or precomputed colors"):
        GaussianRasterizer(_settings(antialiasing=True))(means3D=torch.zeros(5, 3), means2D=torch.zeros(5, 3),
                                                         opacities=torch.zeros(5, 1), scales=torch.zeros(5, 3),
                                                         rotations=torch.zeros(5, 4))


def test_renderer_reads_pipe_antialiasing():
    from contextgs_amd.renderer import _raster_settings
    from contextgs_amd.synth import SynthPipe

    class Cam:
        image_height, image_width, FoVx, FoVy = 16, 16, 1.0, 1.0
        world_view_transform = full_proj_transform = torch.eye(4)
        camera_center = torch.zeros(3)

    class AAPipe(SynthPipe):
        antialiasing = True

    assert _raster_settings(Cam, SynthPipe(), torch.zeros(3), 1.0).antialiasing is False
    assert _raster_settings(Cam, AAPipe(), torch.zeros(3), 1.0).antialiasing is True
