"""Camera gradients without a GPU: the argument rules of cgs_raster_camera_backward (CGS_ERR_ARG with a message, nothing
launched) and the torch pose helper (contextgs_amd/camera_pose.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from contextgs_amd.synth import look_at_camera
from raster_harness import fake_cfg

CGS_ERR_ARG = 1
CGS_RASTER_ANTIALIAS = 1
CGS_RASTER_CAMERA_MAPS = 2
P1 = C.c_void_p(4096)      # a non-NULL stand-in: the checks only look at which pointers are given
BIG = 1 << 40


def _camera(opts=0, P=1, means3D=P1, shs=None, D=0, M=0, opac=None, scales=P1, rotations=P1, cov3D=None, radii=P1, scratch=P1,
            scratch_bytes=BIG, d_colors=None, d_opac=None, d_view=P1, d_proj=P1, d_campos=None, work=P1, work_bytes=BIG, cfg=None):
    from contextgs_amd import _lib
    L = _lib.lib()
    rc = L.cgs_raster_camera_backward(C.byref(cfg or fake_cfg()), P, means3D, shs, D, M, opac, scales, rotations, cov3D, radii,
                                      scratch, scratch_bytes, d_colors, d_opac, opts, d_view, d_proj, d_campos, work, work_bytes, None)
    return rc, L.cgs_last_error().decode()


def test_new_symbols_resolve():
    from contextgs_amd import _lib
    L = _lib.lib()
    for n in ("cgs_raster_camera_bytes", "cgs_raster_camera_backward"):
        assert hasattr(L, n) and n in _lib.SIGNATURES
    assert L.cgs_raster_camera_bytes(0) > 0
    assert L.cgs_raster_camera_bytes(6_000_000) < (1 << 20)      # per-workgroup rows, not per-Gaussian


@pytest.mark.parametrize("opts", [4, 8, 0x80000000, 7, 0xFFFFFFFF])
def test_unknown_option_bits_are_refused(opts):
    rc, msg = _camera(opts, opac=P1, d_opac=P1)
    assert rc == CGS_ERR_ARG and "unknown option bits" in msg and "cgs_raster_camera_backward" in msg, msg


@pytest.mark.parametrize("kw, needle", [
    (dict(d_view=None, d_proj=None), "no output given"),
    (dict(d_campos=P1), "dL_dcampos needs shs"),
    (dict(d_campos=P1, shs=P1, D=1, M=4, d_colors=P1, cfg="nocampos"), "dL_dcampos needs shs and cfg->campos"),
    (dict(d_campos=P1, shs=P1, D=4, M=16, d_colors=P1), "sh_degree 4 outside 0..3"),
    (dict(d_campos=P1, shs=P1, D=2, M=8, d_colors=P1), "degree 2 needs 9..16"),
    (dict(d_campos=P1, shs=P1, D=1, M=4), "NULL input"),                  # the SH term reads dL_dcolors
    (dict(work=None), "work missing or too small"),
    (dict(work_bytes=64), "work missing or too small"),
    (dict(scales=None, rotations=None), "scale/rotation pair or precomputed 3D covariance"),
    (dict(cov3D=P1), "scale/rotation pair or precomputed 3D covariance"),
    (dict(rotations=None), "scale/rotation pair or precomputed 3D covariance"),
    (dict(means3D=None), "NULL input"),
    (dict(radii=None), "NULL input"),
    (dict(scratch=None), "NULL input"),
    (dict(scratch_bytes=8), "scratch too small"),
    (dict(opts=CGS_RASTER_ANTIALIAS), "NULL input"),                        # antialiasing reads opacities and dL_dopacities
    (dict(opts=CGS_RASTER_ANTIALIAS, opac=P1), "NULL input"),
    (dict(opts=CGS_RASTER_ANTIALIAS, d_opac=P1), "NULL input"),
    (dict(P=-1), "P out of range"),
])
def test_argument_errors(kw, needle):
    kw = dict(kw)
    if kw.get("cfg") == "nocampos":
        kw["cfg"] = fake_cfg(campos=False)
    rc, msg = _camera(**kw)
    assert rc == CGS_ERR_ARG and needle in msg, msg
    assert "cgs_raster_camera_backward" in msg


def test_maps_option_asks_for_the_larger_scratch():
    from contextgs_amd import _lib
    L = _lib.lib()
    P = 1000
    plain, aux = L.cgs_raster_bwd_scratch_bytes(P), L.cgs_raster_bwd_aux_scratch_bytes(P)
    assert aux > plain
    rc, msg = _camera(CGS_RASTER_CAMERA_MAPS, P=P, scratch_bytes=plain)
    assert rc == CGS_ERR_ARG and "scratch too small" in msg, msg
    rc, msg = _camera(0, P=P, scratch_bytes=plain - 1)
    assert rc == CGS_ERR_ARG and "scratch too small" in msg, msg


def test_camera_tensors_are_inputs_of_the_node_and_cpu_tensors_are_refused():
    import math
    from contextgs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    V = torch.eye(4, requires_grad=True)
    rs = GaussianRasterizationSettings(16, 16, math.tan(0.5), math.tan(0.5), torch.zeros(3), 1.0, V, torch.eye(4), 1,
                                       torch.zeros(3), False, False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        GaussianRasterizer(rs)(means3D=torch.zeros(5, 3), means2D=torch.zeros(5, 3), opacities=torch.zeros(5, 1),
                               colors_precomp=torch.zeros(5, 3), scales=torch.zeros(5, 3), rotations=torch.zeros(5, 4))


# ---- the pose helper ---------------------------------------------------------------------------------------------------
def _cam():
    return look_at_camera((0.7, -3.0, 0.4), (0.1, 0, 0), 64, 48, fovx_deg=50.0).to_torch("cpu")


def test_trainable_camera_at_zero_is_the_wrapped_camera():
    from contextgs_amd.camera_pose import TrainableCamera
    cam = _cam()
    cam.uid = 17
    tc = TrainableCamera(cam)
    assert list(n for n, _ in tc.named_parameters()) == ["xi"] and tc.xi.shape == (6,) and not tc.xi.any()
    assert (tc.image_height, tc.image_width, tc.FoVx, tc.FoVy) == (cam.image_height, cam.image_width, cam.FoVx, cam.FoVy)
    assert tc.uid == 17                                     # everything else reads through
    V, PM, c = tc.world_view_transform, tc.full_proj_transform, tc.camera_center
    assert V.dtype == PM.dtype == c.dtype == torch.float32 and V.requires_grad and PM.requires_grad and c.requires_grad
    eps = float(np.finfo(np.float32).eps)
    for got, want in ((V, cam.world_view_transform), (PM, cam.full_proj_transform), (c, cam.camera_center)):
        assert (got - want).abs().max() <= eps * want.abs().max(), (got, want)


@pytest.mark.parametrize("w", [(0.0, 0.0, 0.0), (1e-6, -2e-6, 3e-7), (0.02, -0.01, 0.015), (1.2, -0.7, 2.1), (3.0, 0.5, -0.2)])
def test_exp_is_a_rotation(w):
    from contextgs_amd.camera_pose import se3_exp, so3_exp
    w = torch.tensor(w, dtype=torch.float64)
    R = so3_exp(w)
    assert (R.T @ R - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-14
    assert abs(float(torch.linalg.det(R)) - 1.0) < 1e-14
    assert (R @ w - w).abs().max() < 1e-14                  # the axis stays
    th = float(w.norm())
    assert abs(float(torch.trace(R)) - (1 + 2 * np.cos(th))) < 1e-13
    E = se3_exp(torch.cat([w, torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64)]))
    assert torch.equal(E[:3, :3], R.T) and torch.equal(E[:, 3], torch.tensor([0, 0, 0, 1], dtype=torch.float64))
    assert torch.equal(E[3, :3], torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64))


def test_pose_tensors_are_consistent():
    """V P = PM and inv(V)[3, :3] = camera_center away from xi = 0, to the fp32 rounding the wrapped camera's PM0 and centre
    were stored with."""
    from contextgs_amd.camera_pose import TrainableCamera, pose_tensors
    tc = TrainableCamera(_cam(), dtype=torch.float64)
    xi = torch.tensor([0.03, -0.02, 0.05, 0.1, -0.04, 0.07], dtype=torch.float64)
    V, PM, c = pose_tensors(xi, tc.V0, tc.P, tc.V0_inv, tc.PM0, tc.c0)
    eps = float(np.finfo(np.float32).eps)
    assert (PM - V @ tc.P).abs().max() <= eps * PM.abs().max()
    assert (torch.linalg.inv(V)[3, :3] - c).abs().max() <= eps * c.abs().max()
    assert (V[:, 3] - torch.tensor([0, 0, 0, 1.0], dtype=torch.float64)).abs().max() < 1e-15


@pytest.mark.parametrize("xi0", [(0.0,) * 6, (1e-5, 0, 0, 0, 0, 0), (0.03, -0.02, 0.05, 0.1, -0.04, 0.07)])
def test_pose_autograd_against_gradcheck(xi0):
    from contextgs_amd.camera_pose import TrainableCamera, pose_tensors
    tc = TrainableCamera(_cam(), dtype=torch.float64)
    xi = torch.tensor(xi0, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x: pose_tensors(x, tc.V0, tc.P, tc.V0_inv, tc.PM0, tc.c0), (xi,), eps=1e-6, atol=1e-7, rtol=1e-6)


def test_render_sends_a_trainable_camera_down_the_unfused_path():
    from contextgs_amd import renderer
    from contextgs_amd.camera_pose import TrainableCamera
    tc = TrainableCamera(_cam())
    d = renderer._DetachedCamera(tc)
    assert not d.world_view_transform.requires_grad and not d.full_proj_transform.requires_grad
    assert not d.camera_center.requires_grad and d.image_height == 48 and d.FoVx == tc.FoVx
    assert torch.equal(d.camera_center, tc.camera_center.detach())
