"""GPU parity of the rasterizer's SH-colour and precomputed-covariance forms against the project's own
colors_precomp + scales/rotations form, with torch restating the part the new kernels take over:

  shs            vs  colors_precomp = sh_eval_torch(shs, means3D, campos, D)   (autograd through the torch SH)
  cov3D_precomp  vs  scales + rotations, cov6 = strip_symmetric(L L^T) built in torch from scale_modifier * s and q

Tolerances as tests/test_raster_gpu.py: gradients 2e-4 of each tensor's max magnitude, images by RMSE plus a max-abs
allowance on a 1e-4 fraction of the values.
"""
import math

import numpy as np
import pytest
import torch

from contextgs_amd.synth import look_at_camera, random_gaussians

pytestmark = pytest.mark.gpu

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435)

CASES = [(1, 64, 48), (64, 128, 96), (4000, 256, 256), (30000, 800, 800), (200000, 1920, 1080)]


def sh_eval_unclamped(shs, means3D, campos, D):
    d = means3D - campos[None, :]
    d = d / d.norm(dim=1, keepdim=True)
    x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    s = shs
    r = C0 * s[:, 0]
    if D > 0:
        r = r - C1 * y * s[:, 1] + C1 * z * s[:, 2] - C1 * x * s[:, 3]
        if D > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            r = r + C2[0] * xy * s[:, 4] + C2[1] * yz * s[:, 5] + C2[2] * (2 * zz - xx - yy) * s[:, 6] + \
                C2[3] * xz * s[:, 7] + C2[4] * (xx - yy) * s[:, 8]
            if D > 2:
                r = r + C3[0] * y * (3 * xx - yy) * s[:, 9] + C3[1] * xy * z * s[:, 10] + \
                    C3[2] * y * (4 * zz - xx - yy) * s[:, 11] + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * s[:, 12] + \
                    C3[4] * x * (4 * zz - xx - yy) * s[:, 13] + C3[5] * z * (xx - yy) * s[:, 14] + \
                    C3[6] * x * (xx - 3 * yy) * s[:, 15]
    return r + 0.5


def sh_eval_torch(shs, means3D, campos, D):
    """The colour the SH form evaluates: standard 3DGS SH of degree D, + 0.5, clamped at 0 per channel."""
    return torch.clamp_min(sh_eval_unclamped(shs, means3D, campos, D), 0.0)


def quat_to_rot(q):
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]      # used as given, like the kernels
    return torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)


def cov6_torch(scales, rotations, scale_modifier):
    L = quat_to_rot(rotations) * (scale_modifier * scales)[:, None, :]
    S = L @ L.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=1)


def _scene(P, W, H, seed):
    cam = look_at_camera((0.4, -2.2, 0.6), (0, 0, 0), W, H, fovx_deg=60.0)
    g = random_gaussians(P, seed=seed, extent=1.0)
    if P >= 20:     # some Gaussians behind the near plane: every 20th moved behind the camera
        eye = np.array([0.4, -2.2, 0.6], dtype=np.float32)
        g["means3D"][::20] = eye + 0.3 * (eye - g["means3D"][::20])
    return cam, g


def _settings(cam, D=1, scale_modifier=1.0, debug=False):
    from contextgs_amd.rasterizer import GaussianRasterizationSettings
    c = cam.to_torch("cuda")
    return GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width,
        tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
        bg=torch.tensor((0.1, 0.2, 0.3), dtype=torch.float32, device="cuda"), scale_modifier=scale_modifier,
        viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform, sh_degree=D,
        campos=c.camera_center, prefiltered=False, debug=debug)


def _shs(P, M, seed, clamp_dc=True):
    rng = np.random.default_rng(seed + 1000)
    sh = rng.normal(0.0, 0.25, size=(P, M, 3)).astype(np.float32)
    if clamp_dc:     # DC terms so that a good share of channels clamp: C0 * sh0 + 0.5 in [-0.5, 1.0]
        sh[:, 0, :] = (rng.uniform(-1.0, 0.5, size=(P, 3)) / C0).astype(np.float32)
    return sh


def _leaf(a):
    return torch.tensor(a, device="cuda", requires_grad=True)


def _render(rs, w, **kw):
    from contextgs_amd.rasterizer import GaussianRasterizer
    P = kw["means3D"].shape[0]
    means2D = torch.zeros(P, 3, device="cuda", requires_grad=True)
    color, radii = GaussianRasterizer(rs)(means2D=means2D, **kw)
    (color * w).sum().backward()
    torch.cuda.synchronize()
    return color.detach(), radii, means2D.grad


def _close(a, b, what, tol=2e-4, rows=None, allow_frac=0.0):
    """max |a - b| <= tol * max |b|, on every row but at most allow_frac of them (the covariance form's conic differs from
    the scale/rotation form's in the last ulp, which can flip an alpha >= 1/255 decision on a pixel: the same allowance as
    for its radii)."""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    if rows is not None:
        a, b = a[rows], b[rows]
    if not a.numel():
        return
    scale = max(float(b.abs().max()), 1e-12)
    row_err = (a - b).abs().reshape(a.shape[0], -1).amax(dim=1) / scale
    n_bad = int((row_err > tol).sum())
    print(f"[allowance] {what}: {n_bad} of {a.shape[0]} rows beyond {tol:g}, max {float(row_err.max()):.2e}")
    assert n_bad <= int(allow_frac * a.shape[0]), (what, n_bad, float(row_err.max()))


def _check_image(a, b, rmse_max, what="image"):
    d = (a - b).abs().cpu().numpy()
    rmse = float(np.sqrt((d ** 2).mean()))
    assert rmse <= rmse_max, (what, rmse)
    frac = float((d > 2e-5).sum()) / d.size
    assert frac <= 1e-4, (what, frac, d.max())
    assert d.max() <= 1.0 / 255 + 1e-4, (what, d.max())


def _weights(H, W, seed):
    return torch.tensor(np.random.default_rng(seed).normal(size=(3, H, W)).astype(np.float32), device="cuda")


@pytest.mark.parametrize("P, W, H", CASES)
@pytest.mark.parametrize("D, M", [(0, 1), (1, 4), (2, 9), (3, 16), (1, 16)])
def test_sh_matches_torch_sh_through_colors_precomp(P, W, H, D, M):
    cam, g = _scene(P, W, H, seed=P + D)
    sh = _shs(P, M, seed=P + M)
    w = _weights(H, W, seed=1)
    rs = _settings(cam, D=D)
    campos = rs.campos.float()

    ref = {k: _leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations")}
    ref_sh = _leaf(sh)
    colors = sh_eval_torch(ref_sh, ref["means3D"], campos, D)
    c_ref, r_ref, m2_ref = _render(rs, w, means3D=ref["means3D"], opacities=ref["opacities"], colors_precomp=colors,
                                   scales=ref["scales"], rotations=ref["rotations"])

    new = {k: _leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations")}
    new_sh = _leaf(sh)
    c_new, r_new, m2_new = _render(rs, w, means3D=new["means3D"], opacities=new["opacities"], shs=new_sh,
                                   scales=new["scales"], rotations=new["rotations"])

    assert torch.equal(r_ref, r_new)
    _check_image(c_new, c_ref, 1e-6)
    vis = (r_new > 0).cpu()
    _close(new_sh.grad, ref_sh.grad, "dL/dshs")
    _close(new["means3D"].grad, ref["means3D"].grad, "dL/dmeans3D")
    _close(m2_new, m2_ref, "dL/dmeans2D")
    for k in ("opacities", "scales", "rotations"):
        _close(new[k].grad, ref[k].grad, f"dL/d{k}")
    gsh = new_sh.grad.cpu()
    K = (D + 1) ** 2
    assert torch.all(gsh[:, K:] == 0)                    # coefficients above the active degree: exactly 0
    assert torch.all(gsh[~vis] == 0)                     # culled Gaussians: exactly 0
    if P >= 4000:
        with torch.no_grad():
            raw = sh_eval_unclamped(ref_sh, ref["means3D"], campos, D)[vis.cuda()]
        assert float((raw < 0).float().mean()) >= 0.2    # the clamp is exercised


@pytest.mark.parametrize("P, W, H", CASES)
@pytest.mark.parametrize("scale_modifier", [1.0, 0.7])
def test_cov3d_precomp_matches_scales_rotations(P, W, H, scale_modifier):
    cam, g = _scene(P, W, H, seed=P + 7)
    w = _weights(H, W, seed=2)

    ref = {k: _leaf(g[k]) for k in g}
    c_ref, r_ref, m2_ref = _render(_settings(cam, scale_modifier=scale_modifier), w, means3D=ref["means3D"],
                                   opacities=ref["opacities"], colors_precomp=ref["colors"], scales=ref["scales"],
                                   rotations=ref["rotations"])

    new = {k: _leaf(g[k]) for k in g}
    cov6 = cov6_torch(new["scales"], new["rotations"], scale_modifier)
    c_new, r_new, m2_new = _render(_settings(cam, scale_modifier=1.0), w, means3D=new["means3D"],
                                   opacities=new["opacities"], colors_precomp=new["colors"], cov3D_precomp=cov6)

    same = (r_ref == r_new).cpu()
    assert float(same.float().mean()) >= 1 - 1e-4
    _check_image(c_new, c_ref, 1e-5)
    for k in ("scales", "rotations", "means3D", "opacities", "colors"):
        _close(new[k].grad, ref[k].grad, f"dL/d{k}", rows=same, allow_frac=1e-4)
    _close(m2_new, m2_ref, "dL/dmeans2D", rows=same, allow_frac=1e-4)


@pytest.mark.parametrize("P, W, H", CASES[2:4])
def test_sh_and_cov3d_precomp_together(P, W, H):
    D, M = 3, 16
    cam, g = _scene(P, W, H, seed=P + 11)
    sh = _shs(P, M, seed=P)
    w = _weights(H, W, seed=3)
    rs = _settings(cam, D=D)
    campos = rs.campos.float()

    ref = {k: _leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations")}
    ref_sh = _leaf(sh)
    c_ref, r_ref, _ = _render(rs, w, means3D=ref["means3D"], opacities=ref["opacities"],
                              colors_precomp=sh_eval_torch(ref_sh, ref["means3D"], campos, D), scales=ref["scales"],
                              rotations=ref["rotations"])
    new = {k: _leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations")}
    new_sh = _leaf(sh)
    c_new, r_new, _ = _render(rs, w, means3D=new["means3D"], opacities=new["opacities"], shs=new_sh,
                              cov3D_precomp=cov6_torch(new["scales"], new["rotations"], 1.0))
    same = (r_ref == r_new).cpu()
    assert float(same.float().mean()) >= 1 - 1e-4
    _check_image(c_new, c_ref, 1e-5)
    _close(new_sh.grad, ref_sh.grad, "dL/dshs", rows=same, allow_frac=1e-4)
    for k in ("means3D", "opacities", "scales", "rotations"):
        _close(new[k].grad, ref[k].grad, f"dL/d{k}", rows=same, allow_frac=1e-4)


@pytest.mark.parametrize("P, W, H", CASES)
def test_visible_filter_with_cov3d_precomp(P, W, H):
    from contextgs_amd.rasterizer import GaussianRasterizer
    cam, g = _scene(P, W, H, seed=P + 5)
    rast = GaussianRasterizer(_settings(cam, scale_modifier=0.8))
    t = {k: torch.tensor(v, device="cuda") for k, v in g.items()}
    r_ref = rast.visible_filter(t["means3D"], t["scales"], t["rotations"])
    r_new = rast.visible_filter(t["means3D"], cov3D_precomp=cov6_torch(t["scales"], t["rotations"], 0.8))
    assert r_new.dtype == torch.int32 and r_new.shape == (P,)
    assert float((r_ref == r_new).float().mean()) >= 1 - 1e-4


@pytest.mark.parametrize("form", ["shs", "cov", "both"])
def test_each_form_is_bitwise_stable(form):
    from contextgs_amd.rasterizer import GaussianRasterizer
    P, W, H = 30000, 800, 600
    cam, g = _scene(P, W, H, seed=9)
    rs = _settings(cam, D=3, debug=True)
    t = {k: torch.tensor(v, device="cuda") for k, v in g.items()}
    kw = dict(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"])
    if form in ("shs", "both"):
        kw["shs"] = torch.tensor(_shs(P, 16, seed=9), device="cuda")
    else:
        kw["colors_precomp"] = t["colors"]
    if form in ("cov", "both"):
        kw["cov3D_precomp"] = cov6_torch(t["scales"], t["rotations"], 1.0)
    else:
        kw.update(scales=t["scales"], rotations=t["rotations"])
    a, ra = GaussianRasterizer(rs)(**kw)
    b, rb = GaussianRasterizer(rs)(**kw)
    assert torch.equal(a, b) and torch.equal(ra, rb)


@pytest.mark.parametrize("form", ["shs", "cov", "both"])
def test_empty_input_every_form(form):
    from contextgs_amd.rasterizer import GaussianRasterizer
    cam = look_at_camera((0.4, -2.2, 0.6), (0, 0, 0), 64, 48)
    rs = _settings(cam, D=2)
    z = lambda *s: torch.zeros(*s, device="cuda", requires_grad=True)
    kw = dict(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1))
    if form in ("shs", "both"):
        kw["shs"] = z(0, 9, 3)
    else:
        kw["colors_precomp"] = z(0, 3)
    if form in ("cov", "both"):
        kw["cov3D_precomp"] = z(0, 6)
    else:
        kw.update(scales=z(0, 3), rotations=z(0, 4))
    color, radii = GaussianRasterizer(rs)(**kw)
    color.sum().backward()
    torch.cuda.synchronize()
    assert radii.shape == (0,)
    bg = torch.tensor((0.1, 0.2, 0.3), device="cuda")[:, None, None].expand(3, 48, 64)
    assert torch.allclose(color.detach(), bg)
    rast = GaussianRasterizer(rs)
    assert rast.visible_filter(kw["means3D"].detach(), cov3D_precomp=torch.zeros(0, 6, device="cuda")).shape == (0,)
