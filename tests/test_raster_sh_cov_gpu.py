"""GPU parity of the rasterizer's SH-colour and precomputed-covariance forms against the project's own
colors_precomp + scales/rotations form, with torch restating the part the new kernels take over:

  shs            vs  colors_precomp = sh_eval_torch(shs, means3D, campos, D)   (autograd through the torch SH)
  cov3D_precomp  vs  scales + rotations, cov6 = strip_symmetric(L L^T) built in torch from scale_modifier * s and q

Tolerances as tests/test_raster_gpu.py: gradients 2e-4 of each tensor's max magnitude, images by RMSE plus a max-abs
allowance on a 1e-4 fraction of the values.
"""
import numpy as np
import pytest
import torch

from contextgs_amd.synth import look_at_camera
from raster_harness import check_image, close, cov6_torch, leaf, scene, settings, sh_eval_torch, sh_eval_unclamped, shs

pytestmark = pytest.mark.gpu

CASES = [(1, 64, 48), (64, 128, 96), (4000, 256, 256), (30000, 800, 800), (200000, 1920, 1080)]


def _render(rs, w, **kw):
    from contextgs_amd.rasterizer import GaussianRasterizer
    P = kw["means3D"].shape[0]
    means2D = torch.zeros(P, 3, device="cuda", requires_grad=True)
    color, radii = GaussianRasterizer(rs)(means2D=means2D, **kw)
    (color * w).sum().backward()
    torch.cuda.synchronize()
    return color.detach(), radii, means2D.grad


def _weights(H, W, seed):
    return torch.tensor(np.random.default_rng(seed).normal(size=(3, H, W)).astype(np.float32), device="cuda")


@pytest.mark.parametrize("P, W, H", CASES)
@pytest.mark.parametrize("D, M", [(0, 1), (1, 4), (2, 9), (3, 16), (1, 16)])
def test_sh_matches_torch_sh_through_colors_precomp(P, W, H, D, M):
    cam, g = scene(P, W, H, seed=P + D)
    sh = shs(P, M, seed=P + M)
    w = _weights(H, W, seed=1)
    rs = settings(cam, bg=(0.1, 0.2, 0.3), D=D)
    campos = rs.campos.float()

    ref = {k: leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations")}
    ref_sh = leaf(sh)
    colors = sh_eval_torch(ref_sh, ref["means3D"], campos, D)
    c_ref, r_ref, m2_ref = _render(rs, w, means3D=ref["means3D"], opacities=ref["opacities"], colors_precomp=colors,
                                   scales=ref["scales"], rotations=ref["rotations"])

    new = {k: leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations")}
    new_sh = leaf(sh)
    c_new, r_new, m2_new = _render(rs, w, means3D=new["means3D"], opacities=new["opacities"], shs=new_sh,
                                   scales=new["scales"], rotations=new["rotations"])

    assert torch.equal(r_ref, r_new)
    check_image(c_new, c_ref, 1e-6)
    vis = (r_new > 0).cpu()
    close(new_sh.grad, ref_sh.grad, "dL/dshs", allow_frac=0.0)
    close(new["means3D"].grad, ref["means3D"].grad, "dL/dmeans3D", allow_frac=0.0)
    close(m2_new, m2_ref, "dL/dmeans2D", allow_frac=0.0)
    for k in ("opacities", "scales", "rotations"):
        close(new[k].grad, ref[k].grad, f"dL/d{k}", allow_frac=0.0)
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
    cam, g = scene(P, W, H, seed=P + 7)
    w = _weights(H, W, seed=2)

    ref = {k: leaf(g[k]) for k in g}
    c_ref, r_ref, m2_ref = _render(settings(cam, bg=(0.1, 0.2, 0.3), scale_modifier=scale_modifier), w, means3D=ref["means3D"],
                                   opacities=ref["opacities"], colors_precomp=ref["colors"], scales=ref["scales"],
                                   rotations=ref["rotations"])

    new = {k: leaf(g[k]) for k in g}
    cov6 = cov6_torch(new["scales"], new["rotations"], scale_modifier)
    c_new, r_new, m2_new = _render(settings(cam, bg=(0.1, 0.2, 0.3), scale_modifier=1.0), w, means3D=new["means3D"],
                                   opacities=new["opacities"], colors_precomp=new["colors"], cov3D_precomp=cov6)

    same = (r_ref == r_new).cpu()
    assert float(same.float().mean()) >= 1 - 1e-4
    check_image(c_new, c_ref, 1e-5)
    for k in ("scales", "rotations", "means3D", "opacities", "colors"):
        close(new[k].grad, ref[k].grad, f"dL/d{k}", rows=same, allow_frac=1e-4)
    close(m2_new, m2_ref, "dL/dmeans2D", rows=same, allow_frac=1e-4)


@pytest.mark.parametrize("P, W, H", CASES[2:4])
def test_sh_and_cov3d_precomp_together(P, W, H):
    D, M = 3, 16
    cam, g = scene(P, W, H, seed=P + 11)
    sh = shs(P, M, seed=P)
    w = _weights(H, W, seed=3)
    rs = settings(cam, bg=(0.1, 0.2, 0.3), D=D)
    campos = rs.campos.float()

    ref = {k: leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations")}
    ref_sh = leaf(sh)
    c_ref, r_ref, _ = _render(rs, w, means3D=ref["means3D"], opacities=ref["opacities"],
                              colors_precomp=sh_eval_torch(ref_sh, ref["means3D"], campos, D), scales=ref["scales"],
                              rotations=ref["rotations"])
    new = {k: leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations")}
    new_sh = leaf(sh)
    c_new, r_new, _ = _render(rs, w, means3D=new["means3D"], opacities=new["opacities"], shs=new_sh,
                              cov3D_precomp=cov6_torch(new["scales"], new["rotations"], 1.0))
    same = (r_ref == r_new).cpu()
    assert float(same.float().mean()) >= 1 - 1e-4
    check_image(c_new, c_ref, 1e-5)
    close(new_sh.grad, ref_sh.grad, "dL/dshs", rows=same, allow_frac=1e-4)
    for k in ("means3D", "opacities", "scales", "rotations"):
        close(new[k].grad, ref[k].grad, f"dL/d{k}", rows=same, allow_frac=1e-4)


@pytest.mark.parametrize("P, W, H", CASES)
def test_visible_filter_with_cov3d_precomp(P, W, H):
    from contextgs_amd.rasterizer import GaussianRasterizer
    cam, g = scene(P, W, H, seed=P + 5)
    rast = GaussianRasterizer(settings(cam, bg=(0.1, 0.2, 0.3), scale_modifier=0.8))
    t = {k: torch.tensor(v, device="cuda") for k, v in g.items()}
    r_ref = rast.visible_filter(t["means3D"], t["scales"], t["rotations"])
    r_new = rast.visible_filter(t["means3D"], cov3D_precomp=cov6_torch(t["scales"], t["rotations"], 0.8))
    assert r_new.dtype == torch.int32 and r_new.shape == (P,)
    assert float((r_ref == r_new).float().mean()) >= 1 - 1e-4


@pytest.mark.parametrize("form", ["shs", "cov", "both"])
def test_each_form_is_bitwise_stable(form):
    from contextgs_amd.rasterizer import GaussianRasterizer
    P, W, H = 30000, 800, 600
    cam, g = scene(P, W, H, seed=9)
    rs = settings(cam, bg=(0.1, 0.2, 0.3), D=3, debug=True)
    t = {k: torch.tensor(v, device="cuda") for k, v in g.items()}
    kw = dict(means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"])
    if form in ("shs", "both"):
        kw["shs"] = torch.tensor(shs(P, 16, seed=9), device="cuda")
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
    rs = settings(cam, bg=(0.1, 0.2, 0.3), D=2)
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
