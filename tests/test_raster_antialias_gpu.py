"""GPU checks of the rasterizer's antialiasing (upstream's `antialiasing`, csrc/raster_math.h cgs_aa_h): with [[a, b], [b, c]]
the 2-D covariance before the 0.3 px^2 dilation, the blend reads opacity * h, h = sqrt(max(2.5e-5, det / det(+0.3 I))).

Torch restates the part the new kernels take over: an fp64 h_torch(...) differentiable in means3D, scales, rotations and
cov3D, so that an antialiased call with opacities o must match the existing call with opacities o * h_torch(...) (images,
maps, radii, every leaf gradient).  Tolerances as tests/test_raster_gpu.py: images by RMSE plus a max-abs allowance on a 1e-4
fraction of values, gradients 2e-4 of each tensor's max magnitude, allowances printed as [allowance] lines.
"""
import itertools
import math

import numpy as np
import pytest
import torch

from contextgs_amd.synth import look_at_camera, random_gaussians
from raster_harness import BG, R_MIN, check_image, close, h_torch, leaf, model, scene, settings, shs, sigma_rs

pytestmark = pytest.mark.gpu

CASES = [(1, 64, 48), (64, 128, 96), (4000, 256, 256), (30000, 800, 800), (200000, 1920, 1080)]   # test_raster_sh_cov_gpu
FORMS = ["colors+scales", "shs+scales", "colors+cov", "shs+cov"]
MAPS = ("depth", "invdepth", "alpha")


# ---- the torch restatement (fp64): h_torch, sigma_rs of tests/raster_harness.py and ------------------------------------
def sigma_cov6(cov6):
    c = cov6.double()
    return torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).view(-1, 3, 3)


def _run(form, g, sh, rs, aa_ref, w, aux):
    """One render + backward in `form`.  aa_ref: the AA-off call with opacities o * h_torch (autograd through h_torch)."""
    from contextgs_amd.rasterizer import GaussianRasterizer
    P = g["means3D"].shape[0]
    t = {k: leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
    t["shs"] = leaf(sh)
    m2 = torch.zeros(P, 3, device="cuda", requires_grad=True)
    cov6 = None
    if "cov" in form:
        S = sigma_rs(t["scales"], t["rotations"])
        cov6 = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).float()
    op = t["opacities"]
    if aa_ref:
        Sigma = sigma_cov6(cov6) if cov6 is not None else sigma_rs(t["scales"], t["rotations"])
        h, _ = h_torch(t["means3D"], Sigma, rs)
        op = op * h.float()[:, None]
    kw = dict(means3D=t["means3D"], means2D=m2, opacities=op)
    if "shs" in form:
        kw["shs"] = t["shs"]
    else:
        kw["colors_precomp"] = t["colors"]
    if cov6 is not None:
        kw["cov3D_precomp"] = cov6
    else:
        kw["scales"], kw["rotations"] = t["scales"], t["rotations"]
    if aux:
        color, radii, maps = GaussianRasterizer(rs)(return_aux=True, **kw)
        loss = (color * w["color"]).sum() + sum((maps[k] * w[k]).sum() for k in MAPS)
    else:
        color, radii = GaussianRasterizer(rs)(**kw)
        maps = {}
        loss = (color * w["color"]).sum()
    loss.backward()
    torch.cuda.synchronize()
    o = dict(color=color.detach(), radii=radii, m2=m2.grad, **{k: v.detach() for k, v in maps.items()})
    o.update({k: t[k].grad for k in t})
    return o


# ---- equivalence with the AA-off path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("P, W, H, aux", [c + (False,) for c in CASES] + [c + (True,) for c in CASES[2:]])
@pytest.mark.parametrize("form", FORMS)
def test_matches_the_aa_off_path_with_h_in_torch(P, W, H, aux, form):
    cam, g = scene(P, W, H, seed=P + 5)
    sh = shs(P, 9, seed=P, clamp_dc=False)
    rng = np.random.default_rng(7)
    w = {k: torch.tensor(rng.normal(size=(3 if k == "color" else 1, H, W)).astype(np.float32), device="cuda")
         for k in ("color",) + MAPS}
    new = _run(form, g, sh, settings(cam, aa=True, D=2), False, w, aux)
    ref = _run(form, g, sh, settings(cam, aa=False, D=2), True, w, aux)
    assert torch.equal(new["radii"], ref["radii"])
    check_image(new["color"], ref["color"], 1e-5, f"image {form} P={P}")
    for k in MAPS if aux else ():
        scale = max(float(ref[k].abs().max()), 1e-12)
        check_image(new[k] / scale, ref[k] / scale, 1e-5, f"{k} {form} P={P}")
    keys = ["means3D", "opacities", "m2"] + (["shs"] if "shs" in form else ["colors"]) + \
        (["scales", "rotations"])       # cov form: through cov6_torch to the same leaves
    for k in keys:
        close(new[k], ref[k], f"d{k} {form} aux={aux} P={P}", allow_frac=1e-4)
    if P >= 4000:
        vis = new["radii"] > 0
        assert float(new["opacities"][vis].abs().sum()) > 0


# ---- against the fp32 oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P, W, H", CASES[1:4])
def test_matches_the_oracle_with_the_h_chain(oracle32, P, W, H):
    from contextgs_amd.rasterizer import GaussianRasterizer
    cam, g = scene(P, W, H, seed=P + 13)
    rs = settings(cam, aa=True, D=2)
    gC = np.random.default_rng(P).normal(size=(3, H, W)).astype(np.float32)
    t = {k: leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
    m2 = torch.zeros(P, 3, device="cuda", requires_grad=True)
    color, radii = GaussianRasterizer(rs)(means3D=t["means3D"], means2D=m2, opacities=t["opacities"],
                                          colors_precomp=t["colors"], scales=t["scales"], rotations=t["rotations"])
    (color * torch.tensor(gC, device="cuda")).sum().backward()
    torch.cuda.synchronize()

    # oracle with o * h, then h's chain as a vector-Jacobian product of g * o through h
    q = {k: torch.tensor(g[k], device="cuda", dtype=torch.float64, requires_grad=True)
         for k in ("means3D", "scales", "rotations")}
    h, _ = h_torch(q["means3D"], sigma_rs(q["scales"], q["rotations"]), rs)
    o = torch.tensor(g["opacities"][:, 0], device="cuda", dtype=torch.float64)
    op_eff = (o * h).detach().float().cpu().numpy()[:, None]
    ref = oracle32.render(cam.oracle_dict(bg=BG), g["means3D"], g["colors"], op_eff, g["scales"], g["rotations"], dL_dout=gC)
    geff = torch.tensor(ref["dL_dopacities"], device="cuda", dtype=torch.float64)
    (geff * o * h).sum().backward()
    assert np.array_equal(radii.cpu().numpy(), ref["radii"])
    check_image(color.detach(), torch.tensor(ref["color"], device="cuda"), 1e-5, f"oracle image P={P}")
    close(t["opacities"].grad, (torch.tensor(ref["dL_dopacities"]) * h.detach().float().cpu())[:, None],
           f"oracle dopacities P={P}", allow_frac=2e-3)
    for k, name in (("means3D", "dL_dmeans3D"), ("scales", "dL_dscales"), ("rotations", "dL_drotations")):
        close(t[k].grad, torch.tensor(ref[name]) + q[k].grad.float().cpu(), f"oracle d{k} P={P}", allow_frac=2e-3)
    close(m2.grad, torch.tensor(ref["dL_dmeans2D"]), f"oracle dmeans2D P={P}", allow_frac=2e-3)


# ---- the clamp ----------------------------------------------------------------------------------------------------------
def _record_opacity(P):
    """op_eff as the preprocess kernel wrote it into the geometry records (rec[3 i + 1].y) of the last forward."""
    from contextgs_amd import rasterizer
    geom = rasterizer.last_call["geom_ws"]
    return geom[:48 * P].view(torch.float32).view(P, 12)[:, 5]


def test_clamp_regime():
    from contextgs_amd.rasterizer import GaussianRasterizer
    P, W, H = 3000, 256, 256
    cam, g = scene(P, W, H, seed=41)
    g["means3D"][::20] = g["means3D"][1::20]       # every Gaussian in front of the camera
    rng = np.random.default_rng(41)
    k = np.arange(P)
    # a third points (all three scales ~0), a third needles of zero width (two scales ~0), a third ordinary
    g["scales"][k % 3 == 0] = 1e-7
    g["scales"][k % 3 == 1, 1:] = 1e-7
    g["opacities"][:] = rng.uniform(0.85, 1.0, size=(P, 1)).astype(np.float32)
    g["opacities"][k % 6 == 0] = 0.5             # points at 0.5: op_eff = 0.0025 < 1/255
    rs_on, rs_off = settings(cam, aa=True, D=2), settings(cam, aa=False, D=2)
    w = torch.tensor(rng.normal(size=(3, H, W)).astype(np.float32), device="cuda")

    def run(rs, op):
        t = {k: leaf(g[k]) for k in ("means3D", "scales", "rotations", "colors")}
        t["opacities"] = leaf(op)
        color, radii = GaussianRasterizer(rs)(means3D=t["means3D"], means2D=torch.zeros(P, 3, device="cuda"),
                                              opacities=t["opacities"], colors_precomp=t["colors"], scales=t["scales"],
                                              rotations=t["rotations"])
        (color * w).sum().backward()
        torch.cuda.synchronize()
        return color.detach(), radii, {k: v.grad for k, v in t.items()}

    c_on, r_on, g_on = run(rs_on, g["opacities"])
    op_rec = _record_opacity(P).cpu()
    _, r_off, _ = run(rs_off, g["opacities"])
    assert torch.equal(r_on, r_off)                 # radii do not see h
    t = {k: torch.tensor(g[k], device="cuda") for k in ("means3D", "scales", "rotations")}
    _, r = h_torch(t["means3D"], sigma_rs(t["scales"], t["rotations"]), rs_on)
    clamped = (r <= R_MIN).cpu() & (r_on > 0).cpu()
    assert int(clamped.sum()) >= P // 3          # points and zero-width needles are clamped
    o = torch.tensor(g["opacities"][:, 0])
    assert torch.allclose(op_rec[clamped], 0.005 * o[clamped], rtol=1e-6, atol=0)
    # the clamped Gaussians render as the AA-off call at 0.005 o, and get no h gradient
    op_ref = g["opacities"].copy()
    op_ref[clamped.numpy()] *= np.float32(0.005)
    keep = ~clamped.numpy()
    op_ref[keep] = op_rec.numpy()[keep][:, None]     # the others at the kernel's own op_eff
    c_ref, _, g_ref = run(rs_off, op_ref)
    check_image(c_on, c_ref, 1e-5, "clamp image")
    rows = clamped
    for k in ("means3D", "scales", "rotations"):
        close(g_on[k], g_ref[k], f"clamp d{k}", rows=rows, allow_frac=1e-4)
    close(g_on["opacities"], g_ref["opacities"] * 0.005, "clamp dopacities", rows=rows, allow_frac=1e-4)
    faint = clamped & (o * 0.005 < 1.0 / 255)
    assert int(faint.sum()) > 0
    for k in g_on:
        assert bool((g_on[k][faint.cuda()] == 0).all()), k     # below 1/255: no pixel, no gradient


# ---- needles: the stable d0 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["colors+scales", "colors+cov"])
def test_needles_h_against_fp64(form):
    from contextgs_amd.rasterizer import GaussianRasterizer
    P, W, H = 2000, 800, 600
    cam = look_at_camera((0.0, -3.0, 0.0), (0, 0, 0), W, H, fovx_deg=55.0)
    rng = np.random.default_rng(3)
    g = random_gaussians(P, seed=3, extent=0.8)
    ratio = 10 ** rng.uniform(2, 3, size=P)                       # 100:1 .. 1000:1
    long = rng.uniform(0.05, 0.3, size=P)
    g["scales"] = np.stack([long, long / ratio, long / ratio * rng.uniform(0.5, 2.0, size=P)], 1).astype(np.float32)
    q = rng.normal(size=(P, 4))
    g["rotations"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)     # oblique
    rs = settings(cam, aa=True, D=2)
    t = {k: torch.tensor(g[k], device="cuda") for k in g}
    kw = dict(means3D=t["means3D"], means2D=torch.zeros(P, 3, device="cuda"), opacities=t["opacities"],
              colors_precomp=t["colors"])
    S = sigma_rs(t["scales"], t["rotations"])
    if form == "colors+cov":
        kw["cov3D_precomp"] = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).float()
        S = sigma_cov6(kw["cov3D_precomp"])
    else:
        kw["scales"], kw["rotations"] = t["scales"], t["rotations"]
    with torch.no_grad():
        _, radii = GaussianRasterizer(rs)(**kw)
        torch.cuda.synchronize()
        op = _record_opacity(P).double()
        h64, r64 = h_torch(t["means3D"], S, rs)
    live = (radii > 0) & (r64 > 4 * R_MIN)
    assert int(live.sum()) > P // 2
    h_k = op[live] / t["opacities"][:, 0].double()[live]
    rel = ((h_k - h64[live]).abs() / h64[live]).max().item()
    print(f"[allowance] needles {form}: max |h - h64| / h64 = {rel:.2e} over {int(live.sum())} Gaussians, "
          f"min r {float(r64[live].min()):.2e}")
    # scales/rotations: the sum of squared minors stays within ~1e-6.  cov3D: the fp32 A Sigma A^T of a needle already loses
    # ~3 % of a c - b^2 before the (compensated) subtraction, in the kernel as in any fp32 restatement
    assert rel <= (1e-4 if form == "colors+scales" else 0.1), rel


# ---- what antialiasing is for ------------------------------------------------------------------------------------------
def _sparse_field(W, P=3000, seed=8):
    """P isotropic Gaussians in front of a camera, sigma 0.4 .. 1 px at 1024 px width, opacity 0.8, white on black."""
    rng = np.random.default_rng(seed)
    cam = look_at_camera((0.0, -4.0, 0.0), (0, 0, 0), W, W, fovx_deg=50.0)
    pts = np.stack([rng.uniform(-1.4, 1.4, P), rng.uniform(-0.5, 0.5, P), rng.uniform(-1.4, 1.4, P)], 1).astype(np.float32)
    z = pts[:, 1] + 4.0
    fx1024 = 1024 / (2 * math.tan(math.radians(50.0) / 2))
    sig = rng.uniform(0.4, 1.0, P) * z / fx1024
    g = dict(means3D=pts, scales=np.repeat(sig[:, None], 3, 1).astype(np.float32),
             rotations=np.tile(np.array([1, 0, 0, 0], np.float32), (P, 1)), colors=np.ones((P, 3), np.float32),
             opacities=np.full((P, 1), 0.8, np.float32))
    return cam, g


def test_antialiasing_keeps_brightness_across_resolutions():
    from contextgs_amd.rasterizer import GaussianRasterizer
    mean = {}
    for aa, W in itertools.product((False, True), (1024, 256)):
        cam, g = _sparse_field(W)
        t = {k: torch.tensor(v, device="cuda") for k, v in g.items()}
        with torch.no_grad():
            color, _ = GaussianRasterizer(settings(cam, aa=aa, D=2, bg=(0.0, 0.0, 0.0)))(
                means3D=t["means3D"], means2D=torch.zeros_like(t["means3D"]), opacities=t["opacities"],
                colors_precomp=t["colors"], scales=t["scales"], rotations=t["rotations"])
        mean[(aa, W)] = float(color.mean())
    off = mean[(False, 256)] / mean[(False, 1024)]
    on = mean[(True, 256)] / mean[(True, 1024)]
    print(f"[allowance] mean intensity 256 / 1024: AA off {off:.3f}, AA on {on:.3f}  ({mean})")
    # measured on MI355X: AA off 6.01, AA on 0.959 (the 4 % lost: splats whose op_eff at 256 px puts part of their
    # footprint under the 1/255 alpha skip)
    assert off > 2.0                                  # without AA the low-resolution view is clearly brighter
    assert 0.9 <= on <= 1.1
    assert abs(math.log(on)) <= 0.15 * abs(math.log(off))     # AA closes most of the gap


# ---- render() -----------------------------------------------------------------------------------------------------------
def _seeded(pc, cam, pipe, bg):
    from contextgs_amd import ctx_ops
    from contextgs_amd.renderer import prefilter_voxel
    torch.manual_seed(0)
    ctx_ops._seed_counter = itertools.count(1)       # the same noise streams in every call
    return prefilter_voxel(cam, pc, pipe, bg)


class _AAPipe:
    convert_SHs_python = False
    compute_cov3D_python = False
    debug = False
    antialiasing = True


@pytest.mark.parametrize("training", [False, True])
def test_render_with_pipe_antialiasing(training):
    from contextgs_amd.rasterizer import GaussianRasterizer
    from contextgs_amd.renderer import _raster_settings, generate_neural_gaussians, render
    pc, cams, pipe, bg = model()
    assert not hasattr(pipe, "antialiasing")
    pc.train(training)
    cam = cams[1]
    with torch.enable_grad() if training else torch.no_grad():
        vis = _seeded(pc, cam, _AAPipe(), bg)
        pkg = render(cam, pc, _AAPipe(), bg, visible_mask=vis, step=1000)
        # the same expanded Gaussians through the drop-in's antialiased call
        vis = _seeded(pc, cam, _AAPipe(), bg)
        out = generate_neural_gaussians(cam, pc, vis, is_training=training, step=1000)
        xyz, color, opacity, scaling, rot = out[:5]
        rs = _raster_settings(cam, _AAPipe(), bg, 1.0)
        assert rs.antialiasing is True
        img, radii = GaussianRasterizer(rs)(means3D=xyz, means2D=torch.zeros_like(xyz), opacities=opacity,
                                            colors_precomp=color, scales=scaling, rotations=rot)
        vis = _seeded(pc, cam, pipe, bg)
        plain = render(cam, pc, pipe, bg, visible_mask=vis, step=1000)
    assert torch.equal(pkg["render"].detach(), img.detach())
    assert torch.equal(pkg["radii"], radii)
    assert torch.equal(pkg["radii"], plain["radii"])
    assert not torch.equal(pkg["render"].detach(), plain["render"].detach())
    if training:
        for _, p in pc.named_parameters():
            p.grad = None
        vis = _seeded(pc, cam, _AAPipe(), bg)
        pkg = render(cam, pc, _AAPipe(), bg, visible_mask=vis, step=1000)
        pkg["render"].mean().backward()
        for name in ("_anchor", "_offset", "_anchor_feat", "_scaling"):
            gr = getattr(pc, name).grad
            assert gr is not None and torch.isfinite(gr).all() and float(gr.abs().sum()) > 0, name


def test_pipe_without_the_attribute_renders_as_before():
    from contextgs_amd.renderer import render
    pc, cams, pipe, bg = model()
    pc.train(False)

    class _Off(_AAPipe):
        antialiasing = False

    with torch.no_grad():
        a = render(cams[2], pc, pipe, bg, visible_mask=_seeded(pc, cams[2], pipe, bg), step=1000)
        b = render(cams[2], pc, _Off(), bg, visible_mask=_seeded(pc, cams[2], pipe, bg), step=1000)
    assert torch.equal(a["render"], b["render"]) and torch.equal(a["radii"], b["radii"])
