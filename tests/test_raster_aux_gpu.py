"""GPU checks of the rasterizer's depth / inverse-depth / alpha maps (csrc/raster_aux.hip) against the existing fp32 oracle.

Each map is the colour blend of a per-Gaussian scalar with a zero background, so the oracle's colour render with
colors = [z, 1/z, 1] and bg = 0 gives depth, invdepth and sum_i w_i, and its final_T gives alpha = 1 - T_final.  The
gradient is that run's backward plus the direct term (dL/dc0 - dL/dc1 / z^2) dz/dmeans3D.  Tolerances as
tests/test_raster_gpu.py: images by RMSE <= 1e-5 plus a max-abs allowance on a 1e-4 fraction (scaled here by each map's
maximum), gradients 2e-4 of each tensor's maximum with a 2e-3 fraction allowance.
"""
import itertools

import numpy as np
import pytest
import torch

from contextgs_amd.synth import look_at_camera, random_gaussians
from raster_harness import (BG, aux_colors, check_grad, check_map, cov6_torch, leaf, model, run, scene, settings, sh_eval_torch,
                            shs, view_z)

pytestmark = pytest.mark.gpu

CASES = [(1, 64, 48), (64, 128, 96), (4000, 256, 256), (30000, 800, 800), (200000, 1920, 1080)]   # test_raster_sh_cov_gpu
MAPS = ("depth", "invdepth", "alpha")


def _run(rs, g, return_aux=True, **kw):
    """raster_harness.run with the maps asked for unless the caller says otherwise."""
    return run(rs, g, return_aux=return_aux, **kw)


def _oracle_aux(oracle, cam, g, z, dl=None):
    return oracle.render(cam.oracle_dict(bg=(0.0, 0.0, 0.0)), g["means3D"], aux_colors(z), g["opacities"], g["scales"],
                         g["rotations"], dL_dout=dl)


# ---- forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P, W, H", CASES)
def test_forward_maps_match_the_oracle(oracle32, P, W, H):
    cam, g = scene(P, W, H, seed=P)
    z, _ = view_z(cam, g["means3D"])
    ref = _oracle_aux(oracle32, cam, g, z)
    rs = settings(cam, debug=(P == 1))          # the smallest case with a synchronised check after every kernel
    out = _run(rs, g)
    plain = _run(rs, g, return_aux=False)
    # no interference: the colour image and radii are those of the plain call, bit for bit
    assert torch.equal(out["color"], plain["color"]) and torch.equal(out["radii"], plain["radii"])
    assert (out["radii"].cpu().numpy() == ref["radii"]).all()
    for k in MAPS:
        assert out[k].shape == (1, H, W) and out[k].dtype == torch.float32
    check_map(out["depth"], ref["color"][0], f"depth P={P}")
    check_map(out["invdepth"], ref["color"][1], f"invdepth P={P}")
    check_map(out["alpha"], ref["color"][2], f"alpha (sum w) P={P}")
    check_map(out["alpha"], 1.0 - ref["final_T"], f"alpha (1 - T) P={P}")
    alpha = out["alpha"].cpu().numpy()[0]
    assert (alpha <= 1.0).all() and (alpha >= 0.0).all()
    assert (out["depth"].cpu().numpy() >= 0).all()


# ---- backward -----------------------------------------------------------------------------------------------------------
BWD_CASES = [(200, 64, 48, 0, 1.0, (0.005, 0.05)), (3000, 256, 256, 1, 1.0, (0.003, 0.04)),
             (20000, 200, 120, 2, 1.2, (0.002, 0.03))]
LOSSES = [("depth",), ("invdepth",), ("alpha",), ("color", "depth", "invdepth", "alpha"), ("depth", "invdepth", "alpha")]


@pytest.mark.parametrize("P, W, H, seed, extent, srange", BWD_CASES)
@pytest.mark.parametrize("keys", LOSSES, ids=["+".join(k) for k in LOSSES])
def test_backward_matches_the_oracle(oracle32, P, W, H, seed, extent, srange, keys):
    cam, g = scene(P, W, H, seed=seed, extent=extent, srange=srange)
    z, dz = view_z(cam, g["means3D"])
    rng = np.random.default_rng(seed + 17)
    gC = rng.normal(size=(3, H, W)).astype(np.float32)
    gm = {k: rng.normal(size=(1, H, W)).astype(np.float32) for k in MAPS}
    loss_w = {k: torch.tensor(gC if k == "color" else gm[k], device="cuda") for k in keys}
    out = _run(settings(cam), g, loss_w=loss_w)

    names = ["dL_dmeans3D", "dL_dmeans2D", "dL_dopacities", "dL_dscales", "dL_drotations"]
    exp = {k: 0.0 for k in names}
    if "color" in keys:
        rc = oracle32.render(cam.oracle_dict(bg=BG), g["means3D"], g["colors"], g["opacities"], g["scales"], g["rotations"],
                             dL_dout=gC)
        for k in names:
            exp[k] = exp[k] + rc[k]
    gaux = np.concatenate([gm[k] if k in keys else np.zeros((1, H, W), np.float32) for k in MAPS], 0)
    ra = _oracle_aux(oracle32, cam, g, z, dl=gaux)
    zs = np.where(z > 0.2, z, 1.0).astype(np.float32)
    direct = (ra["dL_dcolors"][:, 0] - ra["dL_dcolors"][:, 1] / (zs * zs))[:, None] * dz[None, :]
    for k in names:
        exp[k] = exp[k] + ra[k]
    exp["dL_dmeans3D"] = exp["dL_dmeans3D"] + direct

    gr = out["grad"]
    for k, t in (("dL_dmeans3D", "means3D"), ("dL_dmeans2D", "means2D"), ("dL_dopacities", "opacities"),
                 ("dL_dscales", "scales"), ("dL_drotations", "rotations")):
        check_grad(gr[t], exp[k], f"{k} P={P} {'+'.join(keys)}")
    if "color" in keys:
        check_grad(gr["colors"], rc["dL_dcolors"], f"dL_dcolors P={P}")
    else:
        assert gr["colors"] is None          # the maps send nothing to the colour input
    assert float(gr["means3D"].abs().sum()) > 0


# ---- the four argument forms --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P, W, H", CASES[1:4])
@pytest.mark.parametrize("form", ["shs+scales", "shs+cov", "colors+cov"])
def test_all_forms_match_colors_precomp_scales_rotations(P, W, H, form):
    from contextgs_amd.rasterizer import GaussianRasterizer
    D, M = 2, 9
    cam, g = scene(P, W, H, seed=P + 3)
    sh = shs(P, M, seed=P)
    rs = settings(cam, D=D)
    campos = rs.campos.float()
    rng = np.random.default_rng(5)
    w = {k: torch.tensor(rng.normal(size=(3 if k == "color" else 1, H, W)).astype(np.float32), device="cuda")
         for k in ("color",) + MAPS}

    def run(use_shs, use_cov):
        t = {k: leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
        t["shs"] = leaf(sh)
        m2 = torch.zeros(P, 3, device="cuda", requires_grad=True)
        kw = dict(means3D=t["means3D"], means2D=m2, opacities=t["opacities"])
        if use_shs:
            kw["shs"] = t["shs"]
        else:         # the reference form: torch's SH into colors_precomp when the other side uses shs
            kw["colors_precomp"] = sh_eval_torch(t["shs"], t["means3D"], campos, D) if "shs" in form else t["colors"]
        if use_cov:
            kw["cov3D_precomp"] = cov6_torch(t["scales"], t["rotations"], 1.0)
        else:
            kw["scales"], kw["rotations"] = t["scales"], t["rotations"]
        color, radii, aux = GaussianRasterizer(rs)(return_aux=True, **kw)
        ((color * w["color"]).sum() + sum((aux[k] * w[k]).sum() for k in MAPS)).backward()
        torch.cuda.synchronize()
        o = dict(color=color.detach(), radii=radii, m2=m2.grad, **{k: aux[k].detach() for k in MAPS})
        o.update({k: t[k].grad for k in t})
        return o

    ref = run(False, False)
    new = run("shs" in form, "cov" in form)
    same = (ref["radii"] == new["radii"]).cpu()
    assert float(same.float().mean()) >= 1 - 1e-4
    for k in ("color",) + MAPS:
        check_map(new[k], ref[k].cpu().numpy(), f"{k} {form} P={P}")
    rows = same.numpy()
    allow = 1e-4 if "cov" in form else 0.0
    for k in ("means3D", "opacities", "scales", "rotations", "m2") + (("shs",) if "shs" in form else ("colors",)):
        a, b = new[k].cpu().numpy(), ref[k].cpu().numpy()
        check_grad(a[rows].reshape(int(rows.sum()), -1), b[rows].reshape(int(rows.sum()), -1), f"d{k} {form} P={P}",
                    allow_frac=max(allow, 2e-3))


# ---- regimes ------------------------------------------------------------------------------------------------------------
def test_saturated_stack_reaches_termination(oracle32):
    P, W, H = 300, 64, 48
    cam = look_at_camera((0.0, -3.0, 0.0), (0, 0, 0), W, H, fovx_deg=50.0)
    rng = np.random.default_rng(11)
    g = random_gaussians(P, seed=11, extent=0.2, scale_lo=0.15, scale_hi=0.4)
    g["opacities"][:] = rng.uniform(0.9, 0.999, size=g["opacities"].shape).astype(np.float32)
    z, _ = view_z(cam, g["means3D"])
    ref = _oracle_aux(oracle32, cam, g, z)
    assert float(ref["final_T"].min()) < 1e-3         # the stack saturates: pixels stopped on the 1e-4 test
    out = _run(settings(cam), g)
    alpha = out["alpha"].cpu().numpy()[0]
    assert np.abs(alpha - (1.0 - ref["final_T"])).max() <= 1e-6
    assert (alpha <= 1.0).all()
    check_map(out["depth"], ref["color"][0], "depth saturated")
    check_map(out["invdepth"], ref["color"][1], "invdepth saturated")


def test_ragged_image(oracle32):
    P, W, H = 5000, 257, 255
    cam, g = scene(P, W, H, seed=4)
    z, dz = view_z(cam, g["means3D"])
    ref = _oracle_aux(oracle32, cam, g, z)
    out = _run(settings(cam), g)
    for i, k in enumerate(MAPS):
        check_map(out[k], ref["color"][i], f"{k} 257x255")


def test_empty_views_give_zero_maps():
    cam = look_at_camera((0.0, -3.0, 0.0), (0, 0, 0), 80, 64, fovx_deg=50.0)
    rs = settings(cam)
    g = random_gaussians(64, seed=6)
    g["means3D"][:, 1] -= 20.0                        # everything behind the camera
    for gg in (g, {k: v[:0] for k, v in g.items()}):
        out = _run(rs, gg, loss_w={"depth": torch.ones(1, 64, 80, device="cuda")})
        for k in MAPS:
            assert out[k].shape == (1, 64, 80) and bool((out[k] == 0).all()), k
        assert int((out["radii"] > 0).sum()) == 0
        assert bool((out["grad"]["means3D"] == 0).all())


def test_forward_after_a_voided_speculative_render(oracle32):
    from contextgs_amd import rasterizer
    P, W, H = 20000, 320, 240
    cam, g = scene(P, W, H, seed=9)
    z, _ = view_z(cam, g["means3D"])
    ref = _oracle_aux(oracle32, cam, g, z)
    rs = settings(cam)
    rasterizer._pair_capacity[(H, W)] = 1 << 10       # far below the view's pair count: the speculative render is voided
    out = _run(rs, g)
    assert rasterizer.last_call["num_rendered"] > (1 << 10)
    assert rasterizer.last_call["bin_R"] == rasterizer.last_call["num_rendered"]     # re-rendered with the true count
    for i, k in enumerate(MAPS):
        check_map(out[k], ref["color"][i], f"{k} re-rendered")
    again = _run(rs, g)                                   # now with a capacity that holds: the speculative render stands
    for k in MAPS:
        assert torch.equal(again[k], out[k]), k


# ---- no interference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P, W, H", [(3000, 256, 256), (30000, 800, 800)])
def test_colour_only_loss_with_aux_requested_matches_the_plain_call(P, W, H):
    cam, g = scene(P, W, H, seed=21)
    w = torch.tensor(np.random.default_rng(3).normal(size=(3, H, W)).astype(np.float32), device="cuda")
    a = _run(settings(cam), g, return_aux=False, loss_w={"color": w})
    b = _run(settings(cam), g, return_aux=True, loss_w={"color": w})
    assert torch.equal(a["color"], b["color"])
    for k in ("means3D", "means2D", "colors", "opacities", "scales", "rotations"):
        check_grad(b["grad"][k], a["grad"][k].cpu().numpy(), f"d{k} colour-only P={P}")


@pytest.mark.parametrize("P, W, H", [(4000, 256, 256), (200000, 1920, 1080)])
def test_maps_equal_the_colour_blend_of_z(P, W, H):
    cam, g = scene(P, W, H, seed=31)
    z, _ = view_z(cam, g["means3D"])
    out = _run(settings(cam), g)
    blend = _run(settings(cam, bg=(0.0, 0.0, 0.0)), g, return_aux=False, colors=aux_colors(z))["color"]
    for i, k in enumerate(MAPS):
        ref = blend[i:i + 1]
        scale = max(float(ref.abs().max()), 1e-12)
        assert float((out[k] - ref).abs().max()) <= 1e-6 * scale, k


# ---- render() -----------------------------------------------------------------------------------------------------------


def _render(pc, cam, pipe, bg, **kw):
    from contextgs_amd import ctx_ops
    from contextgs_amd.renderer import prefilter_voxel, render
    torch.manual_seed(0)
    ctx_ops._seed_counter = itertools.count(1)       # the same noise streams in every call
    vis = prefilter_voxel(cam, pc, pipe, bg)
    return render(cam, pc, pipe, bg, visible_mask=vis, step=1000, **kw)


@pytest.mark.parametrize("training", [False, True])
def test_render_returns_the_maps(training):
    pc, cams, pipe, bg = model()
    pc.train(training)
    ctx = torch.enable_grad() if training else torch.no_grad()
    with ctx:
        plain = _render(pc, cams[1], pipe, bg)
        pkg = _render(pc, cams[1], pipe, bg, return_aux=True)
    for k in plain:
        assert k in pkg, k
    for k in MAPS:
        assert pkg[k].shape == (1, 180, 320) and pkg[k].dtype == torch.float32, k
    assert torch.equal(pkg["render"].detach(), plain["render"].detach())
    assert torch.equal(pkg["radii"], plain["radii"])
    assert float(pkg["alpha"].max()) > 0.5 and float(pkg["alpha"].max()) <= 1.0
    assert float(pkg["depth"].max()) > 0
    if training:
        for _, p in pc.named_parameters():
            p.grad = None
        pkg = _render(pc, cams[1], pipe, bg, return_aux=True)
        (pkg["depth"].mean() + (1.0 - pkg["alpha"]).abs().mean()).backward()
        for name in ("_anchor", "_offset", "_anchor_feat", "_scaling"):
            gr = getattr(pc, name).grad
            assert gr is not None and torch.isfinite(gr).all() and float(gr.abs().sum()) > 0, name
