"""GPU checks of the rasterizer's depth-distortion and median-depth maps (`return_geometry=True`, csrc/raster_geom_maps.hip)
against the existing oracle, unchanged, used as a per-pixel decomposition (tests/raster_geom_ref.py has the reference).

Scenes: the four named scenes of tests/raster_harness.py: `ragged` (200 Gaussians at 40x24: 3x2 tiles, ragged right and bottom
edges, some Gaussians behind the near plane), `single` (1 Gaussian at 64x48), `long` (700 faint Gaussians over one 16x16 tile:
the lists cross the 256-entry batch boundary twice and no pixel stops early), `saturated` (300 near-opaque Gaussians over one
tile: early stops and the 0.99 cap).

Tolerances.  `distortion`, `median_depth`: `check_map` of tests/raster_harness.py: RMSE <= 1e-5 of the map's maximum and at most
a 1e-4 share of values beyond 2e-5.  `median_id` must be equal, and `median_depth` is compared, on every pixel whose reference
margin to 0.5 (raster_geom_ref.geom_maps) exceeds 1e-4; at most 1 % of the pixels may be excluded that way.  Gradients:
`check_grad`: at most a 2e-3 share of entries beyond 2e-4 of the tensor's maximum.  These caps are conditions, not measurements: every
scene was first run on the CPU with the fp32 oracle's decomposition and gradients against the fp64 oracle's under the same
checks at cap = 0.5 (`fp32_oracle_within_half_caps` below is that run), and kept only because the fp32 oracle alone stays
within HALF of every cap; a scene that does not gets another seed, never another cap.
References are computed once per scene and shared; nobody writes into them.
"""
import itertools
import math

import numpy as np
import pytest
import torch

import raster_geom_ref as ref
from contextgs_amd.synth import look_at_camera, random_gaussians
from raster_harness import BG, check_grad, check_map, cov6_torch, leaf, memo, model, named_scene, np_of, run, scene, settings, shs

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-4
AUX = ("depth", "invdepth", "alpha")
DECOMPOSED = ("ragged", "long", "saturated", "single")
LOSSES = ("distortion", "median", "both", "everything")


def _weights(name):
    """The upstream gradients of a scene: random normal, fixed per scene."""
    cam, _ = named_scene(name)
    H, W = cam.image_height, cam.image_width
    rng = np.random.default_rng(100 + DECOMPOSED.index(name))
    return {"distortion": rng.normal(size=(1, H, W)).astype(np.float32),
            "median_depth": rng.normal(size=(1, H, W)).astype(np.float32),
            "color": rng.normal(size=(3, H, W)).astype(np.float32),
            **{k: (0.3 * rng.normal(size=(1, H, W))).astype(np.float32) for k in AUX}}


def reference(oracle, name):
    """{"dec", "maps", "z", "grads": {"distortion", "median", "colour+aux"} -> per-input gradients} from one oracle."""
    cam, g = named_scene(name)
    H, W = cam.image_height, cam.image_width
    wts = _weights(name)
    dec = ref.decompose(oracle, cam, g)
    z = ref.view_depths(cam, g["means3D"])
    maps = ref.geom_maps(dec["w"], z)
    grads = {"distortion": ref.grad_reference(oracle, cam, g, maps, g_dist=wts["distortion"]),
             "median": ref.grad_reference(oracle, cam, g, maps, g_med=wts["median_depth"])}
    # the colour image and the three return_aux maps: the oracle's own backward, then one call with the per-Gaussian scalars
    # (z, 1 / z, 1) as colours over a zero background for the maps' weight path, and their dL/dz from w in numpy
    cd = cam.oracle_dict(bg=BG)
    r = oracle.render(cd, g["means3D"], g["colors"], g["opacities"], g["scales"], g["rotations"], dL_dout=wts["color"])
    tot = {k: np.asarray(r["dL_d" + k], np.float64).copy() for k in ref.GRAD_KEYS}
    zs = np.where(dec["radii"] > 0, z, 1.0)
    scal = np.stack([zs, 1.0 / zs, np.ones_like(zs)], 1)
    d = np.concatenate([wts[k] for k in AUX], 0)
    r = oracle.render(cam.oracle_dict(bg=(0.0, 0.0, 0.0)), g["means3D"], scal, g["opacities"], g["scales"], g["rotations"],
                      dL_dout=d)
    for k in ref.GRAD_KEYS:
        tot[k] = tot[k].reshape(grads["median"][k].shape) + np.asarray(r["dL_d" + k], np.float64).reshape(grads["median"][k].shape)
    w64 = np.asarray(dec["w"], np.float64)
    dz = w64 @ wts["depth"].reshape(-1).astype(np.float64) - (w64 @ wts["invdepth"].reshape(-1).astype(np.float64)) / zs ** 2
    V = np.asarray(cam.world_view_transform, np.float32).astype(np.float64).reshape(4, 4)
    tot["means3D"] = tot["means3D"] + dz[:, None] * V[None, :3, 2]
    grads["colour+aux"] = tot
    return {"dec": dec, "maps": maps, "z": z, "grads": grads}


def grads_of(R, loss):
    parts = {"distortion": ("distortion",), "median": ("median",), "both": ("distortion", "median"),
             "everything": ("distortion", "median", "colour+aux")}[loss]
    return {k: sum(R["grads"][p][k] for p in parts) for k in ref.GRAD_KEYS}


def check_forward(got, maps, what, cap=1.0):
    """got: {"distortion", "median_depth", "median_id"} as arrays; maps: geom_maps() of the fp64 decomposition."""
    check_map(got["distortion"], maps["distortion"], f"distortion {what}", cap=cap)
    decided = maps["margin"] > 1e-4
    print(f"[allowance] median {what}: {int((~decided).sum())} of {decided.size} pixels are within 1e-4 of the crossing")
    assert (~decided).mean() <= 1e-2 * cap, (what, int((~decided).sum()))
    a, b = np_of(got["median_id"]).reshape(-1), maps["median_id"].reshape(-1)
    assert (a[decided] == b[decided]).all(), (what, int((a[decided] != b[decided]).sum()))
    md = np.where(decided, np_of(got["median_depth"]).reshape(-1), maps["median_depth"])
    check_map(md, maps["median_depth"], f"median_depth {what}", cap=cap)


def check_grads(got, want, what, cap=1.0):
    for k in ref.GRAD_KEYS:
        check_grad(np.asarray(got[k]).reshape(want[k].shape[0], -1), want[k], f"d{k} {what}", allow_frac=2e-3 * cap)


def fp32_oracle_within_half_caps(oracle32, oracle64, name):
    """The CPU run that admits a scene (module docstring): the fp32 oracle alone against the fp64 oracle at half of every cap."""
    R64, R32 = reference(oracle64, name), reference(oracle32, name)
    check_forward(R32["maps"], R64["maps"], f"{name}, fp32 oracle", cap=0.5)
    for loss in LOSSES:
        check_grads(grads_of(R32, loss), grads_of(R64, loss), f"{name} {loss}, fp32 oracle", cap=0.5)


# ---- running the rasterizer --------------------------------------------------------------------------------------------------
def _run(rs, g, geometry=True, absgrad=False, **kw):
    """raster_harness.run with return_geometry=True unless `geometry` is False, and a [P,4] means2D with absgrad."""
    more = dict(return_geometry=True) if geometry else {}
    return run(rs, g, means2D_cols=4 if absgrad else 3, absgrad=absgrad, **more, **kw)


def _loss_w(name, loss):
    wts = _weights(name)
    keys = {"distortion": ("distortion",), "median": ("median_depth",), "both": ("distortion", "median_depth"),
            "everything": ("distortion", "median_depth", "color") + AUX}[loss]
    return {k: wts[k] for k in keys}


def _check_shapes(out, P, H, W):
    assert out["distortion"].shape == (1, H, W) and out["distortion"].dtype == torch.float32
    assert out["median_depth"].shape == (1, H, W) and out["median_depth"].dtype == torch.float32
    assert out["median_id"].shape == (H, W) and out["median_id"].dtype == torch.int32
    assert bool((out["distortion"] >= 0).all())
    assert bool(((out["median_id"] == -1) == (out["median_depth"][0] == 0)).all())
    assert bool(((out["median_id"] >= -1) & (out["median_id"] < max(P, 1))).all())


# ---- forward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DECOMPOSED)
def test_forward_matches_the_fp64_decomposition(oracle64, name):
    cam, g = named_scene(name)
    P, H, W = g["means3D"].shape[0], cam.image_height, cam.image_width
    R = memo(("geom", "ref", name), lambda: reference(oracle64, name))
    dec = R["dec"]
    if name == "long":
        tiles = ((H + 15) // 16) * ((W + 15) // 16)
        assert int(dec["stats"][0]) / tiles > 512 and int(dec["stats"][1]) / tiles > 256     # beyond two 256-entry batches
    if name == "saturated":
        assert float(dec["final_T"].min()) < 1e-3              # pixels stop early: later entries must count nothing
    rs = settings(cam, debug=(name == "single"))
    out = _run(rs, g, return_aux=True)
    plain = _run(rs, g, geometry=False, return_aux=True)
    assert torch.equal(out["color"], plain["color"]) and torch.equal(out["radii"], plain["radii"])
    for k in AUX:
        assert torch.equal(out[k], plain[k]), k
    assert (out["radii"].cpu().numpy() == dec["radii"]).all()
    _check_shapes(out, P, H, W)
    check_forward(out, R["maps"], name)
    if name == "single":
        assert bool((out["distortion"] == 0).all())
    else:
        assert float(out["distortion"].max()) > 0 and int((out["median_id"] >= 0).sum()) > 0
    if name == "long":          # faint Gaussians: most rays never reach one half
        assert int((out["median_id"] < 0).sum()) > 0


# ---- backward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", DECOMPOSED)
def test_backward_matches_the_reference(oracle64, name, loss):
    cam, g = named_scene(name)
    R = memo(("geom", "ref", name), lambda: reference(oracle64, name))
    out = _run(settings(cam), g, loss_w=_loss_w(name, loss), return_aux=(loss == "everything"))
    want = grads_of(R, loss)
    if loss != "everything":
        assert out["grad"]["colors"] is None          # the new maps send nothing to the colour inputs
    got = {k: np_of(out["grad"][k]) for k in ref.GRAD_KEYS}
    if name != "single" or loss == "everything":      # (one Gaussian: no distortion, and its opacity does not reach one half)
        assert max(float(np.abs(want[k]).max()) for k in ref.GRAD_KEYS) > 0
    check_grads(got, want, f"{name} {loss}")


def test_absgrad_takes_the_share_in_the_signed_columns_only(oracle64):
    name = "ragged"
    cam, g = named_scene(name)
    R = memo(("geom", "ref", name), lambda: reference(oracle64, name))
    lw = _loss_w(name, "both")
    out = _run(settings(cam), g, loss_w=lw, absgrad=True)
    m2 = np_of(out["grad"]["means2D"])
    assert m2.shape == (g["means3D"].shape[0], 4) and (m2[:, 2:] == 0).all()      # the colour image got no gradient
    want = grads_of(R, "both")
    check_grad(m2[:, :2], want["means2D"][:, :2], "dmeans2D[:, :2] with absgrad")
    lw = _loss_w(name, "everything")
    out = _run(settings(cam), g, loss_w=lw, absgrad=True, return_aux=True)
    colour_only = _run(settings(cam), g, loss_w={"color": lw["color"]}, absgrad=True, geometry=False)
    check_grad(np_of(out["grad"]["means2D"])[:, 2:], np_of(colour_only["grad"]["means2D"])[:, 2:], "absolute columns")
    check_grad(np_of(out["grad"]["means2D"])[:, :2], grads_of(R, "everything")["means2D"][:, :2], "signed columns, everything")


def test_cov3D_and_shs_form_against_the_plain_form():
    """cov3D_precomp built from the same scales / rotations and SH colours: the maps do not depend on the colour, so maps and
    gradients are those of the plain form; dL/dcov3D_precomp is chained back to scales / rotations by torch."""
    from contextgs_amd.rasterizer import GaussianRasterizer
    name = "ragged"
    cam, g = named_scene(name)
    P = g["means3D"].shape[0]
    lw = _loss_w(name, "both")
    rs = settings(cam, D=2)
    plain = _run(rs, g, loss_w=lw)
    t = {k: leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations")}
    sh = leaf(shs(P, 9, seed=5))
    m2 = torch.zeros(P, 3, device="cuda", requires_grad=True)
    color, radii, ex = GaussianRasterizer(rs)(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], shs=sh,
                                              cov3D_precomp=cov6_torch(t["scales"], t["rotations"], 1.0), return_geometry=True)
    sum((ex[k] * torch.as_tensor(w, device="cuda")).sum() for k, w in lw.items()).backward()
    torch.cuda.synchronize()
    assert torch.equal(radii, plain["radii"]) and sh.grad is None
    check_map(ex["distortion"], np_of(plain["distortion"]), "distortion, shs + cov3D vs plain")
    same = (ex["median_id"] == plain["median_id"])
    assert float(same.float().mean()) >= 0.99
    check_map(torch.where(same, ex["median_depth"][0], plain["median_depth"][0]), np_of(plain["median_depth"]),
               "median_depth, shs + cov3D vs plain")
    for k in ("means3D", "opacities", "scales", "rotations"):
        check_grad(t[k].grad, np_of(plain["grad"][k]), f"d{k}, shs + cov3D vs plain")
    check_grad(m2.grad, np_of(plain["grad"]["means2D"]), "dmeans2D, shs + cov3D vs plain")


def test_antialiasing_against_opacities_premultiplied_by_h():
    """antialiasing=True against a plain call whose opacities are opacity * h, h computed in numpy fp64 (Gaussians large and
    small: h ranges well below 1).  Maps equal; dL/dopacity = h dL/d(opacity h); means2D gets nothing from h."""
    name = "ragged"
    cam, g = named_scene(name)
    lw = _loss_w(name, "both")
    V = np.asarray(cam.world_view_transform, np.float32).astype(np.float64).reshape(4, 4)
    m, s, q = (g[k].astype(np.float64) for k in ("means3D", "scales", "rotations"))
    r, x, y, z = q.T
    Rm = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                   2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    L = Rm * s[:, None, :]
    Sigma = L @ L.transpose(0, 2, 1)
    t = m @ V[:3, :3] + V[3, :3]
    tanx, tany = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    tz = np.where(np.abs(t[:, 2]) > 1e-9, t[:, 2], 1.0)
    tx = np.clip(t[:, 0] / tz, -1.3 * tanx, 1.3 * tanx) * tz
    ty = np.clip(t[:, 1] / tz, -1.3 * tany, 1.3 * tany) * tz
    fx, fy = cam.image_width / (2 * tanx), cam.image_height / (2 * tany)
    z0 = np.zeros_like(tz)
    J = np.stack([fx / tz, z0, -fx * tx / tz ** 2, z0, fy / tz, -fy * ty / tz ** 2], 1).reshape(-1, 2, 3)
    A = J @ V[:3, :3].T
    c2 = A @ Sigma @ A.transpose(0, 2, 1)
    a, b, c = c2[:, 0, 0], c2[:, 0, 1], c2[:, 1, 1]
    h = np.sqrt(np.maximum((a * c - b * b) / ((a + 0.3) * (c + 0.3) - b * b), 2.5e-5))
    aa = _run(settings(cam, aa=True), g, loss_w=lw)
    vis = aa["radii"].cpu().numpy() > 0
    assert float(h[vis].min()) < 0.5 and float(h[vis].max()) > 0.9           # h ~ 1 is not assumed
    g2 = dict(g)
    g2["opacities"] = (g["opacities"].astype(np.float64) * h[:, None]).astype(np.float32)
    pre = _run(settings(cam), g2, loss_w=lw)
    check_map(aa["distortion"], np_of(pre["distortion"]), "distortion, antialiasing vs opacity * h")
    same = (aa["median_id"] == pre["median_id"])
    assert float(same.float().mean()) >= 0.99
    check_map(torch.where(same, aa["median_depth"], pre["median_depth"]), np_of(pre["median_depth"]), "median_depth, antialiasing")
    check_grad(aa["grad"]["means2D"], np_of(pre["grad"]["means2D"]), "dmeans2D, antialiasing vs opacity * h")
    check_grad(aa["grad"]["opacities"], np_of(pre["grad"]["opacities"]) * h[:, None].astype(np.float32),
               "dopacities = h d(opacity h)")


# ---- the camera --------------------------------------------------------------------------------------------------------------
def _quat_to_rot(q):
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)


def test_viewmatrix_gradient_is_the_sum_the_per_gaussian_reference_implies(oracle64):
    """The construction of tests/test_raster_camera_gpu.py (moving the camera by M equals moving the scene by M), restated with
    the world side taken from the REFERENCE per-Gaussian gradients.  M = [[e^k I, 0], [b, 1]], a uniform scale and a translation
    (the subgroup scales / rotations express without a covariance chain): means -> e^k means + b, scales -> e^k scales, so at
    M = I the reference implies dL/dk = sum_i means_i . dL/dmeans_i + scales_i . dL/dscales_i and dL/db = sum_i dL/dmeans_i.
    The camera side is autograd through V = M V0, PM = M PM0 into the node's dL/dviewmatrix and dL/dprojmatrix."""
    from contextgs_amd.rasterizer import GaussianRasterizer
    name = "ragged"
    cam, g = named_scene(name)
    R = memo(("geom", "ref", name), lambda: reference(oracle64, name))
    want = grads_of(R, "distortion")
    P = g["means3D"].shape[0]
    ref_k = float((g["means3D"].astype(np.float64) * want["means3D"]).sum() + (g["scales"].astype(np.float64) * want["scales"]).sum())
    ref_b = want["means3D"].sum(0)
    c = cam.to_torch("cuda")
    theta = torch.zeros(4, device="cuda", requires_grad=True)
    M4 = torch.cat([torch.cat([torch.eye(3, device="cuda") * torch.exp(theta[0]), torch.zeros(3, 1, device="cuda")], dim=1),
                    torch.cat([theta[1:], torch.ones(1, device="cuda")]).unsqueeze(0)], dim=0)
    V, PM = M4 @ c.world_view_transform, M4 @ c.full_proj_transform
    t = {k: torch.tensor(g[k], device="cuda") for k in ("means3D", "opacities", "scales", "rotations", "colors")}
    color, radii, ex = GaussianRasterizer(settings(cam, view=V, proj=PM))(
        means3D=t["means3D"], means2D=torch.zeros(P, 3, device="cuda"), opacities=t["opacities"], colors_precomp=t["colors"],
        scales=t["scales"], rotations=t["rotations"], return_geometry=True)
    (ex["distortion"] * torch.as_tensor(_weights(name)["distortion"], device="cuda")).sum().backward()
    torch.cuda.synchronize()
    got = theta.grad.cpu().numpy().astype(np.float64)
    wantv = np.concatenate([[ref_k], ref_b])
    err = float(np.abs(got - wantv).max() / np.abs(wantv).max())
    print(f"[camera] dL/d(scale, translation): camera side {got}, reference {wantv}, |diff| = {err:.3e} of the maximum")
    assert float(np.abs(wantv).max()) > 0 and err <= GRAD_TOL


# ---- nothing changes without a gradient on the new maps ----------------------------------------------------------------------
def test_without_a_gradient_on_the_new_maps_the_backward_is_the_old_one():
    """Colour (and aux) gradients only: no geometry backward kernel runs, the node's backward call is the one of a call without
    the keyword.  The blend backward sums with float atomics, so bit-equality is asserted for every gradient that two plain
    calls reproduce bit for bit, and all of them stay within `_check_grad`."""
    P, W, H = 3000, 256, 256
    cam, g = scene(P, W, H, 1, 1.0, (0.003, 0.04))
    rs = settings(cam)
    rng = np.random.default_rng(18)
    lw = {"color": rng.normal(size=(3, H, W)).astype(np.float32), "depth": rng.normal(size=(1, H, W)).astype(np.float32)}
    a = _run(rs, g, loss_w=lw, return_aux=True)
    b = _run(rs, g, loss_w=lw, return_aux=True, geometry=False)
    b2 = _run(rs, g, loss_w=lw, return_aux=True, geometry=False)
    assert torch.equal(a["color"], b["color"]) and torch.equal(a["depth"], b["depth"])
    _check_shapes(a, P, H, W)
    for k in ("means2D", "means3D", "opacities", "scales", "rotations", "colors"):
        fixed = torch.equal(b["grad"][k], b2["grad"][k])
        print(f"[geometry] d{k}: two plain calls bit-equal: {fixed}; with return_geometry bit-equal: "
              f"{torch.equal(a['grad'][k], b['grad'][k])}")
        if fixed:
            assert torch.equal(a["grad"][k], b["grad"][k]), k
        check_grad(a["grad"][k], b["grad"][k].cpu().numpy(), f"d{k} with return_geometry vs without")
    only = _run(rs, g, loss_w={"distortion": np.ones((1, H, W), np.float32)})
    assert only["grad"]["colors"] is None and float(only["grad"]["means3D"].abs().sum()) > 0


def test_outputs_and_saved_tensors():
    from contextgs_amd.rasterizer import GaussianRasterizer
    cam, g = scene(2000, 128, 96, 7)
    P = g["means3D"].shape[0]
    t = {k: leaf(v) for k, v in g.items()}
    m2 = torch.zeros(P, 3, device="cuda", requires_grad=True)
    color, radii, ex = GaussianRasterizer(settings(cam))(
        means3D=t["means3D"], means2D=m2, opacities=t["opacities"], colors_precomp=t["colors"], scales=t["scales"],
        rotations=t["rotations"], return_geometry=True, return_aux=True, contrib=True, features=leaf(np.ones((P, 2), np.float32)))
    assert set(ex) >= {"distortion", "median_depth", "median_id", "depth", "top_id", "features"} and "moments" not in ex
    assert ex["median_id"].requires_grad is False and ex["median_id"].grad_fn is None
    for k in ("distortion", "median_depth", "depth", "features"):
        assert ex[k].requires_grad and ex[k].grad_fn is color.grad_fn, k        # one autograd node
    assert ex["features"].shape == (2, 96, 128) and ex["top_id"].shape == (96, 128)
    saved = color.grad_fn.saved_tensors
    assert len(saved) == 14 and saved[-2].shape == (2, 96, 128) and saved[-1].dtype == torch.int32


def test_empty_view_and_no_gaussians():
    cam = look_at_camera((0.0, -3.0, 0.0), (0, 0, 0), 80, 64, fovx_deg=50.0)
    rs = settings(cam)
    g = random_gaussians(64, seed=6)
    g["means3D"][:, 1] -= 20.0                        # everything behind the camera
    for gg in (g, {k: v[:0] for k, v in g.items()}):
        out = _run(rs, gg, loss_w={"distortion": np.ones((1, 64, 80), np.float32), "median_depth": np.ones((1, 64, 80), np.float32)})
        assert out["distortion"].shape == (1, 64, 80) and bool((out["distortion"] == 0).all())
        assert bool((out["median_depth"] == 0).all()) and bool((out["median_id"] == -1).all())
        if gg["means3D"].shape[0]:
            assert bool((out["grad"]["means3D"] == 0).all())


# ---- render() ----------------------------------------------------------------------------------------------------------------
def _render(pc, cam, pipe, bg, **kw):
    from contextgs_amd import ctx_ops
    from contextgs_amd.renderer import prefilter_voxel, render
    torch.manual_seed(0)
    ctx_ops._seed_counter = itertools.count(1)       # the same noise streams in every call
    vis = prefilter_voxel(cam, pc, pipe, bg)
    return render(cam, pc, pipe, bg, visible_mask=vis, step=1000, **kw), vis


def test_render_returns_the_maps_and_the_backward_reaches_the_anchors():
    pc, cams, pipe, bg = model()
    pc.train(True)
    with torch.enable_grad():
        plain, _ = _render(pc, cams[1], pipe, bg)
        pkg, _ = _render(pc, cams[1], pipe, bg, return_geometry=True)
    assert torch.equal(pkg["render"].detach(), plain["render"].detach()) and torch.equal(pkg["radii"], plain["radii"])
    assert pkg["distortion"].shape == (1, 180, 320) and pkg["median_depth"].shape == (1, 180, 320)
    assert pkg["median_id"].shape == (180, 320) and pkg["median_id"].dtype == torch.int32
    assert pkg["median_id"].requires_grad is False and int(pkg["median_id"].max()) < pkg["radii"].shape[0]
    assert float(pkg["distortion"].detach().max()) > 0 and int((pkg["median_id"] >= 0).sum()) > 0
    for _, p in pc.named_parameters():
        p.grad = None
    (pkg["distortion"].mean() + pkg["median_depth"].mean()).backward()
    torch.cuda.synchronize()
    for name in ("_anchor", "_offset", "_anchor_feat", "_scaling"):
        gr = getattr(pc, name).grad
        assert gr is not None and torch.isfinite(gr).all() and float(gr.abs().sum()) > 0, name
    pc.train(False)
    with torch.no_grad():
        ev, _ = _render(pc, cams[1], pipe, bg, return_geometry=True)
    assert ev["distortion"].shape == (1, 180, 320) and ev["median_id"].dtype == torch.int32
