"""GPU checks of the rasterizer's N-channel feature blend (csrc/raster_feat.hip) against the existing fp32 oracle.

The feature map is the colour blend of the table's columns with a zero background, so the oracle renders the table three
columns at a time as `colors` (the last group zero-padded) with bg = 0: `color` of a group is that group of the map,
`dL_dcolors` that group of dL/dfeatures, and the geometry gradients are the sum over the groups (plus the ordinary colour run
and the maps' run of tests/test_raster_aux_gpu.py when those are in the loss).  Tolerances are those of
tests/test_raster_aux_gpu.py, unchanged (`check_map`, `check_grad` of tests/raster_harness.py): maps RMSE <= 1e-5 of the map's
maximum and at most a 1e-4 share of values beyond 2e-5; gradients at most a 2e-3 share of entries beyond 2e-4 of the tensor's
maximum.

Scenes.  Every scene below with an oracle comparison was first run on the CPU with the fp32 oracle against the fp64 oracle
under the same two checks, and kept only because the fp32 oracle alone stays within HALF of those shares there (map RMSE
<= 5e-6 and a <= 5e-5 share beyond 2e-5; gradients a <= 1e-3 share beyond 2e-4), at every C the test uses.
References are computed once per (scene, C) and shared between the tests and loss sets that need them.
"""
import itertools

import numpy as np
import pytest
import torch

from contextgs_amd.synth import look_at_camera, random_gaussians
from raster_harness import (BG, aux_colors, check_grad, check_map, cov6_torch, leaf, memo, model, run, scene, settings,
                            sh_eval_torch, shs, stack_scene, view_z)

pytestmark = pytest.mark.gpu

MAPS = ("depth", "invdepth", "alpha")
GEOM = (("dL_dmeans3D", "means3D"), ("dL_dmeans2D", "means2D"), ("dL_dopacities", "opacities"), ("dL_dscales", "scales"),
        ("dL_drotations", "rotations"))
CMAX = 32


def _table(P, seed, C=CMAX):
    """Signed features; the table of a smaller C is the first C columns of the 32-column one."""
    return np.random.default_rng(1000 + seed).normal(size=(P, CMAX)).astype(np.float32)[:, :C].copy()


def _weights(H, W, seed, C=CMAX):
    return np.random.default_rng(2000 + seed).normal(size=(CMAX, H, W)).astype(np.float32)[:C].copy()


# ---- the oracle, three columns at a time ---------------------------------------------------------------------------------------
def oracle_features(oracle, cam, g, F, dl=None):
    """{"map" [C,H,W], "final_T", "radii", "stats"} and, with dl [C,H,W], "dL_dfeatures" [P,C] and the five geometry
    gradients summed over the groups."""
    P, C = F.shape
    H, W = cam.image_height, cam.image_width
    out = {"map": np.zeros((C, H, W), F.dtype), "dL_dfeatures": np.zeros((P, C), F.dtype)}
    for c0 in range(0, C, 3):
        n = min(3, C - c0)
        cols = np.zeros((P, 3), F.dtype)
        cols[:, :n] = F[:, c0:c0 + n]
        d = None
        if dl is not None:
            d = np.zeros((3, H, W), F.dtype)
            d[:n] = dl[c0:c0 + n]
        r = oracle.render(cam.oracle_dict(bg=(0.0, 0.0, 0.0)), g["means3D"], cols, g["opacities"], g["scales"], g["rotations"],
                          dL_dout=d)
        out["map"][c0:c0 + n] = r["color"][:n]
        out.update(final_T=r["final_T"], radii=r["radii"], stats=r["stats"])
        if dl is not None:
            out["dL_dfeatures"][:, c0:c0 + n] = r["dL_dcolors"][:, :n]
            for k, _ in GEOM:
                out[k] = out.get(k, 0.0) + r[k]
    return out


def _fwd_ref(oracle, name, cam, g, seed):
    P = g["means3D"].shape[0]
    return memo(("features", "fwd", name), lambda: oracle_features(oracle, cam, g, _table(P, seed)))


def _bwd_ref(oracle, name, cam, g, seed, C):
    P = g["means3D"].shape[0]
    H, W = cam.image_height, cam.image_width
    return memo(("features", "bwd", name, C),
                lambda: oracle_features(oracle, cam, g, _table(P, seed, C), dl=_weights(H, W, seed, C)))


# ---- running the rasterizer ---------------------------------------------------------------------------------------------------
def _run(rs, g, F=None, **kw):
    """raster_harness.run with the feature table F."""
    return run(rs, g, features=F, **kw)


def _check_all_grads(out, exp, ref_f, what):
    for k, t in GEOM:
        check_grad(out["grad"][t], exp[k], f"{k} {what}")
    check_grad(out["grad"]["features"], ref_f["dL_dfeatures"], f"dL_dfeatures {what}")


# ---- forward ------------------------------------------------------------------------------------------------------------------
FWD_CASES = [(1, 64, 48), (64, 128, 96), (4000, 256, 256)]


@pytest.mark.parametrize("P, W, H", FWD_CASES)
@pytest.mark.parametrize("C", [1, 3, 5, 8, 17, 32])
def test_forward_matches_the_oracle(oracle32, P, W, H, C):
    cam, g = scene(P, W, H, P)
    ref = _fwd_ref(oracle32, f"scene{P}", cam, g, P)
    rs = settings(cam, debug=(P == 1))          # the smallest case with a synchronised check after every kernel
    out = _run(rs, g, F=_table(P, P, C))
    plain = _run(rs, g)
    # no interference: the colour image and radii are those of the plain call, bit for bit
    assert torch.equal(out["color"], plain["color"]) and torch.equal(out["radii"], plain["radii"])
    assert (out["radii"].cpu().numpy() == ref["radii"]).all()
    assert out["features"].shape == (C, H, W) and out["features"].dtype == torch.float32
    scale = float(np.abs(ref["map"][:C]).max())
    for c in range(C):      # per channel, each against the whole map's maximum
        a = out["features"][c].cpu().numpy()
        assert np.abs(a - ref["map"][c]).max() <= 1e-3 * max(scale, 1e-12), c      # (a wrong channel is off by order 1)
    check_map(out["features"], ref["map"][:C], f"features P={P} C={C}")


# ---- backward -----------------------------------------------------------------------------------------------------------------
BWD_CASES = [(200, 64, 48, 0, 1.0, (0.005, 0.05)), (3000, 256, 256, 1, 1.0, (0.003, 0.04))]
LOSSES = [("features",), ("color", "features"), ("color", "depth", "invdepth", "alpha", "features")]


def _colour_ref(oracle, name, cam, g, gC):
    return memo(("features", "colour", name),
                lambda: oracle.render(cam.oracle_dict(bg=BG), g["means3D"], g["colors"], g["opacities"], g["scales"], g["rotations"],
                                      dL_dout=gC))


def _aux_ref(oracle, name, cam, g, gm):
    def make():
        z, dz = view_z(cam, g["means3D"])
        ra = oracle.render(cam.oracle_dict(bg=(0.0, 0.0, 0.0)), g["means3D"], aux_colors(z), g["opacities"], g["scales"],
                           g["rotations"], dL_dout=np.concatenate([gm[k] for k in MAPS], 0))
        zs = np.where(z > 0.2, z, 1.0).astype(np.float32)
        ra = dict(ra)
        ra["dL_dmeans3D"] = ra["dL_dmeans3D"] + (ra["dL_dcolors"][:, 0] - ra["dL_dcolors"][:, 1] / (zs * zs))[:, None] * dz[None, :]
        return ra
    return memo(("features", "aux", name), make)


@pytest.mark.parametrize("P, W, H, seed, extent, srange", BWD_CASES)
@pytest.mark.parametrize("C", [1, 5, 32])
@pytest.mark.parametrize("keys", LOSSES, ids=["+".join(k) for k in LOSSES])
def test_backward_matches_the_oracle(oracle32, P, W, H, seed, extent, srange, C, keys):
    cam, g = scene(P, W, H, seed, extent, srange)
    name = f"bwd{P}"
    rf = _bwd_ref(oracle32, name, cam, g, seed, C)
    rng = np.random.default_rng(seed + 17)
    gC = rng.normal(size=(3, H, W)).astype(np.float32)
    gm = {k: rng.normal(size=(1, H, W)).astype(np.float32) for k in MAPS}
    loss_w = {k: (_weights(H, W, seed, C) if k == "features" else gC if k == "color" else gm[k]) for k in keys}
    out = _run(settings(cam), g, F=_table(P, seed, C), return_aux="depth" in keys, loss_w=loss_w)

    exp = {k: rf[k] for k, _ in GEOM}
    if "color" in keys:
        rc = _colour_ref(oracle32, name, cam, g, gC)
        exp = {k: exp[k] + rc[k] for k in exp}
    if "depth" in keys:
        ra = _aux_ref(oracle32, name, cam, g, gm)
        exp = {k: exp[k] + ra[k] for k in exp}
    _check_all_grads(out, exp, rf, f"P={P} C={C} {'+'.join(keys)}")
    if "color" in keys:
        check_grad(out["grad"]["colors"], rc["dL_dcolors"], f"dL_dcolors P={P}")
    else:
        assert out["grad"]["colors"] is None          # the features send nothing to the colour input
    assert float(out["grad"]["means3D"].abs().sum()) > 0


# ---- regimes ------------------------------------------------------------------------------------------------------------------
def test_lists_longer_than_one_staged_batch(oracle32):
    """The oracle's stats are [(tile, Gaussian) pairs, pairs the blend loops visited (per tile: the maximum over its pixels)],
    so "more than two 256-entry batches per tile" is stats[0] over the number of tiles (here 638 entries per tile; the ratio
    stats[0] / stats[1] is near 1 in any scene).  The kernels walk up to the last visited entry (464 per tile here, no pixel
    stopped early): also asserted to lie beyond the first batch."""
    C = 5
    cam, g = stack_scene("long", 64, 48)
    P, H, W = g["means3D"].shape[0], cam.image_height, cam.image_width
    tiles = ((H + 15) // 16) * ((W + 15) // 16)
    rf = _bwd_ref(oracle32, "long", cam, g, 12, C)
    assert float(rf["final_T"].min()) > 1e-4                       # no pixel stopped early
    assert int(rf["stats"][0]) / tiles > 512                       # more than two 256-entry batches per tile
    assert int(rf["stats"][1]) / tiles > 256                       # and the walk goes beyond the first
    out = _run(settings(cam), g, F=_table(P, 12, C), loss_w={"features": _weights(H, W, 12, C)})
    check_map(out["features"], rf["map"], "features, long lists")
    _check_all_grads(out, rf, rf, "long lists")


def test_saturated_stack(oracle32):
    cam, g = stack_scene("saturated", 64, 48)
    ref = memo(("features", "fwd", "saturated"), lambda: oracle_features(oracle32, cam, g, g["colors"]))
    assert float(ref["final_T"].min()) < 1e-3         # the stack saturates: pixels stopped on the 1e-4 test
    out = _run(settings(cam, bg=(0.0, 0.0, 0.0)), g, F=g["colors"])
    check_map(out["features"], ref["map"], "features saturated")
    scale = float(out["color"].abs().max())
    assert float((out["features"] - out["color"]).abs().max()) <= 1e-6 * scale


def test_ragged_image(oracle32):
    P, W, H, C = 500, 65, 47, 5
    cam, g = scene(P, W, H, 4)
    rf = _bwd_ref(oracle32, "ragged", cam, g, 4, C)
    out = _run(settings(cam), g, F=_table(P, 4, C), loss_w={"features": _weights(H, W, 4, C)})
    check_map(out["features"], rf["map"], "features 65x47")
    _check_all_grads(out, rf, rf, "65x47")


def test_empty_inputs_give_zero_maps_and_gradients():
    C = 4
    cam = look_at_camera((0.0, -3.0, 0.0), (0, 0, 0), 80, 64, fovx_deg=50.0)
    rs = settings(cam)
    g = random_gaussians(64, seed=6)
    g["means3D"][:, 1] -= 20.0                        # everything behind the camera
    for gg in (g, {k: v[:0] for k, v in g.items()}):
        P = gg["means3D"].shape[0]
        out = _run(rs, gg, F=_table(64, 6, C)[:P], loss_w={"features": torch.ones(C, 64, 80, device="cuda")})
        assert out["features"].shape == (C, 64, 80) and bool((out["features"] == 0).all())
        assert int((out["radii"] > 0).sum()) == 0
        assert bool((out["grad"]["means3D"] == 0).all())
        assert out["grad"]["features"].shape == (P, C) and bool((out["grad"]["features"] == 0).all())


def test_forward_after_a_voided_speculative_render(oracle32):
    from contextgs_amd import rasterizer
    P, W, H, C = 20000, 320, 240, 5
    cam, g = scene(P, W, H, 9)
    F = _table(P, 9, C)
    ref = oracle_features(oracle32, cam, g, F)
    rs = settings(cam)
    rasterizer._pair_capacity[(H, W)] = 1 << 10       # far below the view's pair count: the speculative render is voided
    out = _run(rs, g, F=F)
    assert rasterizer.last_call["num_rendered"] > (1 << 10)
    assert rasterizer.last_call["bin_R"] == rasterizer.last_call["num_rendered"]     # re-rendered with the true count
    check_map(out["features"], ref["map"], "features re-rendered")
    again = _run(rs, g, F=F)                              # now with a capacity that holds: the speculative render stands
    assert torch.equal(again["features"], out["features"])


# ---- one walk for every instance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ragged 40x24", "long lists"])
def test_a_channel_is_the_same_bits_in_every_instance(which):
    """One fixed column, blended as channel 0 of tables with C = 1, 5, 9, 17 (the 4-, 8-, 16- and 32-channel instances of the
    forward kernel) whose other columns are random: channel 0 of the four maps is bit-identical, because every instance walks
    the same entries in the same order and adds with the same fmaf.  Ragged tiles (40x24 = 3 x 2 tiles, cut right and bottom),
    and the scene with more than two 256-entry batches per tile."""
    cam, g = scene(200, 40, 24, 3, 1.0, (0.02, 0.12)) if which.startswith("ragged") else stack_scene("long", 64, 48)
    P = g["means3D"].shape[0]
    rs = settings(cam)
    f = _table(P, 77, 1)
    maps = {}
    for C in (1, 5, 9, 17):
        F = np.concatenate([f, _table(P, 78 + C, C - 1)], 1) if C > 1 else f
        maps[C] = _run(rs, g, F=F)["features"]
        assert maps[C].shape == (C, cam.image_height, cam.image_width)
    assert float(maps[1].abs().max()) > 0
    for C in (5, 9, 17):
        assert torch.equal(maps[C][0], maps[1][0]), C


# ---- the four argument forms --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["shs+scales", "shs+cov", "colors+cov"])
def test_all_forms_match_colors_precomp_scales_rotations(form):
    from contextgs_amd.rasterizer import GaussianRasterizer
    P, W, H, C, D, M = 4000, 256, 256, 5, 2, 9
    cam, g = scene(P, W, H, P + 3)
    sh = shs(P, M, seed=P)
    rs = settings(cam, D=D)
    campos = rs.campos.float()
    F = _table(P, 5, C)
    w = {"color": torch.tensor(np.random.default_rng(5).normal(size=(3, H, W)).astype(np.float32), device="cuda"),
         "features": torch.tensor(_weights(H, W, 5, C), device="cuda")}

    def run(use_shs, use_cov):
        t = {k: leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
        t["shs"], t["features"] = leaf(sh), leaf(F)
        m2 = torch.zeros(P, 3, device="cuda", requires_grad=True)
        kw = dict(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], features=t["features"])
        if use_shs:
            kw["shs"] = t["shs"]
        else:         # the reference form: torch's SH into colors_precomp when the other side uses shs
            kw["colors_precomp"] = sh_eval_torch(t["shs"], t["means3D"], campos, D) if "shs" in form else t["colors"]
        if use_cov:
            kw["cov3D_precomp"] = cov6_torch(t["scales"], t["rotations"], 1.0)
        else:
            kw["scales"], kw["rotations"] = t["scales"], t["rotations"]
        color, radii, extras = GaussianRasterizer(rs)(**kw)
        ((color * w["color"]).sum() + (extras["features"] * w["features"]).sum()).backward()
        torch.cuda.synchronize()
        o = dict(color=color.detach(), radii=radii, m2=m2.grad, fmap=extras["features"].detach())
        o.update({k: t[k].grad for k in t})
        return o

    ref = run(False, False)
    new = run("shs" in form, "cov" in form)
    same = (ref["radii"] == new["radii"]).cpu()
    assert float(same.float().mean()) >= 1 - 1e-4
    for k in ("color", "fmap"):
        check_map(new[k], ref[k].cpu().numpy(), f"{k} {form}")
    rows = same.numpy()
    allow = 1e-4 if "cov" in form else 0.0
    for k in ("means3D", "opacities", "scales", "rotations", "m2", "features") + (("shs",) if "shs" in form else ("colors",)):
        a, b = new[k].cpu().numpy(), ref[k].cpu().numpy()
        check_grad(a[rows].reshape(int(rows.sum()), -1), b[rows].reshape(int(rows.sum()), -1), f"d{k} {form}",
                    allow_frac=max(allow, 2e-3))


# ---- antialiasing -------------------------------------------------------------------------------------------------------------
def test_antialiasing_reads_the_compensated_opacity():
    P, W, H, C = 2000, 128, 96, 5
    cam, g = scene(P, W, H, 7)
    rs = settings(cam, aa=True)
    F = _table(P, 7, C)
    F[:, 2] = 1.0                                   # a column of ones blends to the alpha map
    out = _run(rs, g, F=F, return_aux=True)
    check_map(out["features"][2], out["alpha"].cpu().numpy(), "ones column vs alpha, antialiasing, C=5")
    ones = np.ones((P, 1), np.float32)
    w = _weights(H, W, 7, 1)
    a = _run(rs, g, F=ones, return_aux=True, loss_w={"features": w})
    b = _run(rs, g, F=ones, return_aux=True, loss_w={"alpha": w})
    check_map(a["features"], a["alpha"].cpu().numpy(), "ones [P,1] vs alpha, antialiasing")
    check_grad(a["grad"]["opacities"], b["grad"]["opacities"].cpu().numpy(), "dL_dopacities features vs alpha, antialiasing")
    for k in ("means3D", "scales", "rotations", "means2D"):
        check_grad(a["grad"][k], b["grad"][k].cpu().numpy(), f"d{k} features vs alpha, antialiasing")
    no_aa = _run(settings(cam), g, F=ones)
    assert not torch.equal(no_aa["features"], a["features"])


# ---- camera gradients ---------------------------------------------------------------------------------------------------------
def test_camera_gradients_equal_those_of_the_colour_blend_of_the_table():
    from contextgs_amd.rasterizer import GaussianRasterizer
    GRAD_TOL = 2e-4         # tests/test_raster_camera_gpu.py: of the tensor's maximum
    P, W, H, C = 2000, 160, 120, 3
    cam, g = scene(P, W, H, 13)
    F = _table(P, 13, C)
    w = torch.tensor(_weights(H, W, 13, C), device="cuda")
    c = cam.to_torch("cuda")

    def run(as_features):
        V, PM = c.world_view_transform.clone().requires_grad_(True), c.full_proj_transform.clone().requires_grad_(True)
        rs = settings(cam, bg=(0.0, 0.0, 0.0), view=V, proj=PM)
        t = {k: leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations")}
        kw = dict(means3D=t["means3D"], means2D=torch.zeros(P, 3, device="cuda", requires_grad=True), opacities=t["opacities"],
                  scales=t["scales"], rotations=t["rotations"])
        if as_features:
            _, _, ex = GaussianRasterizer(rs)(colors_precomp=leaf(g["colors"]), features=leaf(F), **kw)
            img = ex["features"]
        else:
            img, _ = GaussianRasterizer(rs)(colors_precomp=leaf(F), **kw)
        (img * w).sum().backward()
        torch.cuda.synchronize()
        return V.grad, PM.grad

    (fV, fPM), (cV, cPM) = run(True), run(False)
    assert fV is not None and fPM is not None
    for name, a, b in (("viewmatrix", fV, cV), ("projmatrix", fPM, cPM)):
        rel = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
        print(f"[camera] dL/d{name}: features vs colour blend {rel:.3e} of the tensor maximum")
        assert float(b.abs().max()) > 0 and rel <= GRAD_TOL, (name, rel)


# ---- render() -----------------------------------------------------------------------------------------------------------------
def _render(pc, cam, pipe, bg, **kw):
    from contextgs_amd import ctx_ops
    from contextgs_amd.renderer import prefilter_voxel, render
    torch.manual_seed(0)
    ctx_ops._seed_counter = itertools.count(1)       # the same noise streams in every call
    vis = prefilter_voxel(cam, pc, pipe, bg)
    return render(cam, pc, pipe, bg, visible_mask=vis, step=1000, **kw), vis


@pytest.mark.parametrize("training", [False, True])
def test_render_blends_anchor_features(training):
    pc, cams, pipe, bg = model()
    pc.train(training)
    N = pc.get_anchor.shape[0]
    af = torch.ones(N, 1, device="cuda", requires_grad=training)
    with (torch.enable_grad() if training else torch.no_grad()):
        plain, _ = _render(pc, cams[1], pipe, bg)
        aux, _ = _render(pc, cams[1], pipe, bg, return_aux=True)
        pkg, vis = _render(pc, cams[1], pipe, bg, anchor_features=af)
    for k in plain:
        assert k in pkg, k
    assert pkg["features"].shape == (1, 180, 320) and pkg["features"].dtype == torch.float32
    assert torch.equal(pkg["render"].detach(), plain["render"].detach())
    assert torch.equal(pkg["radii"], plain["radii"])
    check_map(pkg["features"], aux["alpha"].detach().cpu().numpy(), f"render() features of ones vs alpha, training={training}")
    assert float(pkg["features"].max()) > 0.5
    if training:
        pkg["features"].sum().backward()
        gr = af.grad
        assert gr is not None and bool(torch.isfinite(gr).all()) and bool((gr >= 0).all())
        assert bool((gr[~vis] == 0).all()) and float(gr[vis].sum()) > 0
        total, want = float(gr.double().sum()), float(pkg["features"].detach().double().sum())
        print(f"[render] sum of dL/danchor_features {total:.6f} vs sum of the map {want:.6f}")
        assert abs(total - want) <= 1e-4 * abs(want)
