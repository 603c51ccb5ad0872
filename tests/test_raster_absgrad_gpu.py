"""GPU checks of the rasterizer's absolute screen-space gradients (`absgrad=True`, cgs_raster_backward_abs, the ABS instance of
csrc/raster_blend_rows.hip) against the UNCHANGED fp32 oracle.

The reference.  The oracle's dL_dmeans2D is linear in dL_dout and no forward decision depends on dL_dout, so a run with dL_dout
zeroed outside one pixel returns exactly that pixel's term dL_p/d(mean2D).  The reference for the absolute columns is therefore
the oracle called once per pixel with the absolute values of dL_dmeans2D[:, :2] summed (`_abs_ref`), computed once per scene and
shared.  On the CPU, on all five scenes, this fp32 reference against the same construction on the fp64 oracle has no entry
beyond 2e-4 of the maximum (worst 1.6e-6), the fp64 per-pixel sum reproduces the oracle's ordinary dL_dmeans2D to 1e-15, and the
absolute sums are 2.3-11 x the signed ones: a kernel that returned the signed gradient would fail every scene.

Tolerance: `_check_grad` of tests/test_raster_features_gpu.py, a copy: at most a 2e-3 share of entries beyond 2e-4 of the
tensor's maximum.

Scenes: the constructions of tests/test_raster_features_gpu.py (`_scene`, `_stack_scene`) at images small enough for a per-pixel
reference in 1-6 s, bg = (0.1, 0.25, 0.4), normal loss weights from default_rng(5)."""
import functools
import itertools

import numpy as np
import pytest
import torch

from contextgs_amd.synth import look_at_camera, random_gaussians

pytestmark = pytest.mark.gpu

BG = (0.1, 0.25, 0.4)
MAPS = ("depth", "invdepth", "alpha")
OTHER = (("dL_dmeans3D", "means3D"), ("dL_dopacities", "opacities"), ("dL_dscales", "scales"), ("dL_drotations", "rotations"),
         ("dL_dcolors", "colors"))
GRAD_TOL = 2e-4         # tests/test_raster_camera_gpu.py: of the tensor's maximum


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def _scene(P, W, H, seed, extent=1.0, srange=(0.005, 0.05)):
    cam = look_at_camera((0.4, -2.2, 0.6), (0, 0, 0), W, H, fovx_deg=60.0)
    g = random_gaussians(P, seed=seed, extent=extent, scale_lo=srange[0], scale_hi=srange[1])
    if P >= 20:     # some Gaussians behind the near plane
        eye = np.array([0.4, -2.2, 0.6], dtype=np.float32)
        g["means3D"][::20] = eye + 0.3 * (eye - g["means3D"][::20])
    return cam, g


def _stack_scene(kind, W, H):
    cam = look_at_camera((0.0, -3.0, 0.0), (0, 0, 0), W, H, fovx_deg=50.0)
    if kind == "saturated":
        rng = np.random.default_rng(11)
        g = random_gaussians(300, seed=11, extent=0.2, scale_lo=0.15, scale_hi=0.4)
        g["opacities"][:] = rng.uniform(0.9, 0.999, size=g["opacities"].shape).astype(np.float32)
    else:
        rng = np.random.default_rng(12)
        g = random_gaussians(700, seed=12, extent=0.2, scale_lo=0.15, scale_hi=0.4)
        g["opacities"][:] = rng.uniform(0.005, 0.02, size=g["opacities"].shape).astype(np.float32)
    return cam, g


SCENES = ("s1", "s64", "s300", "sat", "long")


@functools.lru_cache(maxsize=None)
def _named(name):
    return {"s1": lambda: _scene(1, 40, 24, 1),                              # one Gaussian, ragged 3 x 2 tile grid
            "s64": lambda: _scene(64, 40, 24, 64),                           # near-plane culls: rows that must be exactly 0
            "s300": lambda: _scene(300, 40, 24, 7, srange=(0.01, 0.12)),     # 565 pairs, mixed lists
            "sat": lambda: _stack_scene("saturated", 32, 16),                # every pixel stops early (the n_contrib bound)
            "long": lambda: _stack_scene("long", 24, 16)}[name]()           # 700-entry lists, three staged batches


def _loss_weights(H, W):
    return np.random.default_rng(5).normal(size=(3, H, W)).astype(np.float32)


_REFS = {}


def _abs_ref(oracle, name, w=None, key=None):
    """{"abs" [P,2], and the oracle's ordinary backward under the same weights}: computed once, nobody writes into it."""
    key = key or name
    if key not in _REFS:
        cam, g = _named(name)
        H, W = cam.image_height, cam.image_width
        w = _loss_weights(H, W) if w is None else w
        args = (cam.oracle_dict(bg=BG), g["means3D"], g["colors"], g["opacities"], g["scales"], g["rotations"])
        full = oracle.render(*args, dL_dout=w)
        acc = np.zeros((g["means3D"].shape[0], 2), np.float32)
        for y, x in itertools.product(range(H), range(W)):
            if not w[:, y, x].any():
                continue
            d = np.zeros_like(w)
            d[:, y, x] = w[:, y, x]
            acc += np.abs(oracle.render(*args, dL_dout=d)["dL_dmeans2D"][:, :2])
        _REFS[key] = dict(full, abs=acc)
    return _REFS[key]


# ---- running the rasterizer ---------------------------------------------------------------------------------------------------
def _settings(cam, bg=BG, D=1, aa=False, view=None, proj=None, debug=False):
    import math
    from contextgs_amd.rasterizer import GaussianRasterizationSettings
    c = cam.to_torch("cuda")
    return GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=torch.tensor(bg, dtype=torch.float32, device="cuda"), scale_modifier=1.0,
        viewmatrix=c.world_view_transform if view is None else view, projmatrix=c.full_proj_transform if proj is None else proj,
        sh_degree=D, campos=c.camera_center, prefiltered=False, debug=debug, antialiasing=aa)


def _leaf(a):
    return torch.tensor(a, device="cuda", requires_grad=True)


def _run(rs, g, loss_w, absgrad=True, F=None, return_aux=False, opacities=None):
    """Forward and the backward of sum(out * w) over the entries of loss_w (color / depth / invdepth / alpha / features)."""
    from contextgs_amd.rasterizer import GaussianRasterizer
    P = g["means3D"].shape[0]
    t = {k: _leaf(v) for k, v in g.items()}
    if F is not None:
        t["features"] = _leaf(F)
    m2 = torch.zeros(P, 4 if absgrad else 3, device="cuda", requires_grad=True)
    kw = dict(absgrad=True) if absgrad else {}
    res = GaussianRasterizer(rs)(means3D=t["means3D"], means2D=m2, opacities=t["opacities"] if opacities is None else opacities,
                                 colors_precomp=t["colors"], scales=t["scales"], rotations=t["rotations"],
                                 features=t.get("features"), return_aux=return_aux, **kw)
    out = {"color": res[0], "radii": res[1]}
    if len(res) > 2:
        out.update(res[2])
    sum(((out[k] * torch.as_tensor(w, device="cuda")).sum() for k, w in loss_w.items())).backward()
    torch.cuda.synchronize()
    o = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}
    o["grad"] = {k: (None if v.grad is None else v.grad.detach()) for k, v in t.items()}
    o["grad"]["means2D"] = m2.grad
    return o


def _check_grad(a, b, what, allow_frac=2e-3, tol=2e-4):
    a = a.detach().float().cpu().numpy().reshape(a.shape[0], -1) if torch.is_tensor(a) else a
    b = np.asarray(b, dtype=np.float32).reshape(a.shape)
    scale = max(1e-6, float(np.abs(b).max()))
    err = np.abs(a - b) / scale
    n_out = int((err > tol).sum())
    print(f"[allowance] {what}: {n_out} of {err.size} entries beyond {tol:g} of the maximum, worst {err.max():.2e}")
    assert n_out <= allow_frac * err.size, (what, n_out, float(err.max()))


# ---- 1, 2: the oracle and the invariants ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_matches_the_per_pixel_oracle(oracle32, name):
    cam, g = _named(name)
    H, W = cam.image_height, cam.image_width
    P = g["means3D"].shape[0]
    w = _loss_weights(H, W)
    ref = _abs_ref(oracle32, name)
    if name == "sat":
        assert float(ref["final_T"].min()) < 1e-3            # the stack saturates: pixels stopped on the 1e-4 test
    if name == "long":
        tiles = ((H + 15) // 16) * ((W + 15) // 16)
        assert float(ref["final_T"].min()) > 1e-4 and int(ref["stats"][1]) / tiles > 512      # three staged batches walked
    rs = _settings(cam, debug=(name == "s1"))                 # the smallest case with a synchronised check after every kernel
    out = _run(rs, g, {"color": w})
    plain = _run(rs, g, {"color": w}, absgrad=False)
    assert torch.equal(out["color"], plain["color"]) and torch.equal(out["radii"], plain["radii"])
    m2 = out["grad"]["means2D"]
    assert m2.shape == (P, 4) and m2.dtype == torch.float32
    ratio = float(ref["abs"].sum()) / max(float(np.abs(ref["dL_dmeans2D"][:, :2]).sum()), 1e-30)
    print(f"[absgrad] {name}: sum of the absolute columns / sum of |signed| = {ratio:.2f}")
    _check_grad(m2[:, 2:4], ref["abs"], f"absolute columns {name}")
    _check_grad(m2[:, 0:2], ref["dL_dmeans2D"][:, :2], f"signed columns {name}")
    for k, tname in OTHER:
        _check_grad(out["grad"][tname], ref[k], f"{k} {name}")
    # the signed columns are those of the call without the flag (float atomics: equal up to the order of the sums)
    _check_grad(m2[:, 0:2], plain["grad"]["means2D"][:, 0:2].cpu().numpy(), f"signed columns vs the call without the flag {name}")
    # invariants
    culled = (out["radii"] <= 0)
    assert (ref["radii"] <= 0).sum() == int(culled.sum())
    if name == "s64":
        assert int(culled.sum()) > 0
    assert bool((m2[culled] == 0).all())
    assert bool((m2[:, 2:4] >= 0).all())
    for c in (0, 1):
        slack = 1e-4 * float(m2[:, 2 + c].max())
        assert bool((m2[:, 2 + c] + slack >= m2[:, c].abs()).all()), c
    assert ratio > 1.5          # uncorrelated weights: the signed sum cancels, the absolute one does not


def test_one_pixel_has_nothing_to_cancel(oracle32):
    """s1 with loss weights that are non-zero at a single covered pixel: the absolute sum has one term."""
    cam, g = _named("s1")
    H, W = cam.image_height, cam.image_width
    fwd = _abs_ref(oracle32, "s1")
    y, x = np.unravel_index(int(np.argmin(fwd["final_T"])), (H, W))        # the pixel the Gaussian covers best
    assert float(fwd["final_T"][y, x]) < 0.99
    w = np.zeros((3, H, W), np.float32)
    w[:, y, x] = (0.7, -1.1, 0.4)
    m2 = _run(_settings(cam), g, {"color": w})["grad"]["means2D"]
    assert float(m2[:, 0:2].abs().max()) > 0
    assert torch.allclose(m2[:, 2:4], m2[:, 0:2].abs(), rtol=1e-5, atol=0.0)


# ---- 3: forms and options -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form, aa", [pytest.param(f, a, id=f + ("-aa" if a else "")) for a in (False, True)
                                      for f in ("shs+scales", "shs+cov", "colors+cov")])
def test_all_forms_match_colors_precomp_scales_rotations(form, aa):
    """aa: both sides with antialiasing, the ABS and AA instances of the form kernels against those of the plain kernel."""
    from contextgs_amd.rasterizer import GaussianRasterizer
    from test_raster_sh_cov_gpu import _shs, cov6_torch, sh_eval_torch
    P, W, H, D, M = 2000, 128, 96, 2, 9
    cam, g = _scene(P, W, H, P + 3)
    sh = _shs(P, M, seed=P)
    rs = _settings(cam, D=D, aa=aa)
    campos = rs.campos.float()
    w = torch.tensor(np.random.default_rng(5).normal(size=(3, H, W)).astype(np.float32), device="cuda")

    def run(use_shs, use_cov):
        t = {k: _leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
        t["shs"] = _leaf(sh)
        m2 = torch.zeros(P, 4, device="cuda", requires_grad=True)
        kw = dict(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], absgrad=True)
        if use_shs:
            kw["shs"] = t["shs"]
        else:         # the reference form: torch's SH into colors_precomp when the other side uses shs
            kw["colors_precomp"] = sh_eval_torch(t["shs"], t["means3D"], campos, D) if "shs" in form else t["colors"]
        if use_cov:
            kw["cov3D_precomp"] = cov6_torch(t["scales"], t["rotations"], 1.0)
        else:
            kw["scales"], kw["rotations"] = t["scales"], t["rotations"]
        color, radii = GaussianRasterizer(rs)(**kw)
        (color * w).sum().backward()
        torch.cuda.synchronize()
        return dict(radii=radii, m2=m2.grad)

    ref = run(False, False)
    new = run("shs" in form, "cov" in form)
    assert new["m2"].shape == (P, 4) and float(ref["m2"][:, 2:4].max()) > 0
    same = (ref["radii"] == new["radii"]).cpu()
    assert float(same.float().mean()) >= 1 - 1e-4
    rows = same.numpy()
    a, b = new["m2"].cpu().numpy()[rows], ref["m2"].cpu().numpy()[rows]
    _check_grad(a[:, 2:4], b[:, 2:4], f"absolute columns {form}{' aa' if aa else ''}")
    _check_grad(a[:, 0:2], b[:, 0:2], f"signed columns {form}{' aa' if aa else ''}")
    assert bool((new["m2"][new["radii"] <= 0] == 0).all())


def test_antialiasing_reads_the_compensated_opacity():
    from test_raster_antialias_gpu import h_torch, sigma_rs
    P, W, H = 2000, 128, 96
    cam, g = _scene(P, W, H, 7)
    w = _loss_weights(H, W)
    aa = _run(_settings(cam, aa=True), g, {"color": w})
    rs = _settings(cam)
    with torch.no_grad():
        m, s, r = (torch.tensor(g[k], device="cuda") for k in ("means3D", "scales", "rotations"))
        h, _ = h_torch(m, sigma_rs(s, r), rs)
        op = (torch.tensor(g["opacities"], device="cuda").double().reshape(P, -1) * h[:, None]).float().reshape(g["opacities"].shape)
    ref = _run(rs, g, {"color": w}, opacities=op)
    no = _run(rs, g, {"color": w})
    _check_grad(aa["grad"]["means2D"][:, 2:4], ref["grad"]["means2D"][:, 2:4].cpu().numpy(), "absolute columns, antialiasing")
    assert not torch.equal(no["grad"]["means2D"][:, 2:4], aa["grad"]["means2D"][:, 2:4])


# ---- 4: combinations ------------------------------------------------------------------------------------------------------------
def test_maps_and_features_stay_out_of_the_absolute_columns():
    P, W, H, C = 2000, 128, 96, 5
    cam, g = _scene(P, W, H, 7)
    rng = np.random.default_rng(23)
    wc = _loss_weights(H, W)
    F = rng.normal(size=(P, C)).astype(np.float32)
    loss_w = {"color": wc, "features": rng.normal(size=(C, H, W)).astype(np.float32)}
    loss_w.update({k: rng.normal(size=(1, H, W)).astype(np.float32) for k in MAPS})
    rs = _settings(cam)
    both = _run(rs, g, loss_w, F=F, return_aux=True)
    colour = _run(rs, g, {"color": wc})
    a, b = both["grad"]["means2D"], colour["grad"]["means2D"]
    _check_grad(a[:, 2:4], b[:, 2:4].cpu().numpy(), "absolute columns: colour + maps + features vs colour only")
    assert float((a[:, 0:2] - b[:, 0:2]).abs().max()) > 1e-2 * float(b[:, 0:2].abs().max())      # the signed ones carry it all
    assert both["grad"]["features"] is not None and float(both["grad"]["features"].abs().max()) > 0
    # without a gradient on the colour image the absolute columns are zero
    maps_only = _run(rs, g, {k: loss_w[k] for k in MAPS}, return_aux=True)
    assert bool((maps_only["grad"]["means2D"][:, 2:4] == 0).all()) and float(maps_only["grad"]["means2D"][:, 0:2].abs().max()) > 0


@pytest.mark.parametrize("aa", [False, True])
def test_camera_gradient_is_that_of_the_call_without_the_flag(aa):
    from contextgs_amd.rasterizer import GaussianRasterizer
    P, W, H = 2000, 160, 120
    cam, g = _scene(P, W, H, 13)
    w = torch.tensor(_loss_weights(H, W), device="cuda")
    c = cam.to_torch("cuda")

    def run(absgrad):
        V, PM = c.world_view_transform.clone().requires_grad_(True), c.full_proj_transform.clone().requires_grad_(True)
        rs = _settings(cam, view=V, proj=PM, aa=aa)
        t = {k: _leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
        m2 = torch.zeros(P, 4 if absgrad else 3, device="cuda", requires_grad=True)
        img, _ = GaussianRasterizer(rs)(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], colors_precomp=t["colors"],
                                        scales=t["scales"], rotations=t["rotations"], **(dict(absgrad=True) if absgrad else {}))
        (img * w).sum().backward()
        torch.cuda.synchronize()
        return V.grad, PM.grad, m2.grad

    (aV, aPM, am2), (bV, bPM, _) = run(True), run(False)
    assert am2.shape == (P, 4) and float(am2[:, 2:4].max()) > 0
    for name, a, b in (("viewmatrix", aV, bV), ("projmatrix", aPM, bPM)):
        rel = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
        print(f"[camera] dL/d{name}: absgrad vs plain {rel:.3e} of the tensor maximum")
        assert float(b.abs().max()) > 0 and rel <= GRAD_TOL, (name, rel)


# ---- 5: render() and the fused training node ------------------------------------------------------------------------------------
def _model(N=20000, W=320, H=180):
    from contextgs_amd.synth import SynthPipe, make_scene, orbit_cameras
    pc = make_scene(N, seed=0)
    cams = [c.to_torch("cuda") for c in orbit_cameras(4, W, H)]
    return pc, cams, SynthPipe(), torch.zeros(3, device="cuda")


def _train_view(pc, cam, pipe, bg, fuse, absgrad):
    from contextgs_amd import ctx_ops, renderer
    from contextgs_amd.renderer import prefilter_voxel, render
    torch.manual_seed(0)
    ctx_ops._seed_counter = itertools.count(1)       # the same noise streams in every call
    seen = []
    prev, renderer.FUSE_VIEW = renderer.FUSE_VIEW, fuse
    orig = renderer._ExpandRasterize.apply
    renderer._ExpandRasterize.apply = staticmethod(lambda *a: (seen.append(1), orig(*a))[1])
    try:
        vis = prefilter_voxel(cam, pc, pipe, bg)
        pkg = render(cam, pc, pipe, bg, visible_mask=vis, retain_grad=True, step=1000, **(dict(absgrad=True) if absgrad else {}))
        w = torch.randn(pkg["render"].shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
        (pkg["render"] * w).sum().backward()
        torch.cuda.synchronize()
    finally:
        renderer.FUSE_VIEW = prev
        renderer._ExpandRasterize.apply = orig
    assert bool(seen) == fuse           # the flag does not push a training view off the fused node
    return pkg, vis


def _expected_accum(pkg, vis, K, n_slots, cols):
    """What training_statis adds to offset_gradient_accum, in plain torch from columns `cols` of the same gradient."""
    g = pkg["viewspace_points"].grad
    slots = (torch.nonzero(vis)[:, 0][:, None] * K + torch.arange(K, device=vis.device)).reshape(-1)[pkg["selection_mask"].reshape(-1)]
    uf = pkg["visibility_filter"]
    want = torch.zeros(n_slots, dtype=torch.float32, device=vis.device)
    want[slots[uf]] = g[uf][:, cols[0]:cols[1]].norm(dim=1)
    return want


def test_fused_training_view_and_training_statis():
    pc, cams, pipe, bg = _model()
    pc.train()
    K = int(pc.n_offsets)
    fused, vis = _train_view(pc, cams[1], pipe, bg, True, True)
    unfused, _ = _train_view(pc, cams[1], pipe, bg, False, True)
    plain, _ = _train_view(pc, cams[1], pipe, bg, True, False)
    gf, gu, gp = (p["viewspace_points"].grad for p in (fused, unfused, plain))
    P = int(fused["radii"].shape[0])
    assert fused["viewspace_points"].shape == (P, 4) and gf.shape == (P, 4) and gu.shape == (P, 4) and gp.shape == (P, 3)
    assert torch.equal(fused["render"], unfused["render"]) and torch.equal(fused["render"], plain["render"])
    _check_grad(gf[:, 2:4], gu[:, 2:4].cpu().numpy(), "absolute columns, fused vs unfused")
    _check_grad(gf[:, 0:2], gu[:, 0:2].cpu().numpy(), "signed columns, fused vs unfused")
    _check_grad(gf[:, 0:2], gp[:, 0:2].cpu().numpy(), "signed columns, with vs without the flag")
    assert float(gf[:, 2:4].sum()) > 1.5 * float(gf[:, 0:2].abs().sum())
    N = pc.get_anchor.shape[0]          # the four statistics buffers as training_setup creates them
    pc.opacity_accum, pc.anchor_demon = torch.zeros(N, 1, device="cuda"), torch.zeros(N, 1, device="cuda")
    pc.offset_gradient_accum, pc.offset_denom = torch.zeros(N * K, 1, device="cuda"), torch.zeros(N * K, 1, device="cuda")
    for pkg, cols in ((fused, (2, 4)), (plain, (0, 2))):
        before = pc.offset_gradient_accum.clone()
        denom = pc.offset_denom.clone()
        pc.training_statis(pkg["viewspace_points"], pkg["neural_opacity"], pkg["visibility_filter"], pkg["selection_mask"], vis)
        torch.cuda.synchronize()
        got = (pc.offset_gradient_accum - before).reshape(-1)
        want = _expected_accum(pkg, vis, K, got.shape[0], cols)
        assert float(want.max()) > 0
        assert float((got - want).abs().max()) <= 1e-6 * float(want.max()), cols
        assert int((pc.offset_denom - denom).sum()) == int(pkg["visibility_filter"].sum())


# ---- 6: empty cases -------------------------------------------------------------------------------------------------------------
def test_empty_inputs_give_zero_gradients():
    cam = look_at_camera((0.0, -3.0, 0.0), (0, 0, 0), 80, 64, fovx_deg=50.0)
    rs = _settings(cam)
    g = random_gaussians(64, seed=6)
    g["means3D"][:, 1] -= 20.0                        # everything behind the camera
    for gg in (g, {k: v[:0] for k, v in g.items()}):
        P = gg["means3D"].shape[0]
        out = _run(rs, gg, {"color": torch.ones(3, 64, 80, device="cuda")})
        assert int((out["radii"] > 0).sum()) == 0
        m2 = out["grad"]["means2D"]
        assert m2.shape == (P, 4) and bool((m2 == 0).all())
        assert bool((out["grad"]["means3D"] == 0).all())
