"""Gradients for the camera (viewmatrix, projmatrix, campos) on the GPU: csrc/raster_camera.hip through the drop-in rasterizer,
render() and the pose helper.  Every comparison prints its measured value before it asserts (run with -s); what has been
recorded is in profiles/raster_camera.txt.

Bounds.  GRAD_TOL = 2e-4 of the tensor's maximum is the project's standing gradient bound (tests/test_oracle_raster.py,
tests/test_raster_sh_cov_gpu.py).  It is used as it stands: test_every_entry_against_fp64_finite_differences also asserts that the
existing dL/dmeans3D of the same call, summed over Gaussians, misses the fp64 oracle's sum by no more than half of it, the
condition under which the bound is not to be widened."""
import math

import numpy as np
import pytest
import torch

from contextgs_amd.synth import look_at_camera, random_gaussians
from raster_harness import settings, sh_eval_torch, shs

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-4
BG = (0.2, 0.3, 0.1)


# ---- scenes of the finite-difference test (fp64 oracle, colours + scales / rotations) ----------------------------------------
def fd_scene(name):
    """(camera, Gaussians fp64, image weights fp64).  small3..5: the scene of tests/test_oracle_raster.py's
    test_fp64_finite_difference_gradients, seeds 3-5.  large: 2000 Gaussians at 160x120 (all visible, accumulated alpha up to
    0.74), checked on the CPU when this test was written: the central differences of the fp64 oracle with steps 1e-6 and 1e-7
    agree to 3.7e-8 (V) and 6.6e-9 (PM) of the tensor maximum on all 32 entries, i.e. no alpha >= 1/255 or T < 1e-4 decision
    flips inside either step (a scene of the small ones' Gaussian sizes at this count has a few such flips per entry, and seed 0
    of this recipe has one: they show as a disagreement of order 1)."""
    if name.startswith("small"):
        seed, W, H, P = int(name[5:]), 40, 32, 24
        g = random_gaussians(P, seed=seed, extent=0.6, scale_lo=0.03, scale_hi=0.12, dtype=np.float64)
        g["opacities"] = np.clip(g["opacities"], 0.05, 0.6)     # keep away from the 0.99 clamp
        cam = look_at_camera((0.0, -3.0, 0.4), (0, 0, 0), W, H, fovx_deg=50.0)
    else:
        seed, W, H, P = 1, 160, 120, 2000
        g = random_gaussians(P, seed=seed, extent=0.8, scale_lo=0.004, scale_hi=0.012, dtype=np.float64)
        g["opacities"] = np.random.default_rng(seed + 500).uniform(0.02, 0.3, size=(P, 1))
        cam = look_at_camera((0.0, -5.0, 0.8), (0, 0, 0), W, H, fovx_deg=50.0)
    w = np.random.default_rng(seed).normal(size=(3, H, W))
    return cam, g, w


def oracle_loss(oracle, cam, g, w, view=None, proj=None, grads=False):
    kw = cam.oracle_dict(bg=BG)
    if view is not None:
        kw["view"] = view
    if proj is not None:
        kw["proj"] = proj
    res = oracle.render(kw, means3D=g["means3D"], colors=g["colors"], opacities=g["opacities"], scales=g["scales"],
                        rots=g["rotations"], dL_dout=w if grads else None)
    return float((res["color"] * w).sum()), res


def oracle_camera_fd(oracle, cam, g, w, eps):
    """Central differences of the fp64 loss over all 16 + 16 matrix entries, each matrix an independent input."""
    V = np.asarray(cam.world_view_transform, dtype=np.float64).copy()
    PM = np.asarray(cam.full_proj_transform, dtype=np.float64).copy()
    out = []
    for which, M in (("view", V), ("proj", PM)):
        G = np.zeros((4, 4))
        for r in range(4):
            for c in range(4):
                old = M[r, c]
                M[r, c] = old + eps
                lp, _ = oracle_loss(oracle, cam, g, w, V, PM)
                M[r, c] = old - eps
                lm, _ = oracle_loss(oracle, cam, g, w, V, PM)
                M[r, c] = old
                G[r, c] = (lp - lm) / (2 * eps)
        out.append(G)
    return out


def _leaf32(a):
    return torch.tensor(np.asarray(a, dtype=np.float32), device="cuda", requires_grad=True)


def _const(a):
    return torch.tensor(np.asarray(a, dtype=np.float32), device="cuda")


def _rel(a, b):
    """max |a - b| / max |b|"""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


@pytest.mark.parametrize("name", ["small3", "small4", "small5", "large"])
def test_every_entry_against_fp64_finite_differences(oracle64, name):
    """All 32 entries of dL/dviewmatrix and dL/dprojmatrix against central differences of the fp64 oracle's forward (step 1e-6;
    no retry with a smaller step: the scenes are smooth at this step, see fd_scene)."""
    from contextgs_amd.rasterizer import GaussianRasterizer
    cam, g, w = fd_scene(name)
    fdV, fdPM = oracle_camera_fd(oracle64, cam, g, w, 1e-6)
    _, res = oracle_loss(oracle64, cam, g, w, grads=True)
    c = cam.to_torch("cuda")
    V, PM = c.world_view_transform.clone().requires_grad_(True), c.full_proj_transform.clone().requires_grad_(True)
    m3 = _leaf32(g["means3D"])
    P = m3.shape[0]
    color, radii = GaussianRasterizer(settings(cam, bg=BG, view=V, proj=PM))(
        means3D=m3, means2D=torch.zeros(P, 3, device="cuda", requires_grad=True), colors_precomp=_leaf32(g["colors"]),
        opacities=_leaf32(g["opacities"]), scales=_leaf32(g["scales"]), rotations=_leaf32(g["rotations"]))
    (color * _const(w)).sum().backward()
    assert V.grad is not None and PM.grad is not None, "the camera tensors got no gradient"
    assert V.grad.shape == (4, 4) and PM.grad.shape == (4, 4)
    eV, ePM = _rel(V.grad, fdV), _rel(PM.grad, fdPM)
    e_means = _rel(m3.grad.sum(dim=0), res["dL_dmeans3D"].sum(axis=0))
    print(f"[camera-fd] {name}: dV {eV:.3e} dPM {ePM:.3e} of the tensor maximum; sum_i dL/dmeans3D_i vs fp64 {e_means:.3e}")
    assert e_means <= 0.5 * GRAD_TOL, "the bound of this test is tied to the existing gradient's miss: see the module docstring"
    assert eV <= GRAD_TOL and ePM <= GRAD_TOL, (name, eV, ePM)
    assert not V.grad[:, 3].any() and not PM.grad[:, 2].any()
    assert np.all(fdV[:, 3] == 0) and np.all(fdPM[:, 2] == 0)


# ---- the identity render(p A + b, A^T Sigma A; V, PM) == render(p, Sigma; M V, M PM), M = [[A, 0], [b, 1]] ---------------------
def _big_scene(P=120_000, W=640, H=360, seed=21):
    cam = look_at_camera((0.4, -2.2, 0.6), (0, 0, 0), W, H, fovx_deg=60.0)
    g = random_gaussians(P, seed=seed, extent=1.0)
    eye = np.array([0.4, -2.2, 0.6], dtype=np.float32)
    g["means3D"][::20] = eye + 0.3 * (eye - g["means3D"][::20])        # some behind the near plane
    return cam, g


def _quat_to_rot(q):
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)


def _cov_full(scales, rotations):
    L = _quat_to_rot(rotations) * scales[:, None, :]
    return L @ L.transpose(1, 2)


def _cov6(S):
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=1)


def _quat_mul(a, b):
    ar, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    br, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return torch.stack([ar * br - ax * bx - ay * by - az * bz, ar * bx + ax * br + ay * bz - az * by,
                        ar * by - ax * bz + ay * br + az * bx, ar * bz + ax * by - ay * bx + az * br], dim=-1)


def _loss(out, aux, wc, wm, loss):
    total = 0.0
    if loss in ("colour", "both"):
        total = total + (out * wc).sum()
    if loss in ("maps", "both"):
        total = total + (aux["depth"] * wm[0]).sum() + (aux["invdepth"] * wm[1]).sum() + (aux["alpha"] * wm[2]).sum()
    return total


def _identity_sides(cam, g, form, aa, loss, wc, wm):
    """dL/dtheta at theta = 0 from the camera side and from the world side.  cov3D forms: theta = the 12 free entries of M.
    scales + rotations forms: theta = (rotation vector, log scale, translation), the rigid + uniform-scale subgroup, 7
    degrees of freedom (a general A does not map scales / rotations to scales / rotations).  SH forms use degree 0: SH colours of
    degree > 0 are not invariant under a rotation of the scene, the identity holds for view-independent colours only (the SH
    direction's own gradient is test_campos_*)."""
    from contextgs_amd.camera_pose import so3_exp
    from contextgs_amd.rasterizer import GaussianRasterizer
    c = cam.to_torch("cuda")
    V0, PM0 = c.world_view_transform, c.full_proj_transform
    p, s, q = _const(g["means3D"]), _const(g["scales"]), _const(g["rotations"])
    op = _const(g["opacities"])
    P = p.shape[0]
    cov_form, sh_form = form in ("cov", "shs+cov"), form in ("shs", "shs+cov")
    col = dict(colors_precomp=_const(g["colors"]))
    if sh_form:
        sh = torch.zeros(P, 4, 3, device="cuda")
        sh[:, 0] = (_const(g["colors"]) - 0.5) / 0.28209479177387814
        sh[:, 1:] = 0.3        # read by no degree-0 kernel
        col = dict(shs=sh)
    eye3 = torch.eye(3, device="cuda")

    def M_of(theta):
        if cov_form:
            A, b = theta[:9].view(3, 3) + eye3, theta[9:]
        else:
            A, b = so3_exp(theta[:3]).transpose(0, 1) * torch.exp(theta[3]), theta[4:]
        return A, b

    def run(theta, side):
        A, b = M_of(theta)
        geo, V, PM = {}, V0, PM0
        if side == "camera":
            M4 = torch.cat([torch.cat([A, torch.zeros(3, 1, device="cuda")], dim=1),
                            torch.cat([b, torch.ones(1, device="cuda")]).unsqueeze(0)], dim=0)
            V, PM = M4 @ V0, M4 @ PM0
            means = p
            geo = dict(cov3D_precomp=_cov6(_cov_full(s, q))) if cov_form else dict(scales=s, rotations=q)
        else:
            means = p @ A + b
            if cov_form:
                geo = dict(cov3D_precomp=_cov6(A.transpose(0, 1) @ _cov_full(s, q) @ A))
            else:       # A^T Sigma A = e^(2 k) B Sigma B^T with B = so3_exp(w): rotation quaternion (1, w / 2) to first order
                dq = torch.cat([torch.ones(1, device="cuda"), 0.5 * theta[:3]])
                dq = dq / dq.norm()
                geo = dict(scales=s * torch.exp(theta[3]), rotations=_quat_mul(dq.expand(P, 4), q))
        rs = settings(cam, bg=BG, D=0, aa=aa, view=V, proj=PM)
        out, radii, aux = GaussianRasterizer(rs)(means3D=means, means2D=torch.zeros(P, 3, device="cuda"), opacities=op,
                                                 return_aux=True, **col, **geo)
        _loss(out, aux, wc, wm, loss).backward()
        return theta.grad.detach().clone(), int((radii > 0).sum())

    n = 12 if cov_form else 7
    gc, vis = run(torch.zeros(n, device="cuda", requires_grad=True), "camera")
    gw, _ = run(torch.zeros(n, device="cuda", requires_grad=True), "world")
    return gc, gw, vis


@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("loss", ["colour", "maps", "both"])
@pytest.mark.parametrize("form", ["plain", "shs", "cov", "shs+cov"])
def test_identity_camera_side_equals_world_side(form, loss, aa):
    """Where the oracle cannot go (maps, antialiasing, the other forms, a size where the order of the blend's atomics matters):
    moving the camera by M equals moving the scene by M, so dL/dM through G_V V^T + G_PM PM^T (autograd through M V, M PM)
    equals dL/dM through the existing dL/dmeans3D and dL/dcov3D_precomp or dL/dscales, dL/drotations.  Both sides are fp32
    sums over the same blend gradients: GRAD_TOL of max |dL/dM|."""
    cam, g = _big_scene()
    gen = torch.Generator(device="cuda").manual_seed(5)
    wc = torch.randn(3, cam.image_height, cam.image_width, device="cuda", generator=gen)
    wm = torch.randn(3, 1, cam.image_height, cam.image_width, device="cuda", generator=gen) * 0.3
    gc, gw, vis = _identity_sides(cam, g, form, aa, loss, wc, wm)
    err = _rel(gc, gw)
    print(f"[camera-identity] form={form} loss={loss} aa={int(aa)}: visible {vis}, |camera - world| = {err:.3e} of max |dL/dM| "
          f"= {float(gw.abs().max()):.4e}")
    assert vis > 50_000 and float(gw.abs().max()) > 0
    assert err <= GRAD_TOL, (form, loss, aa, gc.tolist(), gw.tolist())


# ---- campos ----------------------------------------------------------------------------------------------------------------
def _sh_scene(D, M, P=120_000, W=640, H=360):
    cam, g = _big_scene(P, W, H, seed=22)
    return cam, g, shs(P, M, 22)


@pytest.mark.parametrize("cov_form", [False, True])
@pytest.mark.parametrize("D, M", [(1, 4), (2, 9), (3, 16), (1, 16)])
def test_campos_against_torch_sh(D, M, cov_form):
    """dL/dcampos of the SH forms against torch autograd through the torch SH evaluation that tests/test_raster_sh_cov_gpu.py
    compares with, feeding colors_precomp; and dL/dcampos == -sum_i of the SH direction's share of dL/dmeans3D (the difference
    between dL/dmeans3D of the shs call and of the colors_precomp call with the same colours)."""
    from contextgs_amd.rasterizer import GaussianRasterizer
    cam, g, sh = _sh_scene(D, M)
    P = sh.shape[0]
    s, q = _const(g["scales"]), _const(g["rotations"])
    geo = dict(cov3D_precomp=_cov6(_cov_full(s, q))) if cov_form else dict(scales=s, rotations=q)
    w = torch.randn(3, cam.image_height, cam.image_width, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    c0 = cam.to_torch("cuda").camera_center
    zeros = lambda: torch.zeros(P, 3, device="cuda")

    ca, ma, sha = c0.clone().requires_grad_(True), _leaf32(g["means3D"]), _const(sh)
    out, _ = GaussianRasterizer(settings(cam, bg=BG, D=D, campos=ca))(means3D=ma, means2D=zeros(), shs=sha,
                                                               opacities=_const(g["opacities"]), **geo)
    (out * w).sum().backward()
    assert ca.grad is not None and ca.grad.shape == (3,)

    cb, mb = c0.clone().requires_grad_(True), _leaf32(g["means3D"])
    colors = sh_eval_torch(sha, mb.detach(), cb, D)
    out_b, _ = GaussianRasterizer(settings(cam, bg=BG, D=D))(means3D=mb, means2D=zeros(), colors_precomp=colors,
                                                       opacities=_const(g["opacities"]), **geo)
    (out_b * w).sum().backward()
    e_torch = _rel(ca.grad, cb.grad)
    share = (ma.grad.double() - mb.grad.double()).sum(dim=0)
    e_share = _rel(ca.grad, -share)
    print(f"[camera-campos] D={D} M={M} cov={int(cov_form)}: vs torch SH {e_torch:.3e}, vs -sum of the direction share "
          f"{e_share:.3e} of max |dL/dcampos| = {float(cb.grad.abs().max()):.4e}")
    assert float(cb.grad.abs().max()) > 0
    assert e_torch <= GRAD_TOL and e_share <= GRAD_TOL, (e_torch, e_share)


def test_campos_without_shs_and_degree_zero():
    from contextgs_amd.rasterizer import GaussianRasterizer
    cam, g, sh = _sh_scene(0, 1, P=5000, W=128, H=96)
    P = sh.shape[0]
    kw = dict(means3D=_leaf32(g["means3D"]), opacities=_const(g["opacities"]), scales=_const(g["scales"]),
              rotations=_const(g["rotations"]))
    c = cam.to_torch("cuda").camera_center.clone().requires_grad_(True)
    out, _ = GaussianRasterizer(settings(cam, bg=BG, D=0, campos=c))(means2D=torch.zeros(P, 3, device="cuda"), shs=_const(sh), **kw)
    out.sum().backward()
    assert c.grad is not None and c.grad.shape == (3,) and not c.grad.any()      # degree 0 has no direction
    c2 = cam.to_torch("cuda").camera_center.clone().requires_grad_(True)
    out, _ = GaussianRasterizer(settings(cam, bg=BG, campos=c2))(means2D=torch.zeros(P, 3, device="cuda"),
                                                           colors_precomp=_const(g["colors"]), **kw)
    out.sum().backward()
    assert c2.grad is None                                                     # unused without shs


# ---- structure ---------------------------------------------------------------------------------------------------------------
def _plain_call(cam, g, w, view=None, proj=None, campos=None, aux=False, aa=False):
    from contextgs_amd.rasterizer import GaussianRasterizer
    leaves = {k: _leaf32(g[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations")}
    P = leaves["means3D"].shape[0]
    m2 = torch.zeros(P, 3, device="cuda", requires_grad=True)
    res = GaussianRasterizer(settings(cam, bg=BG, view=view, proj=proj, campos=campos, aa=aa))(
        means3D=leaves["means3D"], means2D=m2, colors_precomp=leaves["colors"], opacities=leaves["opacities"],
        scales=leaves["scales"], rotations=leaves["rotations"], return_aux=aux)
    (res[0] * w).sum().backward()
    torch.cuda.synchronize()
    leaves["means2D"] = m2
    return res[0].detach(), res[1], {k: v.grad.detach().clone() for k, v in leaves.items()}


def test_structure_transposed_leaves_and_single_tensors():
    """Separate backwards differ by the order of the blend's float atomics, so gradients of two calls are compared within
    what two repeats of the same call differ by (measured here), not bit for bit."""
    cam, g = _big_scene(20_000, 320, 200)
    w = torch.randn(3, 200, 320, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
    c = cam.to_torch("cuda")

    def both():
        V = c.world_view_transform.clone().requires_grad_(True)
        PM = c.full_proj_transform.clone().requires_grad_(True)
        _plain_call(cam, g, w, view=V, proj=PM)
        return V.grad, PM.grad

    (gV, gPM), (gV2, gPM2) = both(), both()
    floorV, floorPM = float((gV - gV2).abs().max()), float((gPM - gPM2).abs().max())
    print(f"[camera-structure] repeat floor dV {floorV:.3e} of {float(gV.abs().max()):.3e}, dPM {floorPM:.3e} of "
          f"{float(gPM.abs().max()):.3e}")

    def same(a, b, floor, ref):
        return float((a - b).abs().max()) <= max(4.0 * floor, 2e-5 * float(ref.abs().max()))

    assert not gV[:, 3].any() and not gPM[:, 2].any()          # never read: exactly 0
    assert gV[:, :3].abs().min() > 0 and gPM[:, [0, 1, 3]].abs().min() > 0
    # the layout scene/cameras.py builds: a leaf used through .transpose(0, 1) receives the transposed gradient
    Vt = c.world_view_transform.t().contiguous().requires_grad_(True)
    PMt = c.full_proj_transform.t().contiguous().requires_grad_(True)
    _plain_call(cam, g, w, view=Vt.transpose(0, 1), proj=PMt.transpose(0, 1))
    assert Vt.grad.shape == (4, 4) and same(Vt.grad, gV.t(), floorV, gV) and same(PMt.grad, gPM.t(), floorPM, gPM)
    assert not Vt.grad[3, :].any() and not PMt.grad[2, :].any()
    # one of the three alone
    V1 = c.world_view_transform.clone().requires_grad_(True)
    PM1 = c.full_proj_transform.clone()
    _plain_call(cam, g, w, view=V1, proj=PM1)
    assert same(V1.grad, gV, floorV, gV) and PM1.grad is None
    PM2 = c.full_proj_transform.clone().requires_grad_(True)
    V2 = c.world_view_transform.clone()
    _plain_call(cam, g, w, view=V2, proj=PM2)
    assert same(PM2.grad, gPM, floorPM, gPM) and V2.grad is None


def test_no_camera_gradient_leaves_the_call_as_it_was():
    """With no camera tensor requiring a gradient: outputs bit-identical to a call whose camera tensors do, and the
    per-Gaussian gradients agree within what two repeats of the same call differ by (float atomics in the blend)."""
    cam, g = _big_scene(60_000, 640, 360)
    w = torch.randn(3, 360, 640, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    c = cam.to_torch("cuda")
    img_a, radii_a, ga = _plain_call(cam, g, w)
    img_b, radii_b, gb = _plain_call(cam, g, w)
    V, PM = c.world_view_transform.clone().requires_grad_(True), c.full_proj_transform.clone().requires_grad_(True)
    img_c, radii_c, gcam = _plain_call(cam, g, w, view=V, proj=PM)
    assert torch.equal(img_a, img_b) and torch.equal(img_a, img_c) and torch.equal(radii_a, radii_c)
    for k in ga:
        floor = float((ga[k] - gb[k]).abs().max())
        diff = float((ga[k] - gcam[k]).abs().max())
        print(f"[camera-structure] {k}: repeat floor {floor:.3e}, with camera gradients {diff:.3e}")
        assert diff <= max(4.0 * floor, 2e-5 * float(ga[k].abs().max())), (k, diff, floor)


@pytest.mark.parametrize("case", ["empty", "all_culled", "one_pixel"])
def test_degenerate_views_give_zero_gradients_of_the_right_shape(case):
    from contextgs_amd.rasterizer import GaussianRasterizer
    W, H = (1, 1) if case == "one_pixel" else (64, 48)
    cam = look_at_camera((0.0, -3.0, 0.4), (0, 0, 0), W, H, fovx_deg=50.0)
    g = random_gaussians(0 if case == "empty" else 200, seed=1, extent=0.5)
    if case == "all_culled":
        g["means3D"][:, 1] -= 10.0          # behind the camera
    if case == "one_pixel":
        g["means3D"][:, 0] += 50.0          # far to the side: the one tile may list them (radii > 0), no splat reaches the pixel
    c = cam.to_torch("cuda")
    V, PM = c.world_view_transform.clone().requires_grad_(True), c.full_proj_transform.clone().requires_grad_(True)
    cp = c.camera_center.clone().requires_grad_(True)
    P = g["means3D"].shape[0]
    sh = torch.zeros(P, 4, 3, device="cuda")
    out, radii = GaussianRasterizer(settings(cam, bg=BG, view=V, proj=PM, campos=cp))(
        means3D=_const(g["means3D"]).reshape(P, 3), means2D=torch.zeros(P, 3, device="cuda"), shs=sh,
        opacities=_const(g["opacities"]).reshape(P, 1), scales=_const(g["scales"]).reshape(P, 3),
        rotations=_const(g["rotations"]).reshape(P, 4))
    if case == "one_pixel":
        assert out.shape == (3, 1, 1) and torch.equal(out.reshape(3), torch.tensor(BG, device="cuda"))     # the background alone
    else:
        assert not (radii > 0).any()
    out.sum().backward()
    for t, shape in ((V, (4, 4)), (PM, (4, 4)), (cp, (3,))):
        assert t.grad is not None and t.grad.shape == shape and not t.grad.any()


def test_c_entry_point_is_bit_reproducible_on_a_frozen_scratch():
    """Two calls of cgs_raster_camera_backward on the scratch one backward left, each with a work buffer of arbitrary contents:
    bit-equal (no float atomics)."""
    import ctypes as C
    from contextgs_amd import _lib, rasterizer
    cam, g = _big_scene(60_000, 640, 360)
    L = _lib.lib()
    c = cam.to_torch("cuda")
    rs = settings(cam, bg=BG)
    cfg = rasterizer._Cfg(rs)
    m, col, op, s, q = (_const(g[k]) for k in ("means3D", "colors", "opacities", "scales", "rotations"))
    P = m.shape[0]
    H, W = cam.image_height, cam.image_width
    stream = _lib.current_stream()
    radii = torch.empty(P, dtype=torch.int32, device="cuda")
    geom = rasterizer._workspace(L.cgs_raster_geom_bytes(P), "cuda")
    img = rasterizer._workspace(L.cgs_raster_img_bytes(H, W), "cuda")
    color = torch.empty(3, H, W, device="cuda")
    ticket = C.c_uint64(0)
    _lib.check(L.cgs_raster_preprocess_launch_opt(cfg.ref, P, _lib.ptr(m), _lib.ptr(col), None, 0, 0, _lib.ptr(op), _lib.ptr(s),
                                                  _lib.ptr(q), None, _lib.ptr(geom), geom.numel(), _lib.ptr(radii), stream,
                                                  C.byref(ticket), 0), "launch")
    binws, bin_R, _ = rasterizer.bin_and_blend(cfg, P, geom, img, color, stream, ticket)
    w = torch.randn(3, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(10))
    acc = torch.zeros(P * 4, device="cuda")
    rest = torch.empty(P * 13, device="cuda")
    scratch = rasterizer._workspace(L.cgs_raster_bwd_scratch_bytes(P), "cuda")
    _lib.check(L.cgs_raster_backward_ex(
        cfg.ref, P, bin_R, _lib.ptr(m), _lib.ptr(col), None, 0, 0, _lib.ptr(op), _lib.ptr(s), _lib.ptr(q), None, _lib.ptr(radii),
        _lib.ptr(geom), geom.numel(), _lib.ptr(binws), binws.numel(), _lib.ptr(img), img.numel(), _lib.ptr(w),
        rest[:3 * P].data_ptr(), rest[3 * P:6 * P].data_ptr(), acc.data_ptr(), acc[3 * P:].data_ptr(), None,
        rest[6 * P:9 * P].data_ptr(), rest[9 * P:].data_ptr(), None, _lib.ptr(scratch), scratch.numel(), stream), "backward")
    outs = []
    for _ in range(2):
        o = torch.full((32,), float("nan"), device="cuda")
        work = torch.randint(0, 255, (int(L.cgs_raster_camera_bytes(P)),), dtype=torch.uint8, device="cuda")   # any contents
        _lib.check(L.cgs_raster_camera_backward(cfg.ref, P, _lib.ptr(m), None, 0, 0, None, _lib.ptr(s), _lib.ptr(q), None,
                                                _lib.ptr(radii), _lib.ptr(scratch), scratch.numel(), None, None, 0,
                                                o[:16].data_ptr(), o[16:].data_ptr(), None, _lib.ptr(work), work.numel(), stream),
                   "camera")
        outs.append(o)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all() and outs[0].abs().max() > 0
    assert torch.equal(outs[0], outs[1])


# ---- render() and pose recovery ------------------------------------------------------------------------------------------------
def _render_setup(N=30000, hw=(270, 480), seed=0):
    import itertools
    from contextgs_amd import ctx_ops
    from contextgs_amd.synth import SynthPipe, make_scene, orbit_cameras
    torch.manual_seed(seed)
    ctx_ops._seed_counter = itertools.count(1)
    pc = make_scene(N, seed=seed)
    cam = orbit_cameras(4, hw[1], hw[0])[1].to_torch("cuda")
    return pc, cam, SynthPipe(), torch.tensor([0.1, 0.2, 0.3], device="cuda")


@pytest.mark.parametrize("training", [False, True])
def test_render_with_a_trainable_camera(training):
    """render(TrainableCamera(cam)) at xi = 0 against render(cam): the three camera tensors are the wrapped camera's bit for bit
    and the unfused path runs the fused path's device functions on the same values, so the image is bit-identical (what
    tests/test_fused_view_gpu.py asks of fused against unfused); xi.grad is finite and non-zero."""
    import itertools
    from contextgs_amd import ctx_ops
    from contextgs_amd.camera_pose import TrainableCamera
    from contextgs_amd.renderer import prefilter_voxel, render
    pc, cam, pipe, bg = _render_setup()
    pc.train(training)
    tc = TrainableCamera(cam)
    assert torch.equal(tc.world_view_transform, cam.world_view_transform)
    assert torch.equal(tc.full_proj_transform, cam.full_proj_transform) and torch.equal(tc.camera_center, cam.camera_center)
    w = torch.randn(3, cam.image_height, cam.image_width, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    images = []
    for camera in (cam, tc):
        torch.manual_seed(0)
        ctx_ops._seed_counter = itertools.count(1)       # the same noise streams in both calls (as tests/test_raster_aux_gpu.py)
        vis = prefilter_voxel(camera, pc, pipe, bg)
        pkg = render(camera, pc, pipe, bg, visible_mask=vis, step=1000)
        images.append(pkg["render"])
    assert torch.equal(images[0].detach(), images[1].detach())
    (images[1] * w).sum().backward()
    assert tc.xi.grad is not None and torch.isfinite(tc.xi.grad).all() and tc.xi.grad.abs().min() > 0, tc.xi.grad


def test_pose_recovery():
    """A target rendered at the true pose; the start is off by about a degree and 1 % of the scene extent; 60 Adam steps on xi
    alone with an L1 image loss.  Condition: the loss, the rotation error and the translation error each end strictly below
    their starting values.  The start / end values are printed."""
    from contextgs_amd.camera_pose import TrainableCamera, pose_tensors
    from contextgs_amd.renderer import prefilter_voxel, render
    pc, cam, pipe, bg = _render_setup()
    pc.eval()
    with torch.no_grad():
        vis = prefilter_voxel(cam, pc, pipe, bg)
        target = render(cam, pc, pipe, bg, visible_mask=vis)["render"].clone()
    tc = TrainableCamera(cam)
    extent = 2.0                # make_scene: anchors on the unit sphere and in [-1, 1]^3
    off = torch.tensor([0.012, -0.008, 0.006, 0.012, -0.01, 0.008], device="cuda")     # 0.9 degrees, 0.0175 = 0.9 % of the extent
    with torch.no_grad():
        tc.xi.copy_(off)

    def errors():
        # the pose error against the true camera: exp(xi) itself, since xi = 0 is the truth
        return tc.pose_delta()

    opt = torch.optim.Adam([tc.xi], lr=1e-3)
    rot0, tr0 = errors()
    losses = []
    for _ in range(60):
        opt.zero_grad(set_to_none=True)
        loss = (render(tc, pc, pipe, bg, visible_mask=vis)["render"] - target).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    with torch.no_grad():
        end = float((render(tc, pc, pipe, bg, visible_mask=vis)["render"] - target).abs().mean())
    rot1, tr1 = errors()
    print(f"[camera-recovery] L1 {losses[0]:.5e} -> {end:.5e}; rotation {math.degrees(rot0):.4f} -> {math.degrees(rot1):.4f} deg; "
          f"translation {tr0:.5f} -> {tr1:.5f} ({100 * tr0 / extent:.2f} % -> {100 * tr1 / extent:.2f} % of the extent)")
    assert end < losses[0] and rot1 < rot0 and tr1 < tr0, (losses[0], end, rot0, rot1, tr0, tr1)
