"""What the rasterizer's tests share: scenes, settings, one run (forward, backward, collect), the checks, the torch-side
reference maths and the fake configuration of the CPU argument checks.  A plain module, imported by bare name like
raster_geom_ref; it imports without a GPU (torch.cuda is touched inside functions only).  tests/test_raster_harness.py pins
the scenes' bytes and the checks' boundaries.

Scenes.  `scene`: a look-at camera over `random_gaussians`, every 20th Gaussian pushed behind the near plane.  `stack_scene`:
the `saturated` (300 nearly opaque, wide Gaussians) and `long` (700 faint, wide ones) stacks.  `named_scene`: `ragged` (200
Gaussians at 40x24: 3x2 tiles, ragged right and bottom edges, some Gaussians behind the near plane), `single` (1 Gaussian at
64x48), and `long` and `saturated` over one 16x16 tile.  Each is built once; every caller gets arrays of its own, and the camera,
which nobody writes to, is shared.

Tolerances.  Maps (`check_map`): RMSE <= 1e-5 of the map's maximum and at most a 1e-4 share of values beyond 2e-5.  Gradients
(`check_grad`): at most a 2e-3 share of entries beyond 2e-4 of the tensor's maximum.  These caps are conditions, not
measurements: every scene with an oracle comparison was first run on the CPU with the fp32 oracle against the fp64 oracle
under the same checks (`cap=0.5`), and kept only because the fp32 oracle alone stays within HALF of every cap; a scene that does
not gets another seed, never another cap.  References are computed once (`memo`) and shared; nobody writes into them.

What stays in the test files, because it is not the same thing: their `_run` wrappers over `run` (a file's own defaults and
argument names; the per-form dispatch of test_raster_antialias_gpu.py and the scene records of test_raster_units_gpu.py run the
rasterizer themselves), the scene tables of test_raster_regimes_gpu.py (`_scene(name, table)`) and raster_units_ref.py, the
image and gradient checks of test_raster_gpu.py, test_raster_edge_gpu.py and test_raster_regimes_gpu.py (numpy arrays, a median
bound, lines of another wording, a module ledger), `_leaf32` of test_raster_camera_gpu.py (casts an fp64 scene), `_eye_settings` and
`_view_cfg` of the normals tests (no camera object; a NULL view matrix) and `_settings(**kw)` of test_raster_antialias.py (the
settings class itself, positionally).
"""
import ctypes
import functools
import math

import numpy as np
import torch

from contextgs_amd.synth import look_at_camera, random_gaussians

BG = (0.1, 0.25, 0.4)
EYE = (0.4, -2.2, 0.6)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _build_scene(P, W, H, seed, extent, srange, eye):
    cam = look_at_camera(eye, (0, 0, 0), W, H, fovx_deg=60.0)
    g = random_gaussians(P, seed=seed, extent=extent, scale_lo=srange[0], scale_hi=srange[1])
    if P >= 20:     # some Gaussians behind the near plane.  The push is about the fixed point EYE whatever `eye` is: a second
        e = np.array(EYE, dtype=np.float32)     # camera looks at the same Gaussians, not at a scene of its own
        g["means3D"][::20] = e + 0.3 * (e - g["means3D"][::20])
    return cam, g


@functools.lru_cache(maxsize=None)
def _build_stack_scene(kind, W, H):
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


def _fresh(built):
    cam, g = built
    return cam, {k: v.copy() for k, v in g.items()}


def scene(P, W, H, seed, extent=1.0, srange=(0.005, 0.05), eye=EYE):
    return _fresh(_build_scene(P, W, H, seed, extent, tuple(srange), tuple(eye)))


def stack_scene(kind, W, H):
    """saturated: 300 nearly opaque, wide Gaussians (pixels stop on the 1e-4 test).  long: 700 faint, wide ones (more than two
    256-entry batches per tile, no pixel stopped early)."""
    return _fresh(_build_stack_scene(kind, W, H))


def named_scene(name):
    if name == "ragged":        # 3 x 2 tiles, ragged right and bottom, some Gaussians behind the near plane
        return scene(200, 40, 24, 3, 1.0, (0.02, 0.12))
    if name == "single":
        return scene(1, 64, 48, 1)
    return stack_scene(name, 16, 16)


def model(N=20000, W=320, H=180):
    """An anchor model, four orbit cameras, the pipe and a black background for the render() tests."""
    from contextgs_amd.synth import SynthPipe, make_scene, orbit_cameras
    pc = make_scene(N, seed=0)
    cams = [c.to_torch("cuda") for c in orbit_cameras(4, W, H)]
    return pc, cams, SynthPipe(), torch.zeros(3, device="cuda")


def loss_weights(H, W):
    return np.random.default_rng(5).normal(size=(3, H, W)).astype(np.float32)


def view_z(cam, means3D):
    """z of p_view = [x y z 1] @ V in fp32, in the kernels' order of operations."""
    V = np.asarray(cam.world_view_transform.detach().cpu().numpy() if hasattr(cam.world_view_transform, "detach")
                   else cam.world_view_transform, dtype=np.float32).reshape(4, 4)
    m = means3D.astype(np.float32)
    return ((V[0, 2] * m[:, 0] + V[1, 2] * m[:, 1]) + V[2, 2] * m[:, 2]) + V[3, 2], V[:3, 2].copy()


def aux_colors(z):
    ok = z > 0.2            # the near cull: other Gaussians never reach a list
    zs = np.where(ok, z, 1.0).astype(np.float32)
    return np.stack([np.where(ok, zs, 0), np.where(ok, np.float32(1.0) / zs, 0), np.where(ok, 1.0, 0)], 1).astype(np.float32)


_REFS = {}


def memo(key, make):
    """References are computed once and shared; nobody writes into them.  Keys carry the file's name: the cache is one."""
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


# ---- running the rasterizer -----------------------------------------------------------------------------------------------------
def settings(cam, *, bg=BG, D=1, debug=False, aa=False, view=None, proj=None, campos=None, scale_modifier=1.0):
    from contextgs_amd.rasterizer import GaussianRasterizationSettings
    c = cam.to_torch("cuda")
    return GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=torch.as_tensor(bg, dtype=torch.float32, device="cuda"),      # (a tuple or a tensor)
        scale_modifier=scale_modifier, viewmatrix=c.world_view_transform if view is None else view,
        projmatrix=c.full_proj_transform if proj is None else proj, sh_degree=D,
        campos=c.camera_center if campos is None else campos, prefiltered=False, debug=debug, antialiasing=aa)


def leaf(a):
    return torch.tensor(a, device="cuda", requires_grad=True)


def np_of(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def run(rs, g, *, loss_w=None, colors=None, opacities=None, means2D_cols=3, **raster_kwargs):
    """Forward on fresh leaves (and backward of sum(out * w) over the entries of loss_w: keys color / depth / invdepth / alpha /
    features / ...) -> {"color", "radii", the extra maps, "grad": {input: gradient or None}, "leaves"}.  `colors` replaces the
    scene's, `opacities` is a tensor passed as it is, `features` (in raster_kwargs) a table that becomes a leaf."""
    from contextgs_amd.rasterizer import GaussianRasterizer
    P = g["means3D"].shape[0]
    t = {k: leaf(v) for k, v in g.items()}
    if colors is not None:
        t["colors"] = leaf(colors)
    if raster_kwargs.get("features") is not None:
        t["features"] = raster_kwargs["features"] = leaf(raster_kwargs["features"])
    m2 = torch.zeros(P, means2D_cols, device="cuda", requires_grad=True)
    res = GaussianRasterizer(rs)(means3D=t["means3D"], means2D=m2, opacities=t["opacities"] if opacities is None else opacities,
                                 colors_precomp=t["colors"], scales=t["scales"], rotations=t["rotations"], **raster_kwargs)
    out = {"color": res[0], "radii": res[1]}
    if len(res) > 2:
        out.update(res[2])
    if loss_w:
        sum(((out[k] * torch.as_tensor(w, device="cuda")).sum() for k, w in loss_w.items())).backward()
    torch.cuda.synchronize()
    o = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}
    o["grad"] = {k: (None if v.grad is None else v.grad.detach()) for k, v in t.items()}
    o["grad"]["means2D"] = m2.grad
    o["leaves"] = t
    return o


# ---- checks ---------------------------------------------------------------------------------------------------------------------
def check_map(a, b, what, cap=1.0):
    a = np_of(a).astype(np.float32).reshape(-1)
    b = np.asarray(b, dtype=np.float32).reshape(-1)
    scale = max(float(np.abs(b).max()), 1e-12)
    d = np.abs(a - b) / scale
    rmse = float(np.sqrt((d ** 2).mean()))
    n_out = int((d > 2e-5).sum())
    print(f"[allowance] {what}: rmse {rmse:.2e}, {n_out} of {d.size} values beyond 2e-5 of the max {scale:.3g}, worst {d.max():.2e}")
    assert rmse <= 1e-5 * cap, (what, rmse)
    assert n_out <= 1e-4 * cap * d.size, (what, n_out, float(d.max()))


def check_grad(a, b, what, allow_frac=2e-3, tol=2e-4):
    a = np_of(a).astype(np.float32)
    a = a.reshape(a.shape[0], -1)
    b = np.asarray(b, dtype=np.float32).reshape(a.shape)
    scale = max(1e-6, float(np.abs(b).max()))
    err = np.abs(a - b) / scale
    n_out = int((err > tol).sum())
    print(f"[allowance] {what}: {n_out} of {err.size} entries beyond {tol:g} of the maximum, worst {err.max():.2e}")
    assert n_out <= allow_frac * err.size, (what, n_out, float(err.max()))


def check_image(a, b, rmse_max, what=None):
    """Two images as tensors.  what=None: checked without an [allowance] line."""
    d = (a - b).abs().cpu().numpy()
    rmse = float(np.sqrt((d ** 2).mean()))
    frac = float((d > 2e-5).sum()) / d.size
    if what is not None:
        print(f"[allowance] {what}: rmse {rmse:.2e}, {frac:.2e} of values beyond 2e-5, max {float(d.max()):.2e}")
    assert rmse <= rmse_max, (what, rmse)
    assert frac <= 1e-4, (what, frac, d.max())
    assert d.max() <= 1.0 / 255 + 1e-4, (what, d.max())


def close(a, b, what, tol=2e-4, rows=None, *, allow_frac):
    """max |a - b| <= tol * max |b| on every row but at most allow_frac of them: a last-ulp difference between the two sides
    (the covariance form's conic, an fp32 h against an fp64 one) can flip an alpha >= 1/255 decision on a pixel."""
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


# ---- the torch restatements: SH colours, covariances, the antialiasing factor ---------------------------------------------------
C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435)
R_MIN = 2.5e-5


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


def shs(P, M, seed, clamp_dc=True):
    rng = np.random.default_rng(seed + 1000)
    sh = rng.normal(0.0, 0.25, size=(P, M, 3)).astype(np.float32)
    if clamp_dc:     # DC terms so that a good share of channels clamp: C0 * sh0 + 0.5 in [-0.5, 1.0]
        sh[:, 0, :] = (rng.uniform(-1.0, 0.5, size=(P, 3)) / C0).astype(np.float32)
    return sh


def quat_to_rot(q):
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]      # used as given, like the kernels
    return torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)


def cov6_torch(scales, rotations, scale_modifier=1.0):
    L = quat_to_rot(rotations) * (scale_modifier * scales)[:, None, :]
    S = L @ L.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=1)


def sigma_rs(scales, rotations, scale_modifier=1.0):
    L = quat_to_rot(rotations.double()) * (scale_modifier * scales.double())[:, None, :]
    return L @ L.transpose(1, 2)


def cov2d_torch(means3D, Sigma, rs):
    """J W Sigma W^T J^T before the dilation, with cgs_jacobian's 1.3 tanfov clamp (fp64)."""
    V = rs.viewmatrix.double()
    m = means3D.double()
    t = m @ V[:3, :3] + V[3, :3]
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    limx, limy = 1.3 * rs.tanfovx, 1.3 * rs.tanfovy
    tx = torch.clamp(tx / tz, -limx, limx) * tz
    ty = torch.clamp(ty / tz, -limy, limy) * tz
    fx = rs.image_width / (2 * rs.tanfovx)
    fy = rs.image_height / (2 * rs.tanfovy)
    z0 = torch.zeros_like(tz)
    J = torch.stack([fx / tz, z0, -fx * tx / (tz * tz), z0, fy / tz, -fy * ty / (tz * tz)], 1).view(-1, 2, 3)
    A = J @ V[:3, :3].T
    return A @ Sigma @ A.transpose(1, 2)


def h_torch(means3D, Sigma, rs):
    """(h, det / det(+0.3 I)): the antialiasing factor sqrt(max(2.5e-5, ratio)) and the ratio, in fp64."""
    c2 = cov2d_torch(means3D, Sigma, rs)
    a, b, c = c2[:, 0, 0], c2[:, 0, 1], c2[:, 1, 1]
    d0 = a * c - b * b
    d1 = (a + 0.3) * (c + 0.3) - b * b
    return torch.sqrt(torch.clamp_min(d0 / d1, R_MIN)), d0 / d1


# ---- the CPU argument checks ----------------------------------------------------------------------------------------------------
def fake_cfg(H=16, W=16, campos=True):
    from contextgs_amd import _lib
    fake = ctypes.c_void_p(256)     # never dereferenced: every call that takes it fails its argument checks first
    return _lib.RasterCfg(image_height=H, image_width=W, tanfovx=0.5, tanfovy=0.5, scale_modifier=1.0, prefiltered=0,
                          debug=0, viewmatrix=fake, projmatrix=fake, campos=fake if campos else None, bg=fake)
