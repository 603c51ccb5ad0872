"""numpy restatements of the normal maps and the normal-consistency regulariser (helper of tests/test_normals*.py; numpy only;
contextgs_amd/normals.py and include/cgs.h have the definitions), in the precision asked for: fp64 is the reference, fp32
is the same formulas in the kernels' number format and shows what the format alone costs.  Also the inputs both test files use.

Everything is in camera space (t = [x y z 1] @ V, x right, y down, z forward) and every normal points away from the camera.
The norm is sqrt(sum of squares) with a gradient that is 0 at 0 (`_safe`), as th.norm's.  The depth backwards are written as
the SCATTER the forward implies (each stencil adds to the four pixels it read, np.add.at); the kernels gather instead."""
import math

import numpy as np


# ---- per-Gaussian normals ----------------------------------------------------------------------------------------------------
def _columns(q):
    """The three columns of R(q) for unit quaternions q [P,4] (r, x, y, z): [P, 3 (column), 3]."""
    r, x, y, z = q.T
    one, two = q.dtype.type(1), q.dtype.type(2)
    return np.stack([
        np.stack([one - two * (y * y + z * z), two * (x * y + r * z), two * (x * z - r * y)], 1),
        np.stack([two * (x * y - r * z), one - two * (x * x + z * z), two * (y * z + r * x)], 1),
        np.stack([two * (x * z + r * y), two * (y * z - r * x), one - two * (x * x + y * y)], 1)], 1)


def gaussian_normals(means3D, scales, rotations, V, dtype=np.float64):
    """{"n": [P,3], "k": [P], "sign": [P], "margin": [P] = |n^ . t^| (how far the sign is from falling the other way)}.
    V: the 4x4 view matrix the rasterizer reads (row-vector convention)."""
    m, s, q, V = (np.asarray(a, np.float32).astype(dtype) for a in (means3D, scales, rotations, V))
    V = V.reshape(4, 4)
    P = m.shape[0]
    k = np.argmin(s, axis=1) if P else np.zeros(0, np.int64)      # (argmin: the first of equal minima)
    qn = q / np.sqrt((q * q).sum(1, keepdims=True))
    nw = _columns(qn)[np.arange(P), k]
    nv = nw @ V[:3, :3]
    t = m @ V[:3, :3] + V[3, :3]
    dot = (nv * t).sum(1)
    sign = np.where(dot >= 0, 1, -1).astype(dtype)
    margin = np.abs(dot) / np.maximum(np.linalg.norm(t, axis=1) * np.linalg.norm(nv, axis=1), 1e-300)
    return {"n": sign[:, None] * nv, "k": k, "sign": sign, "margin": margin}


def gaussian_normals_bwd(means3D, scales, rotations, V, g, dtype=np.float64):
    """dL/drotations [P,4] from g = dL/dn [P,3], analytically (tests/test_normals.py checks it against central differences)."""
    f = gaussian_normals(means3D, scales, rotations, V, dtype)
    q = np.asarray(rotations, np.float32).astype(dtype)
    V = np.asarray(V, np.float32).astype(dtype).reshape(4, 4)
    g = np.asarray(g, np.float32).astype(dtype) * f["sign"][:, None]
    gw = g @ V[:3, :3].T                                   # dL/dn_w
    ln = np.sqrt((q * q).sum(1, keepdims=True))
    r, x, y, z = (q / ln).T
    g0, g1, g2 = gw.T
    two, four = dtype(2), dtype(4)
    per_k = [
        np.stack([two * (z * g1 - y * g2), two * (y * g1 + z * g2), -four * y * g0 + two * (x * g1 - r * g2),
                  -four * z * g0 + two * (r * g1 + x * g2)], 1),
        np.stack([two * (x * g2 - z * g0), -four * x * g1 + two * (y * g0 + r * g2), two * (x * g0 + z * g2),
                  -four * z * g1 + two * (y * g2 - r * g0)], 1),
        np.stack([two * (y * g0 - x * g1), -four * x * g2 + two * (z * g0 - r * g1), -four * y * g2 + two * (r * g0 + z * g1),
                  two * (x * g0 + y * g1)], 1)]
    dq = np.stack(per_k, 1)[np.arange(q.shape[0]), f["k"]]
    qn = q / ln
    return (dq - qn * (qn * dq).sum(1, keepdims=True)) / ln


# ---- depth normals ---------------------------------------------------------------------------------------------------------------
def _safe(n):
    """(|n|, 1 / |n| or 0 where |n| = 0) over axis 0."""
    ln = np.sqrt((n * n).sum(0))
    with np.errstate(divide="ignore"):
        return ln, np.where(ln > 0, n.dtype.type(1) / np.where(ln > 0, ln, 1), 0).astype(n.dtype)


def _stencil(depth, tanfovx, tanfovy, dtype):
    d = np.asarray(depth, np.float32).astype(dtype)
    d = d.reshape(d.shape[-2:])
    H, W = d.shape
    fx, fy = dtype(W) / (dtype(2) * dtype(np.float32(tanfovx))), dtype(H) / (dtype(2) * dtype(np.float32(tanfovy)))
    a = (np.arange(W, dtype=dtype) - dtype(0.5) * dtype(W))[None, :]
    b = (np.arange(H, dtype=dtype) - dtype(0.5) * dtype(H))[:, None]
    p = np.stack([d * a / fx, d * b / fy, d])
    vp, vm = np.minimum(np.arange(H) + 1, H - 1), np.maximum(np.arange(H) - 1, 0)
    up, um = np.minimum(np.arange(W) + 1, W - 1), np.maximum(np.arange(W) - 1, 0)
    d0 = p[:, vp, :] - p[:, vm, :]
    d1 = p[:, :, up] - p[:, :, um]
    n = np.cross(d0, d1, axis=0)
    return {"d0": d0, "d1": d1, "n": n, "idx": (vp, vm, up, um), "ab": (a, b, fx, fy)}


def depth_normals(depth, tanfovx, tanfovy, eps=0.0, dtype=np.float64):
    """[3,H,W]: N = -n / (|n| + eps), 0 where the denominator is 0."""
    s = _stencil(depth, tanfovx, tanfovy, dtype)
    ln, _ = _safe(s["n"])
    den = ln + dtype(eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, -s["n"] / np.where(den > 0, den, 1), 0).astype(dtype)


def depth_normals_bwd(depth, tanfovx, tanfovy, eps, G, dtype=np.float64):
    """dL/ddepth [H,W] from G = dL/dN [3,H,W] (a float32 input)."""
    return _depth_bwd(depth, tanfovx, tanfovy, eps, np.asarray(G, np.float32).astype(dtype), dtype)


# ---- the regulariser ---------------------------------------------------------------------------------------------------------
def normal_consistency(normals, depth, tanfovx, tanfovy, weight=None, eps=0.0, dtype=np.float64):
    """[H,W]: E = 1 - m sum_c normals_c N_c."""
    N = depth_normals(depth, tanfovx, tanfovy, eps, dtype)
    nm = np.asarray(normals, np.float32).astype(dtype)
    m = dtype(1) if weight is None else np.asarray(weight, np.float32).astype(dtype).reshape(N.shape[1:])
    return dtype(1) - m * (nm * N).sum(0)


def normal_consistency_bwd(normals, depth, tanfovx, tanfovy, weight, eps, gE, dtype=np.float64):
    """(dL/dnormals [3,H,W], dL/ddepth [H,W]) from gE = dL/dE [H,W]; the weight gets none."""
    N = depth_normals(depth, tanfovx, tanfovy, eps, dtype)
    nm = np.asarray(normals, np.float32).astype(dtype)
    m = dtype(1) if weight is None else np.asarray(weight, np.float32).astype(dtype).reshape(N.shape[1:])
    k = -m * np.asarray(gE, np.float32).astype(dtype).reshape(N.shape[1:])
    return k * N, _depth_bwd(depth, tanfovx, tanfovy, eps, k * nm, dtype)


def _depth_bwd(depth, tanfovx, tanfovy, eps, G, dtype):
    """dL/ddepth from G = dL/dN in `dtype`: dL/dn = -G / den + n (G . n) / (|n| den^2), dL/dd0 = d1 x dL/dn, dL/dd1 = dL/dn x d0,
    each stencil adding to the four pixels it read."""
    s = _stencil(depth, tanfovx, tanfovy, dtype)
    n, d0, d1 = s["n"], s["d0"], s["d1"]
    ln, inv_ln = _safe(n)
    den = ln + dtype(eps)
    inv_den = np.where(den > 0, dtype(1) / np.where(den > 0, den, 1), 0).astype(dtype)
    gn = -G * inv_den + n * ((G * n).sum(0) * inv_ln * inv_den * inv_den)
    g0, g1 = np.cross(d1, gn, axis=0), np.cross(gn, d0, axis=0)
    vp, vm, up, um = s["idx"]
    gp = np.zeros_like(n)
    rows, cols = gp.transpose(1, 0, 2), gp.transpose(2, 0, 1)
    np.add.at(rows, vp, g0.transpose(1, 0, 2))
    np.add.at(rows, vm, -g0.transpose(1, 0, 2))
    np.add.at(cols, up, g1.transpose(2, 0, 1))
    np.add.at(cols, um, -g1.transpose(2, 0, 1))
    a, b, fx, fy = s["ab"]
    return gp[0] * a / fx + gp[1] * b / fy + gp[2]


# ---- the inputs of both test files -------------------------------------------------------------------------------------------
TAN = (0.62, 0.41)          # tanfovx, tanfovy of the per-pixel cases
SHAPES = ((24, 40), (17, 33), (48, 64))
THIN = ((1, 1), (1, 37), (33, 1))       # one pixel wide or high: everything is exactly zero
HOLE = (slice(5, 9), slice(10, 20))     # rows 5-8, columns 10-19: an undrawn region


def depth_case(kind, H, W, hole=True):
    """float32 [1,H,W].  smooth: a tilted, gently curved surface around depth 2; rough: the same plus 2 % noise; constant: 2.
    smooth and rough have the zero hole when it fits."""
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind == "constant":
        return np.full((1, H, W), 2.0, np.float32)
    d = 2.0 + 0.012 * u - 0.02 * v + 0.15 * np.sin(0.23 * u + 0.1) * np.cos(0.31 * v) + 0.0004 * (u - 0.4 * W) * (v - 0.6 * H)
    if kind == "rough":
        d = d + np.random.default_rng(H * 1000 + W).uniform(-0.04, 0.04, size=d.shape)
    elif kind != "smooth":
        raise ValueError(kind)
    if hole and H > HOLE[0].stop and W > HOLE[1].stop:
        d[HOLE] = 0.0
    return d[None].astype(np.float32)


def pixel_inputs(kind, H, W):
    """{"depth" [1,H,W], "normals" [3,H,W], "weight" [1,H,W], "gN" [3,H,W], "gE" [1,H,W]} float32, fixed per (kind, H, W)."""
    rng = np.random.default_rng(7 + 31 * H + W + (0 if kind == "smooth" else 5))
    f = lambda a: np.ascontiguousarray(a.astype(np.float32))
    return {"depth": depth_case(kind, H, W), "normals": f(rng.normal(size=(3, H, W))), "weight": f(rng.uniform(0.0, 1.0, (1, H, W))),
            "gN": f(rng.normal(size=(3, H, W))), "gE": f(rng.normal(size=(1, H, W)))}


def view_matrix():
    from contextgs_amd.synth import look_at_camera
    return np.asarray(look_at_camera((0.4, -2.2, 0.6), (0, 0, 0), 40, 24, fovx_deg=60.0).world_view_transform, np.float32)


def gaussian_inputs(P, seed=0):
    """{"means3D", "scales", "rotations", "g" = dL/dn} float32: quaternions of random length 0.3..3, rows with two (every 5th:
    the two smallest; every 7th: the two largest) or three (every 11th) equal scales, every 4th Gaussian behind the camera."""
    rng = np.random.default_rng(seed)
    m = rng.uniform(-1.0, 1.0, (P, 3))
    eye = np.array([0.4, -2.2, 0.6])
    m[::4] = eye + 0.5 * (eye - m[::4])
    s = np.exp(rng.uniform(np.log(0.01), np.log(0.2), (P, 3)))
    lo, hi = s.min(1), s.max(1)
    s[::5] = np.stack([hi[::5], lo[::5], lo[::5]], 1)
    s[::7] = np.stack([hi[::7], lo[::7], hi[::7]], 1)
    s[::11] = lo[::11, None]
    q = rng.normal(size=(P, 4))
    q *= rng.uniform(0.3, 3.0, (P, 1)) / np.linalg.norm(q, axis=1, keepdims=True)
    f = lambda a: np.ascontiguousarray(a.astype(np.float32))
    return {"means3D": f(m), "scales": f(s), "rotations": f(q), "g": f(rng.normal(size=(P, 3)))}


def _rot_to_quat(R):
    """(r, x, y, z) of a proper rotation matrix, the branch with the largest pivot."""
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    return np.array(q)


def plane_scene(W=64, H=48, tilt_deg=30.0, seed=2):
    """(camera, Gaussians): a dense grid of nearly opaque, flat Gaussians on a plane through the origin tilted `tilt_deg` about
    the vertical axis against a camera at (0, -3, 0) that looks along +y.  The smallest scale is along the plane normal, at a
    random position among the three axes; the in-plane axes are turned by a random angle and every axis is flipped at random
    (the rotation stays proper), so that the per-Gaussian normals as stored point to either side of the plane."""
    from contextgs_amd.synth import look_at_camera
    cam = look_at_camera((0.0, -3.0, 0.0), (0, 0, 0), W, H, fovx_deg=60.0)
    rng = np.random.default_rng(seed)
    c, s = math.cos(math.radians(tilt_deg)), math.sin(math.radians(tilt_deg))
    e1, e2, nrm = np.array([c, s, 0.0]), np.array([0.0, 0.0, 1.0]), np.array([-s, c, 0.0])
    aa, bb = np.meshgrid(np.arange(-2.7, 2.71, 0.15), np.arange(-1.8, 1.81, 0.15))
    means = aa.reshape(-1, 1) * e1 + bb.reshape(-1, 1) * e2
    P = means.shape[0]
    quats, scales = np.zeros((P, 4)), np.zeros((P, 3))
    for i in range(P):
        th = rng.uniform(0, 2 * math.pi)
        t1 = math.cos(th) * e1 + math.sin(th) * e2
        t2 = -math.sin(th) * e1 + math.cos(th) * e2
        k = int(rng.integers(0, 3))
        axes = [None] * 3
        axes[k] = nrm * rng.choice([-1.0, 1.0])
        axes[(k + 1) % 3] = t1 * rng.choice([-1.0, 1.0])
        axes[(k + 2) % 3] = np.cross(axes[k], axes[(k + 1) % 3])        # cyclic order: det = +1
        quats[i] = _rot_to_quat(np.stack(axes, 1))
        scales[i] = 0.12
        scales[i, k] = 0.004
    f = lambda a: np.ascontiguousarray(a.astype(np.float32))
    g = dict(means3D=f(means), scales=f(scales), rotations=f(quats), colors=f(rng.random((P, 3))),
             opacities=f(np.full((P, 1), 0.99)))
    return cam, g


def hemisphere_agreement(normals, depth, alpha, tanfovx, tanfovy, border=4):
    """(the mean of normals . depth_normals(depth / alpha) / alpha over pixels with alpha > 0.9 at least `border` px from the
    image edge, the number of such pixels), from maps [3,H,W], [1,H,W], [1,H,W]; fp64."""
    normals, depth, alpha = (np.asarray(a, np.float64) for a in (normals, depth, alpha))
    a = alpha.reshape(alpha.shape[-2:])
    d = depth.reshape(a.shape) / np.maximum(a, 1e-6)
    N = depth_normals(d.astype(np.float32), tanfovx, tanfovy, 0.0)
    mask = a > 0.9
    mask[:border] = mask[-border:] = False
    mask[:, :border] = mask[:, -border:] = False
    dots = (normals * N).sum(0) / np.maximum(a, 1e-6)
    return float(dots[mask].mean()), int(mask.sum())


# ---- the project's tolerance caps (copies of tests/test_raster_geom_gpu.py's _check_map / _check_grad) ---------------------------
def check_map(a, b, what, cap=1.0):
    """RMSE <= 1e-5 of the reference map's maximum and at most a 1e-4 share of values beyond 2e-5 of it."""
    a = np.asarray(a, dtype=np.float32).reshape(-1)
    b = np.asarray(b, dtype=np.float32).reshape(-1)
    scale = max(float(np.abs(b).max()), 1e-12)
    d = np.abs(a - b) / scale
    rmse = float(np.sqrt((d ** 2).mean()))
    n_out = int((d > 2e-5).sum())
    print(f"[allowance] {what}: rmse {rmse:.2e}, {n_out} of {d.size} values beyond 2e-5 of the max {scale:.3g}, worst {d.max():.2e}")
    assert rmse <= 1e-5 * cap, (what, rmse)
    assert n_out <= 1e-4 * cap * d.size, (what, n_out, float(d.max()))


def check_grad(a, b, what, cap=1.0, allow_frac=2e-3, tol=2e-4):
    """At most a 2e-3 share of entries beyond 2e-4 of the reference tensor's maximum."""
    a = np.asarray(a, dtype=np.float32).reshape(-1)
    b = np.asarray(b, dtype=np.float32).reshape(-1)
    scale = max(1e-6, float(np.abs(b).max()))
    err = np.abs(a - b) / scale
    n_out = int((err > tol).sum())
    print(f"[allowance] {what}: {n_out} of {err.size} entries beyond {tol:g} of the maximum {scale:.3g}, worst {err.max():.2e}")
    assert n_out <= allow_frac * cap * err.size, (what, n_out, float(err.max()))
