"""fp64 reference of the rasterizer's depth-distortion and median-depth maps (helper of tests/test_raster_geom*.py; numpy only).

Everything follows from the matrix w[i, p] of blending weights (w > 0 for the contributors of pixel p, 0 otherwise) and the
view depths z[i], with the contributors of a pixel ordered by (z, index), T_1 = 1, T_{i+1} = T_i (1 - alpha_i),
w_i = alpha_i T_i, A_i = sum_{k<=i} w_k, D_i = sum_{k<=i} w_k z_k:

  distortion[p]   = 2 sum_i w_i (z_i A_{i-1} - D_{i-1})
  median_depth[p] = z_m, m = the first contributor with T_m (1 - alpha_m) = 1 - A_m < 0.5 (0 where none), median_id[p] = m (-1)
  e_i(p)          = 2 [z_i A_{i-1} - D_{i-1} + (D_n - D_i) - z_i (A_n - A_i)]        = d distortion / d w_i
  zterm_i(p)      = 2 w_i (A_{i-1} - (A_n - A_i))                                    = d distortion / d z_i

`decompose` gets w from the unchanged oracle: oracle.render(colors = ones, bg = 0, dL_dout one-hot at pixel p on channel c)
returns dL_dcolors[:, c] = w_i(p), three pixels per call through the three channels (the construction of `decompose()` in
tests/test_raster_contrib_gpu.py, restated).  `grad_reference` gets the gradients the same way: with colours g[p] e_i(p) and the
same one-hot dL_dout the oracle's backward IS the weight-path gradient of g[p] distortion[p]; the direct terms through z are
added in numpy.
"""
import numpy as np


# ---- one list, in list order (the definitions; used by the reference's own tests) ----------------------------------------------
def list_weights(alpha):
    """w_i = alpha_i T_i of one front-to-back list of alphas."""
    alpha = np.asarray(alpha, np.float64)
    T = np.concatenate([[1.0], np.cumprod(1.0 - alpha)[:-1]])
    return alpha * T


def list_distortion(w, z):
    """The running sum 2 sum_i w_i (z_i A_{i-1} - D_{i-1}) of one list, in the order given (nothing is sorted)."""
    w, z = np.asarray(w, np.float64), np.asarray(z, np.float64)
    A = np.cumsum(w) - w
    D = np.cumsum(w * z) - w * z
    return float(2.0 * np.sum(w * (z * A - D)))


def list_distortion_pairs(w, z):
    """sum_{i,j} w_i w_j |z_i - z_j|, the O(n^2) double sum."""
    w, z = np.asarray(w, np.float64), np.asarray(z, np.float64)
    return float(np.sum(w[:, None] * w[None, :] * np.abs(z[:, None] - z[None, :])))


def list_terms(w, z):
    """(e_i, zterm_i) of one list in the order given."""
    w, z = np.asarray(w, np.float64), np.asarray(z, np.float64)
    A, D = np.cumsum(w), np.cumsum(w * z)
    Ap, Dp = A - w, D - w * z
    e = 2.0 * (z * Ap - Dp + (D[-1] - D) - z * (A[-1] - A))
    return e, 2.0 * w * (Ap - (A[-1] - A))


# ---- a whole view ------------------------------------------------------------------------------------------------------------
def view_depths(cam, means3D):
    """z_i = ([p, 1] V)[2] in fp64 from the float32 matrix the rasterizer reads (row-vector convention)."""
    V = np.asarray(cam.world_view_transform, np.float32).astype(np.float64).reshape(4, 4)
    return np.asarray(means3D, np.float64) @ V[:3, 2] + V[3, 2]


def geom_maps(w, z):
    """From w [P, N] and z [P]: {"distortion", "median_depth" [N] fp64, "median_id" [N] int32, "margin" [N], "e", "zterm" [P, N]
    in the rows' own order}.  margin[p] = min(|T_m (1 - alpha_m) - 0.5|, the same of the contributor before it) (1 before the
    first), or |T_final - 0.5| where nobody crosses: how far the pixel's choice is from falling the other way."""
    w = np.asarray(w, np.float64)
    z = np.asarray(z, np.float64)
    P, N = w.shape
    order = np.lexsort((np.arange(P), z))
    ws, zs = w[order], z[order][:, None]
    A, D = np.cumsum(ws, 0), np.cumsum(ws * zs, 0)
    Ap, Dp = A - ws, D - ws * zs
    An, Dn = (A[-1], D[-1]) if P else (np.zeros(N), np.zeros(N))
    dist = 2.0 * np.sum(ws * (zs * Ap - Dp), 0)
    T_after = 1.0 - A
    crossed = (T_after < 0.5) & (ws > 0)
    has = crossed.any(0) if P else np.zeros(N, bool)
    m = crossed.argmax(0) if P else np.zeros(N, np.int64)
    med_id = np.where(has, order[m] if P else 0, -1).astype(np.int32)
    med_z = np.where(has, zs[m, 0] if P else 0.0, 0.0)
    T_all = np.concatenate([np.ones((1, N)), T_after], 0)
    margin = np.abs(T_all - 0.5).min(0)      # T falls monotonically: the minimum sits at m or m - 1 (at n where nobody crosses)
    e = np.zeros_like(w)
    zterm = np.zeros_like(w)
    e[order] = 2.0 * (zs * Ap - Dp + (Dn - D) - zs * (An - A))
    zterm[order] = 2.0 * ws * (Ap - (An - A))
    return {"distortion": dist, "median_depth": med_z, "median_id": med_id, "margin": margin, "e": e, "zterm": zterm}


def _triples(n):
    for p0 in range(0, n, 3):
        yield [p for p in range(p0, min(p0 + 3, n))]


def decompose(oracle, cam, g):
    """{"w": [P, H*W] in the oracle's precision, "final_T", "radii", "stats"}: three pixels per oracle call."""
    P = g["means3D"].shape[0]
    H, W = cam.image_height, cam.image_width
    ones = np.ones((P, 3), np.float32)
    cd = cam.oracle_dict(bg=(0.0, 0.0, 0.0))
    w = np.zeros((P, H * W), oracle.dtype)
    d = np.zeros((3, H, W), np.float32)
    r = None
    for ps in _triples(H * W):
        for c, p in enumerate(ps):
            d[c].flat[p] = 1.0
        r = oracle.render(cd, g["means3D"], ones, g["opacities"], g["scales"], g["rotations"], dL_dout=d)
        for c, p in enumerate(ps):
            d[c].flat[p] = 0.0
            w[:, p] = r["dL_dcolors"][:, c]
    return {"w": w, "final_T": r["final_T"], "radii": r["radii"], "stats": r["stats"]}


GRAD_KEYS = ("means3D", "means2D", "opacities", "scales", "rotations")


def grad_reference(oracle, cam, g, maps, g_dist=None, g_med=None, opacities=None):
    """Gradients of sum_p g_dist[p] distortion[p] + g_med[p] median_depth[p] with respect to means3D, means2D, opacities, scales
    and rotations, in the oracle's conventions, as fp64 arrays.  maps: geom_maps() of the fp64 decomposition; g_dist, g_med:
    [H*W] or None.  Weight path: one oracle call per three pixels with dL_dout one-hot and colours g_dist[p] e_i(p) over a zero
    background.  Direct path: (sum_p g_dist[p] zterm_i(p) + sum_{p: median_id[p] = i} g_med[p]) V[:3, 2].  opacities: what the
    oracle is rendered with when it is not g["opacities"] (antialiasing: opacity * h)."""
    P = g["means3D"].shape[0]
    H, W = cam.image_height, cam.image_width
    N = H * W
    out = {"means3D": np.zeros((P, 3)), "means2D": np.zeros((P, 3)), "opacities": np.zeros(P), "scales": np.zeros((P, 3)),
           "rotations": np.zeros((P, 4))}
    dz = np.zeros(P)
    if g_dist is not None:
        g_dist = np.asarray(g_dist, np.float64).reshape(N)
        cd = cam.oracle_dict(bg=(0.0, 0.0, 0.0))
        op = g["opacities"] if opacities is None else opacities
        d = np.zeros((3, H, W), np.float32)
        col = np.zeros((P, 3), np.float64)
        for ps in _triples(N):
            col[:] = 0.0
            for c, p in enumerate(ps):
                d[c].flat[p] = 1.0
                col[:, c] = g_dist[p] * maps["e"][:, p]
            r = oracle.render(cd, g["means3D"], col, op, g["scales"], g["rotations"], dL_dout=d)
            for c, p in enumerate(ps):
                d[c].flat[p] = 0.0
            for k in GRAD_KEYS:
                out[k] += np.asarray(r["dL_d" + k], np.float64).reshape(out[k].shape)
        dz += maps["zterm"] @ g_dist
    if g_med is not None:
        g_med = np.asarray(g_med, np.float64).reshape(N)
        hit = maps["median_id"] >= 0
        np.add.at(dz, maps["median_id"][hit], g_med[hit])
    V = np.asarray(cam.world_view_transform, np.float32).astype(np.float64).reshape(4, 4)
    out["means3D"] += dz[:, None] * V[None, :3, 2]
    out["dz"] = dz
    return out
