"""The bilateral grid of contextgs_amd/bilagrid.py in numpy: the slice, its two gradients, the TV term and its gradient, with a
`dtype` argument (float64 is the reference, float32 the budget probe), the cases the tests run and the per-element budgets.

Definition (include/cgs.h above cgs_bilagrid_slice_fwd):  G [12, L, Gh, Gw], image [3, H, W], pixel (y, x) = (r, g, b)
  gx = (x + .5) / W (Gw - 1), gy = (y + .5) / H (Gh - 1), z = .299 r + .587 g + .114 b, gz = clamp(z (L - 1), 0, L - 1)
  axis of n nodes: i0 = clamp(floor(g), 0, n - 1), i1 = min(i0 + 1, n - 1), f = g - i0, weights 1 - f on i0, f on i1
  A = sum_corners wz wy wx G[:, zi, yi, xi];  out_i = sum_j A[4 i + j] rgb_j + A[4 i + 3]
  dA[4 i + j] = dout_i rgb_j (rgb_3 = 1);  dG[c, corner] += w_corner dA[c]
  dimg_j = sum_i A[4 i + j] dout_i + lum_j (L - 1) m sum_c dA[c] dAdz[c],  dAdz = sum_xy-corners wy wx (G[z1] - G[z0]),
  m = [0 < z (L - 1) < L - 1]

Budgets.  They come from this reference alone.  EPS = 2^-24 (one float32 rounding, relative).  Every budget has two parts.

(a) Arithmetic: K * EPS * S_e, S_e = the sum of the absolute values of the terms of element e (fp64), K = the roundings on the
    longest chain from the inputs to the element.  Counts (an fma is one rounding):
      a corner weight        1 - f per axis (3, each on its own factor), wy wx (1), wz (wy wx) (1); the weight used in dAdz: 3
      A[c]                   weight 5, one fma per corner into the running sum (8)                                  K_A    = 13
      out_i                  A, then 4 fmas                                                                         K_OUT  = 17
      dimg_j, first term     A, one product and 2 fmas, the fma that adds the second term                           K_DI1  = 17
      dimg_j, second term    dAdz: weight 3, G1 - G0 (1), 4 fmas = 8; dA (1); 12 fmas into s; s (L - 1) (1);
                             the rounded constant lum_j (1)                                                         K_DI2  = 23
      dG addend              weight 5, dA (1), the fma (1)                                                          K_DG   = 7
      dG[e], TV              + n_e * EPS * S_e for the sum of n_e addends in ANY order (n_e counted on the reference:
                             pixel corners of non-zero weight; differences)
      TV addend              difference (1, squared: 2), the square (1), the rounded 1 / count (1), the fma (1),
                             1 / N rounded and applied (2)                                                          K_TV   = 7
      dTV[e]                 difference (1), two adds per axis (2), rounded 1 / count (1), 3 fmas, g * (2 / N) (2),
                             the last product (1)                                                                   K_DTV  = 10
(b) Coordinates: the kernel's float32 gx, gy, gz differ from the fp64 ones by at most
      d_gx = K_C * EPS * gx, K_C = 3  ((x + .5) is exact; the quotient, the product, and one to spare),  d_gy alike,
      d_gz = K_Z * EPS * (L - 1) (.299 |r| + .587 |g| + .114 |b|) m, K_Z = 5  (rounded constant, product, two sums, the scale;
             a clamped pixel stays clamped: the case builder keeps z (L - 1) 1e-3 away from every integer),
    and f = g - i0 is exact.  gx and gy are never within 1 / (2 W) of an integer ((2 x + 1)(Gw - 1) is odd times Gw - 1, 2 W k is
    even times W: their difference is a non-zero integer), so float32 and fp64 agree on every i0.  Each quantity is multilinear in
    the weights, so its change is at most d_g times the absolute slope along that axis, bounded by replacing the two weights of
    that axis by 1 and every grid value by its absolute value:  slope_x(A[c]) = sum_{z,y corners} wz wy (|G[x1]| + |G[x0]|), etc.
"""
from __future__ import annotations

import functools

import numpy as np

EPS = 2.0 ** -24
LUM = (0.299, 0.587, 0.114)
K_A, K_OUT, K_DI1, K_DI2, K_DG, K_TV, K_DTV, K_C, K_Z = 13, 17, 17, 23, 7, 7, 10, 3, 5
GZ_MARGIN = 1e-3
VARIANTS = ("corner_aligned", "unclamped_grad", "swapped_z", "no_bias")

# (L, Gh, Gw, H, W, kind).  The first seven are the issue's; (40, 6, 6, 9, 11) is a grid too fine for the LDS stage (the kernels
# read the nodes through the cache), (2, 2, 3, 70, 90) a cell large enough to be split over several workgroups.
CASES = [(8, 16, 16, 37, 53, "wide"), (2, 3, 4, 5, 7, "wide"), (1, 1, 1, 3, 3, "wide"), (3, 1, 5, 1, 9, "wide"),
         (4, 2, 2, 64, 1, "wide"), (8, 16, 16, 130, 258, "wide"), (2, 2, 2, 8, 8, "dark"),
         (40, 6, 6, 9, 11, "wide"), (2, 2, 3, 70, 90, "wide")]
TV_CASES = [(1, 8, 16, 16), (3, 2, 3, 4), (3, 1, 1, 1), (1, 3, 1, 5), (3, 4, 2, 1), (3, 2, 2, 2)]       # (N, L, Gh, Gw)


def case_id(case):
    return "x".join(str(v) for v in case)


def _axis(g, n, dtype):
    i0 = np.clip(np.floor(g), 0, n - 1).astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), g - i0.astype(dtype)


def luminance_scaled(img, L, dtype=np.float64):
    I = img.astype(dtype)
    return (dtype(LUM[0]) * I[0] + dtype(LUM[1]) * I[1] + dtype(LUM[2]) * I[2]) * dtype(L - 1)


def slice_all(grid, img, dout, dtype=np.float64, variant=None, budgets=False):
    """{'out', 'dimg', 'dgrid'} (+ 'b_out', 'b_dimg', 'b_dgrid' with budgets=True) of one grid [12,L,Gh,Gw] and image [3,H,W]."""
    G, I, D = grid.astype(dtype), img.astype(dtype), dout.astype(dtype)
    _, L, Gh, Gw = G.shape
    _, H, W = I.shape
    one = dtype(1)
    if variant == "corner_aligned":
        gx = np.arange(W, dtype=dtype) / dtype(max(W - 1, 1)) * dtype(Gw - 1)
        gy = np.arange(H, dtype=dtype) / dtype(max(H - 1, 1)) * dtype(Gh - 1)
    else:
        gx = (np.arange(W, dtype=dtype) + dtype(0.5)) / dtype(W) * dtype(Gw - 1)
        gy = (np.arange(H, dtype=dtype) + dtype(0.5)) / dtype(H) * dtype(Gh - 1)
    zs = luminance_scaled(I, L, dtype)
    gz = np.clip(zs, dtype(0), dtype(L - 1))
    m = ((zs > 0) & (zs < L - 1)).astype(dtype)
    x0, x1, fx = (a[None, :] for a in _axis(gx, Gw, dtype))
    y0, y1, fy = (a[:, None] for a in _axis(gy, Gh, dtype))
    z0, z1, fz = _axis(gz, L, dtype)
    wz2 = (fz, one - fz) if variant == "swapped_z" else (one - fz, fz)
    full = np.broadcast_to
    px = np.stack([I[0], I[1], I[2], np.zeros_like(I[0]) if variant == "no_bias" else np.ones_like(I[0])])
    dA = (D[:, None] * px[None]).reshape(12, H, W)
    A, dAdz = np.zeros((12, H, W), dtype), np.zeros((12, H, W), dtype)
    dG = np.zeros_like(G)
    if budgets:
        absA, Bx, By, Bz, Cx, Cy = (np.zeros((12, H, W), dtype) for _ in range(6))
        d_gx = (K_C * EPS * np.abs(gx))[None, :]
        d_gy = (K_C * EPS * np.abs(gy))[:, None]
        d_gz = K_Z * EPS * (L - 1) * (LUM[0] * np.abs(I[0]) + LUM[1] * np.abs(I[1]) + LUM[2] * np.abs(I[2])) * m
        S_dG, C_dG, n_dG = np.zeros_like(G), np.zeros_like(G), np.zeros_like(G)
    for zc in (0, 1):
        for yc in (0, 1):
            for xc in (0, 1):
                wz, wy, wx = wz2[zc], (fy if yc else one - fy), (fx if xc else one - fx)
                zi, yi, xi = (z1 if zc else z0), full(y1 if yc else y0, (H, W)), full(x1 if xc else x0, (H, W))
                w = wz * wy * wx
                Gc = G[:, zi, yi, xi]
                A += w * Gc
                dAdz += (wy * wx) * (Gc if zc else -Gc)
                np.add.at(dG, (slice(None), zi, yi, xi), w * dA)
                if budgets:
                    aG, adA = np.abs(Gc), np.abs(dA)
                    absA += w * aG
                    Bx += wz * wy * aG
                    By += wz * wx * aG
                    Bz += wy * wx * aG
                    Cx += wy * aG
                    Cy += wx * aG
                    np.add.at(S_dG, (slice(None), zi, yi, xi), w * adA)
                    np.add.at(C_dG, (slice(None), zi, yi, xi), (d_gx * wz * wy + d_gy * wz * wx + d_gz * wy * wx) * adA)
                    np.add.at(n_dG, (slice(None), zi, yi, xi), full((w > 0).astype(dtype), (12, H, W)))
    A4, dA4 = A.reshape(3, 4, H, W), dA.reshape(3, 4, H, W)
    out = (A4 * px[None]).sum(axis=1)
    s = (dA * dAdz).sum(axis=0)
    if variant == "unclamped_grad":
        m = np.ones_like(m)
    lum = np.array(LUM, dtype)[:, None, None]
    dimg = (A4[:, :3] * D[:, None]).sum(axis=0) + lum * dtype(L - 1) * m * s
    res = {"out": out, "dimg": dimg, "dgrid": dG, "gz_raw": zs}
    if budgets:
        apx, aD = np.abs(px), np.abs(D)
        r4 = lambda a: a.reshape(3, 4, H, W)
        res["b_out"] = K_OUT * EPS * (r4(absA) * apx[None]).sum(axis=1) + sum(
            d * (r4(B) * apx[None]).sum(axis=1) for d, B in ((d_gx, Bx), (d_gy, By), (d_gz, Bz)))
        first = K_DI1 * EPS * (r4(absA)[:, :3] * aD[:, None]).sum(axis=0) + sum(
            d * (r4(B)[:, :3] * aD[:, None]).sum(axis=0) for d, B in ((d_gx, Bx), (d_gy, By), (d_gz, Bz)))
        adA = np.abs(dA)
        second = lum * (L - 1) * m * (K_DI2 * EPS * (adA * Bz).sum(axis=0) + (adA * (d_gx * Cx + d_gy * Cy)).sum(axis=0))
        res["b_dimg"] = first + second
        res["b_dgrid"] = (K_DG + n_dG) * EPS * S_dG + C_dG
    return res


def tv_all(grids, g=1.0, dtype=np.float64, budgets=False):
    """{'tv', 'dgrids'} (+ 'b_tv', 'b_dgrids') of grids [N,12,L,Gh,Gw] and the upstream gradient g."""
    G = grids.astype(dtype)
    N = G.shape[0]
    tv, S, n_add = dtype(0), 0.0, 0
    dG, SdG = np.zeros_like(G), np.zeros_like(G)
    for axis in (2, 3, 4):
        if G.shape[axis] < 2:
            continue
        d = np.diff(G, axis=axis)
        inv = dtype(1) / dtype(d[0].size)
        tv += (d * d).sum() * inv / dtype(N)
        n_add += d.size
        k = dtype(2) * dtype(g) * inv / dtype(N)
        lo = [slice(None)] * 5
        hi = [slice(None)] * 5
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        dG[tuple(hi)] += k * d
        dG[tuple(lo)] -= k * d
        SdG[tuple(hi)] += abs(k) * np.abs(d)
        SdG[tuple(lo)] += abs(k) * np.abs(d)
    res = {"tv": tv, "dgrids": dG}
    if budgets:
        res["b_tv"] = (K_TV + n_add) * EPS * float(tv)          # every addend is >= 0: S = the value
        res["b_dgrids"] = K_DTV * EPS * SdG
    return res


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def make_inputs(case):
    """(grid, img, dout) float32 of a case, deterministic.  `wide` images are drawn in [-0.3, 1.3] around a shared base so that
    the luminance saturates at both ends; `dark` ones in [-0.3, -0.01] (gz = 0 everywhere: the upper z nodes are never reached).
    Then the green channel of every pixel whose fp64 z (L - 1) is within GZ_MARGIN of an integer is nudged until none is."""
    L, Gh, Gw, H, W, kind = case
    rng = np.random.default_rng(1000 * L + 100 * Gh + 10 * Gw + H * W)
    grid = (np.eye(3, 4).reshape(12, 1, 1, 1) + rng.normal(0.0, 0.3, (12, L, Gh, Gw))).astype(np.float32)
    if kind == "dark":
        img = rng.uniform(-0.3, -0.01, (3, H, W))
    else:
        img = np.clip(rng.uniform(-0.3, 1.3, (1, H, W)) + rng.uniform(-0.15, 0.15, (3, H, W)), -0.3, 1.3)
    img = img.astype(np.float32)
    if L > 1:
        step = np.float32(4.0 * GZ_MARGIN / (L - 1))               # moves z (L - 1) by 0.587 * 4e-3
        for _ in range(64):
            zs = luminance_scaled(img, L)
            near = np.abs(zs - np.round(zs)) < GZ_MARGIN
            if not near.any():
                break
            img[1][near] += step
        else:
            raise AssertionError("the nudge did not converge")
    dout = rng.normal(0.0, 1.0, (3, H, W)).astype(np.float32)
    return grid, img, dout


class Reference:
    def __init__(self, case):
        self.case = case
        self.grid, self.img, self.dout = make_inputs(case)
        self.r64 = slice_all(self.grid, self.img, self.dout, np.float64, budgets=True)

    def ratio(self, what, got):
        return ratio(got, self.r64[what], self.r64["b_" + what])


def ratio(got, want, budget):
    """max |got - want| / budget; an element of budget 0 must be exact (inf otherwise)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    budget = np.broadcast_to(np.asarray(budget, np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(budget > 0, err / budget, np.where(err == 0, 0.0, np.inf))
    return float(r.max())


@functools.lru_cache(maxsize=None)
def reference(case):
    return Reference(case)


def make_grids(tv_case):
    N, L, Gh, Gw = tv_case
    rng = np.random.default_rng(7 + N * 1000 + L * 100 + Gh * 10 + Gw)
    return (np.eye(3, 4).reshape(1, 12, 1, 1, 1) + rng.normal(0.0, 0.3, (N, 12, L, Gh, Gw))).astype(np.float32)


TV_G = -1.75


@functools.lru_cache(maxsize=None)
def tv_reference(tv_case):
    grids = make_grids(tv_case)
    return grids, tv_all(grids, TV_G, np.float64, budgets=True)
