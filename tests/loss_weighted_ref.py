"""The weighted / exposed training image loss from the oracle (a helper, not a test): shared by tests/test_loss_weighted.py (CPU:
the maths and the budget's teeth) and tests/test_loss_weighted_gpu.py (the `l1_ssim_w_*` kernels of csrc/loss.hip).

Built only from oracle.loss_ref.l1_ssim_terms / l1_ssim_grads (the unweighted filters) and numpy, in a given dtype:
    x'_c = sum_k x_k E[k,c] + E[c,3]                       (exposure E [3,4]; without it x' = x)
    S = sum_p w_p,  L1 = sum w |x' - y| / (C S),  SSIM = sum w ssim(x', y) / (C S),  (0, 1) when S == 0
    the SSIM map and the three derivative maps of (x', y) times w: what the forward kernel keeps
    G = dL/dx' from the WEIGHTED maps through the unweighted backward filter, the L1 part w sign(x' - y) / (C S)
    dL/dx_k = sum_c E[k,c] G_c,  dL/dE[k,c] = sum_p x_k G_c,  dL/dE[c,3] = sum_p G_c
It knows nothing of tiles except the tile size it is handed for the per-tile sums; the fp32 form of dE sums each tile in fp32 and
the tiles in fp64.

Budgets follow loss_cases.Reference with the same FACTOR = 4, every one measured from the oracle and never from the kernel:
  per-pixel quantities   FACTOR max|q32 - q64| + FACTOR eps32 max|q64|
  per-tile sums          FACTOR |sum32 - sum64| + 1e-6 (pixels of the tile inside the image)
  scalars                L1 1e-6 absolute; SSIM FACTOR |s32 - s64| + 2e-6
  dE, per entry          FACTOR |dE32 - dE64| + FACTOR eps32 sum_p |term_p|, term_p = x_k(p) G_c(p) or G_c(p) in fp64: the
                         any-order fp32 summation bound times the same factor (the kernel's order is not the oracle's)
`wrong=` states five deliberately wrong variants for the CPU test of the budget's teeth.
"""
import functools
import zlib

import numpy as np

import loss_cases as lc
from oracle import loss_ref

FACTOR, EPS32, TILE = lc.FACTOR, lc.EPS32, lc.TILE
MAPS = lc.MAPS
WEIGHTS = ("ones", "soft", "binary", "left0", "zero")
EXPOSURES = ("identity", "generic", "perm")
PERM = (2, 0, 1)                                  # x'_c = x_PERM[c]
WRONG = ("E_T", "bias_row", "norm_chw", "w_inputs", "l1_unweighted")

# (shape, content, weight pattern or None, exposure or None): the smallest shapes of loss_cases.SIZES at which each mechanism can
# go wrong.  Weights only: one pixel, inside the halo, four tiles with C = 4, C = 2, three tile columns, two tile rows.  With an
# exposure (C = 3): one row of three tiles, a tap at distance 5, 37 / 38 (the neighbour tile's halo), 27 / 31 (in-tile columns
# outside the image), a one-pixel second tile, two tile rows, an interior corner.
W_SHAPES = [(1, 1, 1), (2, 4, 5), (4, 33, 33), (2, 65, 38), (3, 33, 65), (3, 64, 32)]
E_SHAPES = [(3, 1, 65), (3, 33, 6), (3, 37, 11), (3, 38, 27), (3, 38, 31), (3, 32, 33), (3, 64, 32), (3, 33, 65)]
# the finish loops' second trip (256 threads): 330 forward partials; 2 x 129 = 258 tiles of dE partials (and 774 forward partials)
BIG_CASES = [((3, 289, 321), "noise", "soft", "generic"), ((3, 33, 4100), "noise", "soft", "generic")]
CASES = ([(s, "noise", p, None) for s in W_SHAPES for p in WEIGHTS]
         + [(s, "noise", p, e) for s in E_SHAPES for p, e in ((None, "identity"), (None, "perm"), (None, "generic"), ("soft", "generic"))]
         + [(s, "noise", "left0", "generic") for s in E_SHAPES if s[2] > 32]
         + [((3, 33, 65), cls, p, e) for cls in ("eq_px", "flat")
            for p, e in (("soft", None), ("left0", None), (None, "generic"), ("binary", "generic"), ("left0", "generic"))])
TEETH_CASES = [((3, 33, 65), "noise", "soft", "generic"), ((3, 38, 27), "noise", "binary", "generic"),
               ((3, 33, 65), "noise", "left0", "generic")]


def weight(shape, pattern):
    """float32 [H,W]."""
    C, H, W = shape
    r = np.random.default_rng(zlib.crc32(repr((tuple(shape), "w", pattern)).encode()))
    if pattern == "ones":
        w = np.ones((H, W))
    elif pattern == "soft":
        w = r.random((H, W))
    elif pattern == "binary":                      # random 8 x 8 blocks of 0 / 1; the first block is 1 so that S > 0 at every shape
        b = r.random((-(-H // 8), -(-W // 8))) < 0.5
        b[0, 0] = True
        w = np.kron(b, np.ones((8, 8)))[:H, :W]
    elif pattern == "left0":                       # the first tile column carries no weight
        w = np.ones((H, W))
        w[:, :32] = 0.0
    elif pattern == "zero":
        w = np.zeros((H, W))
    else:
        raise ValueError(pattern)
    return np.ascontiguousarray(w, dtype=np.float32)


def exposure(name):
    """float32 [3,4]: the 3x3 colour matrix (x' = x @ E[:, :3]) and the bias column."""
    if name == "identity":
        E = np.eye(3, 4)
    elif name == "generic":                        # off-diagonal entries of both signs, a bias of both signs
        E = np.array([[1.10, -0.07, 0.04, 0.03],
                      [0.06, 0.92, -0.09, -0.02],
                      [-0.05, 0.08, 1.05, 0.01]])
    elif name == "perm":
        E = np.zeros((3, 4))
        for c, k in enumerate(PERM):
            E[k, c] = 1.0
    else:
        raise ValueError(name)
    return np.ascontiguousarray(E, dtype=np.float32)


def expose(x, E, wrong=None):
    """x' of x [3,H,W] in x's dtype."""
    if E is None:
        return x
    E = E.astype(x.dtype)
    M = E[:, :3].T if wrong == "E_T" else E[:, :3]
    bias = E.reshape(4, 3)[3] if wrong == "bias_row" else E[:, 3]
    return np.stack([(x[0] * M[0, c] + x[1] * M[1, c]) + x[2] * M[2, c] + bias[c] for c in range(3)])


def outputs(img, gt, w, E, dtype, tile=TILE, wrong=None):
    """Everything an implementation produces, from the oracle in `dtype`; w [H,W] or None, E [3,4] or None."""
    C, H, W = img.shape
    x, y = img.astype(dtype), gt.astype(dtype)
    wd = (np.ones((H, W)) if w is None else w).astype(dtype)
    xp = expose(x, E, wrong)
    xin, yin, wmap = (xp * wd, y * wd, np.ones((H, W), dtype=dtype)) if wrong == "w_inputs" else (xp, y, wd)
    t = loss_ref.l1_ssim_terms(xin, yin, dtype, tile)
    o = {"x": x, "xp": xp, "E": None if E is None else E.astype(dtype), "w": wd}
    for q in ("ssim", "absdiff") + MAPS:
        o[q] = t[q] * wmap
    w3 = np.ascontiguousarray(np.broadcast_to(wd, (C, H, W)))
    o["tile_l1"], o["tile_ssim"], o["tile_w"] = (loss_ref._tile_sums(a, tile) for a in (o["absdiff"], o["ssim"], w3))
    cs = float(C) * float(wd.sum(dtype=np.float64))
    if wrong == "norm_chw":
        cs = float(C * H * W)
    o["cs"] = cs
    if cs > 0.0:
        o["l1"], o["ssim_mean"] = float(o["absdiff"].sum(dtype=np.float64)) / cs, float(o["ssim"].sum(dtype=np.float64)) / cs
        # l1_ssim_grads divides by the pixel count: put C S in its place
        scale = dtype(float(x.size) / cs)
        g_l1, g_ssim = loss_ref.l1_ssim_grads(xin, yin, o["dmu1"], o["ds1"], o["ds12"], dtype)
        o["G_l1"] = g_l1 * (scale if wrong == "l1_unweighted" else scale * wd)
        o["G_ssim"] = g_ssim * (scale * wd if wrong == "w_inputs" else scale)        # (the chain rule of the wrong variant's own inputs)
    else:
        o["l1"], o["ssim_mean"] = 0.0, 1.0
        o["G_l1"], o["G_ssim"] = np.zeros_like(x), np.zeros_like(x)
    o["tile"] = tile
    return o


def loss_value(o, lam=0.2):
    return (1.0 - lam) * o["l1"] + lam * (1.0 - o["ssim_mean"])


def grads(o, g0, g1):
    """(dL/dx [C,H,W], dL/dE [3,4] or None, sum_p |term_p| [3,4] or None) of L = g0 L1 + g1 SSIM."""
    dt = o["x"].dtype.type
    G = dt(g0) * o["G_l1"] + dt(g1) * o["G_ssim"]
    E = o["E"]
    if E is None:
        return G, None, None
    x = o["x"]
    dx = np.stack([(E[k, 0] * G[0] + E[k, 1] * G[1]) + E[k, 2] * G[2] for k in range(3)])
    dE, mag = np.zeros((3, 4)), np.zeros((3, 4))
    for c in range(3):
        terms = [x[k] * G[c] for k in range(3)] + [G[c]]
        for k, term in enumerate(terms):
            at = (k, c) if k < 3 else (c, 3)
            dE[at] = loss_ref._tile_sums(term[None], o["tile"]).sum(dtype=np.float64)       # a tile in `dtype`, the tiles in fp64
            mag[at] = np.abs(term.astype(np.float64)).sum()
    return dx, dE, mag


class WeightedReference:
    """The fp64 oracle of one (image pair, weight, exposure), the fp32 oracle's distance from it, and the budgets that follow."""

    def __init__(self, img, gt, w, E, tile=TILE):
        self.img, self.gt, self.w, self.Em, self.shape, self.tile = img, gt, w, E, img.shape, tile
        self.o32, self.o64 = outputs(img, gt, w, E, np.float32, tile), outputs(img, gt, w, E, np.float64, tile)
        self.npix = lc.tile_pixels(img.shape, tile)
        for o in (self.o32, self.o64):
            for v in o.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)

    @functools.lru_cache(maxsize=None)
    def _grads(self, pair):
        return grads(self.o32, *pair), grads(self.o64, *pair)

    def _pair(self, q):
        if isinstance(q, str):
            return self.o32[q], self.o64[q]
        g32, g64 = self._grads(tuple(float(v) for v in q))
        return g32[0], g64[0]

    def budget(self, q, factor=FACTOR):
        a, b = self._pair(q)
        return factor * float(np.abs(a.astype(np.float64) - b).max()) + factor * EPS32 * float(np.abs(b).max())

    def error(self, q, got):
        ref = self._pair(q)[1]
        got = np.asarray(got)
        assert got.shape == ref.shape, (got.shape, ref.shape)
        return np.abs(got.astype(np.float64) - ref)

    def ratio(self, q, got, factor=FACTOR):
        """max |got - fp64| / budget of a per-pixel quantity: a weighted map by name, or dL/dx by its pair (g0, g1)."""
        return lc._ratio(self.error(q, got), self.budget(q, factor))

    def dE_ratio(self, pair, got, factor=FACTOR):
        g32, g64 = self._grads(tuple(float(v) for v in pair))
        got = np.asarray(got, dtype=np.float64).reshape(3, 4)
        return lc._ratio(np.abs(got - g64[1]), factor * np.abs(g32[1] - g64[1]) + factor * EPS32 * g64[2])

    def tile_ratio(self, name, got, factor=FACTOR):
        a, b = self.o32[name].astype(np.float64), self.o64[name]
        got = np.asarray(got, dtype=np.float64).reshape(b.shape)
        return lc._ratio(np.abs(got - b), factor * np.abs(a - b) + 1e-6 * self.npix)

    def l1_ratio(self, got):
        return lc._ratio(np.abs(np.float64(got) - self.o64["l1"]), 1e-6)

    def ssim_ratio(self, got, factor=FACTOR):
        return lc._ratio(np.abs(np.float64(got) - self.o64["ssim_mean"]),
                         factor * abs(self.o32["ssim_mean"] - self.o64["ssim_mean"]) + 2e-6)

    def ratios(self, out, factor=FACTOR, g=lc.G_DEFAULT):
        """Ratio per quantity of an `outputs`-like dict of another implementation (whatever of it is present)."""
        r = {}
        for q in ("ssim",) + MAPS:
            if q in out:
                r[q] = self.ratio(q, out[q], factor)
        for q in ("tile_l1", "tile_ssim", "tile_w"):
            if q in out:
                r[q] = self.tile_ratio(q, out[q], factor)
        if "l1" in out:
            r["l1"] = self.l1_ratio(out["l1"])
        if "ssim_mean" in out:
            r["ssim_mean"] = self.ssim_ratio(out["ssim_mean"], factor)
        if "G_l1" in out:
            dx, dE, _ = grads(out, *g)
            r["grad"] = self.ratio(g, dx, factor)
            if dE is not None:
                r["dE"] = self.dE_ratio(g, dE, factor)
        return r


@functools.lru_cache(maxsize=None)
def reference(shape, cls, wname, ename):
    """The shared, read-only WeightedReference of a case: contents of loss_cases.images, a weight pattern or None, an exposure or None."""
    img, gt = lc.images(shape, cls)
    img.setflags(write=False)
    gt.setflags(write=False)
    return WeightedReference(img, gt, None if wname is None else weight(shape, wname), None if ename is None else exposure(ename))


def case_id(case):
    shape, cls, wname, ename = case
    return f"{lc.case_id((shape, cls))}-w:{wname}-E:{ename}"
