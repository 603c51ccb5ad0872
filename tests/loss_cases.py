"""Shapes, image contents and error budgets of the fused L1 / SSIM loss (a helper, not a test): shared by
tests/test_loss_edges.py (CPU: the budget has teeth) and tests/test_loss_edges_gpu.py (the HIP kernels of csrc/loss.hip).

The kernel works on TILE x TILE output tiles of one channel with a halo of 5 and filters in groups of four columns / rows; the
oracle (oracle/loss_ref.py) knows none of that and takes the tile size as an argument.  Each size below is the smallest at which
one mechanism can go wrong, as a height and as a width:
   1  one pixel: ten of the eleven taps are padding, one thread of the workgroup writes
   4  exactly one register group of four outputs, the rest of the row is out of the image
   5  the halo's own width: every tap at distance 5 is padding
   6  the first size at which a tap at distance 5 reads a pixel
  10  one short of the window: no pixel has its whole support inside the image
  11  the window: only the centre pixel has its whole support inside the image
  27  the last pixel's taps end on column 31: INSIDE the tile but outside the image, zero by the bounds test alone
  28  a multiple of four: the tile's last register group lies wholly outside the image
  31  one short of the tile: one idle output lane per row, the right halo is all padding
  32  exactly one tile: no second tile, the halo on every side is padding
  33  a second tile one pixel wide, whose whole filter support is the first tile's interior
  37  the second tile's five columns are exactly what the first tile's halo reads (columns 32..36)
  38  the first column (37) that no tap of the first tile reaches
  64  two full tiles: halos cross the border both ways and there is no edge tile
  65  three tiles: full, full, one pixel
C = 1..4 moves the channel stride of the map buffer ([3][C][H][W]) and the partials' order (channel, tile row, tile column).

Contents (numpy, one fixed seed per case):
  noise  gt uniform 0..1, img = clip(gt + 0.1 N): the generic case; it carries the tap-level sensitivity
  same   img == gt: L1 exactly 0, sign(0) = 0, SSIM = 1
  flat   0.5 everywhere, img steps to 0.75 on the right half: zero variance, e11 - mu^2 cancels against C2 = 9e-4
  sat    gt = 1, the lower half of img = 0
  black  gt = 0, img sparse 1e-3: the denominators sit at C1 C2
  hdr    values up to 8
  smooth a low-frequency sinusoid, img = gt + 0.01 N
  eq_px  noise with every third pixel of img equal to gt: sign 0 and sign +-1 inside one tile

Error budget of a case and a per-pixel quantity q (the SSIM map, the three derivative maps, a gradient): measured from the oracle,
never from the kernel.  E_q = max over pixels |q(fp32 oracle) - q(fp64 oracle)|; a value passes at pixel p when
    |q[p] - q_fp64[p]| <= FACTOR E_q + FACTOR eps32 max|q_fp64|,   FACTOR = 4:
the kernel and the fp32 oracle are two fp32 evaluations of the same sums in the same tap order (they differ by FMA contraction
and the division forms), each within about E of fp64; the remaining factor of two is there because E is a sample maximum, not a
bound.  Per-tile sums: FACTOR |sum32 - sum64| + 1e-6 (pixels of the tile inside the image).  Scalars: L1 1e-6 (absolute),
SSIM FACTOR |s32 - s64| + 2e-6: the floors tests/test_loss.py uses.
"""
import functools
import zlib

import numpy as np

from oracle import loss_ref

TILE = 32
FACTOR = 4.0
EPS32 = float(np.finfo(np.float32).eps)
SIZES = (1, 4, 5, 6, 10, 11, 27, 28, 31, 32, 33, 37, 38, 64, 65)
SHAPES = [
    (1, 1, 1), (2, 4, 5),                                                  # both dimensions inside the halo
    (2, 37, 1), (3, 65, 4), (4, 38, 5), (3, 33, 6), (2, 64, 10), (3, 37, 11), (3, 38, 27), (4, 33, 28), (3, 38, 31),
    (3, 1, 65), (2, 4, 37), (2, 5, 43), (3, 6, 33), (4, 10, 38), (3, 11, 64), (2, 27, 33), (3, 28, 65), (3, 31, 37),
    (3, 32, 33), (3, 64, 32),
    (3, 33, 65), (4, 33, 33), (2, 65, 38),                                 # four tiles and more: an interior corner
]
CLASSES = ("noise", "same", "flat", "sat", "black", "hdr", "smooth", "eq_px")
CLASS_SHAPES = [(1, 1, 1), (2, 5, 43), (3, 33, 65), (3, 64, 32)]
CASES = [(s, "noise") for s in SHAPES] + [(s, c) for c in CLASSES[1:] for s in CLASS_SHAPES]
NOISE_CASES = [c for c in CASES if c[1] == "noise"]
BIG_CASES = [((3, 289, 321), "noise"), ((1, 33, 8200), "noise")]       # 330 and 257 partials: the finish kernel's second trip
MAPS = ("dmu1", "ds1", "ds12")
G_PAIRS = ((1.0, 0.0), (0.0, 1.0), (0.8, -0.2))
G_DEFAULT = (0.8, -0.2)                                                 # d[(1 - l) L1 + l (1 - SSIM)], l = 0.2


def case_id(case):
    (C, H, W), cls = case
    return f"{cls}-{C}x{H}x{W}"


def images(shape, cls):
    """(img, gt), float32 [C,H,W]."""
    C, H, W = shape
    r = np.random.default_rng(zlib.crc32(repr((tuple(shape), cls)).encode()))
    if cls in ("noise", "eq_px"):
        gt = r.random(shape)
        img = np.clip(gt + 0.1 * r.normal(size=shape), 0.0, 1.0)
        if cls == "eq_px":
            eq = (np.arange(C * H * W) % 3 == 0).reshape(shape)
            img = np.where(eq, gt, img)
    elif cls == "same":
        gt = r.random(shape)
        img = gt.copy()
    elif cls == "flat":
        gt = np.full(shape, 0.5)
        img = gt.copy()
        img[:, :, W // 2:] = 0.75
    elif cls == "sat":
        gt = np.ones(shape)
        img = gt.copy()
        img[:, H // 2:, :] = 0.0
    elif cls == "black":
        gt = np.zeros(shape)
        img = np.where(r.random(shape) < 0.07, 1e-3, 0.0)
    elif cls == "hdr":
        gt = 8.0 * r.random(shape)
        img = np.clip(gt + 0.8 * r.normal(size=shape), 0.0, 8.0)
    elif cls == "smooth":
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        gt = 0.5 + 0.4 * np.sin(2 * np.pi * (xx / 97.0 + yy / 61.0) + np.arange(C)[:, None, None])
        img = gt + 0.01 * r.normal(size=shape)
    else:
        raise ValueError(cls)
    return np.ascontiguousarray(img, dtype=np.float32), np.ascontiguousarray(gt, dtype=np.float32)


def outputs(img, gt, dtype, tile=TILE, g=G_DEFAULT, filt=None):
    """Everything an implementation of the loss produces, from the oracle in `dtype`: the SSIM map, the three derivative maps, the
    per-tile sums, the two means, the two gradients and their combination `grad` = g[0] dL1 + g[1] dSSIM."""
    o = loss_ref.l1_ssim_terms(img, gt, dtype, tile, filt)
    o["g_l1"], o["g_ssim"] = loss_ref.l1_ssim_grads(img, gt, o["dmu1"], o["ds1"], o["ds12"], dtype, filt)
    o["l1"] = float(o["absdiff"].mean(dtype=np.float64))
    o["ssim_mean"] = float(o["ssim"].mean(dtype=np.float64))
    o["grad"] = combine(o, *g)
    return o


def combine(o, g0, g1):
    dt = o["g_ssim"].dtype.type
    return dt(g0) * o["g_l1"] + dt(g1) * o["g_ssim"]


def tile_pixels(shape, tile=TILE):
    """[C, tile rows, tile columns]: pixels of each tile that lie inside the image."""
    return loss_ref._tile_sums(np.ones(shape, dtype=np.float64), tile)


class Reference:
    """The fp64 oracle of one image pair, the fp32 oracle's distance from it, and the budgets that follow."""

    def __init__(self, img, gt, tile=TILE):
        self.img, self.gt, self.shape, self.tile = img, gt, img.shape, tile
        self.o32, self.o64 = outputs(img, gt, np.float32, tile), outputs(img, gt, np.float64, tile)
        self.npix = tile_pixels(img.shape, tile)
        for o in (self.o32, self.o64):
            for v in o.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)

    # -- per-pixel quantities: "ssim", "dmu1", "ds1", "ds12", or a gradient named by its pair (g0, g1)
    def _pair(self, q):
        if isinstance(q, str):
            return self.o32[q], self.o64[q]
        return combine(self.o32, *q), combine(self.o64, *q)

    def E(self, q):
        a, b = self._pair(q)
        return float(np.abs(a.astype(np.float64) - b).max())

    def budget(self, q, factor=FACTOR):
        return factor * self.E(q) + factor * EPS32 * float(np.abs(self._pair(q)[1]).max())

    def error(self, q, got):
        """|got - fp64| per pixel."""
        ref = self._pair(q)[1]
        got = np.asarray(got)
        assert got.shape == ref.shape, (got.shape, ref.shape)
        return np.abs(got.astype(np.float64) - ref)

    def ratio(self, q, got, factor=FACTOR):
        """max |got - fp64| / budget: <= 1 passes (0 / 0 = 0; a non-finite value never passes)."""
        return _ratio(self.error(q, got), self.budget(q, factor))

    def where(self, q, got):
        """(c, y, x) of the largest error and its offsets inside the tile: for a finding's report."""
        e = self.error(q, got)
        c, y, x = np.unravel_index(int(np.nanargmax(e)), e.shape)
        return {"pixel": (int(c), int(y), int(x)), "in_tile": (int(y) % self.tile, int(x) % self.tile), "error": float(e[c, y, x])}

    # -- per-tile sums and scalars
    def tile_ratio(self, name, got, factor=FACTOR):
        a, b = self.o32[name].astype(np.float64), self.o64[name]
        got = np.asarray(got, dtype=np.float64).reshape(b.shape)
        return _ratio(np.abs(got - b), factor * np.abs(a - b) + 1e-6 * self.npix)

    def l1_ratio(self, got):
        return _ratio(np.abs(np.float64(got) - self.o64["l1"]), 1e-6)

    def ssim_ratio(self, got, factor=FACTOR):
        return _ratio(np.abs(np.float64(got) - self.o64["ssim_mean"]), factor * abs(self.o32["ssim_mean"] - self.o64["ssim_mean"]) + 2e-6)

    def ratios(self, out, factor=FACTOR, g=G_DEFAULT):
        """Ratio per quantity of a whole `outputs`-like dict (whatever of it is present)."""
        r = {}
        for q in ("ssim",) + MAPS:
            if q in out:
                r[q] = self.ratio(q, out[q], factor)
        if "grad" in out:
            r["grad"] = self.ratio(g, out["grad"], factor)
        for q in ("tile_l1", "tile_ssim"):
            if q in out:
                r[q] = self.tile_ratio(q, out[q], factor)
        if "l1" in out:
            r["l1"] = self.l1_ratio(out["l1"])
        if "ssim_mean" in out:
            r["ssim_mean"] = self.ssim_ratio(out["ssim_mean"], factor)
        return r


def _ratio(err, budget):
    err, budget = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(budget, dtype=np.float64), np.shape(err))
    if not np.isfinite(err).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / budget)
    return float(np.max(r)) if r.size else 0.0


@functools.lru_cache(maxsize=None)
def reference(shape, cls):
    """The shared, read-only Reference of a case."""
    img, gt = images(shape, cls)
    img.setflags(write=False)
    gt.setflags(write=False)
    return Reference(img, gt)
