"""The depth-prior losses of contextgs_amd/depth_prior.py in numpy fp64, written from the definition (include/cgs.h above
cgs_depth_prior_fwd), the cases the tests run and the budget of every output.

Definition.  x (rendered), y (prior), m (weight; 1 without a mask, [byte != 0] for bool / uint8), n = H W pixels.  Pixels of m = 0
are selected out before any arithmetic (their x, y may be NaN or Inf) and have gradient +0.
  M = sum m, Sx = sum m x, Sy = sum m y, Sxx = sum m x^2, Syy, Sxy;  Vx = M Sxx - Sx^2, Vy = M Syy - Sy^2, C = M Sxy - Sx Sy
  lstsq: a = C / Vy, b = (Sx - a Sy) / M;  Vy <= 1e-12 M Syy: a = 0, b = Sx / M;  M = 0: a = b = 0
  r = x - (a y + b);  L1 = sum m |r| / N, L2 = sum m r^2 / N, N = M ("mask") or n ("image"), 0 when N = 0 or M = 0
  dL/dx_p = g m_p w(r_p) / N, w = sign(r) or 2 r;  dL/da = -(g / N) sum m w y, dL/db = -(g / N) sum m w  (a given affine only)
  Pearson = 1 - rho, rho = C / sqrt(Vx Vy);  dL/dx_p = g m_p (c2 x_p + c1 y_p + c0) with s = sqrt(Vx Vy), c1 = -M / s,
  c2 = rho M / Vx, c0 = Sy / s - rho Sx / Vx;  Vx <= 1e-12 M Sxx or Vy <= 1e-12 M Syy: L = 1, gradient 0
The moments here are `fsum` of the fp64 products (a sum carried with 64 bits or exactly and rounded once: the reference's own
sums add nothing next to the budgets), and the sums of |r|, r^2, w y, w likewise.

Budgets.  They come from this file alone: u = 2^-53, EPS = 2^-24.
  moment       an fp64 accumulation of n terms in ANY order is within (n - 1) u sum |term| of the exact sum (first order); a product
               of three fp32 factors (a float weight) is rounded once more.  e_q = (n + 2) u sum |term_q| for each of the six.
  closed forms the class E below carries (value, error bound) through +, -, *, /, sqrt: the partial derivative of each operation
               times its operands' bounds, plus one rounding u |result| per operation.  a, b, rho, the Pearson coefficients,
               1 / N and the least-squares L2 value (Vx - a C) / (M N) get their bounds this way from the e_q.  A degenerate branch
               gives exact constants (a = 0; c0 = c1 = c2 = 0, L = 1); the case builder keeps every other case a factor 1000
               away from the threshold on either side, so the branch cannot differ.
  residual     r_p is formed from fp64 coefficients: d r_p = da |y_p| + db + 4 u (|x_p| + |a y_p| + |b|).  A GIVEN (a, b) is
               exact (da = db = 0), and then r_p = 0 is computed as exactly 0 (x_p is then the exactly representable a y_p + b).
  summed value sum m rho(r): (n + 2) u sum m rho(r_p) + sum m d rho_p, d rho = d r (L1) or 2 |r| d r + d r^2 (L2); times 1 / N
               with its bound; 4 u |L| for the last operations.
  output       every output is rounded to fp32 once: + EPS |value|.
  gradient     element v_p = g m_p w(r_p) / N: EPS |v_p| + |v_p| (d(1/N) N + 4 u) + |g| m_p d w_p / N, d w = 2 d r (L2), 0 (L1, see
               below); Pearson: EPS |v_p| + |g| m_p (dc2 |x_p| + dc1 |y_p| + dc0 + 4 u (|c2 x_p| + |c1 y_p| + |c0|)), i.e. the
               coefficient error times (|x_p| + |y_p| + 1).
  da, db       EPS |v| + |v| (d(1/N) N + 4 u) + |g| / N ((n + 2) u sum |term| + sum m d w_p (|y_p| or 1)).
  L1 signs     sign(r_p) is stable when |r_p| > d r_p (or r_p = 0 with a given affine).  `sign_stable` says whether that holds for
               every masked pixel; the case builder's seeds make it hold wherever the fit leaves a residual, and the tests assert
               it.  Where the fit is exact in exact arithmetic (x = y; at most two pixels selected; a constant x) the sign
               of r_p is decided by rounding alone and no seed can change that: there `sign_stable` is False by construction
               (`fit_exact` True) and the budget of such an element is the subgradient interval, |g| m_p / N.
No pixel is excluded from any comparison.
"""
from __future__ import annotations

import functools
import math
import zlib

import numpy as np

U = 2.0 ** -53
EPS = 2.0 ** -24
DEGENERATE = 1e-12
G = -1.75                                       # the upstream gradient of every gradient here

# kernel constants the largest shape is derived from (csrc/depth_prior.hip): a workgroup record per DP_TILE pixels, added by a
# finishing workgroup of DP_THREADS threads
DP_TILE, DP_THREADS = 1024, 256
BIG = (257, 1024)                               # 263168 pixels = 257 records: one more than the finishing workgroup has threads
assert (BIG[0] * BIG[1] + DP_TILE - 1) // DP_TILE == DP_THREADS + 1

# The kernels take 16-byte accesses (4-byte for a byte mask) for every full quad of pixels when every plane is aligned, and go pixel
# by pixel for the last partial quad and when a plane is not aligned.  (16, 64) is one full workgroup tile and BIG is a multiple
# of 4 as well (no partial quad); 1x1 is a partial quad alone; 1x63, 17x33 and 3x1025 end in quads of 3, 1 and 1 pixels.
SHAPES = [(1, 1), (1, 63), (17, 33), (16, 64), (3, 1025), BIG]
MASKS = ("none", "float", "bool", "uint8")
VALUES = ("offset", "neg", "same", "const_prior", "const_render", "zero_mask", "one_pixel", "nonfinite")
MODES = tuple(f"{k}-{al}-{mo}" for k in ("l1", "l2") for al in ("affine", "lstsq", "default") for mo in ("mask", "image")) + \
    ("pearson", "scale_shift")

# (H, W, values, mask): the matrix on every shape with the offset values, then the value cases at 17x33
CASES = [(H, W, "offset", mk) for (H, W) in SHAPES for mk in MASKS] + \
        [(17, 33, v, mk) for v in VALUES[1:5] for mk in ("none", "float")] + \
        [(17, 33, v, mk) for v in VALUES[5:] for mk in ("float", "bool")]


def case_id(case):
    return "-".join(str(v) for v in case)


# ---- (value, error bound) arithmetic ------------------------------------------------------------------------------------------------
class E:
    """A number known to within `err`; every operation adds its partial derivatives times the operands' bounds and one rounding."""

    def __init__(self, val, err=0.0):
        self.val, self.err = float(val), float(err)

    @staticmethod
    def of(v):
        return v if isinstance(v, E) else E(v)

    def _r(self, val, err):
        return E(val, err + U * abs(val))

    def __add__(self, o):
        o = E.of(o)
        return self._r(self.val + o.val, self.err + o.err)

    def __sub__(self, o):
        o = E.of(o)
        return self._r(self.val - o.val, self.err + o.err)

    def __rsub__(self, o):
        return E.of(o) - self

    def __neg__(self):
        return E(-self.val, self.err)

    def __mul__(self, o):
        o = E.of(o)
        return self._r(self.val * o.val, abs(self.val) * o.err + abs(o.val) * self.err + self.err * o.err)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = E.of(o)
        lo = abs(o.val) - o.err
        assert lo > 0, "a divisor not known to be non-zero"
        q = self.val / o.val
        return self._r(q, (self.err + abs(q) * o.err) / lo)

    def __rtruediv__(self, o):
        return E.of(o) / self

    def sqrt(self):
        assert self.val - self.err > 0
        return self._r(math.sqrt(self.val), self.err / (2.0 * math.sqrt(self.val - self.err)))


_WIDE = np.finfo(np.longdouble).eps <= 2.0 ** -63


def fsum(a):
    """The sum of fp64 terms, rounded once for every purpose here: a pairwise sum with a 64-bit significand where the platform's
    long double has one (error below 2^-58 of sum |term|), math.fsum otherwise."""
    a = np.asarray(a, np.float64).ravel()
    return float(np.sum(a, dtype=np.longdouble)) if _WIDE else math.fsum(a.tolist())


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def given_affine(values):
    """The (a, b) of the `affine` modes, float32 values (exact on the device)."""
    a, b = {"neg": (-0.47, 2.95), "same": (0.9, 0.05), "const_render": (0.3, 3.0)}.get(values, (0.0069, 4.0004))
    return float(np.float32(a)), float(np.float32(b))


# seeds other than 0: the cases whose seed 0 leaves some |r_p| of the least-squares L1 residual inside the bound on the device's error in
# r_p (`sign_stable`, checked on the CPU by tests/test_depth_prior.py)
SEEDS = {(257, 1024, "offset", "float"): 1, (257, 1024, "offset", "bool"): 1}


@functools.lru_cache(maxsize=None)
def make_inputs(H, W, values, mask, seed=None):
    """(x, y, mask array or None) of a case: float32 planes, the mask in its own type."""
    seed = SEEDS.get((H, W, values, mask), 0) if seed is None else seed
    rng = np.random.default_rng(zlib.crc32(repr((H, W, values, mask, seed)).encode()))
    y = rng.uniform(0.1, 2.0, (H, W))
    noise = rng.normal(0.0, 1.0, (H, W))
    x = 4.0 + 0.01 * (0.7 * y + 0.3 * noise)
    if values == "neg":
        x = 3.0 - 0.5 * y + 0.05 * noise
    elif values == "same":
        x = y.copy()
    elif values == "const_prior":
        y = np.full((H, W), 0.5)
    elif values == "const_render":
        x = np.full((H, W), 3.25)
    x, y = x.astype(np.float32), y.astype(np.float32)
    if values == "same":
        x = y.copy()
    keep = rng.uniform(size=(H, W)) > 0.3
    keep.flat[0] = True
    if values == "zero_mask":
        keep[:] = False
    elif values == "one_pixel":
        keep[:] = False
        keep[H // 2, W // 3] = True
    m = None
    if mask == "float":
        m = (keep * rng.uniform(0.25, 2.0, (H, W))).astype(np.float32)
    elif mask == "bool":
        m = keep.copy()
    elif mask == "uint8":
        m = (keep * rng.choice([1, 7, 255], size=(H, W))).astype(np.uint8)
    else:
        assert values not in ("zero_mask", "one_pixel", "nonfinite")
    if values == "nonfinite":
        off = np.flatnonzero(~keep)
        bad = np.array([np.nan, np.inf, -np.inf], np.float32)
        x.flat[off] = bad[np.arange(off.size) % 3]
        y.flat[off] = bad[(np.arange(off.size) + 1) % 3]
    for a in (x, y) + ((m,) if m is not None else ()):
        a.setflags(write=False)
    return x, y, m


def weights(m, shape):
    if m is None:
        return np.ones(shape, np.float64)
    if m.dtype == np.float32:
        return m.astype(np.float64)
    return (m != 0).astype(np.float64)


def moments(x, y, w, dtype=np.float64):
    """(M, Sx, Sy, Sxx, Syy, Sxy) over the selected pixels.  float64: math.fsum (the reference).  float32: the products and a running
    sum in float32 — the probe that shows the budgets have teeth."""
    sel = w != 0
    ws, xs, ys = w[sel], x[sel].astype(np.float64), y[sel].astype(np.float64)
    terms = (ws, ws * xs, ws * ys, ws * xs * xs, ws * ys * ys, ws * xs * ys)
    if dtype == np.float64:
        return tuple(fsum(t) for t in terms)
    return tuple(float(np.cumsum(t.astype(np.float32), dtype=np.float32)[-1]) if t.size else 0.0 for t in terms)


class Inputs:
    """The planes of (H, W, values, mask), their moments with bounds, and everything the modes share."""

    def __init__(self, H, W, values, mask, x=None):
        """x: another fp64 plane in place of the case's own (the finite differences of tests/test_depth_prior.py)."""
        self.key = (H, W, values, mask)
        self.x, self.y, self.m = make_inputs(H, W, values, mask)
        if x is not None:
            self.x = x
        self.n = H * W
        self.w = weights(self.m, (H, W))
        self.sel = self.w != 0
        self.xs = np.where(self.sel, self.x, 0).astype(np.float64)      # selected out: never seen
        self.ys = np.where(self.sel, self.y, 0).astype(np.float64)
        self.mom = moments(self.x, self.y, self.w)
        sel, w, xs, ys = self.sel, self.w, self.xs, self.ys
        absterms = (w, w * np.abs(xs), w * np.abs(ys), w * xs * xs, w * ys * ys, w * np.abs(xs * ys))
        self.mom_e = tuple(E(v, (self.n + 2) * U * fsum(t[sel])) for v, t in zip(self.mom, absterms))
        M, Sx, Sy, Sxx, Syy, Sxy = self.mom
        self.Vx, self.Vy = M * Sxx - Sx * Sx, M * Syy - Sy * Sy
        self.degx, self.degy = not self.Vx > DEGENERATE * M * Sxx, not self.Vy > DEGENERATE * M * Syy
        for V, S, deg in ((self.Vx, Sxx, self.degx), (self.Vy, Syy, self.degy)):
            if deg:
                assert abs(V) <= 1e-3 * DEGENERATE * M * S, "a degenerate case must be degenerate by a wide margin"
            else:
                assert V > 1000 * DEGENERATE * M * S, "too close to the degenerate branch"
        # the least-squares residual is identically zero in exact arithmetic: rounding alone decides its sign
        self.fit_exact = values == "same" or int(sel.sum()) <= 2 or self.degx

    @functools.cached_property
    def lstsq(self):
        """(a, b) as E."""
        M, Sx, Sy, Sxx, Syy, Sxy = self.mom_e
        if M.val == 0:
            return E(0.0), E(0.0)
        if self.degy:
            return E(0.0), Sx / M
        a = (M * Sxy - Sx * Sy) / (M * Syy - Sy * Sy)
        return a, (Sx - a * Sy) / M

    def inv_n(self, mean_over):
        M = self.mom_e[0]
        if mean_over == "image":
            return E(1.0) / E(float(self.n))
        return E(1.0) / M if M.val > 0 else E(0.0)


@functools.lru_cache(maxsize=None)
def inputs(H, W, values, mask):
    return Inputs(H, W, values, mask)


# ---- the modes ----------------------------------------------------------------------------------------------------------------------
def affine_mode(inp, kind, align, mean_over, moments_override=None, flip=None, affine=None):
    """{'loss', 'dx', 'a', 'b'} (+ 'da', 'db' for a given affine) and their budgets 'b_*'; `sign_stable` for L1.
    moments_override / flip build the wrong variants of tests/test_depth_prior.py (their budgets mean nothing); `affine` replaces
    the case's given (a, b)."""
    x, y, w, sel, n = inp.xs, inp.ys, inp.w, inp.sel, inp.n
    exact = align != "lstsq"
    if align == "affine":
        a, b = (E(v) for v in (affine or given_affine(inp.key[2])))
    elif align == "default":
        a, b = E(1.0), E(0.0)
    elif moments_override is not None:
        a, b = (E(v) for v in lstsq_plain(moments_override))
    else:
        a, b = inp.lstsq
    inv = inp.inv_n(mean_over)
    if flip == "n_for_m":
        inv = inp.inv_n("image" if mean_over == "mask" else "mask")
    M = inp.mom[0]
    r = x - (a.val * y + b.val)
    dr = a.err * np.abs(y) + b.err + 4 * U * (np.abs(x) + np.abs(a.val * y) + abs(b.val))
    if exact:
        dr = np.where(r == 0, 0.0, dr)
    l1 = kind == "l1"
    rho = np.abs(r) if l1 else r * r
    drho = dr if l1 else 2 * np.abs(r) * dr + dr * dr
    S = fsum((w * rho)[sel])
    dS = (n + 2) * U * S + fsum((w * drho)[sel])
    res = {"a": a.val, "b": b.val, "b_a": a.err + EPS * abs(a.val), "b_b": b.err + EPS * abs(b.val)}
    loss = S * inv.val if M > 0 else 0.0
    res["loss"] = loss
    res["b_loss"] = dS * inv.val + S * inv.err + 4 * U * abs(loss) + EPS * abs(loss)
    if kind == "l2" and align == "lstsq" and M > 0 and moments_override is None:
        # the closed form (Vx - a C) / (M N), carried from the moments' bounds
        Me, Sx, Sy, Sxx, Syy, Sxy = inp.mom_e
        closed = ((Me * Sxx - Sx * Sx) - a * (Me * Sxy - Sx * Sy)) / Me * inv
        res["b_loss"] = closed.err + abs(closed.val - loss) + EPS * abs(loss)
    wr = np.sign(r) if l1 else 2 * r
    dw = np.zeros_like(r) if l1 else 2 * dr
    sgn = -1.0 if flip == "sign" else 1.0
    k = sgn * G * inv.val
    dx = np.where(sel & (wr != 0), k * w * wr, 0.0)
    rel =(inv.err / inv.val if inv.val > 0 else 0.0) + 4 * U
    b_dx = EPS * np.abs(dx) + np.abs(dx) * rel + abs(k) * w * dw
    if l1:
        unstable = sel & ~((np.abs(r) > dr) | (exact & (r == 0)))
        res["sign_stable"] = not unstable.any()
        b_dx = b_dx + np.where(unstable, abs(k) * w, 0.0)
    res["dx"], res["b_dx"] = dx, b_dx
    if align != "lstsq":
        for name, f in (("da", y), ("db", np.ones_like(y))):
            t = (w * wr * f)[sel]
            v = -k * fsum(t)
            res[name] = v
            res["b_" + name] = EPS * abs(v) + abs(v) * rel + abs(k) * ((n + 2) * U * fsum(np.abs(t)) + fsum((w * dw * np.abs(f))[sel]))
    return res


def lstsq_plain(mom):
    """(a, b) of six plain numbers by the closed form (for the float32-moment probe)."""
    M, Sx, Sy, Sxx, Syy, Sxy = mom
    if M == 0:
        return 0.0, 0.0
    Vy = M * Syy - Sy * Sy
    a = 0.0 if not Vy > DEGENERATE * M * Syy else (M * Sxy - Sx * Sy) / Vy
    return a, (Sx - a * Sy) / M


def pearson_plain(mom):
    """(loss, c0, c1, c2) of six plain numbers."""
    M, Sx, Sy, Sxx, Syy, Sxy = mom
    Vx, Vy, C = M * Sxx - Sx * Sx, M * Syy - Sy * Sy, M * Sxy - Sx * Sy
    if not Vx > DEGENERATE * M * Sxx or not Vy > DEGENERATE * M * Syy:
        return 1.0, 0.0, 0.0, 0.0
    s = math.sqrt(Vx * Vy)
    rho = C / s
    return 1.0 - rho, Sy / s - rho * Sx / Vx, -M / s, rho * M / Vx


def pearson_mode(inp, moments_override=None, flip=None):
    x, y, w, sel = inp.xs, inp.ys, inp.w, inp.sel
    if moments_override is not None:
        loss, c0, c1, c2 = pearson_plain(moments_override)
        return {"loss": loss, "dx": np.where(sel, G * w * (c2 * x + c1 * y + c0), 0.0)}
    sgn = -1.0 if flip == "sign" else 1.0
    if inp.degx or inp.degy:
        z = np.zeros_like(x)
        return {"loss": 1.0, "b_loss": 0.0, "dx": z, "b_dx": z}
    M, Sx, Sy, Sxx, Syy, Sxy = inp.mom_e
    Vx, Vy, C = M * Sxx - Sx * Sx, M * Syy - Sy * Sy, M * Sxy - Sx * Sy
    s = (Vx * Vy).sqrt()
    rho = C / s
    loss = 1.0 - rho
    c1, c2, c0 = -(M / s), rho * M / Vx, Sy / s - rho * Sx / Vx
    # the value itself in the centred form, which does not cancel
    t = -((M.val * y - Sy.val) / s.val - rho.val * (M.val * x - Sx.val) / Vx.val)
    dx = np.where(sel, sgn * G * w * t, 0.0)
    dt = c2.err * np.abs(x) + c1.err * np.abs(y) + c0.err + 4 * U * (np.abs(c2.val * x) + np.abs(c1.val * y) + abs(c0.val))
    return {"loss": loss.val, "b_loss": loss.err + EPS * abs(loss.val), "dx": dx, "b_dx": EPS * np.abs(dx) + abs(G) * w * dt}


def scale_shift_mode(inp):
    a, b = inp.lstsq
    return {"a": a.val, "b": b.val, "b_a": a.err + EPS * abs(a.val), "b_b": b.err + EPS * abs(b.val)}


class Reference:
    """One (case, mode): `.r64` holds the values and budgets, `.ratio(name, got)` the largest error over budget."""

    def __init__(self, case, mode, inp=None):
        self.case, self.mode = case, mode
        self.inp = inp if inp is not None else inputs(*case)
        if mode == "pearson":
            self.r64 = pearson_mode(self.inp)
        elif mode == "scale_shift":
            self.r64 = scale_shift_mode(self.inp)
        else:
            self.kind, self.align, self.mean_over = mode.split("-")
            self.r64 = affine_mode(self.inp, self.kind, self.align, self.mean_over)

    def ratio(self, name, got):
        return ratio(got, self.r64[name], self.r64["b_" + name])


def ratio(got, want, budget):
    """max |got - want| / budget; an element of budget 0 must be exact (inf otherwise); a non-finite `got` is inf."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - want)
    budget = np.broadcast_to(np.asarray(budget, np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(budget > 0, err / budget, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(got), r, np.inf)
    return float(r.max())


@functools.lru_cache(maxsize=None)
def reference(case, mode=None):
    """reference(case) with a 5-tuple (H, W, values, mask, mode), or reference((H, W, values, mask), mode)."""
    if mode is None:
        case, mode = tuple(case[:4]), case[4]
    return Reference(tuple(case), mode)
