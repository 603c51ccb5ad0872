"""fp64 restatement of the discretised-Gaussian rate (a helper, not a test): utils/entropy_models.py:37-50.

Written from the definition, not from csrc/rate_math.h:
  xc   = clamp(x, x_mean - 15000 q, x_mean + 15000 q)   (use_clamp; detached bounds, gradient 1 on the edges)
  s    = max(scale, 1e-9)                               (the bound as the fp32 reference holds it: float32(1e-9))
  zu   = (xc + q/2 - mean) / (s sqrt 2),  zl = (xc - q/2 - mean) / (s sqrt 2)
  lik  = |Phi(xc + q/2) - Phi(xc - q/2)| = 0.5 (erfc(zl) - erfc(zu)) for zl > 0, 0.5 (erfc(-zu) - erfc(-zl)) otherwise:
         a difference of two SMALL numbers on either side, so the tails lose nothing to cancellation
  bits = -log2(max(lik, 1e-6)), gradient zero where lik < 1e-6 (Low_bound, :141-156; the bound is float32(1e-6) there)
and the gradients by autograd.

The error unit of one element is u = 6e-8 / lik + 1e-6 (1 + max(zu^2, zl^2)): one fp32 spacing near 1 in each CDF relative to
the likelihood, plus a few roundings of z carried through exp(-z^2).  bits are measured in u / ln 2 (plus LOG_FLOOR
max(1, |bits|), the absolute error of a hardware log2 near an argument of 1), the gradients in u M (plus 2^-126: fp32 results
below it may be flushed to zero) with
  g_z = log2(e) / lik pi^-1/2 exp(-z^2),  k = 1 / (s sqrt 2)
  M_x = M_mean = (|g_zu| + |g_zl|) k,  M_q = M_x / 2,  M_scale = (|g_zu zu| + |g_zl zl|) / s       (each times |g_bits|).

Classes of an element (fp64 values):
  dead       exp(-z^2) underflows for both edges (tiny scales): lik is exactly 0 or 1, bits the bound's or exactly 0, gradients 0
  bounded    lik < 1e-6 - 3e-7: bits = -log2(float32(1e-6)) within 1e-5, gradients exactly 0
  undecided  |lik - 1e-6| <= 3e-7: fp32 may land on either side of the bound; either outcome is accepted
  unit       everything else: errors in units

Inputs (`draw`) are exact on a grid: x - mean, mean and x_mean are multiples of 2^-12, q a positive multiple of 2^-11, so
x +- q/2 - mean is exact in fp32 and the rounding of that difference (up to 9e-5 of the likelihood on generic inputs, shared by
the reference's fp32 formula and the kernels) hides nothing.  `scale` is any fp32 value.
"""
import functools
import math

import numpy as np
import torch

SQRT2 = math.sqrt(2.0)
LOG2E = 1.0 / math.log(2.0)
BOUND = float(np.float32(1e-6))
MIN_SCALE = float(np.float32(1e-9))
BITS_BOUND = -math.log2(BOUND)
BAND = 3e-7
LOG_FLOOR = 4 * 2.0 ** -22
FLUSH = 2.0 ** -126                   # a gradient below the smallest normal fp32 number may be flushed to zero
SUM_RTOL = 2e-5                       # summation allowance of a sum of elements (the one test_level_rate grants)
GRID, QGRID = 2.0 ** -12, 2.0 ** -11
NAMES = ("bits", "gx", "gm", "gs", "gq")
REGIMES = ("body", "switch", "tail", "tiny", "clamp")


class _LowBound(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lik, bound):
        ctx.save_for_backward(lik)
        ctx.bound = bound
        return lik.clamp(min=bound)

    @staticmethod
    def backward(ctx, g):
        lik, = ctx.saved_tensors
        return torch.where(lik < ctx.bound, torch.zeros_like(g), g), None


def _t64(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def _leaves(x, mean, scale, q, dtype):
    shape = np.broadcast_shapes(*(np.shape(a) for a in (x, mean, scale, q)))
    return [_t64(np.broadcast_to(np.asarray(a, dtype=np.float64), shape)).to(dtype).requires_grad_(True) for a in (x, mean, scale, q)]


def _clamped(x, q, x_mean, use_clamp):
    if not use_clamp:
        return x
    xm = _t64(x_mean).to(x.dtype)
    return torch.clamp(x, min=(xm - 15000 * q).detach(), max=(xm + 15000 * q).detach())


class Ref:
    """Per-element fp64 values of one call (numpy arrays of the broadcast shape) and the tolerance of every output."""

    def errors(self, units, **got):
        """Checks the outputs `got` (any of bits, gx, gm, gs, gq; arrays of the reference's shape) element by element: the
        dead, bounded and undecided classes by their exact statements (AssertionError), the rest -> {name: error in units}
        (arrays; nan outside the unit class).  `units` scales the bound the undecided elements may use."""
        out = {}
        for name, a in got.items():
            a = np.asarray(a, dtype=np.float64).reshape(self.bits.shape)
            want = getattr(self, name)
            assert np.isfinite(a).all(), (name, "not finite", int((~np.isfinite(a)).sum()))
            want = np.where(self.undecided, self.free[name], want)
            err = np.maximum(np.abs(a - want) - (self.floor if name == "bits" else FLUSH), 0.0)
            one = np.where(self.unit | self.undecided, self.tol1[name], 1.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                err = np.where(one > 0, err / one, np.where(err == 0, 0.0, np.inf))       # (g_bits == 0: exactly 0)
            if name == "bits":
                full = self.dead & (self.lik == 1)
                assert (a[full] == 0).all() and (np.abs(a[self.dead & ~full] - BITS_BOUND) <= 1e-5).all(), (name, "dead")
                assert (np.abs(a[self.bounded] - BITS_BOUND) <= 1e-5).all(), (name, "bounded", a[self.bounded])
                floored = np.abs(a - BITS_BOUND) <= 1e-5
            else:
                assert (a[self.dead] == 0).all(), (name, "dead")
                assert (a[self.bounded] == 0).all(), (name, "bounded", a[self.bounded][a[self.bounded] != 0])
                floored = a == 0
            assert (floored | (err <= units))[self.undecided].all(), (name, "undecided")
            out[name] = np.where(self.unit, err, np.nan)
        return out

    def tol(self, name, units):
        """Absolute tolerance of every element's `name` at `units` units (0 for dead, 1e-5 / 0 for bounded elements)."""
        t = np.where(self.unit, units * self.tol1[name] + (self.floor if name == "bits" else FLUSH), 0.0)
        assert not self.undecided.any()
        return t + (1e-5 * (self.bounded | (self.dead & (self.lik == 0))) if name == "bits" else 0.0)

    def sum_tol(self, name, units, weight, axes=None, index=None, size=None):
        """Tolerance of sum(weight * name) over `axes`, or scattered by `index` into `size` bins: sum of the elements'
        tolerances plus SUM_RTOL of the sum of magnitudes.  -> (the fp64 sum, its tolerance)."""
        v = getattr(self, name) * weight
        t = self.tol(name, units) * np.abs(weight) + SUM_RTOL * np.abs(v)
        if index is None:
            return v.sum(axis=axes), t.sum(axis=axes)
        return (np.bincount(index.ravel(), v.ravel(), size), np.bincount(index.ravel(), t.ravel(), size))


def likelihood64(X, M, S, Q, x_mean=None, use_clamp=False):
    """(likelihood, zu, zl, clamped scale) of float64 tensors, in the cancellation-free form."""
    xc = _clamped(X, Q, x_mean, use_clamp)
    s = S.clamp(min=MIN_SCALE)
    zu, zl = (xc + 0.5 * Q - M) / s / SQRT2, (xc - 0.5 * Q - M) / s / SQRT2
    lik = torch.abs(torch.where(zl > 0, 0.5 * (torch.erfc(zl) - torch.erfc(zu)), 0.5 * (torch.erfc(-zu) - torch.erfc(-zl))))
    return lik, zu, zl, s


def bits64(X, M, S, Q, x_mean=None, use_clamp=False):
    """bits of float64 tensors (differentiable: what eg_fp64 takes its gradients from)."""
    return -torch.log2(_LowBound.apply(likelihood64(X, M, S, Q, x_mean, use_clamp)[0], BOUND))


def eg_fp64(x, mean, scale, q, x_mean=None, use_clamp=False, g_bits=None):
    """The rate of every element in float64 -> Ref (bits, gx, gm, gs, gq, lik, zu, zl, Mx, Mq, Ms, u and the classes).
    The operands broadcast; gradients are per element of the broadcast shape (a shared q: sum them).  g_bits: upstream
    gradient per element (default 1)."""
    X, M, S, Q = _leaves(x, mean, scale, q, torch.float64)
    gb = np.broadcast_to(np.asarray(1.0 if g_bits is None else g_bits, dtype=np.float64), X.shape)
    lik, zu, zl, s = likelihood64(X, M, S, Q, x_mean, use_clamp)
    bits = -torch.log2(_LowBound.apply(lik, BOUND))
    free = -torch.log2(lik.clamp(min=1e-300))                # without the bound: what an undecided element may also give
    r = Ref()
    n = lambda t: t.detach().numpy()
    r.bits, r.lik, r.zu, r.zl, r.s = n(bits), n(lik), n(zu), n(zl), n(s)
    r.gx, r.gm, r.gs, r.gq = (n(t) for t in torch.autograd.grad((bits * _t64(gb)).sum(), [X, M, S, Q], retain_graph=True))
    r.free = dict(zip(NAMES, [n(free)] + [n(t) for t in torch.autograd.grad((free * _t64(gb)).sum(), [X, M, S, Q])]))
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        lk = np.maximum(r.lik, 1e-300)
        # (+ 2^-126: below it an fp32 exp(-z^2) is flushed to zero)
        gzu = LOG2E / lk / math.sqrt(math.pi) * (np.exp(-r.zu ** 2) + 2.0 ** -126) * np.abs(gb)
        gzl = LOG2E / lk / math.sqrt(math.pi) * (np.exp(-r.zl ** 2) + 2.0 ** -126) * np.abs(gb)
        k = 1.0 / (r.s * SQRT2)
        r.Mx = (gzu + gzl) * k
        r.Mq = 0.5 * r.Mx
        r.Ms = (gzu * np.abs(r.zu) + gzl * np.abs(r.zl)) / r.s
        r.dead = (np.exp(-r.zu ** 2) == 0) & (np.exp(-r.zl ** 2) == 0)
        r.u = np.where(r.dead, 0.0, 6e-8 / lk + 1e-6 * (1 + np.maximum(r.zu ** 2, r.zl ** 2)))
    assert ((r.lik[r.dead] == 0) | (r.lik[r.dead] == 1)).all()
    r.undecided = ~r.dead & (np.abs(r.lik - 1e-6) <= BAND)
    r.bounded = ~r.dead & ~r.undecided & (r.lik < 1e-6)
    r.unit = ~r.dead & ~r.undecided & ~r.bounded
    r.floor = LOG_FLOOR * np.maximum(1.0, np.abs(r.bits))
    # one unit of every output (the floors, LOG_FLOOR of the bits and FLUSH of the gradients, come on top: errors, tol)
    with np.errstate(over="ignore", invalid="ignore"):
        r.tol1 = dict(bits=r.u * LOG2E, gx=r.u * r.Mx, gm=r.u * r.Mx, gs=r.u * r.Ms, gq=r.u * r.Mq)
    return r


def eg_plain_fp64(x, mean, scale, q, x_mean=None, use_clamp=False):
    """The reference's expression as it stands (Normal.cdf), in float64 -> (likelihood, bits)."""
    X, M, S, Q = (t.detach() for t in _leaves(x, mean, scale, q, torch.float64))
    n = torch.distributions.Normal(M, S.clamp(min=MIN_SCALE), validate_args=False)
    xc = _clamped(X, Q, x_mean, use_clamp)
    lik = torch.abs(n.cdf(xc + 0.5 * Q) - n.cdf(xc - 0.5 * Q))
    return lik.numpy(), (-torch.log2(lik.clamp(min=BOUND))).numpy()


def eg_literal_fp32(x, mean, scale, q, x_mean=None, use_clamp=False, g_bits=None):
    """The reference's literal expression in float32 on the CPU -> {bits, gx, gm, gs, gq, lik} (float32 arrays): how much
    error the fp32 formula carries by itself."""
    X, M, S, Q = _leaves(x, mean, scale, q, torch.float32)
    gb = np.broadcast_to(np.asarray(1.0 if g_bits is None else g_bits, dtype=np.float32), X.shape)
    xc = _clamped(X, Q, x_mean, use_clamp)
    n = torch.distributions.Normal(M, torch.clamp(S, min=1e-9), validate_args=False)
    lik = torch.abs(n.cdf(xc + 0.5 * Q) - n.cdf(xc - 0.5 * Q))
    bits = -torch.log2(_LowBound.apply(lik, float(np.float32(1e-6))))
    (bits * torch.from_numpy(np.array(gb))).sum().backward()
    return dict(bits=bits.detach().numpy(), lik=lik.detach().numpy(), gx=X.grad.numpy(), gm=M.grad.numpy(), gs=S.grad.numpy(),
                gq=Q.grad.numpy())


# ---- inputs -------------------------------------------------------------------------------------------------------------------
X_MEAN = 0.25
BODY, SWITCH, TAIL, TINY, CLAMP, CENTRE = range(6)     # (CENTRE: x = mean, what undecided elements are redrawn as)
TINY_SCALES = np.array([-1.0, 0.0, 1e-12, np.float32(1e-9), np.nextafter(np.float32(1e-9), np.float32(0)),
                        np.nextafter(np.float32(1e-9), np.float32(1))], dtype=np.float32)
_f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)


def _grid(v, step):
    return np.round(np.asarray(v, dtype=np.float64) / step) * step


def _logu(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def assert_exact(x, mean, q, x_mean=None, use_clamp=False):
    """x +- q/2 - mean (after the clamp) carries no rounding in float32, and the operands are on their grids."""
    x, mean, q = np.broadcast_arrays(*(np.asarray(a, dtype=np.float32) for a in (x, mean, q)))
    x64, m64, q64 = x.astype(np.float64), mean.astype(np.float64), q.astype(np.float64)
    assert (q > 0).all() and (_grid(q64, QGRID) == q64).all() and (_grid(m64, GRID) == m64).all() and (_grid(x64, GRID) == x64).all()
    if use_clamp:
        xm = np.broadcast_to(np.asarray(x_mean, dtype=np.float32), x.shape)
        lo, hi = xm - np.float32(15000) * q, xm + np.float32(15000) * q
        lo64, hi64 = xm.astype(np.float64) - 15000 * q64, xm.astype(np.float64) + 15000 * q64
        x, x64 = np.minimum(np.maximum(x, lo), hi), np.minimum(np.maximum(x64, lo64), hi64)
        assert (x == x64).all()               # (a bound far from x may round: it decides nothing)
    h = np.float32(0.5)
    assert ((x + h * q) - mean == (x64 + 0.5 * q64) - m64).all() and ((x - h * q) - mean == (x64 - 0.5 * q64) - m64).all()


def draw_q(rng, n):
    """(q, the scale that goes with it): q = w scale on its grid, w log-uniform in [1e-2, 8], scale in [2e-2, 3], q <= 8."""
    s0 = _logu(rng, 2e-2, 3.0, n)
    return np.clip(_grid(_logu(rng, 1e-2, 8.0, n) * s0, QGRID), QGRID, 8.0), s0


def scale_for(rng, q):
    """A scale for a given q (one q shared by many elements): q / w clipped to [2e-2, 3], w log-uniform in [1e-2, 8]."""
    return np.clip(q / _logu(rng, 1e-2, 8.0, np.shape(q)), 2e-2, 3.0)


def build(regime, q, s0, rng, s_fixed=False, mean=None, x_mean=X_MEAN):
    """Elements of the regimes `regime` (ints, any shape) for the step sizes q (same shape, on the 2^-11 grid) -> (x, mean,
    scale) float32.  s0: the scale to aim for; unless s_fixed it is lowered where |x - mean| would pass 8, replaced by the
    tiny scales in the tiny regime, and set so that the chosen edge is exact in the switch regime.  mean: given (on the 2^-12
    grid) or drawn in [-4, 4] (next to the clamped value in the clamp regime, which needs a free mean and q <= 1/8)."""
    regime, q, s0 = np.broadcast_arrays(np.asarray(regime), np.asarray(q, dtype=np.float64), np.asarray(s0, dtype=np.float64))
    n = regime.shape
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    idx = np.arange(regime.size).reshape(n)
    # body / tail: a target z = (x - mean) / scale
    z = np.where(regime == TAIL, sign * rng.uniform(3, 6.5, n), rng.uniform(-3, 3, n))
    s = s0 if s_fixed else np.minimum(s0, 8.0 / np.maximum(np.abs(z), 1e-3))
    d = _grid(z * s, GRID)
    on = (regime == BODY) & (idx % 16 == 5)                 # one body element in 16: zu or zl exactly 0
    d = np.where(on, sign * q / 2, d)
    d = np.where(regime == CENTRE, 0.0, d)
    # switch: one edge of the cell at |z_edge| / sqrt 2 = 1 +- 1e-3, on either side of where an erf changes its polynomial
    t = sign * (1 + np.where(rng.random(n) < 0.5, -1e-3, 1e-3))
    p = _grid(t * SQRT2 * s0, GRID)
    p = np.where(p == 0, sign * GRID, p)
    sw = regime == SWITCH
    if not s_fixed:
        s = np.where(sw, p / (t * SQRT2), s)
    d = np.where(sw, np.where(rng.random(n) < 0.5, p - q / 2, p + q / 2), d)
    # tiny scale: x - mean inside and outside +- q/2
    ty = regime == TINY
    if not s_fixed:
        s = np.where(ty, TINY_SCALES[idx % len(TINY_SCALES)].astype(np.float64), s)
    inside = (idx // len(TINY_SCALES)) % 2 == 0
    d_in = sign * np.minimum(_grid(rng.uniform(0, 1, n) * q / 2, GRID), q / 2 - GRID)
    d = np.where(ty, np.where(inside, d_in, sign * (q / 2 + GRID + _grid(rng.uniform(0, 4, n), GRID))), d)
    m = _grid(rng.uniform(-4, 4, n), GRID) if mean is None else np.broadcast_to(np.asarray(mean, dtype=np.float64), n)
    x = m + d
    # clamp: x inside the range, exactly on an edge, beyond it; the mean within 2 scales of the clamped value
    cl = regime == CLAMP
    if cl.any():
        assert mean is None and (q[cl] <= 0.125).all()
        where = idx % 3
        edge = x_mean + sign * 15000 * q
        xc = np.where(where == 0, x_mean + _grid(rng.uniform(-0.9, 0.9, n) * 15000 * q, GRID), edge)
        xb = np.where(where == 2, edge + sign * (GRID + _grid(_logu(rng, 1e-3, 50.0, n), GRID)), xc)
        x = np.where(cl, xb, x)
        m = np.where(cl, xc - _grid(rng.uniform(-2, 2, n) * s, GRID), m)
    return _f32(x), _f32(m), _f32(s)


@functools.lru_cache(maxsize=None)
def draw(regime, n, seed=0, use_clamp=False, q_layout="elem", cols=50):
    """n elements of one regime (a name of REGIMES) -> (x, mean, scale, q, x_mean, use_clamp), exact on the grid (asserted).
    q_layout: "elem" one q per element, "row" one per `cols` elements, "scalar" one for all; q is returned per element."""
    rid = REGIMES.index(regime)
    rng = np.random.default_rng(1000 * rid + 10 * seed + ("elem", "row", "scalar").index(q_layout))
    qrng = np.random.default_rng(10 * seed + 7)                  # (a shared q does not depend on the regime)
    if q_layout == "elem":
        q, s0 = draw_q(rng, n)
    else:
        q = draw_q(qrng, -(-n // cols) if q_layout == "row" else 1)[0]
        q = np.repeat(q, cols)[:n] if q_layout == "row" else np.full(n, q[0])
        s0 = scale_for(rng, q)
    if rid == CLAMP:
        q, use_clamp = np.full(n, QGRID), True
    x, mean, s = build(np.full(n, rid), q, s0, rng)
    q = _f32(q)
    assert_exact(x, mean, q, X_MEAN, use_clamp)
    for a in (x, mean, s, q):
        a.setflags(write=False)
    return x, mean, s, q, X_MEAN, bool(use_clamp)


def g_bits(n, seed=0):
    """Upstream gradients of both signs, every eighth exactly 0."""
    g = np.random.default_rng(77 + seed).normal(size=n).astype(np.float32)
    g[np.arange(n) % 8 == 3] = 0.0
    return g


@functools.lru_cache(maxsize=None)
def case(regime, n, seed=0, use_clamp=False, q_layout="elem", cols=50):
    """(inputs, g_bits, Ref) of `draw`, computed once and shared; read-only."""
    inp = draw(regime, n, seed, use_clamp, q_layout, cols)
    g = g_bits(n, seed)
    return inp, g, eg_fp64(*inp, g_bits=g)


def mixed_regimes(rng, shape, clamp_rows=None):
    """A regime per element of a [rows, cols] block: body, switch, tail, tiny scale in equal shares, and the clamp regime for
    half of the elements of the rows `clamp_rows` (a bool per row: those rows' q must be 2^-11 .. 1/8)."""
    r = rng.integers(0, 4, shape)
    if clamp_rows is not None:
        r = np.where(np.asarray(clamp_rows)[:, None] & (rng.random(shape) < 0.5), CLAMP, r)
    return r


def settle(regime, q, s0, seed, x_mean, use_clamp, override=None, **kw):
    """build(), with the elements whose likelihood is undecided redrawn at the centre of their cell until none is left: the
    inputs of the kernels whose outputs are sums.  x_mean broadcasts against the elements; override(x, mean, scale) -> x may
    replace values.  Every pass draws the same random numbers (`seed`), so only the redrawn elements change.
    -> (x, mean, scale, regime)."""
    regime = np.array(np.broadcast_to(regime, np.shape(q)))
    for _ in range(4):
        x, mean, s = build(regime, q, s0, np.random.default_rng(seed), x_mean=x_mean, **kw)
        if override is not None:
            x = override(x, mean, s)
        und = eg_fp64(x, mean, s, q, x_mean, use_clamp).undecided
        if not und.any():
            assert_exact(x, mean, _f32(q), x_mean, use_clamp)
            return x, mean, s, regime
        regime[und] = CENTRE
        override = None if override is None else (lambda x_, m_, s_, f=override, keep=~und: np.where(keep, f(x_, m_, s_), x_))
    raise AssertionError("undecided elements left")
