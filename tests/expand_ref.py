"""fp64 restatement of the anchor -> Gaussian expansion (a helper, not a test): gaussian_renderer/__init__.py:112-145.

Written from those lines, not from csrc/expand.hip.  With op_raw [n, K], color_in [n, 3K], cov_in [n, 7K] the three MLP outputs,
masks [n, K], anchor [n, 3] and grid_scaling [n, 6] / grid_offsets [n, K, 3] (rows src_row[n] of larger arrays when given):
  neural_opacity = op_raw * mask                       per slot (n K rows)
  mask           = neural_opacity > 0                  the survivors; every output below keeps their rows, in slot order
  opacity        = neural_opacity[mask],  color = color_in[mask]
  scaling        = gs[3:6] * sigmoid(cov[0:3])
  rot            = cov[3:7] / max(||cov[3:7]||, eps)   eps = float32(1e-12) (F.normalize)
  xyz            = anchor + offset * gs[0:3]
and the gradients of sum <output, weight> over any subset of the six differentiable outputs by autograd.  `_evaluate` states
this once for a dtype: torch float64 is the reference, torch float32 on the CPU is "the literal" (what the formula costs in fp32
by itself); the per-anchor sums (d_anchor, d_gscaling) are taken over the anchor's K slots in slot order in both.

The error unit of one element is u = 2^-24 * (the sum of the magnitudes of the terms of its expression, in fp64):
  xyz            |anchor| + |off gs|
  scaling        |gs3 sig| (1 + (1 - sig) |s|)                  the argument error of a hardware exp grows with |s|
  rot_i          |r_i|
  d_offsets      |gx gs|
  d_cov[0:3]     |g_scaling gs3| sig (1 + (1 - sig) |s|)
  d_cov[3:7]     (|g_i| + |r_i| sum_k |r_k g_k|) / max(||q||, eps)
  d_op_raw       (|g_no| + |g_opacity|) |mask|,     d_mask: the same with |op_raw|
  d_anchor       sum_k |gx|
  d_gscaling     [0:3] sum_k |gx off|,  [3:6] sum_k |g_scaling sig| (1 + (1 - sig) |s|)
Where sig, or the product f sig of sig with the factor f that multiplies it, is below 2^-126 (subnormal in fp32: a result
there may be flushed to zero, and 1 / (1 + inf) is zero), the term has the floor 2^-126 max(|f|, 1) on top (nothing for f = 0):
an error of 2^-126 in sig times f, or the whole product lost.  f = gs3 for scaling, g_scaling gs3 for d_cov[0:3], g_scaling in the
sum of d_gscaling[3:6].  An element whose unit is 0 (then its fp64 value is 0 too, `assert_units_positive`) must be exactly 0.

Exact statements (`check_exact`): neural_opacity == float32(op_raw * mask) (the fp64 product of two fp32 numbers is exact: one
rounding), mask == (that > 0), color / opacity / d_color_in are bit copies, the gradient rows of non-survivors are exactly 0
except d_op_raw / d_mask (which carry the g_neural_opacity term alone), and the rows of d_gscaling / d_offsets that src_row does
not name are exactly 0.

Inputs (`draw`) are seeded fp32 values, one regime per slot, mixed within a call:
  body        ordinary values
  gate        op_raw * mask = +0, -0, negative, +-2^-126 (as +-2^-63 * 2^-63: no gradient of it is subnormal), 1, fractional
              masks in (0, 1)
  sigmoid     s = +-{0, 1e-3, 1, 10, 17, 30, 80, 87, 88, 89, 100, 1e4}
  quaternion  all zero; one-hot +-1 (the output is exact); ||q|| = 1e-25, 1e-18, 1e-13 (below eps), 1e-11, 1, 1e15 (above)
  geometry    offset * gs within 1e-6 .. 1e-2 of -anchor; |anchor| runs up to 1e4 for every regime
and the gate modes all / none (P = 0) / first / last (a single survivor in the first or the last slot).
Conditions asserted on every draw (`assert_conditions`), so that no element ever has to be left out of a comparison:
no product op_raw * mask with 0 < |.| < 2^-126 (fp32 and fp64 could gate it differently), no ||q|| in (0.5e-12, 2e-12),
|q_i| <= 1e18 (beyond it the squares overflow in fp32, in the reference too: a known limit, not under test).
"""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

EPS = float(np.float32(1e-12))
U = 2.0 ** -24
TINY = 2.0 ** -126
# What the fp32 literal needs on these inputs, in units: measured by test_expand_ref.py, rounded up to one decimal.  The kernels
# replace libm's exp and the IEEE divisions by 1-ulp hardware forms (v_exp_f32, v_rcp_f32), about one more rounding of the size
# the literal already makes: twice the literal's bound.  Neither number is taken from the kernels' results.
UNITS_LITERAL = 7.3
UNITS_KERNEL = 2 * UNITS_LITERAL

VALUES = ("xyz", "color", "opacity", "scaling", "rot", "neural_opacity")
WIDTH = dict(xyz=3, color=3, opacity=1, scaling=3, rot=4, neural_opacity=1)
GRADS = ("d_anchor", "d_gscaling", "d_offsets", "d_mask", "d_op_raw", "d_color_in", "d_cov_in")
REGIMES = ("body", "gate", "sigmoid", "quaternion", "geometry")
BODY, GATE, SIGMOID, QUAT, GEOM = range(5)
SIGMOID_S = np.array([0, 1e-3, 1, 10, 17, 30, 80, 87, 88, 89, 100, 1e4], dtype=np.float32)
QUAT_NORMS = np.array([1e-25, 1e-18, 1e-13, 1e-11, 1, 1e15])
_h = np.float32(2.0 ** -63)
# (op_raw, mask) pairs of the gate regime
GATE_PAIRS = np.array([(0.0, 1.0), (-0.0, 1.0), (0.5, 0.0), (0.5, -0.0), (-0.5, 0.0), (-0.3, 1.0), (-0.7, 0.5), (0.3, -1.0),
                       (_h, _h), (-_h, _h), (_h, -_h), (-_h, -_h), (1.0, 1.0), (0.8, 0.25), (0.6, 0.75), (-0.6, 0.75),
                       (0.999, 2.0 ** -20)], dtype=np.float32)


# ---- the statement --------------------------------------------------------------------------------------------------------------
def _evaluate(c, dtype):
    """Lines 112-145 on the case `c` in `dtype` -> a namespace of the leaves, the seven outputs and `rep` (the per-slot copy
    of [grid_scaling, anchor], whose gradient is summed over an anchor's slots by `_gradients`)."""
    t = lambda a: torch.from_numpy(np.array(a)).to(dtype).requires_grad_(True)
    e = types.SimpleNamespace(anchor=t(c.anchor), gscaling=t(c.gscaling), offsets=t(c.offsets), masks=t(c.masks), op_raw=t(c.op_raw),
                              color_in=t(c.color_in), cov_in=t(c.cov_in), dtype=dtype)
    n, K = c.n, c.K
    idx = None if c.src_row is None else torch.from_numpy(c.src_row)
    grid_scaling = e.gscaling if idx is None else e.gscaling[idx]
    grid_offsets = e.offsets if idx is None else e.offsets[idx]
    neural_opacity = e.op_raw.reshape(-1, 1) * e.masks.reshape(-1, 1)                                  # :112-114
    mask = (neural_opacity > 0.0).view(-1)                                                             # :115-116
    opacity = neural_opacity[mask]                                                                     # :119
    color = e.color_in.reshape(n * K, 3)                                                               # :122-123
    scale_rot = e.cov_in.reshape(n * K, 7)                                                             # :126-127
    offsets = grid_offsets.reshape(-1, 3)                                                              # :129
    concatenated = torch.cat([grid_scaling, e.anchor], dim=-1)                                         # :132
    e.rep = concatenated.unsqueeze(1).expand(n, K, 9).reshape(n * K, 9)                                # :133 'n c -> (n k) c'
    masked = torch.cat([e.rep, color, scale_rot, offsets], dim=-1)[mask]                               # :134-136
    scaling_repeat, repeat_anchor, color, scale_rot, offsets = masked.split([6, 3, 3, 7, 3], dim=-1)   # :137
    scaling = scaling_repeat[:, 3:] * torch.sigmoid(scale_rot[:, :3])                                  # :140
    rot = F.normalize(scale_rot[:, 3:7], eps=EPS)                                                      # :142
    xyz = repeat_anchor + offsets * scaling_repeat[:, :3]                                              # :144-145
    e.out = dict(xyz=xyz, color=color, opacity=opacity, scaling=scaling, rot=rot, neural_opacity=neural_opacity)
    e.mask = mask.numpy().copy()
    return e


def _gradients(c, e, weights):
    """Gradients of sum <output, weight> over the outputs named in `weights` -> {name: array of e.dtype}; d_anchor and
    d_gscaling are the sums of the per-slot gradients over an anchor's K slots, in slot order."""
    n, K = c.n, c.K
    loss = sum((e.out[k] * torch.from_numpy(np.array(w)).to(e.dtype)).sum() for k, w in weights.items())
    leaves = [e.rep, e.offsets, e.masks, e.op_raw, e.color_in, e.cov_in]
    got = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
    got = [torch.zeros_like(l) if g is None else g for g, l in zip(got, leaves)]
    g_rep = got[0].reshape(n, K, 9)
    acc = torch.zeros(n, 9, dtype=e.dtype)
    for k in range(K):
        acc = acc + g_rep[:, k]
    d_gs = torch.zeros_like(e.gscaling)
    d_gs[torch.arange(n) if c.src_row is None else torch.from_numpy(c.src_row)] = acc[:, :6]
    out = dict(d_anchor=acc[:, 6:], d_gscaling=d_gs, d_offsets=got[1], d_mask=got[2], d_op_raw=got[3], d_color_in=got[4],
               d_cov_in=got[5])
    return {k: v.detach().numpy() for k, v in out.items()}


class Ref:
    """The fp64 values of one case (numpy arrays), their units, and `grads(weights)`."""

    def __init__(self, c):
        self.c = c
        self.e = _evaluate(c, torch.float64)
        self.values = {k: v.detach().numpy() for k, v in self.e.out.items()}
        self.mask = self.e.mask
        self.sel = np.nonzero(self.mask)[0]
        self.P = int(self.mask.sum())
        n, K = c.n, c.K
        rows = np.arange(n) if c.src_row is None else c.src_row
        f = lambda a: np.asarray(a, dtype=np.float64)
        self.rows = rows
        self.gs = np.repeat(f(c.gscaling)[rows], K, axis=0)                           # per slot [nK, 6]
        self.off = f(c.offsets)[rows].reshape(n * K, 3)
        self.anchor = np.repeat(f(c.anchor), K, axis=0)
        cov = f(c.cov_in).reshape(n * K, 7)
        self.s, q = cov[:, :3], cov[:, 3:]
        with np.errstate(over="ignore"):
            self.sig, one_m = 1.0 / (1.0 + np.exp(-self.s)), 1.0 / (1.0 + np.exp(self.s))      # (1 - sig without cancellation)
        self.amp = 1.0 + one_m * np.abs(self.s)
        self.floor = lambda f: TINY * np.maximum(np.abs(f), 1.0) * ((f != 0) & (self.sig * np.minimum(np.abs(f), 1.0) < TINY))
        self.den = np.maximum(np.sqrt((q * q).sum(1, keepdims=True)), EPS)
        self.r = q / self.den
        sel = self.sel
        self.value_units = dict(
            xyz=U * (np.abs(self.anchor) + np.abs(self.off * self.gs[:, :3]))[sel],
            scaling=(U * np.abs(self.gs[:, 3:] * self.sig) * self.amp + self.floor(self.gs[:, 3:]))[sel],
            rot=U * np.abs(self.r)[sel])
        assert np.array_equal(self.values["neural_opacity"].ravel() > 0, self.mask)

    def grads(self, weights):
        """-> ({name: fp64 gradient}, {name: unit of every element}) of sum <output, weight> over the outputs in `weights`."""
        c, n, K, sel = self.c, self.c.n, self.c.K, self.sel
        g = _gradients(c, self.e, weights)

        def slot(name):                    # the weight of a per-Gaussian output on its slot, 0 on the others
            a = np.zeros((n * K, WIDTH[name]))
            if name in weights:
                a[sel] = np.abs(np.asarray(weights[name], dtype=np.float64))
            return a
        gx, gsc, gr, gop = slot("xyz"), slot("scaling"), slot("rot"), slot("opacity")
        gno = np.abs(np.asarray(weights["neural_opacity"], dtype=np.float64)) if "neural_opacity" in weights else np.zeros((n * K, 1))
        sum_k = lambda a: a.reshape(n, K, -1).sum(1)

        def src(a):                        # per-anchor / per-slot rows -> the rows of the source arrays
            o = np.zeros((c.gscaling.shape[0],) + a.shape[1:])
            o[self.rows] = a
            return o
        u_sig = U * np.abs(gsc * self.gs[:, 3:]) * self.sig * self.amp + self.floor(gsc * self.gs[:, 3:])
        u_q = U * (gr + np.abs(self.r) * (np.abs(self.r) * gr).sum(1, keepdims=True)) / self.den
        u_gs = np.concatenate([U * sum_k(gx * np.abs(self.off)),
                               U * sum_k(gsc * self.sig * self.amp) + sum_k(self.floor(gsc))], axis=1)
        m, o = np.abs(np.asarray(c.masks, np.float64)).reshape(-1, 1), np.abs(np.asarray(c.op_raw, np.float64)).reshape(-1, 1)
        units = dict(d_anchor=U * sum_k(gx), d_gscaling=src(u_gs),
                     d_offsets=src((U * gx * np.abs(self.gs[:, :3])).reshape(n, K, 3)),
                     d_mask=(U * (gno + gop) * o).reshape(n, K), d_op_raw=(U * (gno + gop) * m).reshape(n, K),
                     d_color_in=np.zeros((n, 3 * K)), d_cov_in=np.concatenate([u_sig, u_q], axis=1).reshape(n, 7 * K))
        return g, units


def literal_fp32(c, weights_list):
    """The same statement in torch float32 on the CPU -> (values, [gradients of every weights dict]) as float32 arrays."""
    e = _evaluate(c, torch.float32)
    return {k: v.detach().numpy() for k, v in e.out.items()}, [_gradients(c, e, w) for w in weights_list]


def units_error(got, want, unit, what=""):
    """|got - want| in units, element by element; where the unit is 0 the element must be equal (AssertionError)."""
    got, want = np.asarray(got, dtype=np.float64).reshape(np.shape(want)), np.asarray(want, dtype=np.float64)
    assert np.isfinite(got).all(), (what, "not finite", int((~np.isfinite(got)).sum()))
    err = np.abs(got - want)
    zero = unit == 0
    assert (err[zero] == 0).all(), (what, "an element with unit 0 differs", int((err[zero] != 0).sum()))
    return np.where(zero, 0.0, err / np.where(zero, 1.0, unit))


def assert_units_positive(value, unit, what=""):
    assert (unit >= 0).all() and np.isfinite(unit).all(), what
    assert (unit[np.asarray(value) != 0] > 0).all(), (what, "a non-zero value with a zero unit")


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32).ravel(), np.ascontiguousarray(b, np.float32).view(np.uint32).ravel())


def check_exact(ref, values=None, mask=None, grads=None, weights=None, src_grads=True):
    """The statements that are equalities.  values / grads: fp32 arrays of a kernel (or of the literal); weights: the
    upstream gradients the `grads` were taken with.  src_grads=False: d_gscaling / d_offsets are absent."""
    c, sel = ref.c, ref.sel
    n, K = c.n, c.K
    if values is not None:
        no = (np.asarray(c.op_raw, np.float64) * np.asarray(c.masks, np.float64)).astype(np.float32).reshape(-1, 1)
        assert _same_bits(values["neural_opacity"], no), "neural_opacity != float32(op_raw * mask)"
        if mask is not None:
            assert np.array_equal(np.asarray(mask).ravel().astype(bool), no.ravel() > 0), "mask"
        assert np.asarray(values["xyz"]).shape == (ref.P, 3)
        assert _same_bits(values["opacity"], no[sel]), "opacity"
        assert _same_bits(values["color"], np.asarray(c.color_in).reshape(n * K, 3)[sel]), "color"
    if grads is not None:
        dead = ~ref.mask
        want_col = np.zeros((n * K, 3), np.float32)
        if "color" in weights:
            want_col[sel] = weights["color"]
        if "d_color_in" in grads:
            assert _same_bits(np.asarray(grads["d_color_in"]) + np.float32(0), want_col + np.float32(0)), "d_color_in"     # (-0 + 0 = +0)
            assert (np.asarray(grads["d_cov_in"]).reshape(n * K, 7)[dead] == 0).all(), "d_cov_in of a non-survivor"
        names = ["d_gscaling", "d_offsets"] if src_grads else []
        if src_grads:
            assert (np.asarray(grads["d_offsets"])[ref.rows].reshape(n * K, 3)[dead] == 0).all(), "d_offsets of a non-survivor"
        unread = np.ones(c.gscaling.shape[0], bool)
        unread[ref.rows] = False
        for k in names:
            assert (np.asarray(grads[k])[unread] == 0).all(), (k, "a row that src_row does not name")
        if "neural_opacity" not in weights:
            for k in ("d_op_raw", "d_mask"):
                if k in grads:
                    assert (np.asarray(grads[k]).ravel()[dead] == 0).all(), (k, "non-survivor")


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
class Case(types.SimpleNamespace):
    """anchor [n,3], gscaling [n_src,6], offsets [n_src,K,3], masks / op_raw [n,K], color_in [n,3K], cov_in [n,7K] (float32),
    src_row (int64 [n] or None), regime [n,K]."""

    def inputs(self):
        return self.anchor, self.gscaling, self.offsets, self.masks, self.op_raw, self.color_in, self.cov_in


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def fill_regimes(rng, regime, op_raw, masks, cov, cycle=None):
    """Writes the gate, sigmoid and quaternion regimes' values into op_raw, masks [n,K] and cov [n,K,7] (float32, in place);
    cycle: which of a regime's values a slot takes (default: its index, so that a few slots already cover every value)."""
    n, K = regime.shape
    idx = np.arange(n * K).reshape(n, K) if cycle is None else cycle
    sign = np.where(rng.random((n, K, 7)) < 0.5, -1.0, 1.0)
    g = regime == GATE
    pair = GATE_PAIRS[idx % len(GATE_PAIRS)]
    op_raw[g], masks[g] = pair[..., 0][g], pair[..., 1][g]
    s = regime == SIGMOID
    pick = (3 * idx[..., None] + np.arange(3) * 5) % len(SIGMOID_S)
    cov[..., :3][s] = (SIGMOID_S[pick] * sign[..., :3])[s]
    kind = idx % (2 + len(QUAT_NORMS))
    direction = rng.uniform(0.3, 1.0, (n, K, 4)) * sign[..., 3:]
    direction /= np.sqrt((direction ** 2).sum(-1, keepdims=True))
    onehot = (np.arange(4) == (idx // 8 % 4)[..., None]) * sign[..., 3:4]
    qv = np.where((kind == 0)[..., None], 0.0, np.where((kind == 1)[..., None], onehot,
                                                        direction * QUAT_NORMS[np.maximum(kind - 2, 0)][..., None]))
    cov[..., 3:][regime == QUAT] = qv[regime == QUAT]


def assert_conditions(c):
    prod = np.abs(np.asarray(c.op_raw, np.float64) * np.asarray(c.masks, np.float64))
    assert not ((prod > 0) & (prod < TINY)).any(), "a product op_raw * mask below 2^-126"
    q = np.asarray(c.cov_in, np.float64).reshape(-1, 7)[:, 3:]
    nrm = np.sqrt((q * q).sum(1))
    assert not ((nrm > 0.5e-12) & (nrm < 2e-12)).any(), "a quaternion norm next to eps"
    assert (np.abs(q) <= 1e18).all()
    for a in c.inputs():
        assert a.dtype == np.float32 and np.isfinite(a).all()
    if c.src_row is not None:
        assert len(np.unique(c.src_row)) == c.n and c.src_row.max() < c.gscaling.shape[0]


@functools.lru_cache(maxsize=None)
def draw(n, K, seed=0, src="none", gate="mixed", only=None, n_src=None):
    """A seeded case: a regime per slot (`only`: that regime in every slot).  src: "none" (no src_row), "subset" (a permuted
    subset of n_src rows, 3n + 1 unless given), "perm" (a permutation of n_src = n rows).  gate: "mixed", "all", "none", "first", "last"."""
    rng = np.random.default_rng([n, K, seed, ("none", "subset", "perm").index(src), ("mixed", "all", "none", "first", "last").index(gate),
                                 0 if only is None else 1 + REGIMES.index(only)])
    n_src = (n_src or 3 * n + 1) if src == "subset" else n
    src_row = None if src == "none" else rng.permutation(n_src)[:n].astype(np.int64)
    rows = np.arange(n) if src_row is None else src_row
    regime = rng.integers(0, len(REGIMES), (n, K)) if only is None else np.full((n, K), REGIMES.index(only))
    sgn = lambda shape: np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    anchor = _f32(sgn((n, 3)) * 10.0 ** rng.uniform(-1, 4, (n, 3)))
    gscaling = _f32(10.0 ** rng.uniform(-2, 0, (n_src, 6)))
    offsets = _f32(rng.normal(size=(n_src, K, 3)) * 0.5)
    masks = _f32(rng.random((n, K)) < 0.7)
    op_raw = _f32(np.tanh(rng.normal(size=(n, K))))
    color_in = _f32(rng.random((n, 3 * K)))
    cov = _f32(rng.normal(size=(n, K, 7)))
    fill_regimes(rng, regime, op_raw, masks, cov)
    # geometry: offset * gs next to -anchor
    delta = sgn((n, K, 3)) * 10.0 ** rng.uniform(-6, -2, (n, K, 3))
    near = _f32(-(anchor[:, None, :].astype(np.float64) / gscaling[rows][:, None, :3]) * (1 + delta))
    view = offsets[rows]
    view[regime == GEOM] = near[regime == GEOM]
    offsets[rows] = view
    prod = op_raw.astype(np.float64) * masks
    if gate == "all":
        op_raw[prod <= 0], masks[prod <= 0] = 0.5, 1.0
    elif gate in ("none", "first", "last"):
        op_raw[prod > 0] *= -1
        at = (0, 0) if gate == "first" else (n - 1, K - 1)
        if gate != "none":
            op_raw[at], masks[at] = 0.7, 1.0
    c = Case(n=n, K=K, n_src=n_src, anchor=anchor, gscaling=gscaling, offsets=offsets, masks=masks, op_raw=op_raw, color_in=color_in,
             cov_in=np.ascontiguousarray(cov.reshape(n, 7 * K)), src_row=src_row, regime=regime)
    assert_conditions(c)
    for a in c.inputs():
        a.setflags(write=False)
    return c


def draw_weights(P, slots, seed, names=VALUES):
    """Upstream gradients of the outputs `names` (float32, both signs, every eighth exactly 0)."""
    rng = np.random.default_rng(9000 + seed)
    w = {}
    for k in VALUES:
        a = rng.normal(size=(slots if k == "neural_opacity" else P, WIDTH[k])).astype(np.float32)
        a.ravel()[np.arange(a.size) % 8 == 3] = 0.0
        if k in names:
            w[k] = a
    return w


LOSSES = tuple((k,) for k in VALUES) + (VALUES, VALUES[:5])        # every output alone, all six, all but neural_opacity


# ---- comparing one run ----------------------------------------------------------------------------------------------------------
def slot_regime(ref, name):
    """The regime of every element of the output or gradient `name` (-1: a per-anchor sum, which mixes its slots' regimes)."""
    c = ref.c
    reg = c.regime.reshape(-1)
    if name in WIDTH:
        return np.repeat((reg if name == "neural_opacity" else reg[ref.sel])[:, None], WIDTH[name], axis=1)
    if name in ("d_anchor", "d_gscaling"):
        return np.full((c.n if name == "d_anchor" else c.gscaling.shape[0], 3 if name == "d_anchor" else 6), -1)
    w = dict(d_offsets=3, d_mask=1, d_op_raw=1, d_color_in=3, d_cov_in=7)[name]
    r = np.repeat(c.regime[:, :, None], w, axis=2).reshape(c.n, -1)
    if name == "d_offsets":
        o = np.full((c.gscaling.shape[0], c.K, 3), -1)
        o[ref.rows] = r.reshape(c.n, c.K, 3)
        return o
    return r


class Maxima:
    """Collects the largest error in units per (regime, output)."""

    def __init__(self):
        self.m = {}

    def add(self, ref, name, err):
        if name == "d_cov_in":             # the sigmoid's and the quaternion's columns apart
            e7, r7 = err.reshape(-1, 7), slot_regime(ref, name).reshape(-1, 7)
            for key, cols in (("d_cov[0:3]", slice(0, 3)), ("d_cov[3:7]", slice(3, 7))):
                self._add(key, e7[:, cols], r7[:, cols])
            return
        self._add(name, err, slot_regime(ref, name).reshape(err.shape))

    def _add(self, name, err, reg):
        for i in np.unique(reg):
            key = ("anchor sums" if i < 0 else REGIMES[i], name)
            v = float(err[reg == i].max()) if (reg == i).any() else 0.0
            self.m[key] = max(self.m.get(key, 0.0), v)

    def worst(self):
        return max(self.m.values()) if self.m else 0.0

    def report(self, tag, what):
        names = [k for k in VALUES + GRADS + ("d_cov[0:3]", "d_cov[3:7]") if any(key[1] == k for key in self.m)]
        print(f"[{tag}] {what}: worst {self.worst():.3f}")
        for r in REGIMES + ("anchor sums",):
            row = {k: round(self.m[(r, k)], 3) for k in names if (r, k) in self.m}
            if row:
                print(f"[{tag}]   {r}: {row}")
