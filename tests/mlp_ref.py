"""fp64 restatement of one fused MLP, Linear -> ReLU -> Linear [-> tanh | sigmoid], and of its backward (a helper, not a test).

Written from the nn.Sequential the kernels replace (scene/gaussian_model.py:153-188), in numpy float64, with no torch kernel and no
autograd node: `Ref(x, W1, b1, W2, b2, act, dy)` is plain arithmetic on arrays, so that any kernel that carries such a chain can
be held against it.
  z1 = x W1^T + b1      h = max(z1, 0)      z2 = h W2^T + b2      y = act(z2)
  dz2 = dy act'(y)      dh = dz2 W2         dz1 = dh [z1 > 0]     dx = dz1 W1
  dW2 = dz2^T h         db2 = sum_r dz2     dW1 = dz1^T x         db1 = sum_r dz1
The kernels form act' from their own y: 1 - y y (tanh), y (1 - y) (sigmoid), 1.

The error unit U of an element is one fp32 rounding (u = 2^-24) of the element's own absolute sum, carried through the later
stages by their absolute matrices (all in fp64, nothing taken from a kernel):
  z1, h      u (|W1| |x| + |b1|)                                 (h: 0 where z1 <= 0 - there h is exactly 0)
  z2         |W2| U(h) + u (|W2| h + |b2|)
  y          none: U(z2);   tanh: U(z2) + u |y|;   sigmoid: U(z2) / 4 + u (y (1 - y) (|z2| + 1) + y)
             (|z2|: the rounding of z log2(e) inside the hardware exponential, amplified by the argument)
  dz2        |dy| (|d act'/dy| U(y) + u |act'|) + u |dz2|        (no activation: dz2 is dy itself, U = 0)
             + |act'| U(dy) where the cotangent carries an error unit of its own (`dy_unit`; default: dy is exact)
  dh         U(dz2) |W2| + u |dz2| |W2|
  dz1        U(dh) under the gate
  dx         U(dz1) |W1| + u |dz1| |W1|
  dW2        U(dz2)^T |h| + |dz2|^T U(h) + u |dz2|^T |h|         db2   sum_r U(dz2) + u sum_r |dz2|
  dW1        U(dz1)^T |x| + u |dz1|^T |x|                        db1   sum_r U(dz1) + u sum_r |dz1|
and every U carries an absolute floor of 4 * 2^-126 (flushed denormals), propagated like the rest.
An element's error in units is |got - ref| / U.  One number of units judges every element of every kernel:
UNITS_KERNEL = 2 UNITS_LITERAL, where UNITS_LITERAL is what three fp32 evaluations of the same expressions need on the CPU
(tests/test_mlp_ref.py measures them, rounded up to one decimal):
  (a) `literal_torch`       torch on the CPU with autograd
  (b) `literal_numpy(seq)`  numpy float32, strictly sequential accumulation in every contraction and over the rows
  (c) `literal_numpy(frag)` numpy float32 in the order csrc/mlp_frag.h documents (index k = 16 q + 4 g + j: four interleaved
                            chains g, combined at the end), the row sums as 256-row partials, then summed
The factor 2: the hardware forms (__expf, the reciprocal, the fused accumulate of the MFMA) add at most about one more rounding
of the size the literal already makes.  UNITS_KERNEL stays below the shortest contraction it judges (15 terms: GATE_UNITS), so
that it is sharper than the worst case.

Measured on the CPU, maxima in units over `cpu_cases()` (seven instances x eleven row counts, the live rows of the sparse-cotangent
case, and - literal (a) alone - all 65 553 rows of it, which is where h, a maximum over 6.5 M elements, is largest):
              h      y    dz2    dz1     dx    dW1    db1    dW2    db2  x_row d_anchor
  (a)     6.583  1.627  1.273  4.980  2.091  1.966  1.370  1.838  2.099  2.837  4.396
  (b)     4.928  1.587  1.099  5.364  2.091  1.966  1.479  1.811  2.223  3.302  4.717
  (c)     2.967  1.146  1.099  2.456  1.024  1.966  0.838  1.341  2.099      -      -
(x_row, d_anchor: the input row [feat | view direction | distance] the anchor kernels assemble and the pull-back of its four view
columns to the anchor, `AnchorRows`: (a) torch's autograd of cat / norm / division, (b) the expression csrc/mlp3.hip states.
x_row is judged in units of its own, see AnchorRows, and does not enter UNITS_LITERAL.)

Gates.  A hidden unit with 0 < |z1| <= GATE_UNITS U(z1) could take either ReLU branch in fp32: `draw` draws spare rows, drops the
rows that hold one and asserts that none is left - a condition on the inputs, not an allowance in the comparison.  The planted
zeros are not ambiguous: a dead row has x = 0, so z1 = b1 exactly in every order, and b1 holds exact zeros, negatives and positives
(relu'(0) = 0: nothing reaches dx or dW1 through such a unit).

Inputs (`draw`): one regime per row, mixed within a call.
  body        normal x, weights scaled 1 / sqrt(fan_in)
  dead        x = 0
  saturated   (tanh / sigmoid instances) x scaled by 60: |z2| reaches 30 and beyond with both signs - tanh is exactly +-1 there
  overflow    (the same) x scaled by 250: |z2| beyond 100 with both signs, __expf(-z) is inf
and the cotangent dy: dense (every eighth element 0), or nonzero on a given row set only (`rows`), exactly 0 elsewhere.
"""
import functools
import types

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
FLOOR = 4 * TINY
# What the fp32 literals need on these inputs, in units: measured by test_mlp_ref.py, rounded up to one decimal.  Neither number is
# taken from a kernel's result.
UNITS_LITERAL = 6.6
UNITS_KERNEL = 2 * UNITS_LITERAL
GATE_UNITS = 15.0                      # the shortest contraction judged; the generator keeps every gate this far from 0
assert UNITS_KERNEL < GATE_UNITS

ACT_NONE, ACT_TANH, ACT_SIGMOID = 0, 1, 2
INSTANCES = [(54, 50, 10, 1), (54, 50, 30, 2), (54, 50, 70, 0), (71, 100, 175, 0), (15, 100, 175, 0), (71, 100, 3, 0), (15, 100, 3, 0)]
QUANTITIES = ("h", "y", "dz2", "dz1", "dx", "dW1", "db1", "dW2", "db2")
REGIMES = ("body", "dead", "saturated", "overflow")
BODY, DEAD, SAT, OVER = range(4)
ROW_COUNTS = (1, 15, 16, 17, 33, 255, 256, 257, 511, 513, 2100)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def act_fwd(z, act):
    if act == ACT_TANH:
        return np.tanh(z)
    if act == ACT_SIGMOID:
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-z))
    return z


# ---- the statement and its units --------------------------------------------------------------------------------------------
class Ref:
    """values[k], units[k] for k in QUANTITIES (numpy float64), from float32 (or exact double) operands."""

    def __init__(self, x, W1, b1, W2, b2, act, dy, dy_unit=None):
        x, W1, b1, W2, b2, dy = (_f64(a) for a in (x, W1, b1, W2, b2, dy))
        aW1, aW2 = np.abs(W1), np.abs(W2)
        self.act, self.n = act, x.shape[0]
        z1 = x @ W1.T + b1
        gate = z1 > 0
        Uz1 = U * (np.abs(x) @ aW1.T + np.abs(b1)) + FLOOR
        h = np.where(gate, z1, 0.0)
        Uh = np.where(gate, Uz1, 0.0)
        z2 = h @ W2.T + b2
        Uz2 = Uh @ aW2.T + U * (h @ aW2.T + np.abs(b2)) + FLOOR
        y = act_fwd(z2, act)
        if act == ACT_TANH:
            Uy = Uz2 + U * np.abs(y)
            g, dg = 1.0 - y * y, np.abs(2.0 * y)
        elif act == ACT_SIGMOID:
            with np.errstate(over="ignore"):
                one_m = 1.0 / (1.0 + np.exp(z2))                         # 1 - y without cancellation
            Uy = Uz2 / 4 + U * (y * one_m * (np.abs(z2) + 1.0) + y) + FLOOR
            g, dg = y * one_m, np.abs(one_m - y)
        else:
            Uy, g, dg = Uz2, np.ones_like(y), np.zeros_like(y)
        dz2 = dy * g
        Udz2 = np.zeros_like(dz2) if act == ACT_NONE else np.abs(dy) * (dg * Uy + U * np.abs(g)) + U * np.abs(dz2) + FLOOR
        if dy_unit is not None:                                          # (a cotangent that is itself a computed quantity)
            Udz2 = Udz2 + np.abs(g) * _f64(dy_unit)
        dh = dz2 @ W2
        Udh = Udz2 @ aW2 + U * (np.abs(dz2) @ aW2) + FLOOR
        dz1 = np.where(gate, dh, 0.0)
        Udz1 = np.where(gate, Udh, 0.0)
        dx = dz1 @ W1
        Udx = Udz1 @ aW1 + U * (np.abs(dz1) @ aW1) + FLOOR
        ax, adz1, adz2 = np.abs(x), np.abs(dz1), np.abs(dz2)
        self.values = dict(h=h, y=y, dz2=dz2, dz1=dz1, dx=dx, dW1=dz1.T @ x, db1=dz1.sum(0), dW2=dz2.T @ h, db2=dz2.sum(0))
        self.units = dict(h=Uh, y=Uy, dz2=Udz2, dz1=Udz1, dx=Udx,
                          dW1=Udz1.T @ ax + U * (adz1.T @ ax) + FLOOR, db1=Udz1.sum(0) + U * adz1.sum(0) + FLOOR,
                          dW2=Udz2.T @ h + adz2.T @ Uh + U * (adz2.T @ h) + FLOOR, db2=Udz2.sum(0) + U * adz2.sum(0) + FLOOR)
        self.z1, self.z2, self.gate, self.Uz1 = z1, z2, gate, Uz1
        self.live = np.abs(dy).sum(1) != 0                               # rows whose cotangent is not zero


def units_error(got, want, unit, what=""):
    """|got - want| in units, element by element; where the unit is 0 the element must be equal."""
    want = _f64(want)
    got = _f64(got).reshape(want.shape)
    assert np.isfinite(got).all(), (what, "not finite", int((~np.isfinite(got)).sum()))
    err = np.abs(got - want)
    zero = unit == 0
    assert (err[zero] == 0).all(), (what, "an element with unit 0 differs", int((err[zero] != 0).sum()))
    return np.where(zero, 0.0, err / np.where(zero, 1.0, unit))


def check_exact(ref, got, what=""):
    """The statements that are equalities, on whichever of h, dz1, dz2, dx the dict `got` holds."""
    closed, dead_rows = ~ref.gate, ~ref.live
    for k in ("h", "dz1"):
        if k in got:
            assert (np.asarray(got[k])[closed] == 0).all(), (what, k, "not 0 behind a closed gate")
    for k in ("dz1", "dz2", "dx"):
        if k in got and got[k] is not None:
            assert (np.asarray(got[k])[dead_rows] == 0).all(), (what, k, "not 0 on a row whose cotangent is 0")
    if ref.act == ACT_NONE and "dz2" in got and got["dz2"] is not None:
        assert np.array_equal(np.asarray(got["dz2"], np.float64), ref.values["dz2"]), (what, "dz2 != dy")


class Maxima:
    """The largest error in units per quantity."""

    def __init__(self):
        self.m = {}

    def add(self, name, err):
        self.m[name] = max(self.m.get(name, 0.0), float(np.max(err, initial=0.0)))

    def worst(self):
        return max(self.m.values()) if self.m else 0.0

    def report(self, tag):
        print(f"[mlp-units] {tag}: worst {self.worst():.3f}  " + "  ".join(f"{k} {v:.3f}" for k, v in self.m.items()))


def judge(ref, got, maxima, what, limit=None):
    """Every element of the quantities in `got` within `limit` units (default UNITS_KERNEL) of the reference; the equalities equal."""
    limit = UNITS_KERNEL if limit is None else limit
    check_exact(ref, got, what)
    for k, v in got.items():
        if v is None:
            continue
        err = units_error(v, ref.values[k], ref.units[k], (what, k))
        maxima.add(k, err)
        assert err.max(initial=0.0) <= limit, (what, k, float(err.max()), np.unravel_index(int(err.argmax()), err.shape))


# ---- the anchor kernels' input row and its pull-back ---------------------------------------------------------------------------
class AnchorRows:
    """x[r] = [feat_src[src_row[r]] | (a - cam) / |a - cam| | |a - cam|] and, for the gradient dX of such rows, d_anchor =
    (dv - v (v . dv)) / |u| + v dd  with dv = dX[:, 50:53], dd = dX[:, 53].  Units of their own: u |x| per rounding for the row
    (X_ROUNDINGS: the subtraction, the norm = three squares and two additions under a root, the division, counted rigorously:
    5.5 for the direction, 3.5 for the distance, rounded up), and for d_anchor the first-order carry of U(dv), U(dd) plus one
    rounding of the terms' absolute sum."""
    X_ROUNDINGS = np.array([6.0, 6.0, 6.0, 4.0])

    def __init__(self, feat_src, src_row, anchor, cam):
        self.u = _f64(anchor) - _f64(cam).reshape(1, 3)
        self.d = np.sqrt((self.u * self.u).sum(1, keepdims=True))
        assert (self.d > 0).all()
        self.v = self.u / self.d
        self.x = np.concatenate([_f64(feat_src)[src_row], self.v, self.d], axis=1)
        self.x_unit = np.concatenate([np.zeros((len(src_row), 50)), U * np.abs(self.x[:, 50:])], axis=1)

    def pull_back(self, dX, UdX):
        dv, dd, Udv, Udd = dX[:, 50:53], dX[:, 53:54], UdX[:, 50:53], UdX[:, 53:54]
        v, d, av = self.v, self.d, np.abs(self.v)
        da = (dv - v * (v * dv).sum(1, keepdims=True)) / d + v * dd
        own = (np.abs(dv) + av * (av * np.abs(dv)).sum(1, keepdims=True)) / d + av * np.abs(dd)
        carried = (Udv + av * (av * Udv).sum(1, keepdims=True)) / d + av * Udd
        return da, carried + U * own + FLOOR


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def row_regime(n, act):
    r = np.arange(n)
    reg = np.full(n, BODY)
    reg[r % 16 == 3] = DEAD
    reg[r % 64 == 41] = DEAD
    if act != ACT_NONE:
        reg[(r % 16 == 5) | (r % 16 == 14)] = SAT
        reg[r % 32 == 9] = OVER
    return reg


def ambiguous_rows(x, W1, b1):
    x, W1, b1 = _f64(x), _f64(W1), _f64(b1)
    z1 = x @ W1.T + b1
    Uz1 = U * (np.abs(x) @ np.abs(W1).T + np.abs(b1)) + FLOOR
    return ((z1 != 0) & (np.abs(z1) <= GATE_UNITS * Uz1)).any(1) | ((z1 == 0) & (np.abs(x).sum(1, keepdims=True) != 0)).any(1)


def _weights(rng, cfg):
    in_f, hid, out, _ = cfg
    W1 = _f32(rng.normal(size=(hid, in_f)) / np.sqrt(in_f))
    W2 = _f32(rng.normal(size=(out, hid)) / np.sqrt(hid))
    b1 = _f32(rng.uniform(-1, 1, hid) / np.sqrt(in_f))
    b1[::5] = 0.0                                                        # exact zeros next to both signs
    b2 = _f32(rng.uniform(-1, 1, out) / np.sqrt(hid))
    return W1, b1, W2, b2


REGIME_SCALE = np.array([1.0, 0.0, 60.0, 250.0], np.float32)


def _rows(rng, n, in_f, regime, W1, b1):
    """x [n, in_f] by regime with no ambiguous gate against (W1, b1): about 10 % spare rows, a rejected row takes the next one."""
    spare = n + max(8, n // 10)
    xs = _f32(rng.normal(size=(spare, in_f)))
    scale = REGIME_SCALE[regime][:, None]
    x = _f32(xs[:n] * scale) + np.float32(0)                             # (+0: a dead row holds no -0)
    nxt = n
    for _ in range(8):
        bad = np.nonzero(ambiguous_rows(x, W1, b1))[0]
        if not len(bad):
            break
        assert nxt + len(bad) <= spare, "not enough spare rows"
        x[bad] = xs[nxt:nxt + len(bad)] * scale[bad] + np.float32(0)
        nxt += len(bad)
    assert not ambiguous_rows(x, W1, b1).any(), "an ambiguous ReLU gate is left"
    return x


def _cotangent(rng, n, out, rows):
    dy = _f32(rng.normal(size=(n, out)))
    dy.ravel()[np.arange(dy.size) % 8 == 3] = 0.0
    if rows is not None:
        live = np.zeros(n, bool)
        live[list(rows)] = True
        dy[~live] = 0.0
        dy[np.array(rows), 0] = np.where(dy[np.array(rows), 0] == 0, np.float32(0.5), dy[np.array(rows), 0])   # every chosen row is live
    return dy


def _case(cfg, n, x, W1, b1, W2, b2, dy, regime, rows):
    c = types.SimpleNamespace(cfg=cfg, n=n, x=x, W1=W1, b1=b1, W2=W2, b2=b2, dy=dy, act=cfg[3], regime=regime, rows=rows, row_ids=np.arange(n))
    for a in (x, W1, b1, W2, b2, dy):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def draw(cfg, n, seed=0, rows=None):
    """A seeded case of the instance cfg = (in, hid, out, act) -> x, W1, b1, W2, b2, dy (float32, read-only), regime [n].
    rows (a sorted tuple): dy is nonzero on these rows only."""
    in_f, hid, out, act = cfg
    rng = np.random.default_rng([in_f, hid, out, act, n, seed, 0 if rows is None else 1])
    W1, b1, W2, b2 = _weights(rng, cfg)
    regime = row_regime(n, act)
    x = _rows(rng, n, in_f, regime, W1, b1)
    return _case(cfg, n, x, W1, b1, W2, b2, _cotangent(rng, n, out, rows), regime, rows)


HEADS = INSTANCES[:3]                  # opacity (tanh), color (sigmoid), cov: the three anchor MLPs, one input row


@functools.lru_cache(maxsize=None)
def draw3(n, seed=0, rows=None, dead=True):
    """The three anchor MLPs on one x [n, 54] -> three cases that share x (no gate of any head ambiguous)."""
    rng = np.random.default_rng([3, n, seed, 0 if rows is None else 1])
    w = [_weights(rng, cfg) for cfg in HEADS]
    regime = row_regime(n, ACT_TANH)
    if not dead:
        regime[regime == DEAD] = BODY
    x = _rows(rng, n, 54, regime, np.concatenate([t[0] for t in w]), np.concatenate([t[1] for t in w]))
    return [_case(cfg, n, x, *t, _cotangent(rng, n, cfg[2], rows), regime, rows) for cfg, t in zip(HEADS, w)]


@functools.lru_cache(maxsize=None)
def ref_of(cfg, n, seed=0, rows=None):
    c = draw(cfg, n, seed, rows)
    return Ref(c.x, c.W1, c.b1, c.W2, c.b2, c.act, c.dy)


def sparse_rows(n, cus, tile=16, seed=0, total=600):
    """The rows of the sparse cotangent at n = 256 cus + tail: the first tile and the last 33 rows, the 34 rows around row 256 cus,
    both ends of the first three and the last weight-gradient workgroups' ranges (for every rows-per-workgroup the launch
    arithmetic of csrc/mlp_wgrad.hip can arrive at: ceil(n / blocks) rounded up to a quantum of 8 .. 128 rows), random rows for
    the rest."""
    edge = 256 * cus
    s = set(range(min(tile, n))) | set(range(max(0, n - 33), n)) | set(range(max(0, edge - 17), min(n, edge + 17)))
    for blocks in (cus, 2 * cus):
        per = -(-n // min(blocks, -(-n // 256)))
        for q in (8, 16, 32, 64, 128):
            rpb = -(-per // q) * q
            last = (n - 1) // rpb
            for w in (1, 2, 3, last):
                s |= {w * rpb - 1, w * rpb}
    s = {r for r in s if 0 <= r < n}
    rng = np.random.default_rng(77 + seed)
    while len(s) < min(total, n):
        s.add(int(rng.integers(0, n)))
    return tuple(sorted(s))


def live_rows_only(c):
    """The sparse case `c` without the rows whose cotangent is 0 (they add exact zeros to every row sum and nothing else);
    row_ids keeps the rows' places, which decide the 256-row partials."""
    rows = np.array(c.rows)
    return types.SimpleNamespace(**{**c.__dict__, "n": len(rows), "x": c.x[rows], "dy": c.dy[rows], "regime": c.regime[rows], "row_ids": rows})


SPARSE_N = 256 * 256 + 17              # the GPU file's second-trip size on a part with 256 CUs


def cpu_cases():
    """Every case the literals are measured on: the instances at ROW_COUNTS, and the live rows of the GPU file's sparse-cotangent
    case (at 256 CUs), whose weight gradients sum ~600 rows."""
    for cfg in INSTANCES:
        for n in ROW_COUNTS:
            yield draw(cfg, n), ref_of(cfg, n)
        full = draw(cfg, SPARSE_N, 0, sparse_rows(SPARSE_N, 256))
        c = live_rows_only(full)
        yield c, Ref(c.x, c.W1, c.b1, c.W2, c.b2, c.act, c.dy)
        yield full, Ref(full.x, full.W1, full.b1, full.W2, full.b2, full.act, full.dy)     # (every row: literal (a) alone, the numpy loops are slow)


# ---- the fp32 literals ---------------------------------------------------------------------------------------------------------
def literal_torch(c):
    """(a) torch float32 on the CPU, autograd's backward."""
    import torch
    t = lambda a: torch.from_numpy(np.array(a)).requires_grad_(True)
    x, W1, b1, W2, b2 = (t(a) for a in (c.x, c.W1, c.b1, c.W2, c.b2))
    z1 = torch.nn.functional.linear(x, W1, b1)
    h = torch.relu(z1)
    z2 = torch.nn.functional.linear(h, W2, b2)
    y = torch.tanh(z2) if c.act == ACT_TANH else torch.sigmoid(z2) if c.act == ACT_SIGMOID else z2
    z1.retain_grad()
    z2.retain_grad()
    (y * torch.from_numpy(np.array(c.dy))).sum().backward()
    g = lambda v: v.detach().numpy()
    return dict(h=g(h), y=g(y), dz2=g(z2.grad), dz1=g(z1.grad), dx=g(x.grad), dW1=g(W1.grad), db1=g(b1.grad), dW2=g(W2.grad),
                db2=g(b2.grad))


def _contract_seq(A, B):
    """sum_k A[:, k] B[k, :] in float32, k ascending."""
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in range(A.shape[1]):
        acc = acc + A[:, k:k + 1] * B[k:k + 1, :]
    return acc


def _contract_frag(A, B):
    """The same in the order of csrc/mlp_frag.h: chain g takes the indices 16 q + 4 g + j in (q, j) order; (c0 + c1) + (c2 + c3)."""
    K = A.shape[1]
    chains = [np.zeros((A.shape[0], B.shape[1]), np.float32) for _ in range(4)]
    for q in range((K + 15) // 16):
        for j in range(4):
            for g in range(4):
                k = 16 * q + 4 * g + j
                if k < K:
                    chains[g] = chains[g] + A[:, k:k + 1] * B[k:k + 1, :]
    return (chains[0] + chains[1]) + (chains[2] + chains[3])


def _rows_seq(P, Q, chunk_of=None):
    """sum_r P[r, :, None] Q[r, None, :] in float32, r ascending (Q None: sum_r P[r]); chunk_of: the rows' 256-row partials
    first (sequential inside), then the partials in order."""
    def run(idx):
        acc = np.zeros((P.shape[1],) if Q is None else (P.shape[1], Q.shape[1]), np.float32)
        for r in idx:
            acc = acc + (P[r] if Q is None else P[r][:, None] * Q[r][None, :])
        return acc
    if chunk_of is None:
        return run(range(P.shape[0]))
    total = None
    for ch in np.unique(chunk_of):
        part = run(np.nonzero(chunk_of == ch)[0])
        total = part if total is None else total + part
    return total if total is not None else run([])


def literal_numpy(c, order):
    """(b) order = "seq", (c) order = "frag".  Rows whose cotangent is exactly 0 add exact zeros to every row sum and are left out
    of them (the sparse case: its sums run over the live rows, in row order)."""
    contract = _contract_seq if order == "seq" else _contract_frag
    x, W1, b1, W2, b2, dy = c.x, c.W1, c.b1, c.W2, c.b2, c.dy
    z1 = contract(x, W1.T.copy()) + b1
    h = np.maximum(z1, np.float32(0))
    z2 = contract(h, W2.T.copy()) + b2
    one = np.float32(1)
    if c.act == ACT_TANH:
        y = np.tanh(z2)
        g = one - y * y
    elif c.act == ACT_SIGMOID:
        with np.errstate(over="ignore"):
            y = one / (one + np.exp(-z2))
        g = y * (one - y)
    else:
        y, g = z2, None
    dz2 = dy if g is None else dy * g
    dh = contract(dz2, W2)
    dz1 = np.where(h > 0, dh, np.float32(0))
    dx = contract(dz1, W1)
    live = np.nonzero(np.abs(dy).sum(1) != 0)[0]
    chunk = (c.row_ids[live] // 256) if order == "frag" else None
    P2, P1, H, X = dz2[live], dz1[live], h[live], x[live]
    out = dict(h=h, y=y, dz2=dz2, dz1=dz1, dx=dx, dW1=_rows_seq(P1, X, chunk), db1=_rows_seq(P1, None, chunk),
               dW2=_rows_seq(P2, H, chunk), db2=_rows_seq(P2, None, chunk))
    assert all(v.dtype == np.float32 for v in out.values())
    return out


def _assemble32(feat_src, src_row, anchor, cam):
    """The anchor kernels' input row in float32, as csrc/mlp3.hip states it."""
    u = anchor - cam[None, :]
    d = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])[:, None]
    return np.concatenate([feat_src[src_row], u / d, d], axis=1), u, d


def draw_anchor(n, seed=0, n_src=None, W1=None, b1=None):
    """feat_src [n_src, 50], src_row [n] (distinct), anchor [n, 3], cam [3] (float32; no anchor at the camera); the rows
    src_row names are scaled by regime (no dead rows: a direction is never 0).  W1, b1: no gate of the fp32-assembled row is
    ambiguous against them (a rejected row is drawn again)."""
    rng = np.random.default_rng([n, seed, 54])
    n_src = n_src or n + max(3, n // 4)
    feat = _f32(rng.normal(size=(n_src, 50)))
    feat[::7] = 0.0
    src_row = rng.permutation(n_src)[:n].astype(np.int64)
    regime = row_regime(n, ACT_TANH)
    regime[regime == DEAD] = BODY
    feat[src_row] *= REGIME_SCALE[regime][:, None]
    anchor = _f32(rng.normal(size=(n, 3)) * 2)
    cam = _f32([0.3, -3.0, 0.5])
    for _ in range(8):
        if W1 is None:
            break
        bad = np.nonzero(ambiguous_rows(_assemble32(feat, src_row, anchor, cam)[0], W1, b1))[0]
        if not len(bad):
            break
        feat[src_row[bad]] = _f32(rng.normal(size=(len(bad), 50))) * REGIME_SCALE[regime[bad]][:, None]
        anchor[bad] = _f32(rng.normal(size=(len(bad), 3)) * 2)
    assert W1 is None or not ambiguous_rows(_assemble32(feat, src_row, anchor, cam)[0], W1, b1).any()
    assert (np.abs(anchor.astype(np.float64) - cam).sum(1) > 1e-3).all()
    return types.SimpleNamespace(n=n, n_src=n_src, feat_src=feat, src_row=src_row, anchor=anchor, cam=cam, regime=regime)


def literal_anchor(a, dX, how):
    """The row and the pull-back in float32: how = "torch" (autograd of cat / norm / division), "stated" (csrc/mlp3.hip's lines)."""
    dX = _f32(dX)
    if how == "torch":
        import torch
        anc = torch.from_numpy(np.array(a.anchor)).requires_grad_(True)
        u = anc - torch.from_numpy(np.array(a.cam))
        d = u.norm(dim=1, keepdim=True)
        x = torch.cat([torch.from_numpy(np.array(a.feat_src))[torch.from_numpy(a.src_row)], u / d, d], dim=1)
        (x * torch.from_numpy(dX)).sum().backward()
        return x.detach().numpy(), anc.grad.numpy()
    x, u, d = _assemble32(a.feat_src, a.src_row, a.anchor, a.cam)
    inv = np.float32(1) / d
    v = u * inv
    dv, dd = dX[:, 50:53], dX[:, 53:54]
    dot = ((v[:, 0] * dv[:, 0] + v[:, 1] * dv[:, 1]) + v[:, 2] * dv[:, 2])[:, None]
    da = (dv - v * dot) * inv + v * dd
    assert x.dtype == np.float32 and da.dtype == np.float32
    return x, da
