"""fp64 restatement of one level of the context model's training path, forward and backward (a helper, not a test): what
csrc/ctx_level.hip fuses into one launch per direction.  Written from the reference's level loop (scene/gaussian_model.py:1594-1616)
and the header comments of ctx_level.hip, in numpy float64, with no torch kernel and no autograd node; nothing is taken from a
kernel's output.  The trunk (IN -> 100 -> the 3 step-size outputs, no activation) is mlp_ref.Ref; the rest is stated here.

Forward (r a level row, k = 0, 1, 2 the tensors feat [50], scaling [6], offsets [30], q0 = (1.0, 0.001, 0.2) as float32):
  X[r]     [anchor[a_rows[r]] | base_f[pos[r]] | base_s[pos[r]] | hyp[r]] (in_dim 71), [anchor[a_rows[r]] (mask != 0) | hyp[r]]
           (in_dim 15; a product, -0.0 stays -0.0).  An equality, bit for bit.
  qadj     Ref's z2 = relu(X W1^T + b1) W2q^T + b2q                       U(qadj) = Ref's U(z2)
  t        tanh(qadj)                                                     U(t) = (1 - t^2) U(qadj) + u |t|
  Q        max(q0 (1 + t), 1e-9f)                                         U(Q) = q0 (U(t) + u (1 + t)) + u Q
           (1 + t and 1 - t^2 are formed without cancellation in fp64: 2 / (1 + exp(-2 qadj)) and (1 + t)(2 - (1 + t)))
  y_k      x_k[rows[r]] + noise_k[r] Q[r, k]                              U(y) = |noise| U(Q) + u |noise Q| + u |y|
           and, as an fp32 equality, x_k[rows] + noise_k Q_kernel (a product, then a sum); noise_k = ctx_noise(seed, k) at element
           r width_k + column, the 64-bit statement of oracle/context_ref.py
  sums_k   sum_r sum_c x_k[rows[r], c]                                    U = u sum |x_k[rows]|  (per-lane fp32 partials over the
           lane's tiles, then double: only the fp32 stage rounds, each partial within one rounding of its own absolute sum)
Backward (dy_k, dQ_ext, and for rows with side_map[r] >= 0 row side_map[r] of side_k, side_Q, dx_sub; a NULL operand is zeros):
  dx_k     dx_k[rows[r]] = dy_k[r] (+ side_k[side_map[r]]): ONE fp32 add, an equality; rows no level row names keep what they held
  gQ       dQ_ext + side_Q + sum_c dx_k noise_k                            U = u (|dQ_ext| + |side_Q| + sum_c |dx_k noise_k|)
  d qadj   gQ q0 (1 - t^2) where q0 (1 + t) >= 1e-9f, else 0                 U = q0 (1 - t^2) U(gQ) + |gQ| q0 (2 |t| U(t) + u (1 - t^2))
           exactly 0 (U = 0) where |qadj| >= 12 (fp32 tanh is -1 or 1 and nothing else) and where          + u |d qadj|
           the clamp of a head with q0 2^-24 < 1e-9 is active (below).  Elsewhere behind the clamp the unit stands: an fp32 tanh
           that is one step short of -1 (numpy's float32 tanh is, at qadj = -9.96) opens the gate of q0 = 1, within a unit of 0
  dZ1, dX, dW1, db1, dW2q, db2q   Ref's dz1, dx, dW1, db1, dW2, db2 with the cotangent d qadj and ITS unit (Ref's dy_unit);
           dX[r] += dx_sub[side_map[r]] (one more rounding of the sum); the weight gradients are accumulated onto a constant
           (one more rounding of the sum)
  dX_own   dX once more, in units of the dX product alone.  dX[r] - dx_sub[side_map[r]] lies in the span of the three vectors
           (gate[r] W2q[k]) W1, whatever d qadj the evaluation formed: with the least-squares dq^ [3] of the row (weighted by 1 / U, twice refitted),
           |dX - dx_sub - (gate (dq^ W2q)) W1| is judged in U = (u gate (|dq^| |W2q|)) |W1| + u |gate (dq^ W2q)| |W1| (+ u |dX| where
           dx_sub is added): the unit of dX above is mostly what d qadj carries (6 to 8 u |d qadj| on a body row), and behind it an
           error of the hidden-layer gradient's product with W1 of several of its own units goes unseen (`own_cotangent`)
  d_hyp_rows[rows[r]] = the last 12 columns of dX[r]: an equality with the dX the same call wrote; untouched elsewhere
and every U carries mlp_ref's absolute floor.  An element's error in units is |got - ref| / U; where U is 0 the element is equal.

Near t = -1 the sum 1 + t cancels: fp32 knows it in steps of 2^-24 only, and reaches the clamp (tanh = -1: Q = 1e-9) while the fp64
value q0 (1 + t) is still above it.  U(t) >= u |t| is one such step, so Q (through q0 U(t)) and d qadj (through |gQ| q0 2 |t| U(t),
where 1 - t^2 <= 2 (1 + t)) stay within a unit of the fp64 values whatever side of the clamp fp32 lands on - as long as one step of
1 + t clears the clamp: q0 2^-24 >= 1e-9, which holds for q0 = 1 and 0.2.  There fp32 closes the gate only with t = -1, where
1 - t^2 = 0 gives the same d qadj = 0 as the gate.  For q0 = 0.001 it does not hold: fp32 closes the gate at 1 + t <= 16 steps, and
d qadj jumps by 2 |gQ| 1e-9 = 16.8 units across it.  `draw` therefore treats that head's clamp like a ReLU gate: a row with
|q0 (1 + t) - 1e-9| <= GATE_UNITS U(q0 (1 + t)) on a head with q0 2^-24 < 1e-9 is steered elsewhere, and none is left (asserted; a
condition on the inputs, checked on the CPU, not an allowance in the comparison).

One number of units judges every element of every kernel: UNITS_KERNEL_LEVEL = 2 max(UNITS_LITERAL_LEVEL, mlp_ref.UNITS_LITERAL)
(the factor 2: mlp_ref.py).  UNITS_LITERAL_LEVEL is what three fp32 evaluations of these expressions need on the CPU
(tests/test_ctx_level_ref.py measures them, rounded up to one decimal; neither number is taken from a kernel's result):
  (a) `literal_torch`       torch float32 on the CPU, autograd through the whole composition (clamp, tanh, the trunk)
  (b) `literal_numpy(seq)`  numpy float32, every contraction and row sum strictly sequential
  (c) `literal_numpy(frag)` numpy float32 in the order csrc/mlp_frag.h documents (four interleaved chains), row sums as 256-row
                            partials, the three source sums as per-lane partials over the lane's tiles, then double
Measured maxima in units over `cpu_cases()` (both in_dim at 1, 15, 16, 17, 65, 129, 64 * 256 + 5 and 256 * 256 + 17 rows, dense
cotangents, and the sparse cotangent at the two large counts; every regime in every case of 15 rows or more):
              h   qadj      t      Q     yf     ys     yo   sums     gQ  dqadj    dz1     dX dX_own    dW1    db1   dW2q   db2q
  (a)     5.305  4.779  1.445  1.053  1.005  0.999  0.995  0.528  3.117  1.249  1.216  1.170  2.353  0.442  0.425  0.442  0.127
  (b)     5.580  4.779  1.445  1.138  1.058  0.999  0.995  1.906  4.376  2.292  1.826  1.570  2.336  0.461  0.367  0.473  0.288
  (c)     3.880  2.756  0.989  0.989  0.992  0.999  0.995  0.141  2.528  1.206  1.073  1.072  1.128  0.581  0.282  0.527  0.119
((b) and (c) leave out the dense case of 256 * 256 + 17 rows: their row sums are Python loops.)
UNITS_LITERAL_LEVEL = 5.6 is below mlp_ref.UNITS_LITERAL = 6.6, so the kernels are held to 2 * 6.6 = 13.2 units, below GATE_UNITS = 15:
the generator's gate distance stands.

Inputs (`draw`): one regime per row (r mod 16), mixed within a call.  The three step-size outputs of a row are steered through three
hyper columns that only six large hidden units read (weight +1 / -1 in W1, +1 / -1 in W2q of one head: qadj_k = body + s for an
input s of either sign) next to the random b2q:
  body        normal inputs, weights scaled 1 / sqrt(fan_in)
  dead        every input of the row exactly 0 (a zero anchor row, a zero parent, zero hyper latents; in_dim 15: also a masked
              anchor row): z1 = b1 in any order, and b1 holds exact zeros, negatives and positives
  sat low     qadj <= -12 on one head (each in turn): fp32 tanh is exactly -1, the clamp is active, d qadj is exactly 0
  cancelling  qadj in (-9, -6) on one head: 1 + t is a few fp32 steps wide (q0 = 0.001: outside the clamp's neighbourhood, see
              above)
  cancelled   qadj in (-10.6, -9.05) on one head: fp32 tanh is -1 (1 + t < 2^-25) while fp64 q0 (1 + t) is above the clamp for
              q0 = 1 and 0.2 (the interval (-9, -6) holds no such row: 1 + tanh(-9) = 3.05e-8 > 2^-25)
  sat high    qadj >= 12 on one head: t = 1, d qadj = 0 through 1 - t^2
Indices: a_rows and pos with repeats (several children of one parent), a_rows hits rows 0 and n_anchor - 1, pos hits n_par - 1, rows
is a slice of a permutation of n + 11 rows, side_map a shuffled numbering of ~15 % of the rows.
ReLU gates as in mlp_ref: a row with a hidden unit at 0 < |z1| <= GATE_UNITS U(z1) gets new hyper latents until none is left
(asserted).  Cotangents: dense (every eighth element 0), or nonzero on ~600 rows only (`sparse_rows`: dy, dQ_ext and the side arrays
together), so that a weight gradient of 65 553 rows sums ~600 terms and a dropped or doubled row is thousands of units.
"""
import functools
import types

import numpy as np

import mlp_ref as mr
from mlp_ref import FLOOR, GATE_UNITS, U
from oracle.context_ref import ctx_noise

# What the fp32 literals need on these inputs, in units: measured by test_ctx_level_ref.py, rounded up to one decimal.
UNITS_LITERAL_LEVEL = 5.6
UNITS_KERNEL_LEVEL = 2 * max(UNITS_LITERAL_LEVEL, mr.UNITS_LITERAL)      # 13.2: mlp_ref's literals need more than the head adds
assert UNITS_KERNEL_LEVEL < GATE_UNITS

SEED = 0x5DEECE66D
Q0 = tuple(float(np.float32(q)) for q in (1.0, 0.001, 0.2))             # the product's step sizes, as the float32 the C ABI takes
CLAMP = float(np.float32(1e-9))
WIDTHS = (50, 6, 30)
HID = 100
NAMES = ("f", "s", "o")
BODY, DEAD, SAT_LOW, CANCEL, CANCELLED, SAT_HIGH = range(6)
REGIMES = ("body", "dead", "sat low", "cancelling", "cancelled", "sat high")
TARGET = {SAT_LOW: (-22.0, -12.5), CANCEL: (-9.0, -6.0), CANCELLED: (-10.6, -9.05), SAT_HIGH: (12.5, 22.0)}
STEER_COLS = (2, 6, 11)                # hyper columns (of the 12) that carry the steering input of head 0, 1, 2
STEER_POS, STEER_NEG = (7, 50, 97), (23, 64, 99)       # hidden units relu(+s), relu(-s) of head k (the last tile's units among them)
CPU_CUS = 256
ROW_COUNTS = (1, 15, 16, 17, 65, 129)


def large_counts(cus):
    """The backward's second loop trip (ragged) and the forward's second (the backward's fifth)."""
    return (64 * cus + 5, 256 * cus + 17)


_f64, _f32 = mr._f64, mr._f32


def noise(k, n, seed=SEED):
    return ctx_noise(seed, k, n * WIDTHS[k]).reshape(n, WIDTHS[k])


def sparse_rows(n, cus, total=600):
    """The live rows of the sparse cotangent: the first tile, the last 33 rows, the 34 rows around every trip edge of the backward
    (64 cus k rows) and of the forward (256 cus), random rows for the rest."""
    s = set(range(min(16, n))) | set(range(max(0, n - 33), n))
    for edge in [64 * cus * k for k in range(1, 5)]:
        s |= set(range(edge - 17, edge + 17))
    s = {r for r in s if 0 <= r < n}
    rng = np.random.default_rng(177)
    while len(s) < min(total, n):
        s.add(int(rng.integers(0, n)))
    return tuple(sorted(s))


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def row_regime(n):
    r = np.arange(n)
    reg = np.full(n, BODY)
    head = (r // 16) % 3
    reg[r % 16 == 3] = DEAD
    reg[r % 16 == 5] = SAT_LOW
    reg[r % 16 == 9] = CANCEL
    reg[r % 16 == 12] = SAT_HIGH
    reg[r % 16 == 14] = CANCELLED
    head[r % 16 == 14] = (head[r % 16 == 14] + 1) % 3
    return reg, head


def assemble(c, mask=True, idx=None):
    """The level's MLP input rows in float32 (copies and, at in_dim 15 with a mask, one exact product); idx: these rows only."""
    idx = slice(None) if idx is None else idx
    a_rows = c.a_rows[idx]
    a = c.anchor[a_rows]
    if c.in_dim == 15:
        if mask:
            a = a * (c.a_mask[a_rows] != 0).astype(np.float32)[:, None]
        return _f32(np.concatenate([a, c.hyp[idx]], axis=1))
    return _f32(np.concatenate([a, c.base_f[c.pos[idx]], c.base_s[c.pos[idx]], c.hyp[idx]], axis=1))


def ambiguous_rows(x, W1, b1):
    """mlp_ref's rule: a hidden unit with 0 < |z1| <= GATE_UNITS U(z1), or at 0 by cancellation.  (A unit whose every term is 0 is
    at 0 in any order: the steering units of a row whose steering input is 0.)"""
    x, W1, b1 = _f64(x), _f64(W1), _f64(b1)
    z1 = x @ W1.T + b1
    asum = np.abs(x) @ np.abs(W1).T + np.abs(b1)
    return (((z1 != 0) & (np.abs(z1) <= GATE_UNITS * (U * asum + FLOOR))) | ((z1 == 0) & (asum != 0))).any(1)


def _weights(rng, in_dim):
    W1 = _f32(rng.normal(size=(HID, in_dim)) / np.sqrt(in_dim))
    b1 = _f32(rng.uniform(-1, 1, HID) / np.sqrt(in_dim))
    b1[::5] = 0.0                                                        # exact zeros next to both signs
    W2q = _f32(rng.normal(size=(3, HID)) / np.sqrt(HID))
    b2q = _f32(rng.uniform(-1, 1, 3) / np.sqrt(HID))
    for k in range(3):
        col = in_dim - 12 + STEER_COLS[k]
        W1[:, col] = 0.0
        for unit, sign in ((STEER_POS[k], 1.0), (STEER_NEG[k], -1.0)):
            W1[unit, :] = 0.0
            W1[unit, col] = sign
            b1[unit] = 0.0
            W2q[:, unit] = 0.0
            W2q[k, unit] = sign
    return W1, b1, W2q, b2q


def _head(c, mask=True, idx=None):
    """fp64: the trunk (mlp_ref.Ref, zero cotangent) and the three heads of the case's rows (idx: these rows only)."""
    X = assemble(c, mask, idx)
    tr = mr.Ref(X, c.W1, c.b1, c.W2q, c.b2q, mr.ACT_NONE, np.zeros((X.shape[0], 3)))
    return tr, Head(tr.values["y"], tr.units["y"])


class Head:
    """t, Q, the clamp gate and their units from qadj and its unit."""

    def __init__(self, qadj, Uq):
        q0 = np.array(Q0)
        with np.errstate(over="ignore"):
            self.one_p = 2.0 / (1.0 + np.exp(-2.0 * qadj))               # 1 + t, no cancellation
        self.qadj, self.Uq = qadj, Uq
        self.t = self.one_p - 1.0
        self.g = self.one_p * (2.0 - self.one_p)                         # 1 - t^2
        self.Ut = self.g * Uq + U * np.abs(self.t)
        self.pre = q0 * self.one_p
        self.Upre = q0 * (self.Ut + U * self.one_p) + U * self.pre + FLOOR
        self.Q = np.maximum(self.pre, CLAMP)
        self.UQ = q0 * (self.Ut + U * self.one_p) + U * self.Q + FLOOR
        self.open = self.pre >= CLAMP
        self.jumps = np.array(Q0) * 2.0 ** -24 < CLAMP                   # heads whose clamp is not reached through t = -1 alone
        self.flat = (np.abs(qadj) >= 12.0) | (~self.open & self.jumps[None, :])    # d qadj is exactly 0

    def ambiguous_clamp(self):
        """[n, 3]: the clamp gate could fall either way in fp32 AND the two ways differ by more than a unit (see the docstring)."""
        return self.jumps[None, :] & (np.abs(self.pre - CLAMP) <= GATE_UNITS * self.Upre)


def _case(**kw):
    c = types.SimpleNamespace(**kw)
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def draw(n, in_dim, sparse=False, cus=CPU_CUS, seed=0):
    """A seeded level of n rows: every operand of the forward and the backward (float32 / int64 / int32 / uint8, read-only), the
    regime and the steered head of every row.  sparse: the cotangents are nonzero on sparse_rows(n, cus) only."""
    rng = np.random.default_rng([n, in_dim, int(sparse), seed])
    R = lambda *s: _f32(rng.normal(size=s))
    N, n_par = n + 11, max(2, n // 3) + 1
    za, zm, zp = 5, 7, 0                                                 # a zero anchor row, a masked anchor row, a zero parent
    W1, b1, W2q, b2q = _weights(rng, in_dim)
    regime, head = row_regime(n)
    dead = regime == DEAD
    anchor, base_f, base_s, hyp = R(N, 3), R(n_par, 50), R(n_par, 6), R(n, 12)
    anchor[za], base_f[zp], base_s[zp] = 0.0, 0.0, 0.0
    a_mask = (rng.random(N) < 0.7).astype(np.uint8)
    a_mask[za], a_mask[zm], a_mask[0], a_mask[N - 1] = 1, 0, 1, 1
    a_rows = rng.integers(0, max(1, N // 2), n).astype(np.int64)         # (repeats: ~two children per parent)
    a_rows[a_rows == za] = za + 1
    pos = rng.integers(1, n_par, n).astype(np.int64)
    alive = np.nonzero(~dead)[0]
    a_rows[alive[0]], pos[alive[-1]] = 0, n_par - 1
    if len(alive) > 1:
        a_rows[alive[-1]] = N - 1
    d = np.nonzero(dead)[0]
    a_rows[d], pos[d], hyp[d] = za, zp, 0.0
    if in_dim == 15:
        a_rows[d[1::2]] = zm                                             # (a masked row with both signs: -0.0 and 0.0)
    xf, xs, xo = R(N, 50), R(N, 6), R(N, 30)
    rows = rng.permutation(N)[:n].astype(np.int64)
    c = types.SimpleNamespace(n=n, in_dim=in_dim, N=N, n_par=n_par, anchor=anchor, base_f=base_f, base_s=base_s, hyp=hyp, a_mask=a_mask,
                              a_rows=a_rows, pos=pos, W1=W1, b1=b1, W2q=W2q, b2q=b2q)
    free = np.array([j for j in range(12) if j not in STEER_COLS])
    scols = np.array(STEER_COLS)
    masks = (True, False) if in_dim == 15 else (True,)
    steered = np.nonzero(regime >= SAT_LOW)[0]
    a_rows[alive[a_rows[alive] == zm]] = zm + 1
    a_mask[a_rows[steered]] = 1                                          # (a steered row is the same row with and without the mask)
    # ReLU gates: new hyper latents for a row that holds an ambiguous one (a dead row never does; without the mask the dead rows
    # at the masked anchor row are one and the same ordinary row, which gets a new anchor)
    if in_dim == 15 and len(d) > 1:
        one = d[1:2]
        for _ in range(12):
            if not (ambiguous_rows(assemble(c, False, one), W1, b1).any() or _head(c, False, one)[1].ambiguous_clamp().any()):
                break
            anchor[zm] = R(3)
    todo = alive
    for _ in range(12):
        bad = np.logical_or.reduce([ambiguous_rows(assemble(c, m, todo), W1, b1) for m in masks])
        todo = todo[bad]
        if not len(todo):
            break
        assert not dead[todo].any()
        hyp[todo[:, None], free[None, :]] = R(len(todo), len(free))
    # the steered heads, and the clamp of the head whose gate jumps: a new target until no row is near it
    todo = steered
    for _ in range(60):
        if len(todo):
            lo, hi = np.array([TARGET[g] for g in regime[todo]]).T
            k = head[todo]
            body = _head(c, True, todo)[1].qadj[np.arange(len(todo)), k] - hyp[todo, scols[k]].astype(np.float64)
            hyp[todo, scols[k]] = _f32(rng.uniform(lo, hi) - body)
            todo = todo[np.logical_or.reduce([_head(c, m, todo)[1].ambiguous_clamp().any(1) for m in masks])]
        if not len(todo):
            break
    rest = np.nonzero(regime == BODY)[0]                                 # (a body row that far down: new steering inputs)
    for _ in range(12):
        if len(rest):
            rest = rest[np.logical_or.reduce([_head(c, m, rest)[1].ambiguous_clamp().any(1) for m in masks])]
        if not len(rest):
            break
        assert not dead[rest].any()
        hyp[rest[:, None], scols[None, :]] = R(len(rest), 3)
    # ---- the backward's operands ----
    dys = [R(n, w) for w in WIDTHS]
    dQe = R(n, 3)
    for a in dys + [dQe]:
        a.ravel()[np.arange(a.size) % 8 == 3] = 0.0
    live = None
    if sparse:
        live = np.array(sparse_rows(n, cus))
        off = np.ones(n, bool)
        off[live] = False
        for a in dys + [dQe]:
            a[off] = 0.0
        dQe[live, 0] = np.where(dQe[live, 0] == 0, np.float32(0.5), dQe[live, 0])
    pool = np.arange(n) if live is None else live
    m = max(1, int(round(0.15 * len(pool))))
    sub = rng.permutation(pool)[:m]
    side_map = np.full(n, -1, np.int32)
    side_map[sub] = rng.permutation(m).astype(np.int32)
    side = [R(m, w) for w in WIDTHS]
    c = _case(n=n, in_dim=in_dim, N=N, n_par=n_par, m=m, sparse=sparse, cus=cus, anchor=anchor, base_f=base_f, base_s=base_s, hyp=hyp,
              a_mask=a_mask, a_rows=a_rows, pos=pos, W1=W1, b1=b1, W2q=W2q, b2q=b2q, xf=xf, xs=xs, xo=xo, rows=rows, regime=regime,
              head=head, dyf=dys[0], dys=dys[1], dyo=dys[2], dQe=dQe, side_map=side_map, side_f=side[0], side_s=side[1],
              side_o=side[2], side_Q=R(m, 3), dx_sub=R(m, in_dim), live=live)
    check_inputs(c)
    return c


def check_inputs(c):
    """No ambiguous ReLU gate, no ambiguous clamp gate, every steered row in its interval - with and without the mask."""
    for mask in ((True, False) if c.in_dim == 15 else (True,)):
        X = assemble(c, mask)
        assert not ambiguous_rows(X, c.W1, c.b1).any(), "an ambiguous ReLU gate is left"
        _, hd = _head(c, mask)
        assert not hd.ambiguous_clamp().any(), "an ambiguous clamp gate is left"
        assert not mask or (X[c.regime == DEAD] == 0).all()
        for g, (lo, hi) in TARGET.items():
            r = np.nonzero(c.regime == g)[0]
            q = hd.qadj[r, c.head[r]]
            assert ((q > lo - 1e-3) & (q < hi + 1e-3)).all(), (REGIMES[g], q.min(initial=0), q.max(initial=0))


# ---- the statement and its units ----------------------------------------------------------------------------------------------
QUANTITIES = ("h", "qadj", "t", "Q", "yf", "ys", "yo", "sums", "gQ", "dqadj", "dz1", "dX", "dX_own", "dW1", "db1", "dW2q", "db2q")


class Forward:
    """values[k], units[k] of h, qadj, t, Q, yf, ys, yo, sums; X (float32, the equality)."""

    def __init__(self, c, mask=True):
        self.c, self.mask = c, mask
        self.X = assemble(c, mask)
        self.trunk, hd = _head(c, mask)
        self.head = hd
        self.noise = [noise(k, c.n) for k in range(3)]
        v = dict(h=self.trunk.values["h"], qadj=hd.qadj, t=hd.t, Q=hd.Q)
        u = dict(h=self.trunk.units["h"], qadj=hd.Uq, t=hd.Ut, Q=hd.UQ)
        sums, Usums = [], []
        for k, nm in enumerate(NAMES):
            x = _f64(getattr(c, "x" + nm)[c.rows])
            nz = _f64(self.noise[k])
            nq = nz * hd.Q[:, k:k + 1]
            v["y" + nm] = x + nq
            u["y" + nm] = np.abs(nz) * hd.UQ[:, k:k + 1] + U * np.abs(nq) + U * np.abs(x + nq) + FLOOR
            sums.append(x.sum())
            Usums.append(U * np.abs(x).sum() + FLOOR)
        v["sums"], u["sums"] = np.array(sums), np.array(Usums)
        self.values, self.units = v, u

    def y_from(self, Qk):
        """The fp32 equality: x[rows] + noise * Q of the kernel's own Q (a product, then a sum)."""
        Qk = _f32(Qk)
        return [getattr(self.c, "x" + nm)[self.c.rows] + self.noise[k] * Qk[:, k:k + 1] for k, nm in enumerate(NAMES)]


class Backward:
    """values[k], units[k] of gQ, dqadj, dz1, dX, dW1, db1, dW2q, db2q; dx (the three fp32 equalities, [n, width]).
    dy: which of dyf / dys / dyo are given; dqe, side, dx_sub: whether dQ_ext, the side map with its arrays, dx_sub are."""

    def __init__(self, fwd, dy=(True, True, True), dqe=True, side=True, dx_sub=True):
        c, hd = fwd.c, fwd.head
        sm = c.side_map if side else np.full(c.n, -1, np.int32)
        chosen = np.nonzero(sm >= 0)[0]
        at = sm[chosen]
        gQ = np.zeros((c.n, 3))
        aQ = np.zeros((c.n, 3))
        if dqe:
            gQ += _f64(c.dQe)
            aQ += np.abs(_f64(c.dQe))
        gQ[chosen] += _f64(c.side_Q[at])
        aQ[chosen] += np.abs(_f64(c.side_Q[at]))
        self.dx = []
        for k, nm in enumerate(NAMES):
            d = np.array(getattr(c, "dy" + nm)) if dy[k] else np.zeros((c.n, WIDTHS[k]), np.float32)
            d[chosen] = d[chosen] + getattr(c, "side_" + nm)[at]                   # ONE float32 add
            self.dx.append(d)
            p = _f64(d) * _f64(fwd.noise[k])
            gQ[:, k] += p.sum(1)
            aQ[:, k] += np.abs(p).sum(1)
        UgQ = U * aQ + FLOOR
        q0 = np.array(Q0)
        zero = hd.flat
        dq = np.where(hd.open & ~zero, gQ * q0 * hd.g, 0.0)
        Udq = np.where(zero, 0.0, q0 * hd.g * UgQ + np.abs(gQ) * q0 * (2 * np.abs(hd.t) * hd.Ut + U * hd.g) + U * np.abs(dq) + FLOOR)
        tr = mr.Ref(fwd.X, c.W1, c.b1, c.W2q, c.b2q, mr.ACT_NONE, dq, dy_unit=Udq)
        dX, UdX = tr.values["dx"].copy(), tr.units["dx"].copy()
        if dx_sub and side:
            dX[chosen] += _f64(c.dx_sub[at])
            UdX[chosen] += U * np.abs(dX[chosen])
        self.trunk, self.gate = tr, tr.gate
        self.c, self.sub = c, (chosen, at) if (dx_sub and side) else None
        self.values = dict(gQ=gQ, dqadj=dq, dz1=tr.values["dz1"], dX=dX, dW1=tr.values["dW1"], db1=tr.values["db1"],
                           dW2q=tr.values["dW2"], db2q=tr.values["db2"])
        self.units = dict(gQ=UgQ, dqadj=Udq, dz1=tr.units["dz1"], dX=UdX, dW1=tr.units["dW1"], db1=tr.units["db1"],
                          dW2q=tr.units["dW2"], db2q=tr.units["db2"])
        self.exact_zero = zero


def own_cotangent(bwd, dX):
    """dX in units of the dX product ALONE (see the docstring): |dX - dx_sub - fit| / U with fit = (gate (dq^ W2q)) W1 for the
    least-squares dq^ [n, 3] of every row, U = (u gate (|dq^| |W2q|)) |W1| + u |gate (dq^ W2q)| |W1| (+ u |dX| where dx_sub is added)."""
    c, gate = bwd.c, bwd.gate
    W1, W2q = _f64(c.W1), _f64(c.W2q)
    d = _f64(dX).copy()
    side = np.zeros(d.shape[0])
    if bwd.sub is not None:
        chosen, at = bwd.sub
        d[chosen] -= _f64(c.dx_sub[at])
        side[chosen] = 1.0
    err = np.zeros_like(d)
    nz = np.nonzero(np.abs(d).sum(1) != 0)[0]                            # (a row of zeros is fitted by dq^ = 0 with no error)
    d, side, gate, dXa = d[nz], side[nz], gate[nz], np.abs(_f64(dX))[nz]
    V = np.stack([(gate * W2q[k]) @ W1 for k in range(3)], axis=2)                   # [rows, in_dim, 3]
    aW1, aW2q = np.abs(W1), np.abs(W2q)
    unit = np.ones_like(d)
    for _ in range(3):                 # least squares in the elements' own units: the first fit unweighted, then twice reweighted
        Vw, dw = V / unit[:, :, None], d / unit
        G = np.einsum("rik,ril->rkl", Vw, Vw)
        G += (1e-24 * np.trace(G, axis1=1, axis2=2) + FLOOR)[:, None, None] * np.eye(3)
        dq = np.linalg.solve(G, np.einsum("rik,ri->rk", Vw, dw)[:, :, None])[:, :, 0]
        dz1 = gate * (dq @ W2q)
        unit = (U * gate * (np.abs(dq) @ aW2q)) @ aW1 + U * (np.abs(dz1) @ aW1) + U * side[:, None] * dXa + FLOOR
        unit += 1e-6 * U * np.abs(d).max(1, keepdims=True)                # (the fit's own float64 round-off, where dq^ should be 0)
    err[nz] = np.abs(d - dz1 @ W1) / unit
    return err


def judge(ref, got, maxima, what, limit=None, preload=0.0):
    """Every element of the quantities in the dict `got` within `limit` units (default UNITS_KERNEL_LEVEL) of ref (a Forward or a
    Backward).  preload: the constant the weight-gradient buffers held (one more rounding of the sum)."""
    limit = UNITS_KERNEL_LEVEL if limit is None else limit
    for k, v in got.items():
        want, unit = ref.values[k], ref.units[k]
        if preload and k in ("dW1", "db1", "dW2q", "db2q"):
            want = want + preload
            unit = unit + U * np.abs(want)
        err = mr.units_error(v, want, unit, (what, k))
        maxima.add(k, err)
        assert err.max(initial=0.0) <= limit, (what, k, float(err.max()), np.unravel_index(int(err.argmax()), err.shape))
        if k == "dX":
            err = own_cotangent(ref, v)
            maxima.add("dX_own", err)
            assert err.max(initial=0.0) <= limit, (what, "dX_own", float(err.max()), np.unravel_index(int(err.argmax()), err.shape))


@functools.lru_cache(maxsize=4)
def forward_of(n, in_dim, sparse=False, cus=CPU_CUS, mask=True):
    return Forward(draw(n, in_dim, sparse, cus), mask)


def cpu_cases():
    """Every case the literals are measured on: (case, Forward, Backward), all operands given."""
    for in_dim in (71, 15):
        for n in ROW_COUNTS + large_counts(CPU_CUS):
            for sparse in ((False, True) if n > 1000 else (False,)):
                f = Forward(draw(n, in_dim, sparse))
                yield f.c, f, Backward(f)


# ---- the fp32 literals --------------------------------------------------------------------------------------------------------
def _dx32(c):
    sm = c.side_map
    chosen = np.nonzero(sm >= 0)[0]
    out = []
    for nm in NAMES:
        d = np.array(getattr(c, "dy" + nm))
        d[chosen] = d[chosen] + getattr(c, "side_" + nm)[sm[chosen]]
        out.append(d)
    sQ = np.zeros((c.n, 3), np.float32)
    sQ[chosen] = c.side_Q[sm[chosen]]
    sub = np.zeros((c.n, c.in_dim), np.float32)
    sub[chosen] = c.dx_sub[sm[chosen]]
    return out, sQ, sub


def literal_torch(c, fwd):
    """(a) torch float32 on the CPU, autograd's backward through y = x + noise clamp(q0 (1 + tanh(trunk(X))))."""
    import torch
    T = lambda a: torch.from_numpy(np.array(a))
    G = lambda a: T(a).requires_grad_(True)
    X, W1, b1, W2q, b2q = (G(a) for a in (fwd.X, c.W1, c.b1, c.W2q, c.b2q))
    z1 = torch.nn.functional.linear(X, W1, b1)
    h = torch.relu(z1)
    qadj = torch.nn.functional.linear(h, W2q, b2q)
    t = torch.tanh(qadj)
    Q = (T(np.array(Q0, np.float32)) * (1 + t)).clamp(1e-9)
    for v in (z1, qadj, Q):
        v.retain_grad()
    dx, sQ, sub = _dx32(c)
    xs = [T(getattr(c, "x" + nm)[c.rows]) for nm in NAMES]
    ys = [x + T(fwd.noise[k]) * Q[:, k:k + 1] for k, x in enumerate(xs)]
    (sum((y * T(d)).sum() for y, d in zip(ys, dx)) + (Q * (T(c.dQe) + T(sQ))).sum()).backward()
    g = lambda v: v.detach().numpy()
    return dict(h=g(h), qadj=g(qadj), t=g(t), Q=g(Q), yf=g(ys[0]), ys=g(ys[1]), yo=g(ys[2]), sums=np.array([float(x.sum()) for x in xs]),
                gQ=g(Q.grad), dqadj=g(qadj.grad), dz1=g(z1.grad), dX=g(X.grad) + sub, dW1=g(W1.grad), db1=g(b1.grad),
                dW2q=g(W2q.grad), db2q=g(b2q.grad))


def _dot_rows(A, B, order):
    """sum_c A[r, c] B[r, c] in float32: c ascending, or mlp_frag.h's four interleaved chains."""
    if order == "seq":
        acc = np.zeros(A.shape[0], np.float32)
        for j in range(A.shape[1]):
            acc = acc + A[:, j] * B[:, j]
        return acc
    ch = [np.zeros(A.shape[0], np.float32) for _ in range(4)]
    for j in range(A.shape[1]):
        g = (j % 16) // 4
        ch[g] = ch[g] + A[:, j] * B[:, j]
    return (ch[0] + ch[1]) + (ch[2] + ch[3])


def _sum_all(x, order, cus=CPU_CUS):
    """The sum of a [n, w] float32 array: one sequential float32 chain, or float32 partials per lane (row mod 16, column group, the
    wave's tiles in turn: tile, tile + stride, ...) that are then summed in double."""
    if order == "seq":
        return float(np.add.accumulate(x.ravel(), dtype=np.float32)[-1])
    n, w = x.shape
    tiles = -(-n // 16)
    stride = 16 * 8 * min(-(-tiles // 8), 2 * cus)                       # rows per trip of the forward's grid
    trips = -(-n // stride)
    xp = np.zeros((trips * stride, -(-w // 4) * 4), np.float32)
    xp[:n, :w] = x
    xp = xp.reshape(trips, stride, -1, 4)
    part = np.zeros(xp.shape[1:3], np.float32)
    for tr in range(trips):
        part = part + ((xp[tr, :, :, 0] + xp[tr, :, :, 1]) + (xp[tr, :, :, 2] + xp[tr, :, :, 3]))
    return float(part.astype(np.float64).sum())


def literal_numpy(c, fwd, order):
    """(b) order = "seq", (c) order = "frag": the trunk is mlp_ref.literal_numpy, the head and the noise are stated here."""
    one = np.float32(1)
    base = dict(cfg=(c.in_dim, HID, 3, 0), n=c.n, x=fwd.X, W1=c.W1, b1=c.b1, W2=c.W2q, b2=c.b2q, act=mr.ACT_NONE, row_ids=np.arange(c.n))
    f = mr.literal_numpy(types.SimpleNamespace(dy=np.zeros((c.n, 3), np.float32), **base), order)
    qadj = f["y"]
    t = np.tanh(qadj)
    q0 = np.array(Q0, np.float32)
    pre = q0 * (one + t)
    Q = np.maximum(pre, np.float32(1e-9))
    dx, sQ, sub = _dx32(c)
    xs = [getattr(c, "x" + nm)[c.rows] for nm in NAMES]
    ys = [x + fwd.noise[k] * Q[:, k:k + 1] for k, x in enumerate(xs)]
    gQ = np.stack([_dot_rows(dx[k], fwd.noise[k], order) + (c.dQe[:, k] + sQ[:, k]) for k in range(3)], axis=1)
    dq = np.where(pre >= np.float32(1e-9), gQ * q0 * (one - t * t), np.float32(0))
    b = mr.literal_numpy(types.SimpleNamespace(dy=dq, **base), order)
    out = dict(h=f["h"], qadj=qadj, t=t, Q=Q, yf=ys[0], ys=ys[1], yo=ys[2], sums=np.array([_sum_all(x, order, c.cus) for x in xs]), gQ=gQ,
               dqadj=dq, dz1=b["dz1"], dX=b["dx"] + sub, dW1=b["dW1"], db1=b["db1"], dW2q=b["dW2"], db2q=b["db2"])
    assert all(v.dtype == np.float32 for k, v in out.items() if k != "sums")
    return out


def check_exact(fwd, bwd, got, what=""):
    """The equalities on whatever of h, dz1, dqadj, dX the dict `got` holds."""
    closed = ~fwd.trunk.gate
    for k in ("h", "dz1"):
        if k in got:
            assert (np.asarray(got[k])[closed] == 0).all(), (what, k, "not 0 behind a closed gate")
    if "dqadj" in got:
        assert (np.asarray(got["dqadj"])[bwd.exact_zero] == 0).all(), (what, "d qadj not 0 where tanh is +-1 or the jumping clamp is active")
