"""numpy restatement of the row movers, row accumulators and element-wise noise kernels of csrc/ctx.hip (a helper, not a test):
what tests/test_ctx_rows_gpu.py compares the kernels with, and the drawers of its inputs.  float32 where an operation is a copy,
one product or one add (those are equalities, bit for bit); float64 wherever anything is summed.  Nothing here is taken from a
kernel's output, and nothing needs a GPU.

  rowcat / rowcat_bwd         cat([(src * mask)[idx] ...]) and its pull-back: mode 1 an index_copy of dout * mask, mode 2 the fp64 sum of
                              the terms of every source row with sum |terms| and the number of terms k (bound (k - 1) u sum |terms|)
  gather_rows / scatter_sorted   index_select and zeros().index_copy_()
  add_rows                    out[idx] + g: one fp32 add per element
  mark / zero_unmarked        the stamp array and the rows whose stamp is not the call's generation
  gather_segmented            rows of the virtual concatenation of row blocks (a missing block is zeros)
  csr_seq32 / csr_f64         the per-parent sums over the CSR child lists: sequentially in float32 in child order (what both kernels
                              state: "same additions in the same (child) order per column", an equality) and in fp64 with sum |terms|
  noise_quant                 Q and d qadj in ctx_level_ref's units (its Head on a qadj that is an exact input: U(qadj) = 0), the
                              noise from the integer generator (oracle/context_ref.py:ctx_noise), y against x + u Q_kernel within
                              u (|x + u Q| + |u Q|), dx = dy + side as one fp32 add
  means_bound                 t u sum |v| / count: t fp32 terms per lane (trips of the row loop times the lane's columns per row), the
                              rest of the reduction is in double; the last of the t roundings is the mean's own cast to float

u = 2^-24 throughout (mlp_ref.U).

SECOND_TRIP: every launcher sizes its grid with stream_grid(total, per_block) = min(ceil(total / per_block), 4096); the loops are
grid-stride loops, so a count above 4096 per_block is the first at which a workgroup has to come round again BECAUSE OF THE CAP
(a launcher whose per_block is several times what a workgroup covers per trip already loops below it).  The table holds per_block in
the unit the launcher counts in and an odd remainder; `second_trip(name)` is the count.
"""
import functools
import types

import numpy as np

import ctx_level_ref as lr
import mlp_ref as mr
from mlp_ref import FLOOR, U
from oracle.context_ref import ctx_noise

_f64, _f32 = mr._f64, mr._f32
Q0, CLAMP, SEED = lr.Q0, lr.CLAMP, lr.SEED
UNITS = lr.UNITS_KERNEL_LEVEL          # the limit test_ctx_level_fp64_gpu.py holds the level kernels' Q and d qadj to
AMBIGUOUS_CAP = 0.02                   # the largest share of rows a draw may lose to Head.ambiguous_clamp
GRID_CAP = 256 * 16                    # stream_grid's `cap` (ctx.hip:228)
RC_ROWS = 32


def stream_grid(total, per_block):
    """ctx.hip:226-230."""
    return max(1, min(GRID_CAP, -(-total // per_block)))


# name: (per_block, unit, remainder, the launcher line the per_block was read from)
SECOND_TRIP = {
    "rowcat_fwd":          (256 * 4, "elements", 3),     # ctx.hip:264  stream_grid(n * a.W, 256 * 4)
    "rowcat_bwd":          (256 * 4, "elements", 3),     # ctx.hip:286  stream_grid(n * a.W, 256 * 4)
    "gather_segmented":    (256 * 4, "elements", 5),     # ctx.hip:176  stream_grid(n * w, 256 * 4)
    "add_rows":            (256 * 4, "elements", 7),     # ctx.hip:375  stream_grid(n * w, 256 * 4)
    "rowcat_fwd_lds":      (RC_ROWS, "rows", 17),        # ctx.hip:260-261  min(ceil(n / RC_ROWS), 256 * 8): a cap of its own (CAPS)
    "rowgather4":          (256 * 2, "float4", 5),       # ctx.hip:250  stream_grid(n * (a.W / 4), 256 * 2)
    "scatter_row":         (256, "rows", 3),             # ctx.hip:393, :396  stream_grid(n, 256)
    "gather_row":          (256, "rows", 3),             # ctx.hip:444, :446  stream_grid(n, 256)
    "scatter_vec4_w12":    ((256 // 3) * 2, "rows", 7),  # ctx.hip:399  stream_grid(n, (256 / (w / 4)) * 2)
    "gather_vec4_w12":     ((256 // 3) * 2, "rows", 7),  # ctx.hip:448
    "scatter_generic_w7":  ((256 // 7) * 4, "rows", 5),  # ctx.hip:405  stream_grid(n, (256 / w) * 4)
    "gather_generic_w7":   ((256 // 7) * 4, "rows", 5),  # ctx.hip:454
    "mark_rows":           (256 * 4, "entries", 3),      # ctx.hip:493  stream_grid(n, 256 * 4)
    "zero_unmarked_rows":  (256 * 4, "rows", 3),         # ctx.hip:510  stream_grid(n_full, 256 * 4)
    "noise_quant":         (256 * 4 // 16, "rows", 5),   # ctx.hip:717, :720, :739, :742  stream_grid(n * 16, 256 * 4): 16 lanes per row
    "ctx_gather_bwd4":     (16 * 2, "parents", 5),       # ctx.hip:1048  stream_grid(n_parents, 16 * 2)
    "ctx_gather_bwd":      (4 * 8, "parents", 5),        # ctx.hip:1053  stream_grid(n_parents, 4 * 8)
}
CAPS = {"rowcat_fwd_lds": 256 * 8}     # every other launcher: GRID_CAP
# the thresholds as read off the launchers by hand; test_ctx_rows_ref.py holds them against GRID_CAP * per_block
THRESHOLDS = {"rowcat_fwd": 4194304, "rowcat_bwd": 4194304, "gather_segmented": 4194304, "add_rows": 4194304, "rowcat_fwd_lds": 65536,
              "rowgather4": 2097152, "scatter_row": 1048576, "gather_row": 1048576, "scatter_vec4_w12": 696320, "gather_vec4_w12": 696320,
              "scatter_generic_w7": 589824, "gather_generic_w7": 589824, "mark_rows": 4194304, "zero_unmarked_rows": 4194304,
              "noise_quant": 262144, "ctx_gather_bwd4": 131072, "ctx_gather_bwd": 131072}


def second_trip(name):
    """The count (in the launcher's unit) just above the threshold: the cap's worth of workgroups and an odd remainder."""
    return THRESHOLDS[name] + SECOND_TRIP[name][2]


def rows_for(name, width):
    """The fewest rows of `width` elements (float4: of width / 4) that reach second_trip(name) elements."""
    per_row = width // 4 if SECOND_TRIP[name][1] == "float4" else width
    return -(-second_trip(name) // per_row)


# ---- index lists ------------------------------------------------------------------------------------------------------------------
def draw_idx(rng, n, rows, repeats=True):
    """n row indices into `rows` rows that hit row 0 and row rows - 1 (from n = 2 on); with repeats (from n = 4 on) or distinct."""
    if repeats:
        idx = rng.integers(0, rows, n).astype(np.int64)
        at = rng.permutation(n)
        if n >= 2:
            idx[at[0]], idx[at[1]] = 0, rows - 1
        elif n == 1:
            idx[0] = rows - 1
        if n >= 4:
            idx[at[2]] = idx[at[3]]
        return idx
    assert n <= rows
    if n < 2 or rows < 2:
        return np.full(n, rows - 1, np.int64)
    inner = rng.permutation(np.arange(1, rows - 1, dtype=np.int64))[:n - 2]
    return np.concatenate([[0, rows - 1], inner]).astype(np.int64)[rng.permutation(n)]


def draw_sorted(rng, N, kind):
    """Ascending distinct rows of N for cgs_scatter_rows_sorted, by the name of the list."""
    if kind == "dense":
        idx = np.nonzero(rng.random(N) < 0.9)[0]
    elif kind == "eighth":
        idx = np.nonzero(rng.random(N) < 0.125)[0]
    elif kind == "first":
        idx = np.array([0])
    elif kind == "last":
        idx = np.array([N - 1])
    elif kind == "all":
        idx = np.arange(N)
    elif kind == "gap":                # 100 000 rows in the middle that one thread zeroes
        assert N >= 100_100
        lo = (N - 100_000) // 2
        keep = rng.random(N) < 0.9
        keep[lo:lo + 100_000] = False
        keep[[0, lo - 1, lo + 100_000, N - 1]] = True
        idx = np.nonzero(keep)[0]
    elif kind == "none":
        idx = np.zeros(0, np.int64)
    else:
        raise ValueError(kind)
    if kind in ("dense", "eighth"):
        idx = np.union1d(idx, [0, N - 1])
    return idx.astype(np.int64)


OCCURRENCES = (0, 1, 2, 5, 300)


def draw_occurrences(rng, rows, fill=3):
    """An index list with repeats for rowcat's mode 2: rows with 0, 1, 2, 5 and 300 occurrences, row 0 and the last row among the
    listed ones; the other rows 0 .. fill times."""
    assert rows >= 7
    k = rng.integers(0, fill + 1, rows)
    k[:6] = (300, 0, 1, 2, 5, 0)
    k[rows - 1] = 2
    idx = np.repeat(np.arange(rows, dtype=np.int64), k)
    return idx[rng.permutation(len(idx))]


def draw_summable(rng, shape):
    """Integers in +-2^10 times 2^-8: a row's terms sum exactly in float32 in any order as long as their count stays below 2^13
    (every partial sum is an integer below 2^23 times 2^-8)."""
    return _f32(rng.integers(-1024, 1025, shape) * 2.0 ** -8)


def exactly_summable(terms, idx, rows):
    """Every partial sum of the terms of every row, in any order, is exact in float32: the terms are multiples of one power of two
    q and sum |terms| / q stays below 2^24."""
    t = _f64(terms)
    q = 2.0 ** -8
    asum = np.zeros((rows,) + t.shape[1:])
    np.add.at(asum, idx, np.abs(t))
    return bool((t / q == np.round(t / q)).all() and (asum / q < 2.0 ** 24).all())


# ---- the row movers -----------------------------------------------------------------------------------------------------------------
def _masked(x, mask):
    return x if mask is None else x * (np.asarray(mask) != 0).astype(np.float32)[:, None]     # a product: -x * 0 = -0


def rowcat(parts, n):
    """parts: (x [rows, w] float32, idx int64 [n] or None, mask uint8 [rows] or None) -> [n, sum w] float32."""
    cols = [(_masked(x, m)[:n] if idx is None else _masked(x, m)[idx]) for x, idx, m in parts]
    return _f32(np.concatenate(cols, axis=1))


def rowcat_bwd(dout, parts, n, sentinel):
    """parts: (rows, w, idx or None, mask or None, mode).  Per source: None (mode 0), the float32 array the store form leaves (mode
    1: dout * mask at the listed rows, the sentinel elsewhere), or (fp64 sum, sum |terms|, k [rows]) of the atomic form (mode 2)."""
    out, b = [], 0
    for rows, w, idx, mask, mode in parts:
        g = dout[:, b:b + w]
        b += w
        at = np.arange(n) if idx is None else idx
        if mode == 0:
            out.append(None)
            continue
        term = g if mask is None else g * (np.asarray(mask)[at] != 0).astype(np.float32)[:, None]
        if mode == 1:
            want = np.full((rows, w), sentinel, np.float32)
            want[at] = term
            out.append(want)
        else:
            s, a = np.zeros((rows, w)), np.zeros((rows, w))
            np.add.at(s, at, _f64(term))
            np.add.at(a, at, np.abs(_f64(term)))
            out.append((s, a, np.bincount(at, minlength=rows)))
    return out


def sum_bound(asum, k):
    """(k - 1) u sum |terms| for k fp32 additions onto zero in any order (the first is exact)."""
    return np.maximum(np.asarray(k) - 1, 0).reshape((-1,) + (1,) * (asum.ndim - 1)) * U * asum


def gather_rows(x, idx):
    return _f32(x[idx])


def scatter_sorted(g, idx, N):
    out = np.zeros((N, g.shape[1]), np.float32)
    out[idx] = g
    return out


def add_rows(out, idx, g):
    want = np.array(out, np.float32)
    want[idx] = want[idx] + g            # ONE float32 add per element
    return want


def mark(stamp, idx, gen):
    """The stamps after cgs_mark_rows: an index outside the array is ignored."""
    out = np.array(stamp, np.uint32)
    ok = (idx >= 0) & (idx < len(out))
    out[idx[ok]] = np.uint32(gen)
    return out


def zero_unmarked(stamp, gen, arrays):
    keep = np.asarray(stamp, np.uint32) == np.uint32(gen)
    out = []
    for a in arrays:
        a = np.array(a, np.float32)
        a[~keep] = 0.0
        out.append(a)
    return out


def gather_segmented(blocks, sizes, idx, w):
    """blocks: [size, w] float32 or None (zeros) -> cat(blocks)[idx] (idx None: every row in order)."""
    full = np.concatenate([np.zeros((s, w), np.float32) if b is None else _f32(b) for b, s in zip(blocks, sizes)])
    return full if idx is None else full[idx]


# ---- the CSR parent sums ----------------------------------------------------------------------------------------------------------
CHILD_COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 130)
PARENT_COUNTS = (1, 3, 4, 5, 15, 16, 17)


@functools.lru_cache(maxsize=None)
def draw_csr(n_par, seed=0, mean=5):
    """offs [n_par + 1], order (a permutation of the n_child rows of dout: every row, the last one too, is some parent's child),
    parent_row (distinct rows of an anchor array of n_anchor rows, rows 0 and n_anchor - 1 among them).  The child counts start
    with CHILD_COUNTS, rotated by n_par where fewer than nine parents leave no room for all of them; the rest is Poisson(mean)."""
    rng = np.random.default_rng([n_par, seed, 77])
    cnt = rng.poisson(mean, n_par).astype(np.int64)
    head = np.roll(np.array(CHILD_COUNTS), -2 * n_par)[:n_par]
    cnt[:len(head)] = head
    if cnt.sum() == 0:
        cnt[0] = 5
    if n_par > len(CHILD_COUNTS):
        cnt = cnt[rng.permutation(n_par)]
    offs = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    n_child = int(offs[-1])
    order = rng.permutation(n_child).astype(np.int64)
    n_anchor = 2 * n_par + 7
    parent_row = draw_idx(rng, n_par, n_anchor, repeats=False)
    c = types.SimpleNamespace(n_par=n_par, n_child=n_child, n_anchor=n_anchor, counts=cnt, offs=offs, order=order, parent_row=parent_row)
    for v in (cnt, offs, order, parent_row):
        v.setflags(write=False)
    return c


def csr_seq32(dout, offs, order):
    """sum over a parent's children IN ORDER, in float32, child after child from 0.f: [n_par, W]."""
    cnt = np.diff(offs)
    acc = np.zeros((len(cnt), dout.shape[1]), np.float32)
    for j in range(int(cnt.max(initial=0))):
        p = np.nonzero(cnt > j)[0]
        acc[p] = acc[p] + dout[order[offs[p] + j]]
    return acc


def csr_f64(dout, offs, order):
    """(sum, sum |terms|) in float64."""
    cnt = np.diff(offs)
    parent = np.repeat(np.arange(len(cnt)), cnt)
    s, a = np.zeros((len(cnt), dout.shape[1])), np.zeros((len(cnt), dout.shape[1]))
    rows = _f64(dout[order])
    np.add.at(s, parent, rows)
    np.add.at(a, parent, np.abs(rows))
    return s, a


def csr_store(prev, acc, bit):
    """What a column block holds afterwards: prev + sum in float32 with the accumulate bit, the sum without."""
    return (prev + acc) if bit else np.array(acc, np.float32)


# ---- noise_quant ------------------------------------------------------------------------------------------------------------------
def noise(seed, k, n, width):
    """The integer generator's u [n, width] of tensor k: element r width + c of the stream."""
    return ctx_noise(seed, k, n * width).reshape(n, width)


@functools.lru_cache(maxsize=None)
def draw_qadj(n, seed=0):
    """qadj [n, 3] float32 by ctx_level_ref's regimes (row r: r mod 16; the steered head of a row as in its row_regime): body rows
    2 randn, the others one head in ctx_level_ref.TARGET's interval of the regime next to two body heads."""
    rng = np.random.default_rng([n, seed, 41])
    q = 2.0 * rng.normal(size=(n, 3))
    regime, head = lr.row_regime(n)
    regime[regime == lr.DEAD] = lr.BODY                                  # (no MLP in front: a dead row is a body row here)
    for g, (lo, hi) in lr.TARGET.items():
        r = np.nonzero(regime == g)[0]
        q[r, head[r]] = rng.uniform(lo, hi, len(r))
    q = _f32(q)
    q.setflags(write=False)
    return q


def head_of(qadj):
    """ctx_level_ref.Head of an exact float32 qadj: U(qadj) = 0."""
    q = _f64(qadj)
    return lr.Head(q, np.zeros_like(q))


def literal_gate(qadj):
    """The clamp gate of the float32 literal (numpy): q0 (1 + tanh(qadj)) >= 1e-9f."""
    t = np.tanh(_f32(qadj))
    return np.array(Q0, np.float32) * (np.float32(1) + t) >= np.float32(1e-9)


@functools.lru_cache(maxsize=24)
def draw_nq(n, widths, seed=0, N=None):
    """The operands of cgs_noise_quant_fwd / _bwd at n rows of widths (D, S, O): sources of N = n + 11 rows with mean 0.3, a slice
    `rows` of a permutation, qadj by regime, dense cotangents (every eighth element 0), a side map that numbers about 15 % of the rows
    in shuffled order."""
    rng = np.random.default_rng([n, *widths, seed, 43])
    R = lambda *s: _f32(rng.normal(size=s))
    N = n + 11 if N is None else N
    x = [_f32(R(N, w) + np.float32(0.3)) for w in widths]
    rows = rng.permutation(N)[:n].astype(np.int64)
    dy = [R(n, w) for w in widths]
    dQe = R(n, 3)
    for a in dy + [dQe]:
        a.ravel()[np.arange(a.size) % 8 == 3] = 0.0
    m = max(1, int(round(0.15 * n)))
    side_map = np.full(n, -1, np.int32)
    side_map[rng.permutation(n)[:m]] = rng.permutation(m).astype(np.int32)
    side = [R(m, w) for w in widths]
    c = types.SimpleNamespace(n=n, N=N, m=m, widths=tuple(widths), x=x, rows=rows, qadj=draw_qadj(n, seed), dy=dy, dQe=dQe, side_map=side_map,
                              side=side, side_Q=R(m, 3))
    for v in x + dy + side + [rows, dQe, side_map, c.side_Q]:
        v.setflags(write=False)
    return c


def fraction(err, bound, what=""):
    """|err| / bound element by element; where the bound is 0 the error must be."""
    zero = bound == 0
    assert (err[zero] == 0).all(), (what, "an element whose bound is 0 differs", int((err[zero] != 0).sum()))
    return np.where(zero, 0.0, err / np.where(zero, 1.0, bound))


def y_fraction(x, u, Qk, y, what=""):
    """|y - (x + u Q)| / (u (|x + u Q| + |u Q|)) in float64 from the kernel's own Q [n] (float32, exact in float64): the bound of a
    rounded product and a rounded sum, or of one fused multiply-add."""
    p = _f64(u) * _f64(Qk)[:, None]
    want = _f64(x) + p
    return fraction(np.abs(_f64(y) - want), U * (np.abs(want) + np.abs(p)), what)


def q_units(qadj, Qk, what=""):
    """The kernel's Q in ctx_level_ref's units, ambiguous clamp rows at 0 -> (units [n, 3], ambiguous [n, 3])."""
    hd = head_of(qadj)
    amb = hd.ambiguous_clamp()
    err = mr.units_error(np.where(amb, hd.Q, Qk), hd.Q, hd.UQ, what)
    return err, amb


def dqadj_ref(qadj, dx, u, dQe=None, side_Q=None):
    """d qadj and its unit as ctx_level_ref.Backward states them: gQ = dQ_ext + side_Q + sum_c dx u, d qadj = gQ q0 (1 - t^2) behind
    an open gate, exactly 0 (unit 0) where tanh is +-1 in float32 (|qadj| >= 12) or the jumping head's clamp is active.
    dx: the three float32 [n, w] arrays dy (+ side) or None (zeros); side_Q: [n, 3] with zeros off the side map."""
    hd = head_of(qadj)
    n = len(qadj)
    gQ, aQ = np.zeros((n, 3)), np.zeros((n, 3))
    for extra in (dQe, side_Q):
        if extra is not None:
            gQ += _f64(extra)
            aQ += np.abs(_f64(extra))
    for k in range(3):
        if dx[k] is not None:
            p = _f64(dx[k]) * _f64(u[k])
            gQ[:, k] += p.sum(1)
            aQ[:, k] += np.abs(p).sum(1)
    UgQ = U * aQ + FLOOR
    q0 = np.array(Q0)
    dq = np.where(hd.open & ~hd.flat, gQ * q0 * hd.g, 0.0)
    Udq = np.where(hd.flat, 0.0, q0 * hd.g * UgQ + np.abs(gQ) * q0 * (2 * np.abs(hd.t) * hd.Ut + U * hd.g) + U * np.abs(dq) + FLOOR)
    return dq, Udq, hd


def dx_of(c, dy_given=(True, True, True), side=True):
    """dx_k [n, w] = dy_k (+ side_k[side_map]) in float32: ONE add; a missing dy is zeros."""
    chosen = np.nonzero(c.side_map >= 0)[0] if side else np.zeros(0, np.int64)
    out = []
    for k, w in enumerate(c.widths):
        d = np.array(c.dy[k]) if dy_given[k] else np.zeros((c.n, w), np.float32)
        d[chosen] = d[chosen] + c.side[k][c.side_map[chosen]]
        out.append(d)
    sQ = np.zeros((c.n, 3), np.float32)
    sQ[chosen] = c.side_Q[c.side_map[chosen]]
    return out, sQ


def nq_vec2(widths, aligned8=True):
    """nq_vec2_ok (ctx.hip:701-706): the float2 forward."""
    D, S, O = widths
    return aligned8 and not ((D | S | O) & 1) and D <= 64 and S <= 32 and O <= 32


def nq_bwd_fast(widths):
    """ctx.hip:738: noise_quant_bwd_kernel<true>."""
    D, S, O = widths
    return D <= 64 and S <= 16 and O <= 32


def means_terms(n, width, k, vec2):
    """t: the float32 terms one lane adds up over a forward call of n rows: trips of its row loop times its columns per row (the
    float2 kernel adds 4 per row for the features, two pairs, and 2 for the others, absent pairs as zeros)."""
    grid = stream_grid(n * 16, 256 * 4)
    trips = -(-n // (grid * 16))
    cols = (4 if k == 0 else 2) if vec2 else -(-width // 16)
    return trips * cols


def means_bound(levels, count):
    """levels: (t, sum |v|) per forward call -> the bound of the mean, sum_l t_l u sum |v_l| / count."""
    return sum(t * U * a for t, a in levels) / count if count else 0.0
