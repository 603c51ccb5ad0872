"""tests/ctx_rows_ref.py on the CPU: the drawers give what tests/test_ctx_rows_gpu.py relies on, the references agree with each other,
and the second-trip table agrees with a restatement of stream_grid."""
import numpy as np
import pytest

import ctx_level_ref as lr
import ctx_rows_ref as rr
from ctx_rows_ref import U

NQ_ROWS = (1, 15, 16, 17, 257, 4001)
NQ_SHAPES = ((50, 6, 30), (64, 16, 32), (66, 6, 30), (50, 18, 30), (50, 6, 34), (51, 7, 31))


# ---- the second-trip table ----------------------------------------------------------------------------------------------------------
def _grid(total, per_block, cap=256 * 16):
    blocks = (total + per_block - 1) // per_block
    return 1 if blocks < 1 else min(blocks, cap)


@pytest.mark.parametrize("name", sorted(rr.SECOND_TRIP))
def test_second_trip_table_agrees_with_stream_grid(name):
    per_block, _unit, rem = rr.SECOND_TRIP[name]
    cap = rr.CAPS.get(name, rr.GRID_CAP)
    thr = rr.THRESHOLDS[name]
    assert thr == cap * per_block
    assert _grid(thr, per_block, cap) == cap == -(-thr // per_block)             # the last count the grid still covers in one trip
    assert -(-(thr + 1) // per_block) > cap                                      # one more and a workgroup comes round again
    n = rr.second_trip(name)
    assert n == thr + rem and rem % 2 == 1 and rem < per_block and _grid(n, per_block, cap) == cap
    assert rr.stream_grid(n, per_block) == _grid(n, per_block) and rr.stream_grid(0, per_block) == 1


def test_second_trip_rows_reach_the_count():
    assert set(rr.SECOND_TRIP) == set(rr.THRESHOLDS)
    for name, w in (("rowcat_fwd", 12), ("rowcat_bwd", 12), ("add_rows", 3), ("gather_segmented", 12), ("rowgather4", 12)):
        per_row = w // 4 if name == "rowgather4" else w
        rows = rr.rows_for(name, w)
        assert rows * per_row >= rr.second_trip(name) > (rows - 1) * per_row


# ---- index lists ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rows", [(1, 5), (2, 2), (4, 3), (127, 40), (129, 1000), (1000, 1000)])
def test_index_lists_hit_both_ends(n, rows):
    rng = np.random.default_rng(n)
    idx = rr.draw_idx(rng, n, rows)
    assert idx.dtype == np.int64 and idx.min() >= 0 and idx.max() == rows - 1 and (n < 2 or idx.min() == 0)
    assert n < 4 or len(np.unique(idx)) < n                                      # repeats where they are legal
    if n <= rows:
        d = rr.draw_idx(rng, n, rows, repeats=False)
        assert len(np.unique(d)) == n and d.max() == rows - 1 and (n < 2 or d.min() == 0) and d.min() >= 0


@pytest.mark.parametrize("kind", ["dense", "eighth", "first", "last", "all", "gap", "none"])
def test_sorted_lists_are_ascending_and_distinct(kind):
    N = 100_777
    idx = rr.draw_sorted(np.random.default_rng(1), N, kind)
    assert idx.dtype == np.int64 and (np.diff(idx) > 0).all() and (len(idx) == 0 or (idx[0] >= 0 and idx[-1] < N))
    if kind in ("dense", "eighth", "all", "gap"):
        assert idx[0] == 0 and idx[-1] == N - 1
    if kind == "gap":
        assert np.diff(idx).max() == 100_001                                     # 100 000 unlisted rows between two listed ones
    assert {"first": [0], "last": [N - 1]}.get(kind, list(idx[:1])) == list(idx[:1])
    g = np.random.default_rng(2).normal(size=(len(idx), 3)).astype(np.float32)
    out = rr.scatter_sorted(g, idx, N)
    assert np.array_equal(rr.gather_rows(out, idx), g) and np.count_nonzero(out) <= g.size


def test_occurrence_lists_and_exactly_summable_terms():
    rng = np.random.default_rng(3)
    rows = 400
    idx = rr.draw_occurrences(rng, rows)
    k = np.bincount(idx, minlength=rows)
    assert set(rr.OCCURRENCES) <= set(k.tolist()) and k[0] > 0 and k[rows - 1] > 0 and k.max() == 300
    g = rr.draw_summable(rng, (len(idx), 5))
    assert rr.exactly_summable(g, idx, rows)
    # ... in ANY order: float32 accumulation forwards, backwards and shuffled gives the fp64 sum bit for bit
    (s, a, kk), = rr.rowcat_bwd(g, [(rows, 5, idx, None, 2)], len(idx), 0.0)
    assert np.array_equal(kk, k)
    for order in (np.arange(len(idx)), np.arange(len(idx))[::-1], rng.permutation(len(idx))):
        acc = np.zeros((rows, 5), np.float32)
        for i in order:
            acc[idx[i]] = acc[idx[i]] + g[i]
        assert np.array_equal(acc.astype(np.float64), s)
    assert (rr.sum_bound(a, kk)[kk <= 1] == 0).all()
    # normal draws are NOT: the property is the drawer's, not the check's
    assert not rr.exactly_summable(rng.normal(size=(len(idx), 5)).astype(np.float32), idx, rows)
    # one dropped or doubled row shows
    drop = np.delete(np.arange(len(idx)), 7)
    (s2, _, _), = rr.rowcat_bwd(g[drop], [(rows, 5, idx[drop], None, 2)], len(drop), 0.0)
    assert not np.array_equal(s2, s) or not g[7].any()


def test_rowcat_reference_masks_as_a_product():
    rng = np.random.default_rng(4)
    a = rng.normal(size=(9, 3)).astype(np.float32)
    b = rng.normal(size=(6, 2)).astype(np.float32)
    mask = np.array([1, 0, 1, 1, 0, 1, 1, 1, 0], np.uint8)
    idx = rr.draw_idx(rng, 6, 9)
    out = rr.rowcat([(a, idx, mask), (b, None, None)], 6)
    assert out.shape == (6, 5) and np.array_equal(out[:, 3:], b)
    off = mask[idx] == 0
    assert (out[off, :3] == 0).all() and np.array_equal(np.signbit(out[off, :3]), np.signbit(a[idx][off]))      # -x * 0 = -0
    assert np.array_equal(out[~off, :3], a[idx][~off])
    dout = rng.normal(size=(6, 5)).astype(np.float32)
    distinct = rr.draw_idx(rng, 6, 9, repeats=False)
    want, none = rr.rowcat_bwd(dout, [(9, 3, distinct, mask, 1), (6, 2, None, None, 0)], 6, -7.25)
    assert none is None
    listed = np.zeros(9, bool)
    listed[distinct] = True
    assert (want[~listed] == -7.25).all() and np.array_equal(want[distinct], dout[:, :3] * (mask[distinct] != 0)[:, None])


def test_small_movers():
    rng = np.random.default_rng(5)
    out = rng.normal(size=(20, 3)).astype(np.float32)
    idx = rr.draw_idx(rng, 7, 20, repeats=False)
    g = rng.normal(size=(7, 3)).astype(np.float32)
    want = rr.add_rows(out, idx, g)
    rest = np.ones(20, bool)
    rest[idx] = False
    assert np.array_equal(want[rest], out[rest]) and np.array_equal(want[idx], out[idx] + g) and want.dtype == np.float32
    stamp = rr.mark(np.zeros(20, np.uint32), np.array([0, 19, 5, -1, 20, 25]), 2 ** 32 - 1)
    assert stamp.sum() == 3 * (2 ** 32 - 1) and stamp[[0, 19, 5]].min() == 2 ** 32 - 1
    (z,) = rr.zero_unmarked(stamp, 2 ** 32 - 1, [out])
    assert np.array_equal(z[[0, 5, 19]], out[[0, 5, 19]]) and np.count_nonzero(z) == 9
    (z,) = rr.zero_unmarked(stamp, 1, [out])                                     # a stale stamp counts as unmarked
    assert not z.any()
    seg = rr.gather_segmented([out[:4], None, out[4:]], [4, 3, 16], np.array([0, 4, 6, 7, 22]), 3)
    assert np.array_equal(seg, np.stack([out[0], 0 * out[0], 0 * out[0], out[4], out[19]]))


# ---- the CSR sums -------------------------------------------------------------------------------------------------------------------
def test_csr_draws_hold_every_child_count():
    seen = set()
    for n_par in rr.PARENT_COUNTS + (40, 1000):
        c = rr.draw_csr(n_par)
        assert len(c.offs) == n_par + 1 and c.offs[0] == 0 and c.offs[-1] == c.n_child > 0 and (np.diff(c.offs) >= 0).all()
        assert np.array_equal(np.sort(c.order), np.arange(c.n_child))            # every row of dout, the last too, is a child
        assert len(np.unique(c.parent_row)) == n_par and c.parent_row.max() == c.n_anchor - 1 and (n_par < 2 or c.parent_row.min() == 0)
        seen |= set(c.counts.tolist())
        if n_par >= 15:
            assert set(rr.CHILD_COUNTS) <= set(c.counts.tolist())
    assert set(rr.CHILD_COUNTS) <= seen                                          # ... and the few-parent cases cover them together
    assert 4 < rr.draw_csr(1000).counts.mean() < 7


@pytest.mark.parametrize("n_par", [5, 17, 1000])
def test_sequential_fp32_sums_lie_within_the_fp64_bound(n_par):
    c = rr.draw_csr(n_par)
    dout = np.random.default_rng(n_par).normal(size=(c.n_child, 59)).astype(np.float32)
    seq = rr.csr_seq32(dout, c.offs, c.order)
    s, a = rr.csr_f64(dout, c.offs, c.order)
    assert seq.dtype == np.float32 and (seq[c.counts == 0] == 0).all() and not np.signbit(seq[c.counts == 0]).any()
    one = c.counts == 1
    assert np.array_equal(seq[one].astype(np.float64), s[one])
    frac = rr.fraction(np.abs(seq - s), rr.sum_bound(a, c.counts))
    assert frac.max() <= 1.0 and (n_par < 17 or frac.max() > 0.01)               # inside the bound, and the bound is not idle
    # a literal loop, parent by parent
    for p in range(min(n_par, 12)):
        acc = np.zeros(59, np.float32)
        for ch in c.order[c.offs[p]:c.offs[p + 1]]:
            acc = acc + dout[ch]
        assert np.array_equal(acc, seq[p])
    # the clamped duplicate of the last child added again is outside it wherever the count is no multiple of 4
    p = int(np.nonzero(c.counts % 4 != 0)[0][0])
    dup = seq[p] + dout[c.order[c.offs[p + 1] - 1]]
    assert (np.abs(dup - s[p]) > rr.sum_bound(a, c.counts)[p]).any()
    prev = np.full_like(seq, 1.5)
    assert np.array_equal(rr.csr_store(prev, seq, 1), prev + seq) and np.array_equal(rr.csr_store(prev, seq, 0), seq)


# ---- noise_quant ------------------------------------------------------------------------------------------------------------------
def test_noise_restatement_reproduces_ctx_level_ref():
    for k in range(3):
        assert np.array_equal(rr.noise(lr.SEED, k, 37, lr.WIDTHS[k]), lr.noise(k, 37))
    hi = rr.noise(lr.SEED + (5 << 32), 0, 37, 50)
    assert not np.array_equal(hi, rr.noise(lr.SEED, 0, 37, 50)) and not np.array_equal(hi, rr.noise(lr.SEED + (6 << 32), 0, 37, 50))
    assert np.abs(hi).max() <= 0.5 and hi.dtype == np.float32


@pytest.mark.parametrize("n", NQ_ROWS)
def test_qadj_draws_hold_every_regime_and_few_ambiguous_rows(n):
    q = rr.draw_qadj(n)
    assert q.dtype == np.float32 and q.shape == (n, 3)
    hd = rr.head_of(q)
    regime, head = lr.row_regime(n)
    for g, (lo, hi) in lr.TARGET.items():
        r = np.nonzero(regime == g)[0]
        v = q[r, head[r]]
        assert ((v > lo - 1e-3) & (v < hi + 1e-3)).all()
        assert n < 16 or len(r)
    amb = hd.ambiguous_clamp()
    assert amb.any(1).mean() < rr.AMBIGUOUS_CAP
    # the fp32 literal's own clamp gate differs from the fp64 one on no row outside the ambiguous ones, except where both sides of
    # it give the same values within a unit (the heads whose clamp is reached through t = -1 alone)
    differ = rr.literal_gate(q) != hd.open
    assert not (differ & hd.jumps[None, :] & ~amb).any()
    assert (differ & ~amb).mean() <= 0.1
    if n >= 257:
        assert hd.flat.any() and (~hd.open).any() and (hd.flat & ~hd.open & hd.jumps[None, :]).any()      # the clamp branch is entered


@pytest.mark.parametrize("widths", NQ_SHAPES)
def test_noise_quant_literal_is_inside_the_units(widths):
    """The float32 literal of Q, y and d qadj (numpy) within the limit the GPU test applies, so the limit is not the literal's problem."""
    n = 257
    c = rr.draw_nq(n, widths)
    one = np.float32(1)
    t = np.tanh(c.qadj)
    q0 = np.array(rr.Q0, np.float32)
    pre = q0 * (one + t)
    Q = np.maximum(pre, np.float32(1e-9))
    err, amb = rr.q_units(c.qadj, Q)
    assert err.max() <= rr.UNITS and amb.any(1).mean() < rr.AMBIGUOUS_CAP
    u = [rr.noise(rr.SEED, k, n, w) for k, w in enumerate(widths)]
    for k in range(3):
        y = c.x[k][c.rows] + u[k] * Q[:, k:k + 1]
        assert rr.y_fraction(c.x[k][c.rows], u[k], Q[:, k], y).max() <= 1.0
    dx, sQ = rr.dx_of(c)
    dq, Udq, hd = rr.dqadj_ref(c.qadj, dx, u, c.dQe, sQ)
    gQ = np.stack([(dx[k] * u[k]).sum(1, dtype=np.float32) for k in range(3)], 1) + c.dQe + sQ
    lit = np.where(pre >= np.float32(1e-9), gQ * q0 * (one - t * t), np.float32(0))
    keep = ~hd.ambiguous_clamp()
    e = rr.mr.units_error(np.where(keep, lit, dq), dq, Udq)
    assert e.max() <= rr.UNITS and (lit[hd.flat & keep] == 0).all()
    assert rr.nq_vec2(widths) == (widths in ((50, 6, 30), (64, 16, 32), (50, 18, 30))) and not rr.nq_vec2((50, 6, 30), aligned8=False)
    assert rr.nq_bwd_fast(widths) == (widths in ((50, 6, 30), (64, 16, 32), (51, 7, 31)))


def test_means_bound_counts_the_lane_terms():
    assert rr.means_terms(1, 50, 0, False) == 4 and rr.means_terms(1, 6, 1, False) == 1 and rr.means_terms(1, 30, 2, False) == 2
    assert rr.means_terms(1, 50, 0, True) == 4 and rr.means_terms(1, 6, 1, True) == 2 and rr.means_terms(1, 30, 2, True) == 2
    n = rr.second_trip("noise_quant")
    assert rr.means_terms(n - 5, 50, 0, False) == 4 * 4 and rr.means_terms(n, 50, 0, False) == 5 * 4      # 64 rows per workgroup and trip
    assert rr.means_bound([(4, 10.0), (8, 5.0)], 20) == (40 + 40) * U / 20 and rr.means_bound([(4, 10.0)], 0) == 0.0
    # per-lane float32 partials, then double, then one cast: inside the bound
    c = rr.draw_nq(4001, (50, 6, 30))
    for k, w in enumerate(c.widths):
        v = c.x[k][c.rows]
        lanes = np.zeros((16 * 4096, 16), np.float32)
        grid = rr.stream_grid(c.n * 16, 1024)
        for r in range(c.n):
            for c0 in range(0, w, 16):
                seg = v[r, c0:c0 + 16]
                lanes[r % (grid * 16), :len(seg)] += seg
        got = np.float32(lanes.astype(np.float64).sum() / v.size)
        bound = rr.means_bound([(rr.means_terms(c.n, w, k, False), np.abs(v.astype(np.float64)).sum())], v.size)
        assert abs(float(got) - v.astype(np.float64).mean()) <= bound
        assert abs(v.astype(np.float64).mean() - 0.3) < 0.05 and bound < 1e-5    # a lost workgroup is far outside
