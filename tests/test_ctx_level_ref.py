"""tests/ctx_level_ref.py on the CPU: the fp64 statement of a level against torch's float64 autograd of the same composition, three
fp32 evaluations of it in the statement's units (the measured table is in ctx_level_ref.py's docstring), that the inputs leave no
ambiguous ReLU or clamp gate at every row count the GPU file uses (256 CUs assumed for the CU-sized ones), that every regime is what
it says, and that the noise is ctx_noise at the indices used."""
import numpy as np
import pytest
import torch

import ctx_level_ref as lr
import mlp_ref as mr
from oracle.context_ref import _mix32, ctx_noise

LITERALS = (("a", lr.literal_torch), ("b", lambda c, f: lr.literal_numpy(c, f, "seq")), ("c", lambda c, f: lr.literal_numpy(c, f, "frag")))
ALL_COUNTS = lr.ROW_COUNTS + lr.large_counts(lr.CPU_CUS)


def test_the_statement_is_torch_float64_autograd_of_the_same_composition():
    """Values and every gradient, all operands given, on a case that holds every regime.  (Where the statement says exactly 0 -
    |qadj| >= 12 - float64 still has 1 - t^2 of some 1e-10: the absolute term.)"""
    for in_dim in (71, 15):
        c = lr.draw(129, in_dim)
        f = lr.Forward(c)
        b = lr.Backward(f)
        T = lambda a: torch.from_numpy(np.array(a, np.float64))
        I = lambda a: torch.from_numpy(np.array(a))
        G = lambda a: T(a).requires_grad_(True)
        anchor, hyp, W1, b1, W2q, b2q = (G(getattr(c, k)) for k in ("anchor", "hyp", "W1", "b1", "W2q", "b2q"))
        a = anchor[I(c.a_rows)]
        if in_dim == 15:
            X = torch.cat([a * T(c.a_mask[c.a_rows] != 0)[:, None], hyp], 1)
        else:
            X = torch.cat([a, T(c.base_f)[I(c.pos)], T(c.base_s)[I(c.pos)], hyp], 1)
        X.retain_grad()
        z1 = X @ W1.t() + b1
        qadj = torch.relu(z1) @ W2q.t() + b2q
        Q = (T(lr.Q0) * (1 + torch.tanh(qadj))).clamp(lr.CLAMP)
        for v in (z1, qadj, Q):
            v.retain_grad()
        ys = [T(getattr(c, "x" + nm))[I(c.rows)] + T(f.noise[k]) * Q[:, k:k + 1] for k, nm in enumerate(lr.NAMES)]
        sm = c.side_map
        chosen = np.nonzero(sm >= 0)[0]
        loss = (Q * T(c.dQe)).sum() + (Q[chosen] * T(c.side_Q[sm[chosen]])).sum() + (X[chosen] * T(c.dx_sub[sm[chosen]])).sum()
        for k, nm in enumerate(lr.NAMES):
            assert np.array_equal(b.dx[k][chosen], getattr(c, "dy" + nm)[chosen] + getattr(c, "side_" + nm)[sm[chosen]])
            loss = loss + (ys[k] * T(b.dx[k])).sum()
        loss.backward()
        assert np.array_equal(X.detach().numpy(), f.X.astype(np.float64))
        got = dict(qadj=qadj, Q=Q, yf=ys[0], ys=ys[1], yo=ys[2], gQ=Q.grad, dqadj=qadj.grad, dz1=z1.grad, dX=X.grad, dW1=W1.grad, db1=b1.grad,
                   dW2q=W2q.grad, db2q=b2q.grad)
        for k, v in got.items():
            want = (f if k in f.values else b).values[k]
            v = v.detach().numpy()
            assert np.abs(v - want).max() <= 1e-7 * np.abs(want).max() and np.allclose(v, want, rtol=1e-6, atol=1e-8 * np.abs(want).max()), (in_dim, k)
        assert np.array_equal(hyp.grad.numpy(), X.grad.numpy()[:, in_dim - 12:])


def test_the_fp32_literals_stay_within_the_unit_bound():
    """UNITS_LITERAL_LEVEL is the largest of the three literals over every case, rounded up to one decimal; the kernels' bound is twice
    the larger of it and mlp_ref.UNITS_LITERAL, below the shortest contraction."""
    maxima = {k: mr.Maxima() for k, _ in LITERALS}
    for c, f, b in lr.cpu_cases():
        for k, lit in LITERALS[:1] if (c.n > 20000 and not c.sparse) else LITERALS:      # (every row of the largest: the numpy loops are slow)
            got = lit(c, f)
            lr.check_exact(f, b, got, (k, c.in_dim, c.n))
            for q in lr.QUANTITIES:
                if q == "dX_own":
                    maxima[k].add(q, lr.own_cotangent(b, got["dX"]))
                    continue
                ref = f if q in f.values else b
                maxima[k].add(q, mr.units_error(got[q], ref.values[q], ref.units[q], (k, c.in_dim, c.n, c.sparse, q)))
    print("        " + "".join(f"{q:>7s}" for q in lr.QUANTITIES))
    for k, _ in LITERALS:
        print(f"  ({k})   " + "".join(f"{maxima[k].m[q]:7.3f}" for q in lr.QUANTITIES))
    worst = max(m.worst() for m in maxima.values())
    assert np.ceil(worst * 10) / 10 <= lr.UNITS_LITERAL_LEVEL, worst
    assert lr.UNITS_KERNEL_LEVEL == 2 * max(lr.UNITS_LITERAL_LEVEL, mr.UNITS_LITERAL) and lr.UNITS_KERNEL_LEVEL < lr.GATE_UNITS == 15


@pytest.mark.parametrize("in_dim", [71, 15])
def test_no_gate_is_ambiguous_and_every_regime_occurs(in_dim):
    f32 = np.float32
    for n in ALL_COUNTS:
        for sparse in ((False, True) if n > 1000 else (False,)):
            c = lr.draw(n, in_dim, sparse)
            lr.check_inputs(c)                                           # (asserts: no ReLU gate, no clamp gate, the steered intervals)
            for mask in ((True, False) if in_dim == 15 else (True,)):
                f = lr.Forward(c, mask)
                z1, Uz1 = f.trunk.z1, f.trunk.Uz1
                assert ((z1 == 0) | (np.abs(z1) > lr.UNITS_KERNEL_LEVEL * Uz1)).all()
                hd = f.head
                far = np.abs(hd.pre - lr.CLAMP) > lr.UNITS_KERNEL_LEVEL * hd.Upre
                assert far[:, hd.jumps].all() and list(hd.jumps) == [False, True, False]
            f = lr.Forward(c)
            dead = c.regime == lr.DEAD
            assert (f.X[dead] == 0).all() and (f.trunk.z1[dead] == c.b1.astype(np.float64)).all()
            assert (c.b1 == 0).any() and (c.b1 < 0).any() and (c.b1 > 0).any()
            # indices
            assert c.a_rows[0] == 0 and (n == 1 or (c.a_rows == c.N - 1).any()) and (c.pos == c.n_par - 1).any()
            assert len(np.unique(c.rows)) == n and c.rows.max() < c.N == n + 11
            chosen = c.side_map >= 0
            assert sorted(c.side_map[chosen]) == list(range(c.m)) and (n < 100 or 0.1 < c.m / (len(c.live) if sparse else n) < 0.2)
            if n >= 65:
                assert len(np.unique(c.a_rows)) < 0.8 * n and len(np.unique(c.pos)) < 0.8 * n
                assert (c.side_map[chosen][1:] < c.side_map[chosen][:-1]).any()
            if in_dim == 15:
                assert (c.a_mask[c.a_rows] == 0).any() or n < 15
            if sparse:
                live = np.zeros(n, bool)
                live[c.live] = True
                assert 550 <= len(c.live) <= 700 and all((getattr(c, k)[~live] == 0).all() for k in ("dyf", "dys", "dyo", "dQe"))
                assert not chosen[~live].any()
                b = lr.Backward(f)
                assert not b.trunk.live[~live].any() and (b.values["dX"][~live] == 0).all()
                for edge in (0, n - 1, 64 * lr.CPU_CUS - 1, 64 * lr.CPU_CUS, 256 * lr.CPU_CUS - 1, 256 * lr.CPU_CUS):
                    assert edge >= n or live[edge]
            if n < 15:
                continue
            # the regimes: fp32's tanh (correctly rounded) against the fp64 gate, per head
            hd = f.head
            t32 = hd.t.astype(f32)
            cancelled = (t32 == -1) & (hd.pre > lr.CLAMP)
            both = (t32 == -1) & ~hd.open
            steps = (f32(1) + t32).astype(np.float64) * 2.0 ** 24
            few = (c.regime == lr.CANCEL)[:, None] & (steps >= 1) & (steps <= 200) & (np.arange(3) == c.head[:, None])
            high = (t32 == 1) & (hd.g < 1e-9)
            print(f"[regimes] in_dim {in_dim} n {n} sparse {sparse}: t32 == -1, fp64 above the clamp {cancelled.sum(0)}, clamped in both "
                  f"{both.sum(0)}, cancelling {few.sum(0)}, t32 == 1 {high.sum(0)}")
            heads = sorted(set(c.head[c.regime == lr.CANCELLED]))
            assert cancelled[:, 1].sum() == 0 and all(cancelled[:, k].sum() > 0 for k in heads if k != 1)
            for g, counts in ((lr.SAT_LOW, both.sum(0)), (lr.CANCEL, few.sum(0)), (lr.SAT_HIGH, high.sum(0))):
                assert all(counts[k] > 0 for k in set(c.head[c.regime == g])), (lr.REGIMES[g], counts)
            if n >= 129:
                assert all(set(c.head[c.regime == g]) == {0, 1, 2} for g in (lr.SAT_LOW, lr.CANCEL, lr.CANCELLED, lr.SAT_HIGH))
                # q0 = 0.001 inside (-9, -6): fp32 and fp64 agree on the clamp, on both sides of it
                r = np.nonzero((c.regime == lr.CANCEL) & (c.head == 1))[0]
                pre32 = f32(lr.Q0[1]) * (f32(1) + t32[r, 1])
                assert ((pre32 >= f32(1e-9)) == hd.open[r, 1]).all() and (n < 1000 or (hd.open[r, 1].any() and (~hd.open[r, 1]).any()))
                # q0 = 1 below -9.05: they disagree
                r = np.nonzero((c.regime == lr.CANCELLED) & (c.head == 0))[0]
                assert ((f32(1) + t32[r, 0] < f32(1e-9)) & hd.open[r, 0]).any()


def test_the_noise_is_ctx_noise_at_the_indices_used():
    """Element r * width + column of tensor k, the 64-bit statement; the kernels' 32-bit index form gives the same values there."""
    n = lr.large_counts(lr.CPU_CUS)[1]
    for k, w in enumerate(lr.WIDTHS):
        flat = ctx_noise(lr.SEED, k, n * w)
        assert flat.dtype == np.float32 and flat.min() >= -0.5 and flat.max() < 0.5
        got = lr.noise(k, n)
        for r, col in ((0, 0), (0, w - 1), (1, 0), (n - 1, w - 1), (4097, w // 2)):
            assert got[r, col] == flat[r * w + col]
        assert np.array_equal(lr.noise(k, 17), got[:17])
        with np.errstate(over="ignore"):
            key = _mix32(np.array([(lr.SEED & 0xFFFFFFFF) ^ ((0x9E3779B9 * (k + 1)) & 0xFFFFFFFF)], np.uint32))[0] ^ np.uint32(lr.SEED >> 32)
            h = _mix32(np.arange(n * w, dtype=np.uint32) + key)
        k32 = (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0) - np.float32(0.5)
        assert np.array_equal(k32, flat)


def test_the_units_would_see_a_dropped_row_and_a_prefetch_one_tile_off():
    """What the second-trip cases are for: one live row left out of the sparse case's weight-gradient sums, or the rows of the last
    tile taking the operands of the tile before, is far more than the kernels' bound."""
    n = lr.large_counts(lr.CPU_CUS)[1]
    c = lr.draw(n, 71, True)
    f = lr.Forward(c)
    b = lr.Backward(f)
    r = int(c.live[np.abs(b.values["dqadj"][c.live]).sum(1) > 0][-1])
    short = b.values["dW1"] - np.outer(b.values["dz1"][r], f.X[r].astype(np.float64))
    assert mr.units_error(short, b.values["dW1"], b.units["dW1"]).max() > 10 * lr.UNITS_KERNEL_LEVEL
    off = f.values["Q"].copy()
    off[n - 1] = off[n - 17]
    body = c.regime[n - 1] == lr.BODY and c.regime[n - 17] == lr.BODY
    assert body and mr.units_error(off, f.values["Q"], f.units["Q"])[n - 1].max() > 10 * lr.UNITS_KERNEL_LEVEL


def test_the_own_cotangent_judge_sees_truncated_weights():
    """What dX_own is for: the dX product's weights with their low six mantissa bits cleared (64 u relative at the most) stay within
    dX's unit, most of which d qadj carries, but not within the product's own."""
    for in_dim in (71, 15):
        c = lr.draw(129, in_dim)
        f = lr.Forward(c)
        b = lr.Backward(f)
        got = lr.literal_numpy(c, f, "frag")
        cut = (np.array(c.W1).view(np.uint32) & ~np.uint32(63)).view(np.float32)
        dX = mr._contract_frag(got["dz1"], cut) + lr._dx32(c)[2]
        assert mr.units_error(dX, b.values["dX"], b.units["dX"]).max() < lr.UNITS_KERNEL_LEVEL < lr.own_cotangent(b, dX).max()
        assert lr.own_cotangent(b, got["dX"]).max() < lr.UNITS_LITERAL_LEVEL
