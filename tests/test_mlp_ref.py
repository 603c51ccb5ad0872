"""tests/mlp_ref.py on the CPU: three fp32 evaluations of the fused MLPs' expressions against the fp64 statement in its units
(the measured table is in mlp_ref.py's docstring), that the inputs leave no ambiguous ReLU gate, and that every regime is what
it says."""
import numpy as np
import pytest

import mlp_ref as mr

LITERALS = (("a", mr.literal_torch), ("b", lambda c: mr.literal_numpy(c, "seq")), ("c", lambda c: mr.literal_numpy(c, "frag")))


def _anchor_cases():
    for n in (1, 17, 33, 2100):
        a = mr.draw_anchor(n, seed=n)
        dX = np.random.default_rng(n).normal(size=(n, 54)).astype(np.float32)
        yield a, dX


def test_the_fp32_literals_stay_within_the_unit_bound():
    """UNITS_LITERAL is the largest of the three literals over every case, rounded up to one decimal, and UNITS_KERNEL twice that,
    below the shortest contraction."""
    maxima = {k: mr.Maxima() for k, _ in LITERALS}
    for c, ref in mr.cpu_cases():
        for k, lit in LITERALS[:1] if c.n == mr.SPARSE_N else LITERALS:
            got = lit(c)
            mr.check_exact(ref, got, (k, c.cfg, c.n))
            for q in mr.QUANTITIES:
                maxima[k].add(q, mr.units_error(got[q], ref.values[q], ref.units[q], (k, c.cfg, c.n, q)))
    for a, dX in _anchor_cases():
        rows = mr.AnchorRows(a.feat_src, a.src_row, a.anchor, a.cam)
        want, unit = rows.pull_back(dX.astype(np.float64), np.zeros(dX.shape))
        for k, how in (("a", "torch"), ("b", "stated")):
            x, da = mr.literal_anchor(a, dX, how)
            ex = mr.units_error(x, rows.x, rows.x_unit, (k, "x_row"))
            assert (ex[:, 50:] <= mr.AnchorRows.X_ROUNDINGS).all(), (k, ex[:, 50:].max(0))
            maxima[k].add("x_row", ex)
            maxima[k].add("d_anchor", mr.units_error(da, want, unit, (k, "d_anchor")))
    for k, _ in LITERALS:
        maxima[k].report(f"literal ({k})")
    worst = max(max(v for q, v in m.m.items() if q != "x_row") for m in maxima.values())
    assert np.ceil(worst * 10) / 10 <= mr.UNITS_LITERAL, worst
    assert mr.UNITS_KERNEL == 2 * mr.UNITS_LITERAL and mr.UNITS_KERNEL < mr.GATE_UNITS == 15


def test_no_gate_is_ambiguous_and_every_regime_is_what_it_says():
    for c, ref in mr.cpu_cases():
        assert not mr.ambiguous_rows(c.x, c.W1, c.b1).any()
        z1 = ref.z1
        assert ((z1 == 0) | (np.abs(z1) > mr.UNITS_KERNEL * ref.Uz1)).all()
        dead = c.regime == mr.DEAD
        assert (c.x[dead] == 0).all() and (z1[dead] == c.b1.astype(np.float64)).all()
        if c.rows is not None:
            assert np.array_equal(c.row_ids[ref.live], np.array(c.rows)) and 550 <= len(c.rows) <= 700
    for cfg in mr.INSTANCES:
        c, ref = mr.draw(cfg, 2100), mr.ref_of(cfg, 2100)
        assert (c.b1 == 0).any() and (c.b1 < 0).any() and (c.b1 > 0).any()
        dead = c.regime == mr.DEAD
        assert dead.sum() > 100 and (ref.z1[dead] == 0).any() and (ref.z1[dead] < 0).any() and (ref.z1[dead] > 0).any()
        if cfg[3] != mr.ACT_NONE:
            sat, over = ref.z2[c.regime == mr.SAT], ref.z2[c.regime == mr.OVER]
            assert (sat > 30).any() and (sat < -30).any() and (over > 100).any() and (over < -100).any()
            y32 = ref.values["y"][c.regime == mr.SAT].astype(np.float32)
            assert (y32 == 1).any() and ((y32 == -1).any() if cfg[3] == mr.ACT_TANH else (y32 < 1e-13).any())
        else:
            assert (c.regime <= mr.DEAD).all()
    rows = mr.sparse_rows(256 * 256 + 17, 256)
    for r in list(range(16)) + list(range(65520, 65553)) + list(range(65519, 65553)) + [263, 264, 527, 528, 255, 256, 287, 288]:
        assert r in rows, r


def test_the_reference_backward_passes_a_difference_quotient():
    """The fp64 statement's gradients against central differences of sum(y dy), on ordinary rows (the gates are not smooth)."""
    for cfg in [(54, 50, 10, 1), (54, 50, 30, 2), (15, 100, 3, 0)]:
        c = mr.draw(cfg, 1, seed=5)
        assert c.regime[0] == mr.BODY
        ref = mr.Ref(c.x, c.W1, c.b1, c.W2, c.b2, c.act, c.dy)
        f = lambda **kw: float((mr.Ref(**{**dict(x=c.x, W1=c.W1, b1=c.b1, W2=c.W2, b2=c.b2, act=c.act, dy=c.dy), **kw}).values["y"] * c.dy).sum())
        for name, key in (("x", "dx"), ("W1", "dW1"), ("b1", "db1"), ("W2", "dW2"), ("b2", "db2")):
            base = np.asarray(getattr(c, name), np.float64)
            want = ref.values[key].reshape(base.shape)
            for i in np.random.default_rng(1).choice(base.size, min(base.size, 12), replace=False):
                vals = []
                for s in (1, -1):
                    a = base.copy()
                    a.ravel()[i] += s * 1e-6
                    vals.append(f(**{name: a}))
                assert abs((vals[0] - vals[1]) / 2e-6 - want.ravel()[i]) <= 1e-6 * max(1.0, np.abs(want).max()), (cfg, name, i)


@pytest.mark.parametrize("order", ["seq", "frag"])
def test_the_literals_would_see_a_dropped_row_and_a_dropped_column(order):
    """What the unit is for: one row left out of a 2100-row sum, or the last input column left out of a contraction, is many units."""
    cfg = (54, 50, 30, 2)
    c, ref = mr.draw(cfg, 2100), mr.ref_of(cfg, 2100)
    got = mr.literal_numpy(c, order)
    r = int(np.nonzero(c.regime == mr.BODY)[0][-1])
    short = got["db2"] - got["dz2"][r]
    assert mr.units_error(short, ref.values["db2"], ref.units["db2"]).max() > 10 * mr.UNITS_KERNEL
    x = np.array(c.x)
    x[:, -1] = 0
    cut = mr.literal_numpy(mr.types.SimpleNamespace(**{**c.__dict__, "x": x}), order)
    body = c.regime == mr.BODY
    assert (mr.units_error(cut["y"], ref.values["y"], ref.units["y"])[body].max(1) > mr.UNITS_KERNEL).mean() > 0.9
