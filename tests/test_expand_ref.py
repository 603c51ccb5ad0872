"""tests/expand_ref.py on the CPU: the fp32 literal of gaussian_renderer/__init__.py:112-145 against the fp64 statement in the
closed-form units, that the units are positive wherever a value is not zero, and that every regime is what it says.  The
measured table is in the docstring of tests/test_expand_gpu.py."""
import numpy as np
import pytest

import expand_ref as er

# (n, K, seed): K = 32 makes the longest per-anchor sums; the single-regime draws put every value of a regime into one call
MIXED = [(257, 10, 0), (65, 32, 1), (33, 7, 2), (1, 1, 3), (300, 10, 4)]
SRC = ("none", "subset", "perm")


def _cases():
    for i, (n, K, seed) in enumerate(MIXED):
        yield er.draw(n, K, seed, SRC[i % 3])
    for regime in er.REGIMES:
        yield er.draw(120, 10, 5, "subset", only=regime)
        yield er.draw(40, 32, 6, "none", only=regime)
    for gate in ("all", "none", "first", "last"):
        yield er.draw(33, 7, 7, "perm", gate)


def _measure(c, maxima):
    ref = er.Ref(c)
    weights = [er.draw_weights(ref.P, c.n * c.K, 11 + i, names) for i, names in enumerate(er.LOSSES)]
    values, grads = er.literal_fp32(c, weights)
    er.check_exact(ref, values)
    for k, u in ref.value_units.items():
        er.assert_units_positive(ref.values[k], u, k)
        maxima.add(ref, k, er.units_error(values[k], ref.values[k], u, k))
    for w, g in zip(weights, grads):
        want, units = ref.grads(w)
        er.check_exact(ref, grads=g, weights=w)
        for k in er.GRADS:
            if k != "d_color_in":                 # (a bit copy: its unit is 0 and the comparison an equality)
                er.assert_units_positive(want[k], units[k], k)
            maxima.add(ref, k, er.units_error(g[k], want[k], units[k], (k, tuple(w))))


def test_the_fp32_literal_stays_within_the_unit_bound():
    """The record that the reference's fp32 expression alone meets the condition the kernels are held to (at half the bound);
    the units' positivity is asserted on the way."""
    maxima = er.Maxima()
    for c in _cases():
        _measure(c, maxima)
    maxima.report("expand-units", "fp32 literal (CPU)")
    assert np.ceil(maxima.worst() * 10) / 10 == er.UNITS_LITERAL, maxima.worst()
    assert er.UNITS_KERNEL == 2 * er.UNITS_LITERAL


def test_every_regime_is_what_it_says():
    """(The conditions of expand_ref.assert_conditions are asserted by every draw.)"""
    for c in _cases():
        er.assert_conditions(c)
    for K in (10, 32):
        c = er.draw(120 if K == 10 else 40, K, 5 if K == 10 else 6, "subset" if K == 10 else "none", only="gate")
        no = (c.op_raw.astype(np.float64) * c.masks).astype(np.float32).ravel()
        for v in (np.float32(er.TINY), -np.float32(er.TINY), np.float32(1)):
            assert (no == v).any(), v
        assert ((no == 0) & ~np.signbit(no)).any() and ((no == 0) & np.signbit(no)).any() and (no < 0).any()
        assert ((c.masks > 0) & (c.masks < 1) & (c.op_raw > 0)).any()
        c = er.draw(120 if K == 10 else 40, K, 5 if K == 10 else 6, "subset" if K == 10 else "none", only="sigmoid")
        s = c.cov_in.reshape(-1, 7)[:, :3]
        for v in er.SIGMOID_S:
            assert (s == v).any() and (s == -v).any(), v
        c = er.draw(120 if K == 10 else 40, K, 5 if K == 10 else 6, "subset" if K == 10 else "none", only="quaternion")
        q = c.cov_in.reshape(-1, 7)[:, 3:].astype(np.float64)
        nrm = np.sqrt((q * q).sum(1))
        assert (nrm == 0).any() and ((nrm == 1) & ((q != 0).sum(1) == 1) & (q.min(1) == -1)).any() and ((nrm == 1) & (q.max(1) == 1)).any()
        for v in er.QUAT_NORMS:
            assert (np.abs(nrm / v - 1) < 1e-6).any(), v
        c = er.draw(120 if K == 10 else 40, K, 5 if K == 10 else 6, "subset" if K == 10 else "none", only="geometry")
        ref = er.Ref(c)
        a = np.abs(ref.anchor)
        assert a.max() > 5e3 and (np.abs(ref.values["xyz"]) <= 1.1e-2 * a[ref.sel]).all()
    for gate, want in (("all", 231), ("none", 0), ("first", 1), ("last", 1)):
        c = er.draw(33, 7, 7, "perm", gate)
        alive = (c.op_raw.astype(np.float64) * c.masks > 0).ravel()
        assert alive.sum() == want and (gate != "first" or alive[0]) and (gate != "last" or alive[-1])


@pytest.mark.parametrize("src", SRC)
def test_reference_gradients_pass_gradcheck(src):
    """The fp64 statement's own autograd against finite differences (ordinary values: the regimes' edges are not smooth)."""
    import torch
    c = er.draw(5, 3, 8, src, "all", only="body")
    ref = er.Ref(c)
    w = er.draw_weights(ref.P, 15, 3)
    want, _ = ref.grads(w)
    e, h = ref.e, 1e-6
    base = {k: np.asarray(getattr(c, k), np.float64) for k in ("anchor", "gscaling", "offsets", "cov_in")}
    for k, name in (("anchor", "d_anchor"), ("gscaling", "d_gscaling"), ("offsets", "d_offsets"), ("cov_in", "d_cov_in")):
        fd = np.zeros(base[k].size)
        for i in range(base[k].size):
            vals = []
            for sgn in (1, -1):
                a = base[k].copy()
                a.ravel()[i] += sgn * h * max(1.0, abs(a.ravel()[i]))
                c2 = er.Case(**{**c.__dict__, k: a})
                out = er._evaluate(c2, torch.float64).out
                vals.append(sum(float((out[o].detach().numpy() * w[o]).sum()) for o in w))
            fd[i] = (vals[0] - vals[1]) / (2 * h * max(1.0, abs(base[k].ravel()[i])))
        scale = np.abs(want[name]).max()
        assert np.abs(fd.reshape(want[name].shape) - want[name]).max() <= 1e-5 * scale, (name, src)
    assert e.mask.all()
