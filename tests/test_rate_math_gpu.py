"""csrc/rate_math.h per element against float64, through the three kernel families that include it:
  a. cgs_entropy_gaussian_fwd / _bwd (elementwise.hip), through the C ABI and through entropy_models.Entropy_gaussian
  b. cgs_level_rate_fwd / _bwd (ctx.hip), direct calls at generic D, K, strides and every optional operand
  c. cgs_rate_sub_fwd / _bwd (rate_sub.hip), with W2 = 0 so that b2 carries a known (mean, scale) per column
The reference, the error unit u, the classes of an element and the inputs (exact on a grid, by regime) are tests/rate_ref.py.

UNITS_LITERAL = 1.9: what the reference's own fp32 expression (torch CPU, Normal.cdf) needs on these inputs, measured by
test_the_fp32_literal_stays_within_the_unit_bound and rounded up to one decimal.  UNITS_KERNEL = 2 UNITS_LITERAL = 3.8 for all
three kernel families: the kernels replace three IEEE divisions and libm's erf / exp / log by 1-ulp hardware forms, each about one
more rounding of the size the literal already makes.  It is not taken from the kernels' results.

Measured maxima in units, on an MI355X (bits less the log2 floor; "-": the output is only seen inside a sum, see below):
                                      bits    g_x     g_mean  g_scale  g_q
  fp32 literal (CPU)     body         1.358   0.650   0.650   0.595    1.642
                         switch       1.419   0.200   0.200   0.192    1.543
                         tail         1.490   1.420   1.420   1.417    1.532
                         clamp        1.895   0.024   0.024   0.480    1.754
  entropy_gaussian       body         1.396   0.690   0.690   0.657    1.642
  (50 000 per regime)    switch       1.803   0.235   0.235   0.205    2.018
                         tail         1.490   1.420   1.420   1.416    1.532
                         clamp        1.734   0.025   0.025   0.480    1.842
     sizes, Q layouts, module         1.629   1.389   1.389   1.385    1.832
  level_rate             body         -       0.548   0.548   0.517    -
  (12 calls, a regime    switch       -       0.236   0.236   0.184    -
  per element)           tail         -       1.285   1.285   1.284    -
                         clamp        -       0.057   0.057   0.555    -
  rate_sub               body         -       0.558   -       -        -
  (12 calls, a regime    switch       -       0.187   -       -        -
  per element)           tail         -       1.218   -       -        -
                         m = 1 (db2)  -       -       0.396   0.347    -
The tiny-scale regime has no units: every element is dead (likelihood exactly 0 or 1) and is checked exactly.  The three forward
sums stayed below 0.32 of their tolerance in level_rate and below 0.06 in rate_sub; dQ / side_Q, d_masks, db2 and dW2 are asserted
within theirs (the sum of their elements' tolerances plus 2e-5 of the sum of magnitudes).
The log2 floor LOG_FLOOR max(1, |bits|) = 4 * 2^-22 max(1, |bits|): where bits < 1e-3 (likelihood next to 1) the kernel's bits
were within 0.49 * 2^-22 of fp64 (v_log_f32 on the MI355X; 119 such elements of the body regime).
Undecided share (|lik - 1e-6| <= 3e-7, fp64): body 0, switch 0, clamp 0, tail 3.5 % (3.3 % with one Q per row or a scalar Q);
38 % of the tail regime is below the bound.  The inputs of level_rate and rate_sub hold no undecided element (rate_ref.settle).

That the tests bite (each alteration built once, this file run once on it):
  the erf coefficient 0.6349333 -> 0.6349433: 31 of the 47 GPU tests fail (bits and g_q of the body and switch regimes, dQ /
      side_Q and d_masks of level_rate and rate_sub);
  rate_grads with t.zu in both terms of g.gs: 45 fail (g_scale everywhere);
  rate_elem's scol of kind 1 off by one column: the 12 level_rate tests fail (the forward sums first), nothing else.
"""
import numpy as np
import pytest
import torch

import rate_ref as rr

UNITS_LITERAL = 1.9
UNITS_KERNEL = 2 * UNITS_LITERAL
N_REGIME = 50000
gpu = pytest.mark.gpu


def _maxima(errs):
    return {k: (round(float(np.nanmax(v)), 3) if np.isfinite(v).any() else None) for k, v in errs.items()}


def _assert_units(errs, units, what, regime=None):
    m = _maxima(errs)
    print(f"[rate-units] {what}: {m}")
    if regime is not None:          # (per regime of a mixed call; tiny-scale elements are all dead: no units)
        for i, name in enumerate(rr.REGIMES + ("centre",)):
            if (regime == i).any() and name != "tiny":
                part = _maxima({k: np.where(regime == i, v, np.nan) for k, v in errs.items()})
                print(f"[rate-units]   {what.split()[0]} regime {name}: {part}")
    for k, v in m.items():
        assert v is None or v <= units, (what, k, v, units)


# ---- CPU: the reference itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["body", "switch", "tail", "clamp"])
def test_stable_and_plain_forms_agree(regime):
    inp, _, ref = rr.case(regime, N_REGIME)
    lik, bits = rr.eg_plain_fp64(*inp)
    well = ref.lik > 1e-3
    assert well.sum() > 1000
    assert (np.abs(lik - ref.lik)[well] <= 1e-12 * ref.lik[well]).all()
    assert (np.abs(bits - ref.bits)[well] <= 1e-12 * np.maximum(1.0, ref.bits[well])).all()


def test_reference_gradients_pass_gradcheck():
    x, mean, s, q, xm, _ = rr.draw("body", 48)
    leaves = [torch.from_numpy(np.array(a, dtype=np.float64)).requires_grad_(True) for a in (x, mean, s, q)]
    assert torch.autograd.gradcheck(lambda *a: rr.bits64(*a, xm, True), leaves, eps=1e-7, atol=1e-6, rtol=1e-5)


def _rounding_term(ref, x, mean, q, s, x_mean, name):
    """Inputs off the grid: x +- q/2 - mean carries a rounding of 6e-8 (|x| + |q|/2 + |mean|), i.e. dz = that k in z, times
    |d output / dz|: g_z for the bits; for a gradient M, |dM/dz| <= M (2 max|z| + (e^-zu^2 + e^-zl^2) / (sqrt pi lik)) (the
    exponential and the 1 / lik), and the scale gradient's factor z adds M_x sqrt 2."""
    xc = np.clip(np.abs(x), None, np.abs(x_mean) + 15000 * np.abs(q))
    dz = 6e-8 * (xc + np.abs(q) / 2 + np.abs(mean)) / (ref.s * rr.SQRT2)
    if name == "bits":
        return dz * ref.Mx / (1.0 / (ref.s * rr.SQRT2))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        h = (np.exp(-ref.zu ** 2) + np.exp(-ref.zl ** 2)) / (np.sqrt(np.pi) * np.maximum(ref.lik, 1e-300))
    big = 2 * np.maximum(np.abs(ref.zu), np.abs(ref.zl)) + h
    M = dict(gx=ref.Mx, gm=ref.Mx, gq=ref.Mq, gs=ref.Ms)[name]
    return dz * (M * big + (ref.Mx * rr.SQRT2 if name == "gs" else 0.0))


@pytest.mark.parametrize("which", ["eg", "egc"])
def test_reference_goldens_are_reproduced(which):
    """The reference's own fp32 outputs (tests/golden) lie within the literal's units of eg_fp64, plus the rounding of their
    off-grid arguments."""
    import os

    import golden_inputs as gi
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if which == "eg":
        g = np.load(os.path.join(gold, "elementwise.npz"))
        x, mean, s, Q = gi.elementwise_inputs(257, 1)
        xm = 0.25
    else:
        g = np.load(os.path.join(gold, "entropy_api.npz"))
        x, mean, s, Q = gi.elementwise_inputs(193, 6)
        xm = float(torch.from_numpy(x).mean())
    gw = g[which + "_gw"]
    ref, plain = rr.eg_fp64(x, mean, s, Q, xm, True, g_bits=gw), rr.eg_fp64(x, mean, s, Q, xm, True)
    assert ref.unit.sum() > 0.5 * ref.unit.size and ref.dead.any() and ref.bounded.any()
    got = dict(bits=g[which + "_bits"], gx=g[which + "_gx"], gm=g[which + "_gmean"], gs=g[which + "_gscale"])
    for name, a in got.items():
        a = a.astype(np.float64)
        assert (np.abs(a[ref.bounded | (ref.dead & (ref.lik == 0))] - (rr.BITS_BOUND if name == "bits" else 0.0)) <= 1e-5).all(), name
        tol = UNITS_LITERAL * ref.tol1[name] + _rounding_term(ref, x, mean, Q, s, xm, name)
        if name == "bits":                                   # (its rounding term carries no |g_bits|)
            tol = UNITS_LITERAL * ref.tol1["bits"] + ref.floor + _rounding_term(plain, x, mean, Q, s, xm, "bits")
        err = np.abs(a - getattr(ref, name))
        assert (err <= tol)[ref.unit].all(), (name, np.nanmax(np.where(ref.unit, err / tol, np.nan)))
    # g_Q: one per row, a sum of the row's elements; an undecided element may contribute its gradient or nothing
    tol = np.where(ref.unit, UNITS_LITERAL * ref.tol1["gq"] + _rounding_term(ref, x, mean, Q, s, xm, "gq"), 0.0)
    tol = tol + np.where(ref.undecided, np.abs(ref.free["gq"]), 0.0) + rr.SUM_RTOL * np.abs(ref.gq)
    assert (np.abs(g[which + "_gQ"][:, 0] - ref.gq.sum(1)) <= tol.sum(1)).all()


def test_the_fp32_literal_stays_within_the_unit_bound():
    """The record that the reference's fp32 expression alone meets the condition the kernels are held to (at half the bound)."""
    worst = 0.0
    for regime in rr.REGIMES:
        inp, g, ref = rr.case(regime, N_REGIME)
        lit = rr.eg_literal_fp32(*inp, g_bits=g)
        errs = ref.errors(UNITS_LITERAL, **{k: lit[k] for k in rr.NAMES})
        _assert_units(errs, UNITS_LITERAL, f"literal {regime}")
        if ref.unit.any():
            worst = max(worst, max(v for v in _maxima(errs).values() if v is not None))
            assert np.abs(lit["lik"] - ref.lik).max() <= 1.3e-7
    assert np.ceil(worst * 10) / 10 == UNITS_LITERAL, worst


def test_the_undecided_band_is_small_and_every_regime_is_what_it_says():
    for regime in ("body", "switch", "tail", "clamp"):
        for layout in ("elem", "row", "scalar"):
            ref = rr.case(regime, N_REGIME, q_layout=layout)[2]
            und = ref.undecided.mean()
            assert und <= (0.05 if regime == "tail" else 0.0), (regime, layout, und)
            if layout == "scalar":
                continue
            # zu > zl always (q > 0): (+, +), (+, -), (-, -) are the combinations there are; the fourth is an edge exactly on
            # the mean (zu or zl = 0), which the body regime holds by construction
            combos = [((ref.zu > 0) & (ref.zl > 0)).sum(), ((ref.zu > 0) & (ref.zl < 0)).sum(), ((ref.zu < 0) & (ref.zl < 0)).sum()]
            assert min(combos) > 0, (regime, layout, combos)
            assert regime != "body" or min((ref.zu == 0).sum(), (ref.zl == 0).sum()) > 100
    tail = rr.case("tail", N_REGIME)[2]
    assert 0.3 <= tail.bounded.mean() <= 0.5
    sw = rr.case("switch", N_REGIME)[2]
    edge = np.minimum(np.abs(np.abs(np.abs(sw.zu) - 1) - 1e-3), np.abs(np.abs(np.abs(sw.zl) - 1) - 1e-3))
    assert (edge <= 2e-6).all(), edge.max()
    for a in (sw.zu, sw.zl):
        assert ((np.abs(a) > 1) & (np.abs(a) < 1.0011)).any() and ((np.abs(a) < 1) & (np.abs(a) > 0.9989)).any()
    tiny = rr.case("tiny", 1200)[2]
    assert tiny.dead.all() and (tiny.lik == 0).any() and (tiny.lik == 1).any()
    inp, _, cl = rr.case("clamp", N_REGIME)
    assert cl.unit.all()
    where = _clamp_where(inp)
    assert min((where == k).sum() for k in range(3)) > 1000


def _clamp_where(inp):
    """0 inside the clamp range, 1 exactly on an edge, 2 beyond."""
    x, _, _, q, xm, _ = inp
    off = np.abs(x.astype(np.float64) - xm) - 15000 * q.astype(np.float64)
    return np.where(off < 0, 0, np.where(off == 0, 1, 2))


# ---- GPU helpers ----------------------------------------------------------------------------------------------------------------
PAD = 64


def T(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _elementwise(inp, g, q_div=1):
    """cgs_entropy_gaussian_fwd / _bwd on the inputs `inp` -> {bits, gx, gm, gs, gq} float32 arrays; the outputs are NaN
    before the call and carry PAD more entries than n, which must stay NaN."""
    from contextgs_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    x, mean, s, q, xm, clamp = inp
    n = x.size
    Q = T(q if q_div == 1 else q[::q_div])
    assert Q.numel() == -(-n // q_div)
    xd, md, sd, gd, xmd = T(x), T(mean), T(s), T(g), T(np.array([xm]))
    out = _nan(5, n + PAD)
    st = _lib.current_stream()
    _lib.check(L.cgs_entropy_gaussian_fwd(p(xd), p(md), p(sd), p(Q), n, q_div, p(xmd), int(clamp), p(out[0]), st), "fwd")
    _lib.check(L.cgs_entropy_gaussian_bwd(p(xd), p(md), p(sd), p(Q), n, q_div, p(xmd), int(clamp), p(gd), p(out[1]), p(out[2]),
                                          p(out[3]), p(out[4]), st), "bwd")
    o = out.cpu().numpy()
    assert np.isnan(o[:, n:]).all() and not np.isnan(o[:, :n]).any()
    return dict(zip(rr.NAMES, o[:, :n]))


def _check_classes(inp, ref, got, regime):
    """The statements of the tiny-scale and clamp regimes that are exact."""
    s, clamp = inp[2], inp[5]
    if regime == "tiny":
        assert all(np.isfinite(v).all() for v in got.values())
        assert (np.minimum(np.abs(got["bits"]), np.abs(got["bits"] - rr.BITS_BOUND)) <= 1e-5).all()      # 0 or the bound's bits
        assert (got["bits"][ref.lik == 1] == 0).all()
        assert (got["gs"][s < np.float32(1e-9)] == 0).all()
    if clamp:
        where = _clamp_where(inp)
        assert (got["gx"][where == 2] == 0).all()
        edge = (where == 1) & (np.abs(ref.gx) > UNITS_KERNEL * ref.tol1["gx"]) & ref.unit
        assert (got["gx"][edge] != 0).all()
        if regime == "clamp":
            assert edge.sum() > 100 and (where == 2).sum() > 100 and (ref.gm[where == 2] != 0).any()


# ---- a. the element-wise kernels ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("regime,use_clamp", [("body", 0), ("body", 1), ("switch", 0), ("switch", 1), ("tail", 0), ("tail", 1),
                                               ("tiny", 0), ("tiny", 1), ("clamp", 1)])
def test_entropy_gaussian_kernels_per_element(regime, use_clamp):
    n = 1200 if regime == "tiny" else N_REGIME
    inp, g, ref = rr.case(regime, n, use_clamp=bool(use_clamp))
    got = _elementwise(inp, g)
    _assert_units(ref.errors(UNITS_KERNEL, **got), UNITS_KERNEL, f"entropy_gaussian {regime} clamp={use_clamp}")
    _check_classes(inp, ref, got, regime)
    near1 = ref.unit & (ref.bits < 1e-3)
    if near1.any():
        print(f"[rate-units] log2 floor {regime}: max |bits - fp64| where bits < 1e-3 = "
              f"{np.abs(got['bits'] - ref.bits)[near1].max() / 2.0 ** -22:.3f} * 2^-22 over {int(near1.sum())}")


@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
@pytest.mark.parametrize("layout", ["elem", "row"])
def test_entropy_gaussian_kernels_at_every_size_and_q_layout(n, layout):
    """Block edges (256 threads) and one Q per row of 50: body and tail elements alternate by block of 64 (a shared q is the
    same in both regimes)."""
    parts = [rr.case(regime, n, 3, True, layout) for regime in ("body", "tail")]
    pick = (np.arange(n) // 64) % 2 == 1
    inp = tuple(np.where(pick, parts[1][0][i], parts[0][0][i]) for i in range(4)) + (rr.X_MEAN, True)
    g = rr.g_bits(n, 3)
    ref = rr.eg_fp64(*inp, g_bits=g)
    got = _elementwise(inp, g, 1 if layout == "elem" else 50)
    _assert_units(ref.errors(UNITS_KERNEL, **got), UNITS_KERNEL, f"entropy_gaussian n={n} {layout}")


@gpu
@pytest.mark.parametrize("form,use_clamp", [("scalar", False), ("scalar", True), ("row", True), ("elem", False)])
def test_entropy_gaussian_module_per_element(form, use_clamp, monkeypatch):
    """entropy_models.Entropy_gaussian: the scalar-Q, one-Q-per-row and element-wise-Q forms through autograd."""
    from contextgs_amd import encodings
    from contextgs_amd.entropy_models import Entropy_gaussian
    monkeypatch.setattr(encodings, "use_clamp", use_clamp)
    rows, cols = 301, 50
    n = rows * cols
    parts = [rr.case(regime, n, 5, use_clamp, form, cols) for regime in ("body", "switch", "tail")]
    pick = (np.arange(n) // cols) % 3
    inp = tuple(np.choose(pick, [p[0][i] for p in parts]) for i in range(4)) + (rr.X_MEAN, use_clamp)
    x, mean, s, q = (a.reshape(rows, cols) for a in inp[:4])
    g = rr.g_bits(n, 5)
    ref = rr.eg_fp64(*inp, g_bits=g)
    xd, md, sd = (T(a).requires_grad_(True) for a in (x, mean, s))
    if form == "scalar":
        assert (q == q[0, 0]).all()
        eg, Qd = Entropy_gaussian(Q=float(q[0, 0])), None
    else:
        eg, Qd = Entropy_gaussian(Q=1), T(q if form == "elem" else q[:, :1]).requires_grad_(True)
    bits = eg(xd, md, sd, Qd, torch.tensor(rr.X_MEAN, device="cuda") if use_clamp else None)
    (bits * T(g.reshape(rows, cols))).sum().backward()
    got = dict(bits=bits.detach().cpu().numpy().ravel(), gx=xd.grad.cpu().numpy().ravel(), gm=md.grad.cpu().numpy().ravel(),
               gs=sd.grad.cpu().numpy().ravel())
    if form == "elem":
        got["gq"] = Qd.grad.cpu().numpy().ravel()
    _assert_units(ref.errors(UNITS_KERNEL, **got), UNITS_KERNEL, f"Entropy_gaussian {form} clamp={use_clamp}")
    if form == "row":       # the row's gradient is the sum of its elements': undecided elements may add theirs or nothing
        tol = np.where(ref.unit, UNITS_KERNEL * ref.tol1["gq"], 0.0) + np.where(ref.undecided, np.abs(ref.free["gq"]), 0.0)
        tol = (tol + rr.SUM_RTOL * np.abs(ref.gq)).reshape(rows, cols).sum(1)
        assert (np.abs(Qd.grad.cpu().numpy()[:, 0] - ref.gq.reshape(rows, cols).sum(1)) <= tol).all()


# ---- b. the per-level kernels ---------------------------------------------------------------------------------------------------
X_MEANS = np.array([0.25, -0.5, 0.125])
G_SUMS = np.array([0.7, -1.3, 2.1], dtype=np.float32)


def _kinds(D, K):
    return np.concatenate([np.zeros(D, int), np.ones(6, int), np.full(3 * K, 2)])


def _level_case(D, K, n_sub, use_clamp, with_loc, with_grows, with_masks, seed):
    """Inputs of one cgs_level_rate call: every element of every chosen row has its own regime."""
    rng = np.random.default_rng(seed)
    E, kind = D + 6 + 3 * K, _kinds(D, K)
    n_l = 2 * n_sub + 3 if with_loc else n_sub
    loc = rng.permutation(n_l)[:n_sub] if with_loc else np.arange(n_sub)
    Q = rr.draw_q(rng, (n_l, 3))[0]
    clamp_rows = None
    if use_clamp:
        clamp_rows = np.arange(n_sub) % 3 == 0
        Q[loc[clamp_rows]] = rr.QGRID * np.array([1, 2, 3])
    q = Q[loc][:, kind]
    regime = rr.mixed_regimes(rng, (n_sub, E), clamp_rows)
    xm = np.broadcast_to(X_MEANS[kind], (n_sub, E))
    x, mean, s, regime = rr.settle(regime, q, rr.scale_for(rng, q), seed + 1, xm, use_clamp)
    n_anchor = n_sub + 5
    grows = rng.integers(0, n_anchor, n_sub) if with_grows else np.arange(n_sub)
    masks = (rng.random((n_anchor, K)) < 0.6).astype(np.float32) if with_masks else None
    w = np.ones((n_sub, E), dtype=np.float32)
    if with_masks:
        w[:, D + 6:] = np.repeat(masks[grows], 3, axis=1)
    ref = rr.eg_fp64(x, mean, s, q, xm, use_clamp, g_bits=G_SUMS[kind][None, :] * w)
    return dict(D=D, K=K, E=E, kind=kind, n_l=n_l, loc=loc, Q=Q, x=x, mean=mean, s=s, grows=grows, masks=masks, w=w, ref=ref,
                n_anchor=n_anchor, rng=rng, regime=regime)


LEVEL_CASES = [
    # D, K, n_sub, extra columns of pred, loc, grows, masks, compact, use_clamp
    (50, 10, 257, 3, 1, 1, 1, 0, 1),
    (50, 10, 33, 0, 0, 0, 0, 0, 0),
    (50, 10, 3, 64, 1, 0, 1, 1, 1),
    (32, 4, 33, 3, 1, 1, 0, 1, 0),
    (32, 4, 2, 0, 0, 1, 1, 0, 1),
    (64, 12, 257, 64, 1, 1, 1, 1, 0),
    (64, 12, 1, 3, 1, 0, 1, 0, 1),
    (1, 1, 257, 0, 1, 1, 1, 0, 1),
    (1, 1, 3, 64, 0, 0, 0, 1, 0),
    (50, 20, 33, 64, 1, 1, 1, 0, 1),
    (50, 20, 2, 3, 0, 1, 0, 1, 0),
    (50, 20, 1, 0, 1, 0, 1, 1, 1),
]


@gpu
@pytest.mark.parametrize("D,K,n_sub,extra,with_loc,with_grows,with_masks,compact,use_clamp", LEVEL_CASES)
def test_level_rate_kernels_per_element(D, K, n_sub, extra, with_loc, with_grows, with_masks, compact, use_clamp):
    from contextgs_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    c = _level_case(D, K, n_sub, use_clamp, with_loc, with_grows, with_masks, 100 * D + 10 * K + n_sub)
    E, kind, ref, loc, rng = c["E"], c["kind"], c["ref"], c["loc"], c["rng"]
    n_l, ldp, O = c["n_l"], 2 * E + extra, 3 * K
    ys = [rng.normal(size=(n_l, wd)).astype(np.float32) for wd in (D, 6, O)]
    for k, y in enumerate(ys):
        y[loc] = c["x"][:, kind == k]
    pred = rng.normal(size=(n_sub, ldp)).astype(np.float32)
    cols = dict(mf=(0, D), sf=(D, D), ms=(2 * D, 6), ss=(2 * D + 6, 6), mo=(2 * D + 12, O), so=(2 * D + 12 + O, O))
    for k, (mc, sc) in enumerate((("mf", "sf"), ("ms", "ss"), ("mo", "so"))):
        pred[:, cols[mc][0]:sum(cols[mc])] = c["mean"][:, kind == k]
        pred[:, cols[sc][0]:sum(cols[sc])] = c["s"][:, kind == k]
    yd, Qd, predd, xmd, gsd = [T(y) for y in ys], T(c["Q"]), T(pred), T(X_MEANS), T(G_SUMS)
    locd = T(loc, np.int64) if with_loc else None
    growsd = T(c["grows"], np.int64) if with_grows else None
    md = T(c["masks"]) if with_masks else None
    st = _lib.current_stream()
    args = (p(yd[0]), p(yd[1]), p(yd[2]), p(Qd), p(locd), p(predd), p(md), p(growsd), p(xmd), int(use_clamp), n_sub, D, K, ldp)

    # forward: the three sums, twice
    bw = c["w"] * 1.0
    want = np.array([(ref.bits * bw)[:, kind == k].sum() for k in range(3)])
    tol = np.array([(ref.tol("bits", UNITS_KERNEL) * bw + rr.SUM_RTOL * np.abs(ref.bits * bw))[:, kind == k].sum() for k in range(3)])
    sums = torch.zeros(2, 3, device="cuda")
    for i in range(2):
        _lib.check(L.cgs_level_rate_fwd(*args, p(sums[i]), st), "level_rate_fwd")
    sums = sums.cpu().numpy().astype(np.float64)
    print(f"[rate-units] level_rate sums D={D} K={K} n_sub={n_sub}: error / tolerance {np.abs(sums[0] - want) / tol}")
    assert (np.abs(sums - want) <= tol).all(), (sums, want, tol)
    assert (np.abs(sums[0] - sums[1]) <= tol).all()

    # backward
    n_out = n_sub if compact else n_l
    d_pred, d_y, dQ = _nan(n_sub, ldp), [_nan(n_out, wd) for wd in (D, 6, O)], _nan(n_out, 3)
    d_masks = torch.zeros(c["n_anchor"], K, device="cuda") if with_masks else _nan(c["n_anchor"], K)
    _lib.check(L.cgs_level_rate_bwd(*args, p(gsd), p(d_pred), p(d_y[0]), p(d_y[1]), p(d_y[2]), p(dQ), p(d_masks), int(compact), st),
               "level_rate_bwd")
    d_pred, dQ, d_masks = d_pred.cpu().numpy(), dQ.cpu().numpy(), d_masks.cpu().numpy()
    d_y = [t.cpu().numpy() for t in d_y]
    out_rows = np.arange(n_sub) if compact else loc
    got = dict(gx=np.empty((n_sub, E), np.float32), gm=np.empty((n_sub, E), np.float32), gs=np.empty((n_sub, E), np.float32))
    for k, (mc, sc) in enumerate((("mf", "sf"), ("ms", "ss"), ("mo", "so"))):
        got["gx"][:, kind == k] = d_y[k][out_rows]
        got["gm"][:, kind == k] = d_pred[:, cols[mc][0]:sum(cols[mc])]
        got["gs"][:, kind == k] = d_pred[:, cols[sc][0]:sum(cols[sc])]
    _assert_units(ref.errors(UNITS_KERNEL, **got), UNITS_KERNEL, f"level_rate D={D} K={K} n_sub={n_sub}", c["regime"])
    assert (d_pred[:, 2 * E:] == 0).all()
    other = np.setdiff1d(np.arange(n_out), out_rows)
    assert all(np.isnan(t[other]).all() for t in d_y + [dQ])
    # dQ: per chosen row and kind, the sum of the row's elements
    for k in range(3):
        want, tol = ref.sum_tol("gq", UNITS_KERNEL, (kind == k)[None, :] * 1.0, axes=1)
        assert (np.abs(dQ[out_rows, k] - want) <= tol).all(), (k, np.abs(dQ[out_rows, k] - want) / tol)
    # d_masks[grow, j] = g_sums[2] * the bits of the offsets 3j .. 3j + 2 of every chosen row with that anchor row
    if with_masks:
        off = kind == 2
        index = (c["grows"][:, None] * K + np.arange(O)[None, :] // 3)
        plain = rr.eg_fp64(c["x"][:, off], c["mean"][:, off], c["s"][:, off], c["Q"][loc][:, 2:3], X_MEANS[2], use_clamp)
        want, tol = plain.sum_tol("bits", UNITS_KERNEL, np.full((n_sub, O), float(G_SUMS[2])), index=index, size=c["n_anchor"] * K)
        assert (np.abs(d_masks.ravel() - want) <= tol).all(), np.nanmax(np.abs(d_masks.ravel() - want) / np.maximum(tol, 1e-30))
        assert (d_masks.ravel()[np.bincount(index.ravel(), minlength=want.size) == 0] == 0).all()
    else:
        assert np.isnan(d_masks).all()


# ---- c. the fused rate-subset kernels -------------------------------------------------------------------------------------------
RS_D, RS_K, RS_E = 50, 10, 86
RS_COL = dict(mean=[0, 100, 112], scale=[50, 106, 142], width=[50, 6, 30])       # the blocks of mlp_grid's second layer


def _rate_sub_case(m, in_dim, use_clamp, seed):
    """W2 = 0: column e of the 86 elements has mean b2[.] and scale b2[.]; the regime of an element changes with its row (x, Q)
    and its column (mean, scale: tiny-scale columns, and with use_clamp columns whose mean sits next to a clamp bound)."""
    rng = np.random.default_rng(seed)
    kind = _kinds(RS_D, RS_K)
    n = 3 * m + 5
    loc = np.sort(rng.permutation(n)[:m])
    Q = np.clip(rr._grid(rr._logu(rng, 2.0 ** -6, 1.0, (n, 3)), rr.QGRID), rr.QGRID, None)
    s_col = rr._logu(rng, 5e-2, 1.2, RS_E)
    tiny_cols = np.array([3, 17, 49, 52, 60, 85])
    s_col[tiny_cols] = rr.TINY_SCALES
    mean_col = rr._grid(rng.uniform(-4, 4, RS_E), rr.GRID)
    regime = rng.integers(0, 3, (m, RS_E))
    regime[:, tiny_cols] = rr.TINY
    override = None
    if use_clamp:
        clamp_rows = np.arange(m) % 3 == 0
        Q[loc[clamp_rows]] = rr.QGRID * np.array([1, 2, 3])
        clamp_cols = np.array([1, 20, 48, 51, 54, 57, 70, 84])
        sgn = np.where(np.arange(len(clamp_cols)) % 2 == 0, 1.0, -1.0)
        s_col[clamp_cols] = rr._logu(rng, 2e-2, 0.1, len(clamp_cols))
        edge = X_MEANS[kind[clamp_cols]] + sgn * 15000 * rr.QGRID * (1 + kind[clamp_cols])
        mean_col[clamp_cols] = edge - rr._grid(rng.uniform(-2, 2, len(clamp_cols)) * s_col[clamp_cols], rr.GRID)
        beyond = rr._grid(rr._logu(rng, 1e-3, 50.0, (m, len(clamp_cols))), rr.GRID) * (np.arange(m)[:, None] % 2)

        def override(x, mean, s):
            x = x.copy()
            rows = np.nonzero(clamp_rows)[0]
            x[np.ix_(rows, clamp_cols)] = (edge[None, :] + sgn[None, :] * beyond)[rows]
            return x
    q = Q[loc][:, kind]
    xm = np.broadcast_to(X_MEANS[kind], (m, RS_E))
    x, mean, s, regime = rr.settle(regime, q, np.broadcast_to(s_col, (m, RS_E)), seed + 1, xm, use_clamp, override=override, s_fixed=True,
                              mean=np.broadcast_to(mean_col, (m, RS_E)))
    assert (mean == mean_col.astype(np.float32)).all() and (s == s_col.astype(np.float32)).all()
    masks = (rng.random((m, RS_K)) < 0.6).astype(np.float32)
    w = np.ones((m, RS_E), dtype=np.float32)
    w[:, 56:] = np.repeat(masks, 3, axis=1)
    ref = rr.eg_fp64(x, mean, s, q, xm, use_clamp, g_bits=G_SUMS[kind][None, :] * w)
    b2 = rng.normal(size=175).astype(np.float32)
    for k in range(3):
        b2[RS_COL["mean"][k]:RS_COL["mean"][k] + RS_COL["width"][k]] = mean_col[kind == k]
        b2[RS_COL["scale"][k]:RS_COL["scale"][k] + RS_COL["width"][k]] = s_col[kind == k]
    return dict(kind=kind, n=n, loc=loc, Q=Q, x=x, q=q, xm=xm, mean=mean, s=s, masks=masks, w=w, ref=ref, b2=b2, rng=rng,
                regime=regime)


def _rate_sub_run(c, in_dim, m, use_clamp):
    """cgs_rate_sub_fwd (twice, on zeroed sums) and cgs_rate_sub_bwd on the case c with random X, W1, b1 and W2 = 0 -> the
    outputs as numpy arrays (NaN before the call) and the fp64 hidden layer with the error bound of its fp32 evaluation."""
    from contextgs_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    kind, loc, rng, n = c["kind"], c["loc"], c["rng"], c["n"]
    X = rng.normal(size=(n, in_dim)).astype(np.float32)
    W1, b1 = (rng.normal(size=(100, in_dim)) * 0.2).astype(np.float32), (rng.normal(size=100) * 0.1).astype(np.float32)
    W2 = np.zeros((175, 100), dtype=np.float32)
    ys = [rng.normal(size=(n, wd)).astype(np.float32) for wd in (50, 6, 30)]
    for k, y in enumerate(ys):
        y[loc] = c["x"][:, kind == k]
    Xd, W1d, b1d, W2d, b2d, Qd, md, xmd, gsd = map(T, (X, W1, b1, W2, c["b2"], c["Q"], c["masks"], X_MEANS, G_SUMS))
    yd, locd = [T(y) for y in ys], T(loc, np.int64)
    st = _lib.current_stream()
    args = (in_dim, p(Xd), n, p(locd), m, p(W1d), p(b1d), p(W2d), p(b2d), p(yd[0]), p(yd[1]), p(yd[2]), p(Qd), p(md), p(xmd),
            int(use_clamp))
    sums = torch.zeros(2, 3, device="cuda")
    for i in range(2):
        _lib.check(L.cgs_rate_sub_fwd(*args, p(sums[i]), st), "rate_sub_fwd")
    out = dict(side_f=_nan(m, 50), side_s=_nan(m, 6), side_o=_nan(m, 30), side_Q=_nan(m, 3), dx=_nan(m, in_dim), dm=_nan(m, 10),
               dW1=_nan(100, in_dim), db1=_nan(100), dW2=_nan(175, 100), db2=_nan(175))
    ws = torch.empty(int(L.cgs_rate_sub_bwd_scratch_bytes(in_dim, m)), dtype=torch.uint8, device="cuda")
    _lib.check(L.cgs_rate_sub_bwd(*args, p(gsd), *(p(out[k]) for k in out), p(ws), ws.numel(), st), "rate_sub_bwd")
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["sums"] = sums.cpu().numpy().astype(np.float64)
    X64, W64, b64 = X[loc].astype(np.float64), W1.astype(np.float64), b1.astype(np.float64)
    out["H"] = np.maximum(X64 @ W64.T + b64, 0.0)
    # error of the fp32 hidden layer: (in_dim + 2) roundings of 2^-24 on the sum of magnitudes
    out["dH"] = (in_dim + 2) * 2.0 ** -24 * (np.abs(X64) @ np.abs(W64).T + np.abs(b64))
    return out


@gpu
@pytest.mark.parametrize("in_dim,m,use_clamp", [(15, 1, 1), (15, 15, 0), (15, 16, 1), (15, 17, 0), (15, 33, 1), (15, 129, 1),
                                                 (71, 1, 0), (71, 15, 1), (71, 16, 0), (71, 17, 1), (71, 33, 0), (71, 129, 1)])
def test_rate_sub_kernels_per_element(in_dim, m, use_clamp):
    c = _rate_sub_case(m, in_dim, use_clamp, 1000 * in_dim + m)
    kind, ref = c["kind"], c["ref"]
    o = _rate_sub_run(c, in_dim, m, use_clamp)
    for k, a in o.items():
        assert not np.isnan(a).any(), k                      # every entry written
    side, side_Q, dx, dm = [o["side_f"], o["side_s"], o["side_o"]], o["side_Q"], o["dx"], o["dm"]
    dW1, db1, dW2, db2, sums, H, dH = o["dW1"], o["db1"], o["dW2"], o["db2"], o["sums"], o["H"], o["dH"]
    # forward sums, twice
    bw = c["w"] * 1.0
    want = np.array([(ref.bits * bw)[:, kind == k].sum() for k in range(3)])
    tol = np.array([(ref.tol("bits", UNITS_KERNEL) * bw + rr.SUM_RTOL * np.abs(ref.bits * bw))[:, kind == k].sum() for k in range(3)])
    print(f"[rate-units] rate_sub sums in_dim={in_dim} m={m}: error / tolerance {np.abs(sums[0] - want) / tol}")
    assert (np.abs(sums - want) <= tol).all(), (sums, want, tol)
    assert (np.abs(sums[0] - sums[1]) <= tol).all()
    gx = np.empty((m, RS_E), np.float32)
    for k in range(3):
        gx[:, kind == k] = side[k]
    _assert_units(ref.errors(UNITS_KERNEL, gx=gx), UNITS_KERNEL, f"rate_sub in_dim={in_dim} m={m}", c["regime"])
    for k in range(3):
        want, tol = ref.sum_tol("gq", UNITS_KERNEL, (kind == k)[None, :] * 1.0, axes=1)
        assert (np.abs(side_Q[:, k] - want) <= tol).all(), (k, np.abs(side_Q[:, k] - want) / tol)
    off = kind == 2
    plain = rr.eg_fp64(c["x"][:, off], c["mean"][:, off], c["s"][:, off], c["q"][:, off], X_MEANS[2], use_clamp)
    index = np.arange(m)[:, None] * RS_K + np.arange(30)[None, :] // 3
    want, tol = plain.sum_tol("bits", UNITS_KERNEL, np.full((m, 30), float(G_SUMS[2])), index=index, size=m * RS_K)
    assert (np.abs(dm.ravel() - want) <= tol).all(), np.nanmax(np.abs(dm.ravel() - want) / np.maximum(tol, 1e-30))
    # db2: column sums of the mean / scale gradients (m = 1: the element itself); dW2 = dP^T H
    ones = np.ones((m, RS_E))
    if m == 1:
        errs = ref.errors(UNITS_KERNEL, gm=np.concatenate([db2[RS_COL["mean"][k]:][:RS_COL["width"][k]] for k in range(3)]),
                          gs=np.concatenate([db2[RS_COL["scale"][k]:][:RS_COL["width"][k]] for k in range(3)]))
        _assert_units(errs, UNITS_KERNEL, f"rate_sub db2 in_dim={in_dim} m=1")
    for name, where in (("gm", "mean"), ("gs", "scale")):
        want, tol = ref.sum_tol(name, UNITS_KERNEL, ones, axes=0)
        g, t1 = getattr(ref, name), ref.tol(name, UNITS_KERNEL)
        wantW = g.T @ H
        tolW = t1.T @ H + np.abs(g).T @ (dH + rr.SUM_RTOL * H)
        for k in range(3):
            rows = slice(RS_COL[where][k], RS_COL[where][k] + RS_COL["width"][k])
            assert (np.abs(db2[rows] - want[kind == k]) <= tol[kind == k]).all(), (name, k)
            assert (np.abs(dW2[rows] - wantW[kind == k]) <= tolW[kind == k]).all(), \
                (name, k, np.nanmax(np.abs(dW2[rows] - wantW[kind == k]) / np.maximum(tolW[kind == k], 1e-300)))
    assert (dW2[172:] == 0).all() and (db2[172:] == 0).all()
    # W2 = 0: nothing flows back into the hidden layer
    assert (dx == 0).all() and (dW1 == 0).all() and (db1 == 0).all()
