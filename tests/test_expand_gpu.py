"""The anchor -> Gaussian expansion per element against float64 (tests/expand_ref.py: the reference, the error unit u of every
element, the exact statements, the inputs by regime), through the kernels that state its maths:
  a. renderer._ExpandGaussians (csrc/expand.hip), forward and backward, every regime mixed per slot in one call
  b. cgs_expand_count / _write / _backward through the C ABI, and the survivor scan (cgs_scan_exclusive_u8_total, prims.hip)
     up to its recursive branch
  c. anchor_gen.anchor_gen (the tail of csrc/anchor_gen.hip) with W1 = b1 = 0, so that the second layers' biases steer the slots
csrc/expand_raster.hip is not here: its forward is asserted bit-equal to the unfused node by test_fused_view_gpu.py.

UNITS_LITERAL = 7.3: what the reference's own fp32 expression (torch on the CPU, autograd's backward, the per-anchor sums in slot
order) needs on these inputs, measured by test_expand_ref.py and rounded up to one decimal; its largest entry is the quaternion
gradient, which autograd evaluates as g / |q| - q (sum g q / |q|^2) / |q|.  UNITS_KERNEL = 2 UNITS_LITERAL = 14.6: the kernels
replace libm's exp and the IEEE divisions by 1-ulp hardware forms, about one more rounding of the size the literal already makes.
Neither number is taken from the kernels' results.

Measured maxima in units (one regime per slot; "anchor sums": d_anchor / d_gscaling mix the regimes of an anchor's slots):
                                       xyz  scaling      rot    d_off d_cov0:3 d_cov3:7 d_op_raw   d_mask d_anchor  d_gscal
  fp32 literal      body             1.233    2.216    2.257    0.985    1.540    5.858    0.998    1.710        -        -
                    gate             1.264    2.306    2.513    0.989    1.648    7.213    1.634    1.621        -        -
                    sigmoid          1.327    1.520    2.941    0.992    1.398    6.168    0.970    1.723        -        -
                    quaternion       1.198    2.432    1.957    0.994    1.565    4.952    0.995    1.668        -        -
                    geometry         0.495    2.241    2.422    0.994    1.680    6.904    1.000    1.565        -        -
                    anchor sums          -        -        -        -        -        -        -        -    1.901    3.529
  _ExpandGaussians  body             1.251    2.456    2.985    0.998    1.780    7.509    1.000    1.949        -        -
                    gate             1.343    2.555    2.785    0.997    1.659    8.010    1.744    1.758        -        -
                    sigmoid          1.349    1.588    2.923    0.997    1.389    8.945    0.999    1.768        -        -
                    quaternion       1.423    2.588    2.833    0.998    1.686    8.279    0.999    1.843        -        -
                    geometry         0.499    2.583    2.958    0.995    1.776    7.711    1.000    1.830        -        -
                    anchor sums          -        -        -        -        -        -        -        -    2.511    4.321
  C ABI             body             1.143    2.430    2.906    0.990    1.487    6.992    0.998    1.733        -        -
                    gate             1.349    2.204    2.620    0.988    1.517    6.893    1.699    1.773        -        -
                    sigmoid          1.215    1.564    2.848    0.990    1.261    7.215    0.996    1.752        -        -
                    quaternion       1.225    2.488    2.691    0.987    1.619    7.465    0.996    1.644        -        -
                    geometry         0.493    2.308    2.730    0.992    1.485    7.320    0.999    1.866        -        -
                    anchor sums          -        -        -        -        -        -        -        -    2.091    3.102
  anchor_gen        gate             1.062    0.796    1.772    0.915        -        -        -    1.330        -        -
                    sigmoid          1.051    0.695    1.772    0.936        -        -        -    1.489        -        -
                    quaternion       0.839    0.696    0.929    0.874        -        -        -    1.257        -        -
                    geometry         0.463    0.695    1.772    0.909        -        -        -    1.716        -        -
                    anchor sums          -        -        -        -        -        -        -        -    1.403    1.895
(fp32 literal: torch on the CPU; the others on an MI355X.  _ExpandGaussians: the 47 node tests; C ABI: the five direct calls.)
d_color_in, color, opacity, neural_opacity and the mask have no units: they are equalities.  In anchor_gen every slot carries
sigmoid and quaternion values (slot k of every anchor the same ones); its rows are named by the mask's and the offsets' regime,
else "sigmoid" for even and "quaternion" for odd k.  d_cov_in stays inside that node: its column sums over the anchors, the cov
head's bias gradient, stayed below 0.09 of their tolerance (the elements' own plus n - 1 roundings of the sum).
The kernels' quaternion gradient (g - r (r.g)) / |q| reads the rounded r (up to 3 units itself) twice; it is the largest entry
of both the literal and the kernels.

That the tests bite (each alteration built once into a copy of the library, this file run once on it; arithmetic only, no index
or bound changed, in csrc/expand.hip and in the same line of csrc/anchor_gen.hip's tail where it has one):
  v > 0.f -> v >= 0.f: 52 of the 58 tests fail (the survivor count and mask first; every family, the scan test and the
      argument test included, since +-0 products survive);
  dsr[c] with gs[c] in place of gs[3 + c]: 50 fail (d_cov[0:3] of the node and the C ABI, the cov head's db2 of anchor_gen);
  the quaternion backward without its - r dot projection: 49 fail (d_cov[3:7], by 2^24 units; db2 in anchor_gen);
  term[6 + c] = gsc without sig: 50 fail (d_gscaling[3:6] in all three families).
  Before the db2 check was added, the second and third alteration passed all four anchor_gen tests: d_cov_in is not an output
  of the fused node.  What still passes under an alteration are the tests it cannot reach: the all-survive cases and a lone
  n = K = 1 slot under the first; the none-survive cases, n = K = 1 without a survivor, the argument and the scan test under
  the three backward alterations.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import expand_ref as er
from expand_ref import UNITS_KERNEL

pytestmark = pytest.mark.gpu
PAD = 8
SHAPES = [(1, 1), (1, 32), (33, 7), (37, 7), (31, 10), (32, 10), (33, 10), (65, 32), (205, 10), (4099, 10)]
SRC = ("none", "subset", "perm")
ERR_ARG, ERR_WORKSPACE = 1, 3


def T(a):
    return torch.from_numpy(np.array(a)).cuda()


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _compare(ref, maxima, what, values=None, mask=None, grads=None, weights=None, names=er.GRADS):
    """Every element of `values` / `grads` within UNITS_KERNEL units of the reference (collected in `maxima`), the exact
    statements equal."""
    if values is not None:
        er.check_exact(ref, values, mask)
        for k, u in ref.value_units.items():
            err = er.units_error(values[k], ref.values[k], u, (what, k))
            maxima.add(ref, k, err)
            assert err.max(initial=0.0) <= UNITS_KERNEL, (what, k, float(err.max()))
    if grads is not None:
        want, units = ref.grads(weights)
        er.check_exact(ref, grads=grads, weights=weights, src_grads="d_gscaling" in names)
        for k in names:
            err = er.units_error(grads[k], want[k], units[k], (what, k, tuple(weights)))
            maxima.add(ref, k, err)
            assert err.max(initial=0.0) <= UNITS_KERNEL, (what, k, tuple(weights), float(err.max()))


# ---- a. the autograd node -------------------------------------------------------------------------------------------------------
def _node(c):
    from contextgs_amd.renderer import _ExpandGaussians
    leaves = [T(a).requires_grad_(True) for a in c.inputs()]
    out = _ExpandGaussians.apply(*leaves, c.K, None if c.src_row is None else T(c.src_row))
    return leaves, out


def _node_grads(leaves, out, w):
    loss = sum((out[er.VALUES.index(k)] * T(v)).sum() for k, v in w.items())
    return torch.autograd.grad(loss, leaves, retain_graph=True)


def _check_node(c, what):
    ref = er.Ref(c)
    maxima = er.Maxima()
    leaves, out = _node(c)
    assert out[0].shape[0] == ref.P, (what, out[0].shape[0], ref.P)
    _compare(ref, maxima, what, {k: _np(out[i]) for i, k in enumerate(er.VALUES)}, _np(out[6]))
    for i, names in enumerate(er.LOSSES):
        w = er.draw_weights(ref.P, c.n * c.K, 11 + i, names)
        g = _node_grads(leaves, out, w)
        assert all(a.shape == b.shape for a, b in zip(g, leaves))
        _compare(ref, maxima, what, grads=dict(zip(er.GRADS, map(_np, g))), weights=w)
        if names == er.VALUES:          # the same graph again: the backward has no atomics
            again = _node_grads(leaves, out, w)
            assert all(torch.equal(a, b) for a, b in zip(g, again)), (what, "the backward is not reproducible")
    maxima.report("expand-units", what)


@pytest.mark.parametrize("src", SRC)
@pytest.mark.parametrize("n,K", SHAPES)
def test_expand_node_per_element(n, K, src):
    """Every regime mixed per slot; every output alone, all six, and all but neural_opacity as the loss (an absent gradient
    reaches the kernel as a ctx.P-sized substitute).  src: no src_row, a permuted subset of 3n + 1 rows, a permutation of n rows
    (the route without a zero-fill)."""
    _check_node(er.draw(n, K, 20, src), f"node n={n} K={K} src={src}")


@pytest.mark.parametrize("gate", ["all", "none", "first", "last"])
@pytest.mark.parametrize("n,K,src", [(33, 7, "perm"), (65, 32, "subset"), (205, 10, "none")])
def test_expand_node_gate_extremes(n, K, src, gate):
    """Every slot survives, none does (P = 0: every loss, the one with neural_opacity alone included, runs the backward on empty
    per-Gaussian gradients), one survivor in the first or in the last slot."""
    _check_node(er.draw(n, K, 21, src, gate), f"node n={n} K={K} src={src} gate={gate}")


@pytest.mark.parametrize("regime", er.REGIMES)
def test_expand_node_single_regime(regime):
    """One regime in every slot (all of its values within one call), K = 10 and K = 32."""
    _check_node(er.draw(120, 10, 5, "subset", only=regime), f"node only={regime} K=10")
    _check_node(er.draw(40, 32, 6, "none", only=regime), f"node only={regime} K=32")


# ---- b. the C ABI ---------------------------------------------------------------------------------------------------------------
def _count(n, K, op, m, scratch_less=0, with_flags=True):
    """cgs_expand_count on device operands -> (rc, count, neural_opacity, mask_out, flags, pos); the outputs carry PAD
    entries more than n K, prefilled."""
    from contextgs_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    slots = n * K
    no = _nan(slots + PAD)
    mask_out = torch.full((slots + PAD,), 7, dtype=torch.uint8, device="cuda")
    flags = torch.full((slots + PAD,), 7, dtype=torch.int32, device="cuda") if with_flags else None
    pos = torch.full((slots + PAD,), -1, dtype=torch.int32, device="cuda")
    nbytes = int(L.cgs_expand_scratch_bytes(n, K))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    cnt = C.c_int64(-5)
    rc = L.cgs_expand_count(n, K, p(op), p(m), p(no), p(mask_out), p(flags), p(pos), p(scratch), nbytes - scratch_less, C.byref(cnt),
                            _lib.current_stream())
    torch.cuda.synchronize()
    return rc, int(cnt.value), no, mask_out, flags, pos


@pytest.mark.parametrize("n,K,src", [(1, 1, "none"), (33, 7, "subset"), (65, 32, "perm"), (205, 10, "subset"), (4099, 10, "none")])
def test_expand_c_abi_per_element(n, K, src):
    """The three entry points called directly on prefilled, padded outputs: flags == mask_out, pos == the exclusive sum of the
    flags, the count their sum; values and gradients in units; nothing written past the end, and with a src_row only the rows
    it names."""
    from contextgs_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    c = er.draw(n, K, 22, src)
    ref = er.Ref(c)
    maxima = er.Maxima()
    what = f"C ABI n={n} K={K} src={src}"
    slots, st = n * K, _lib.current_stream()
    anchor, gs, off, m, op, col, cov = (T(a) for a in c.inputs())
    srow = None if c.src_row is None else T(c.src_row)
    rc, P, no, mask_out, flags, pos = _count(n, K, op, m)
    assert rc == 0 and P == ref.P
    f = _np(mask_out)[:slots]
    assert np.array_equal(f, ref.mask.astype(np.uint8)) and np.array_equal(_np(flags)[:slots], f.astype(np.int32))
    assert np.array_equal(_np(pos)[:slots], np.cumsum(f, dtype=np.int64) - f) and P == int(f.sum())
    assert (_np(mask_out)[slots:] == 7).all() and (_np(flags)[slots:] == 7).all() and (_np(pos)[slots:] == -1).all()
    assert np.isnan(_np(no)[slots:]).all()
    out = {k: _nan(P + PAD, er.WIDTH[k]) for k in er.VALUES[:5]}
    _lib.check(L.cgs_expand_write(n, K, p(mask_out), p(pos), p(anchor), p(gs), p(off), p(no), p(col), p(cov), p(out["xyz"]),
                                  p(out["color"]), p(out["opacity"]), p(out["scaling"]), p(out["rot"]), p(srow), st), "cgs_expand_write")
    values = {k: _np(v)[:P] for k, v in out.items()}
    values["neural_opacity"] = _np(no)[:slots].reshape(-1, 1)
    assert all(np.isnan(_np(v)[P:]).all() for v in out.values())
    _compare(ref, maxima, what, values, f)
    unread = np.ones(c.n_src, bool)
    unread[ref.rows] = False
    for names in (er.VALUES, er.VALUES[:5]):                 # with and without g_neural_opacity
        w = er.draw_weights(P, slots, 31, names)
        gw = {k: T(w[k]) for k in names}
        d = dict(d_anchor=_nan(n + PAD, 3), d_gscaling=_nan(c.n_src, 6), d_offsets=_nan(c.n_src, K, 3), d_mask=_nan(n + PAD, K),
                 d_op_raw=_nan(n + PAD, K), d_color_in=_nan(n + PAD, 3 * K), d_cov_in=_nan(n + PAD, 7 * K))
        _lib.check(L.cgs_expand_backward(n, K, p(mask_out), p(pos), p(gs), p(off), p(op), p(m), p(cov), p(gw["xyz"]), p(gw["color"]),
                                         p(gw["opacity"]), p(gw["scaling"]), p(gw["rot"]), p(gw.get("neural_opacity")),
                                         p(d["d_anchor"]), p(d["d_gscaling"]), p(d["d_offsets"]), p(d["d_op_raw"]), p(d["d_mask"]),
                                         p(d["d_color_in"]), p(d["d_cov_in"]), p(srow), st), "cgs_expand_backward")
        g = {k: _np(v) for k, v in d.items()}
        for k in ("d_anchor", "d_mask", "d_op_raw", "d_color_in", "d_cov_in"):
            assert np.isnan(g[k][n:]).all(), k
            g[k] = g[k][:n]
        for k in ("d_gscaling", "d_offsets"):               # the kernel writes the named rows alone (the node zeroes the others)
            assert np.isnan(g[k][unread]).all() and not np.isnan(g[k][ref.rows]).any(), k
            g[k][unread] = 0.0
        _compare(ref, maxima, what, grads=g, weights=w)
    maxima.report("expand-units", what)


def test_expand_c_abi_argument_errors_and_empty_calls():
    from contextgs_amd import _lib
    L = _lib.lib()
    c = er.draw(33, 7, 22, "none")
    op, m = T(c.op_raw), T(c.masks)
    rc, P, no, mask_out, flags, pos = _count(0, 7, op, m)               # n_anchor = 0: zero survivors, nothing touched
    assert rc == 0 and P == 0
    assert np.isnan(_np(no)).all() and (_np(mask_out) == 7).all() and (_np(flags) == 7).all() and (_np(pos) == -1).all()
    args = [None] * 15
    assert L.cgs_expand_write(0, 7, *args) == 0 and L.cgs_expand_backward(0, 7, *([None] * 22)) == 0
    for K in (0, 33):
        rc, P, no, mask_out, flags, pos = _count(33, K, op, m)
        assert rc == ERR_ARG and P == 0 and np.isnan(_np(no)).all() and (_np(pos) == -1).all(), K
        assert L.cgs_expand_write(33, K, *args) == ERR_ARG and L.cgs_expand_backward(33, K, *([None] * 22)) == ERR_ARG
    rc, P, no, mask_out, flags, pos = _count(33, 7, op, m, scratch_less=1)
    assert rc == ERR_WORKSPACE and P == 0 and (_np(pos) == -1).all()
    assert b"scratch" in L.cgs_last_error()
    rc, P, *_ = _count(33, 7, op, m)
    assert rc == 0 and P == er.Ref(c).P


def test_survivor_scan_recursive_branch():
    """K = 8, n_anchor = 4 194 305: 33 554 440 slots = 16385 scan tiles, one more than the self-prefix scan takes: the only
    route into the recursive branch of the scan.  Count-only; operands made on the device."""
    n, K = 4194305, 8
    slots = n * K
    gen = torch.Generator(device="cuda").manual_seed(3)
    op = torch.rand(slots, device="cuda", generator=gen) - 0.3
    m = (torch.rand(slots, device="cuda", generator=gen) < 0.7).float()
    rc, P, no, mask_out, flags, pos = _count(n, K, op, m, with_flags=False)
    assert rc == 0
    want = (op * m) > 0
    assert torch.equal(mask_out[:slots].bool(), want)
    del op, m, no
    f = mask_out[:slots].to(torch.int32)
    excl = torch.cumsum(f, 0, dtype=torch.int32) - f
    assert P == int(want.sum()) and 0.3 * slots < P < 0.7 * slots
    assert torch.equal(pos[:slots], excl)
    assert (pos[slots:] == -1).all() and (mask_out[slots:] == 7).all()


# ---- c. the fused family --------------------------------------------------------------------------------------------------------
AG_K = 10


def _steered_mlps(seed):
    """The 54 -> 50 -> (10 tanh | 30 sigmoid | 70) heads with W1 = b1 = 0: the hidden layer is 0 and every head's output is its
    activation of b2, whatever W2 is.  The cov head's b2 gives slot k of every anchor three sigmoid arguments of the sigmoid
    regime and one quaternion of the quaternion regime (the tenth slot: ordinary values)."""
    import torch.nn as nn
    rng = np.random.default_rng(seed)
    mk = lambda out, act: nn.Sequential(nn.Linear(54, 50), nn.ReLU(True), nn.Linear(50, out), *([act()] if act else [])).cuda()
    mo, mc, mv = mk(10, nn.Tanh), mk(30, nn.Sigmoid), mk(70, None)
    cov = rng.normal(size=(1, AG_K, 7)).astype(np.float32)
    opr, msk = np.zeros((1, AG_K), np.float32), np.zeros((1, AG_K), np.float32)
    regime = np.full((1, AG_K), er.SIGMOID)
    er.fill_regimes(rng, regime, opr, msk, cov, cycle=np.arange(AG_K)[None, :] + 8 * seed)
    regime[:, :9] = er.QUAT
    er.fill_regimes(rng, regime, opr, msk, cov, cycle=np.arange(AG_K)[None, :])
    with torch.no_grad():
        for s in (mo, mc, mv):
            s[0].weight.zero_()
            s[0].bias.zero_()
        mv[2].bias.copy_(T(cov.reshape(70)))
        mo[2].bias.copy_(T(np.array([0.0, -0.0, 0.4, -0.4, 2.0, -2.0, 1e-3, 9.0, 0.7, -0.1], np.float32)))
    return mo, mc, mv, cov.reshape(70)


@pytest.mark.parametrize("fused_wgrad", [False, True])
@pytest.mark.parametrize("n_src,n", [(97, 33), (40, 40)])
def test_anchor_gen_tail_per_element(n_src, n, fused_wgrad, monkeypatch):
    """The mask steers the gate per slot, the offsets the geometry regime; op_raw, color_in and cov_in are the unfused MLP
    kernel's outputs on the same operands, fed to the fp64 reference."""
    from contextgs_amd import anchor_gen, mlp
    monkeypatch.setattr(anchor_gen, "FUSED_WGRAD", fused_wgrad)
    indexed = n_src != n
    base = er.draw(n, AG_K, 23, "subset" if indexed else "none", n_src=n_src if indexed else None)
    assert base.n_src == n_src
    mo, mc, mv, b2 = _steered_mlps(n)
    gen = torch.Generator(device="cuda").manual_seed(n)
    feat_src = torch.randn(n_src, 50, device="cuda", generator=gen).requires_grad_(True)
    row = T(base.src_row) if indexed else None
    cam = torch.tensor([0.3, -3.0, 0.5], device="cuda")
    anchor, gs_src, off_src, masks = (T(a).requires_grad_(True) for a in (base.anchor, base.gscaling, base.offsets, base.masks))
    with torch.no_grad():
        op_raw, color_in, cov_in = mlp.anchor_mlp3_rows(feat_src, row if indexed else torch.arange(n, device="cuda"), anchor, cam,
                                                        mo, mc, mv)
    assert np.array_equal(_np(cov_in), np.broadcast_to(b2, (n, 70)))        # (0 + -0 = +0: equal values, not bits)
    regime = np.where(np.isin(base.regime, (er.GATE, er.GEOM)), base.regime, np.where(np.arange(AG_K) % 2 == 0, er.SIGMOID, er.QUAT))
    c = er.Case(**{**base.__dict__, "op_raw": _np(op_raw).reshape(n, AG_K), "color_in": _np(color_in).reshape(n, 3 * AG_K),
                   "cov_in": _np(cov_in).reshape(n, 7 * AG_K), "regime": regime})
    er.assert_conditions(c)
    ref = er.Ref(c)
    assert 0 < ref.P < n * AG_K
    maxima = er.Maxima()
    what = f"anchor_gen n_src={n_src} n={n} fused_wgrad={fused_wgrad}"
    out = anchor_gen.anchor_gen(feat_src, row, anchor, cam, gs_src, off_src, row, masks, mo, mc, mv)
    assert out[0].shape[0] == ref.P
    _compare(ref, maxima, what, {k: _np(out[i]) for i, k in enumerate(er.VALUES)}, _np(out[6]))
    leaves = [anchor, gs_src, off_src, masks, feat_src, mv[2].bias]
    for names in (er.VALUES, er.VALUES[:5]):
        w = er.draw_weights(ref.P, n * AG_K, 41, names)
        loss = sum((out[er.VALUES.index(k)] * T(v)).sum() for k, v in w.items())
        g = torch.autograd.grad(loss, leaves, retain_graph=True)
        grads = dict(zip(("d_anchor", "d_gscaling", "d_offsets", "d_mask"), map(_np, g[:4])))
        _compare(ref, maxima, what, grads=grads, weights=w, names=("d_anchor", "d_gscaling", "d_offsets", "d_mask"))
        assert not _np(g[4]).any()                           # W1 = 0: nothing flows back through the MLP input
        # d_cov_in stays inside the fused node; its column sums over the anchors are the cov head's bias gradient.  Tolerance:
        # the elements' own, plus n - 1 roundings of the sum on its sum of magnitudes (any order of summation)
        want, units = ref.grads(w)
        tol = UNITS_KERNEL * units["d_cov_in"].sum(0) + (n - 1) * er.U * np.abs(want["d_cov_in"]).sum(0)
        err = np.abs(_np(g[5]).astype(np.float64) - want["d_cov_in"].sum(0))
        print(f"[expand-units] {what} cov head db2: error / tolerance {float((err / np.maximum(tol, 1e-300)).max()):.3f}")
        assert (err <= tol).all(), (what, "db2 of the cov head", float((err / np.maximum(tol, 1e-300)).max()))
    maxima.report("expand-units", what)
