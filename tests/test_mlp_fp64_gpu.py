"""The fused fp32-MFMA MLP kernels (csrc/mlp.hip, mlp_small.hip, mlp3.hip, mlp_wgrad.hip) per element against float64
(tests/mlp_ref.py: the reference, the error unit of every element, the exact statements, the inputs by regime), on every trip of
their loops:
  a. mlp.mlp2 on the seven instances, the recomputing backward on and off, the weight gradients inline and deferred, at the ends
     of a 16-row tile and one, two and several weight-gradient workgroups
  b. the same at n = 256 CUs + 17 (the persistent kernels' second loop trip: one full tile and a one-row tile) with a cotangent
     that is nonzero on ~600 rows, so that a weight gradient sums ~600 terms and a dropped or doubled row is thousands of units
  c. mlp.level_mlp against the composition of its two consumers
  d. mlp.anchor_mlp3 and mlp.anchor_mlp3_rows (the assembled row, the pull-back to the anchor, the scattered feature gradient)
  e. cgs_mlp2_forward / _backward / _backward_rows / _wgrad through the C ABI: the stored h, dz1, dz2, gradient buffers that are
     pre-loaded with a constant, a shuffled dx_rows table, sentinels behind the last row.  No caller inside contextgs_amd/ passes
     a row stride (ldx, ldy, lddx, lddz2) other than the width, so there is no strided case.
Every element of every output within UNITS_KERNEL = 2 UNITS_LITERAL = 13.2 units, the exact statements equal.  UNITS_LITERAL = 6.6
is measured on the CPU (tests/test_mlp_ref.py; table in mlp_ref.py); neither number is taken from a kernel's result.

Measured maxima in units (MI355X, 256 CUs; "-": not an output of that entry point; the literals' rows are mlp_ref.py's):
                                       h      y    dz2    dz1     dx    dW1    db1    dW2    db2  x_row d_feat d_anchor
  literal (a) torch, CPU           6.583  1.627  1.273  4.980  2.091  1.966  1.370  1.838  2.099  2.837      -    4.396
  literal (b) sequential           4.928  1.587  1.099  5.364  2.091  1.966  1.479  1.811  2.223  3.302      -    4.717
  literal (c) mlp_frag.h's order   2.967  1.146  1.099  2.456  1.024  1.966  0.838  1.341  2.099      -      -        -
  mlp2, hidden layer saved (154)       -  1.492      -      -  2.509  1.661  1.476  1.778  1.462      -      -        -
  mlp2, recomputing backward (44)      -  0.881      -      -  2.509  1.262  0.595  1.084  0.554      -      -        -
  mlp2, second loop trip (18)          -  1.611      -      -  1.724  0.347  0.146  0.214  0.295      -      -        -
  level_mlp (48)                       -  1.163      -      -  1.369  1.918  1.672  1.767  1.265      -      -        -
  anchor_mlp3 (17)                     -  1.127      -      -  0.462  1.967  0.858  2.041  2.310      -      -        -
  anchor_mlp3_rows (33)                -  1.788      -      -      -  1.710  0.811  2.459  1.262  3.817  0.509    0.200
  C ABI (16)                       4.441  1.086  1.030  4.041  1.482  0.525  0.158  0.267  0.344      -      -        -
Every kernel stays below the literals' own 6.6, a third of UNITS_KERNEL: no kernel had to change.  x_row is in units of its own
(u |x|, at most 6 for the direction and 4 for the distance, mlp_ref.AnchorRows); the weight gradients of the second-trip case are
small because a unit there is the absolute sum over ~600 live rows and the error of a sum grows like its root.

That the tests bite (each alteration built once into a copy of the library outside the source tree, this file and
tests/test_mlp_gpu.py run once on it; arithmetic only, no index, bound or address changed):
  1. the backward's ReLU gates compare `>= 0.f` (mlp.hip, mlp_small.hip, both gates of mlp3.hip): all 330 tests here fail;
     test_mlp_gpu.py: 46 of 79 fail (test_forward_backward_match_torch 42 / 42, test_anchor_mlp3_matches_three_torch_mlps 4 / 4).
     The old file does see this one: the gates read the saved h = max(z1, 0), so `>=` opens every closed unit, not only the units
     at exactly 0.
  2. the B operand of the second layer's MFMA in mlp2_fwd_kernel with its low six mantissa bits cleared: 80 fail here
     (test_mlp2_every_element 50, the second loop trip 6, test_level_mlp 20, the C ABI 4: y of the 70- and 175-output
     instances, and of the others at single row counts; the tanh and sigmoid heads damp it below the bound at most sizes, and
     the anchor kernels have a forward of their own); test_mlp_gpu.py passes all 79.
  3. frag_act_grad<SIGMOID> times 1 + 2^-17: 36 fail here (test_mlp2_every_element 8: the sigmoid instance at 1, 15, 16 and
     17 rows; test_anchor_mlp3 10: 1, 15, 16, 17 and 33 rows; test_anchor_mlp3_rows 16: 1, 15, 17 and 32 rows; the C ABI 2: the
     sigmoid instance's dz2 at 513 rows); test_mlp_gpu.py passes all 79.  Through the autograd nodes the factor is seen in the
     weight gradients of few rows only: a common relative factor on every term of a long signed sum is small against the
     sum's absolute value, which is the unit; the C ABI cases judge dz2 itself at any row count.
  (A first build of 2. applied __builtin_bit_cast to `acc1[t][rt][r]` directly, which read element 0 of the vector for every r:
  a grossly wrong forward that both files failed.  It was rebuilt through a scalar temporary and run again.)
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

import mlp_ref as mr
from mlp_ref import U, UNITS_KERNEL

pytestmark = pytest.mark.gpu
PAD = 64
SENTINEL = -7.25
VARIANTS = [(cfg, True) for cfg in mr.INSTANCES] + [(cfg, False) for cfg in mr.INSTANCES if cfg[2] == 3]     # (cfg, RECOMPUTE_HIDDEN)
MAXIMA = {}


def T(a):
    return torch.from_numpy(np.array(a)).cuda()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _cus():
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def _maxima(entry):
    return MAXIMA.setdefault(entry, mr.Maxima())


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for entry, m in MAXIMA.items():
        m.report(entry)


def _seq(c):
    in_f, hid, out, act = c.cfg
    layers = [nn.Linear(in_f, hid), nn.ReLU(True), nn.Linear(hid, out)] + ([nn.Tanh()] if act == 1 else [nn.Sigmoid()] if act == 2 else [])
    seq = nn.Sequential(*layers).cuda()
    with torch.no_grad():
        for p, a in zip((seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias), (c.W1, c.b1, c.W2, c.b2)):
            p.copy_(T(a))
    return seq


def _judge(got, want, unit, maxima, key, what):
    err = mr.units_error(got, want, unit, (what, key))
    maxima.add(key, err)
    assert err.max(initial=0.0) <= UNITS_KERNEL, (what, key, float(err.max()), np.unravel_index(int(err.argmax()), err.shape))


class _deferred:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from contextgs_amd import mlp
        self.prev = mlp.defer_weight_gradients(self.on)

    def __exit__(self, *exc):
        from contextgs_amd import mlp
        mlp.defer_weight_gradients(self.prev)


_BIG = {}


def _big_ref(key, make):
    """One reference of the 256-CU size at a time (hundreds of MB each)."""
    if key not in _BIG:
        _BIG.clear()
        _BIG[key] = make()
    return _BIG[key]


# ---- a, b. the autograd node ----------------------------------------------------------------------------------------------------
def _run_mlp2(cfg, recompute, n, defer, rows, monkeypatch, entry):
    from contextgs_amd import mlp
    c = mr.draw(cfg, n, 0, rows)
    ref = mr.ref_of(cfg, n) if rows is None else _big_ref(("mlp2", cfg), lambda: mr.Ref(c.x, c.W1, c.b1, c.W2, c.b2, c.act, c.dy))
    monkeypatch.setattr(mlp, "RECOMPUTE_HIDDEN", recompute)
    seq = _seq(c)
    x = T(c.x).requires_grad_(True)
    with _deferred(defer):
        y = mlp.mlp2(x, seq)
        y.backward(T(c.dy))
    got = dict(y=_np(y), dx=_np(x.grad), dW1=_np(seq[0].weight.grad), db1=_np(seq[0].bias.grad), dW2=_np(seq[2].weight.grad),
               db2=_np(seq[2].bias.grad))
    mr.judge(ref, got, _maxima(entry), (cfg, recompute, n, defer))


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("n", mr.ROW_COUNTS)
@pytest.mark.parametrize("cfg,recompute", VARIANTS)
def test_mlp2_every_element(cfg, recompute, n, defer, monkeypatch):
    _run_mlp2(cfg, recompute, n, defer, None, monkeypatch, "mlp2 recompute" if recompute and cfg[2] == 3 else "mlp2")


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("cfg,recompute", VARIANTS)
def test_mlp2_second_loop_trip_with_a_sparse_cotangent(cfg, recompute, defer, monkeypatch):
    cus = _cus()
    n = 256 * cus + 17
    _run_mlp2(cfg, recompute, n, defer, mr.sparse_rows(n, cus), monkeypatch, "mlp2 second trip")


# ---- c. the level node ----------------------------------------------------------------------------------------------------------
def _loc(n, kind):
    rng = np.random.default_rng(n)
    if kind == "empty":
        return np.zeros(0, np.int64)
    if kind == "one":
        return np.array([n // 2], np.int64)
    if kind == "all":
        return np.arange(n, dtype=np.int64)
    return np.sort(rng.permutation(n)[:max(1, (15 * n) // 100)]).astype(np.int64)


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("kind", ["empty", "one", "some", "all"])
@pytest.mark.parametrize("n", [1, 17, 2100])
@pytest.mark.parametrize("cfg", [(71, 100, 175, 0), (15, 100, 175, 0)])
def test_level_mlp_is_the_sum_of_its_two_consumers(cfg, n, kind, defer):
    """seq(x)[:, 172:] on all rows and seq(x[loc]) on the subset; dx and the module's four weight gradients are the sums of both
    routes (one more rounding of the sum on top of the routes' units)."""
    from contextgs_amd import mlp
    n_stat = 172
    c = mr.draw(cfg, n)
    loc = _loc(n, kind)
    m = len(loc)
    dq = np.ascontiguousarray(c.dy[:, n_stat:])
    dpred = np.random.default_rng(7 + n).normal(size=(m, cfg[2])).astype(np.float32)
    A = mr.Ref(c.x, c.W1, c.b1, c.W2[n_stat:], c.b2[n_stat:], 0, dq)
    B = mr.Ref(c.x[loc], c.W1, c.b1, c.W2, c.b2, 0, dpred)
    seq = _seq(c)
    x = T(c.x).requires_grad_(True)
    with _deferred(defer):
        qadj, pred = mlp.level_mlp(x, T(loc), seq, n_stat)
        ((qadj * T(dq)).sum() + (pred * T(dpred)).sum()).backward()
    what, mx = (cfg, n, kind, defer), _maxima("level_mlp")
    _judge(_np(qadj), A.values["y"], A.units["y"], mx, "y", what)
    _judge(_np(pred), B.values["y"], B.units["y"], mx, "y", what)

    def both(k, place):
        a, ua = A.values[k], A.units[k]
        b, ub = np.zeros_like(a), np.zeros_like(a)
        place(b, B.values[k])
        place(ub, B.units[k])
        return a + b, ua + ub + U * (np.abs(a) + np.abs(b))

    def rows(dst, v):
        dst[loc] = v

    def whole(dst, v):
        dst[...] = v
    want, unit = both("dx", rows)
    _judge(_np(x.grad), want, unit, mx, "dx", what)
    for k, p in (("dW1", seq[0].weight), ("db1", seq[0].bias)):
        want, unit = both(k, whole)
        _judge(_np(p.grad), want, unit, mx, k, what)
    for k, p in (("dW2", seq[2].weight), ("db2", seq[2].bias)):
        g = _np(p.grad)
        _judge(g[:n_stat], B.values[k][:n_stat], B.units[k][:n_stat], mx, k, what)
        a, ua, b, ub = A.values[k], A.units[k], B.values[k][n_stat:], B.units[k][n_stat:]
        _judge(g[n_stat:], a + b, ua + ub + U * (np.abs(a) + np.abs(b)), mx, k, what)


# ---- d. the three anchor MLPs ---------------------------------------------------------------------------------------------------
def _heads_got(ys, seqs):
    got = []
    for y, s in zip(ys, seqs):
        got.append(dict(y=_np(y), dW1=_np(s[0].weight.grad), db1=_np(s[0].bias.grad), dW2=_np(s[2].weight.grad), db2=_np(s[2].bias.grad)))
    return got


def _run_anchor_mlp3(n, defer, rows):
    from contextgs_amd import mlp
    cs = mr.draw3(n, 0, rows)
    make = lambda: [mr.Ref(c.x, c.W1, c.b1, c.W2, c.b2, c.act, c.dy) for c in cs]
    refs = make() if rows is None else _big_ref(("mlp3", n), make)
    seqs = [_seq(c) for c in cs]
    x = T(cs[0].x).requires_grad_(True)
    with _deferred(defer):
        ys = mlp.anchor_mlp3(x, *seqs)
        torch.autograd.backward(list(ys), [T(c.dy) for c in cs])
    what, mx = (n, defer), _maxima("anchor_mlp3")
    for ref, got in zip(refs, _heads_got(ys, seqs)):
        mr.judge(ref, got, mx, what)
    dx = _np(x.grad)
    _judge(dx, sum(r.values["dx"] for r in refs), sum(r.units["dx"] for r in refs), mx, "dx", what)
    live = np.logical_or.reduce([r.live for r in refs])
    assert (dx[~live] == 0).all()


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 33, 2100])
def test_anchor_mlp3_every_element(n, defer):
    _run_anchor_mlp3(n, defer, None)


def test_anchor_mlp3_second_loop_trip_with_a_sparse_cotangent():
    cus = _cus()
    n = 256 * cus + 33
    _run_anchor_mlp3(n, False, mr.sparse_rows(n, cus, tile=32))


def _run_anchor_rows(n, tiled, keep_x, rows, monkeypatch):
    from contextgs_amd import mlp
    cs = mr.draw3(n, 1, rows, dead=False)                      # (the weights and the cotangents; the rows come from the kernel)
    W1cat, b1cat = np.concatenate([c.W1 for c in cs]), np.concatenate([c.b1 for c in cs])
    a = mr.draw_anchor(n, 1, W1=W1cat, b1=b1cat)
    seqs = [_seq(c) for c in cs]
    what, mx = (n, tiled, keep_x), _maxima("anchor_mlp3_rows")
    # the row the forward assembles and stores, in units of its own
    monkeypatch.setattr(mlp, "KEEP_X_OFF", False)
    monkeypatch.setattr(mlp, "M3_TILED", False)
    pre = mlp.anchor_mlp3_rows_launch(T(a.feat_src), T(a.src_row), T(a.anchor), T(a.cam), *seqs)
    xk = _np(pre.x)[:, :54]
    geo = mr.AnchorRows(a.feat_src, a.src_row, a.anchor, a.cam)
    assert np.array_equal(xk[:, :50], a.feat_src[a.src_row])
    ex = mr.units_error(xk, geo.x, geo.x_unit, (what, "x_row"))
    mx.add("x_row", ex)
    assert (ex[:, 50:] <= mr.AnchorRows.X_ROUNDINGS).all(), (what, ex[:, 50:].max(0))
    assert not mr.ambiguous_rows(xk, W1cat, b1cat).any(), "an ambiguous ReLU gate is left"
    make = lambda: [mr.Ref(xk, c.W1, c.b1, c.W2, c.b2, c.act, c.dy) for c in cs]
    refs = make() if rows is None else _big_ref(("rows", n), make)
    # the node under the knobs
    monkeypatch.setattr(mlp, "KEEP_X_OFF", not keep_x)
    monkeypatch.setattr(mlp, "M3_TILED", tiled)
    feat, anchor = T(a.feat_src).requires_grad_(True), T(a.anchor).requires_grad_(True)
    ys = mlp.anchor_mlp3_rows(feat, T(a.src_row), anchor, T(a.cam), *seqs)
    torch.autograd.backward(list(ys), [T(c.dy) for c in cs])
    for ref, got in zip(refs, _heads_got(ys, seqs)):
        mr.judge(ref, got, mx, what)
    dX, UdX = sum(r.values["dx"] for r in refs), sum(r.units["dx"] for r in refs)
    d_src = _np(feat.grad)
    _judge(d_src[a.src_row], dX[:, :50], UdX[:, :50], mx, "d_feat_src", what)
    unread = np.ones(a.n_src, bool)
    unread[a.src_row] = False
    live = np.logical_or.reduce([r.live for r in refs])
    assert (d_src[unread] == 0).all() and (d_src[a.src_row][~live] == 0).all()
    want, unit = geo.pull_back(dX, UdX)
    _judge(_np(anchor.grad), want, unit, mx, "d_anchor", what)
    assert (_np(anchor.grad)[~live] == 0).all()


@pytest.mark.parametrize("keep_x", [True, False])
@pytest.mark.parametrize("tiled", [True, False])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 33, 2100])
def test_anchor_mlp3_rows_every_element(n, tiled, keep_x, monkeypatch):
    _run_anchor_rows(n, tiled, keep_x, None, monkeypatch)


def test_anchor_mlp3_rows_second_loop_trip_with_a_sparse_cotangent(monkeypatch):
    cus = _cus()
    n = 256 * cus + 33
    _run_anchor_rows(n, True, True, mr.sparse_rows(n, cus, tile=32), monkeypatch)


# ---- e. the C ABI ---------------------------------------------------------------------------------------------------------------
def _buf(rows, width, fill=SENTINEL):
    return torch.full((rows * width + PAD,), fill, dtype=torch.float32, device="cuda")


def _body(buf, rows, width):
    assert bool((buf[rows * width:] == SENTINEL).all()), "the padding behind the last row changed"
    return _np(buf[:rows * width].view(rows, width))


@pytest.mark.parametrize("cfg,route", [(cfg, r) for cfg in mr.INSTANCES for r in ("accumulate", "dx_rows")] +
                         [(cfg, "recompute") for cfg in mr.INSTANCES if cfg[2] == 3])
def test_c_abi_adds_into_preloaded_buffers(cfg, route):
    """accumulate: cgs_mlp2_backward with accumulate_dx = 1 into dX, dW*, db* that hold a constant.  dx_rows: the data-only
    cgs_mlp2_backward_rows through a shuffled row table into a larger pre-loaded dX, then cgs_mlp2_wgrad.  recompute: the backward
    without the saved hidden layer (the two tiny-output shapes).  What remains is the constant plus the gradient."""
    from contextgs_amd import _lib
    L = _lib.lib()
    in_f, hid, out, act = cfg
    n, CX, CW = 513, np.float32(0.25), np.float32(-0.5)
    c, ref = mr.draw(cfg, n), mr.ref_of(cfg, n)
    what, mx = (cfg, route), _maxima("C ABI")
    x, W1, b1, W2, b2, dy = (T(t) for t in (c.x, c.W1, c.b1, c.W2, c.b2, c.dy))
    stream = _lib.current_stream()
    y, h = _buf(n, out), _buf(n, hid)
    _lib.check(L.cgs_mlp2_forward(in_f, hid, out, act, _lib.ptr(x), in_f, _lib.ptr(W1), _lib.ptr(b1), _lib.ptr(W2), _lib.ptr(b2),
                                  _lib.ptr(y), out, _lib.ptr(h), n, stream), "cgs_mlp2_forward")
    got = dict(y=_body(y, n, out), h=_body(h, n, hid))
    n_dst = n + 100 if route == "dx_rows" else n
    table = np.random.default_rng(3).permutation(n_dst)[:n].astype(np.int64) if route == "dx_rows" else np.arange(n)
    dX, dz1, dz2 = _buf(n_dst, in_f), _buf(n, hid), _buf(n, out)
    dX[:n_dst * in_f] = float(CX)
    dW = [torch.full(s, float(CW), dtype=torch.float32, device="cuda") for s in ((hid, in_f), (hid,), (out, hid), (out,))]
    ws = torch.empty(int(L.cgs_mlp_wgrad_scratch_bytes()), dtype=torch.uint8, device="cuda")
    p_dz2 = _lib.ptr(dz2) if act else None
    p_y = _lib.ptr(y) if act else None
    if route == "dx_rows":
        tab = T(table)
        _lib.check(L.cgs_mlp2_backward_rows(in_f, hid, out, act, _lib.ptr(x), in_f, _lib.ptr(W1), None, _lib.ptr(W2), p_y, _lib.ptr(dy), out,
                                            _lib.ptr(h), _lib.ptr(dX), in_f, 1, _lib.ptr(tab), _lib.ptr(dz1), p_dz2, None, None, None, None,
                                            n, _lib.ptr(ws), ws.numel(), stream), "cgs_mlp2_backward_rows")
        _lib.check(L.cgs_mlp2_wgrad(in_f, hid, out, _lib.ptr(x), in_f, _lib.ptr(h), p_dz2 if act else _lib.ptr(dy), out, _lib.ptr(dz1),
                                    *[_lib.ptr(t) for t in dW], n, _lib.ptr(ws), ws.numel(), stream), "cgs_mlp2_wgrad")
    else:
        p_h = None if route == "recompute" else _lib.ptr(h)
        _lib.check(L.cgs_mlp2_backward(in_f, hid, out, act, _lib.ptr(x), in_f, _lib.ptr(W1), _lib.ptr(b1), _lib.ptr(W2), p_y, _lib.ptr(dy), out,
                                       p_h, _lib.ptr(dX), in_f, 1, _lib.ptr(dz1), p_dz2, *[_lib.ptr(t) for t in dW], n, _lib.ptr(ws),
                                       ws.numel(), stream), "cgs_mlp2_backward")
    got["dz1"] = _body(dz1, n, hid)
    if act:
        got["dz2"] = _body(dz2, n, out)
    else:
        assert bool((dz2 == SENTINEL).all())
    mr.judge(ref, got, mx, what)
    dxb = _body(dX, n_dst, in_f)
    want = CX + ref.values["dx"]
    _judge(dxb[table], want, ref.units["dx"] + U * np.abs(want), mx, "dx", what)
    untouched = np.ones(n_dst, bool)
    untouched[table] = False
    assert (dxb[untouched] == CX).all() and (dxb[table][~ref.live] == CX).all()
    for k, t in zip(("dW1", "db1", "dW2", "db2"), dW):
        want = CW + ref.values[k]
        _judge(_np(t), want, ref.units[k] + U * np.abs(want), mx, k, what)
