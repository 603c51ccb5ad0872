"""The fused level kernels (csrc/ctx_level.hip) per element against float64 (tests/ctx_level_ref.py: the statement, the error unit of
every element, the equalities, the inputs by regime), through the C ABI, on every trip of their tile loops:
  a. cgs_ctx_level_fwd_h + cgs_ctx_level_bwd_h (the hidden layer handed over) at 1, 15, 16, 17 rows (tile edge), 65 (the backward's
     4-wave workgroup + 1), 129 (the forward's 8-wave workgroup + 1), 64 CUs + 5 (the backward's second trip, ragged) and
     256 CUs + 17 (the forward's second trip - operands that arrive by the prefetch - and the backward's fifth); at the two large
     counts also with cotangents that are nonzero on ~600 rows, so that a weight gradient sums ~600 terms
  b. cgs_ctx_level_fwd + cgs_ctx_level_bwd2 (the recompute) at 17 rows and the two large counts
  c. cgs_ctx_level_bwd at 129 rows
  d. every optional operand NULL, one at a time, at 17 rows and at 64 CUs + 5 (each of them given: a.)
Both in_dim everywhere.  Every output of every call is judged: X bit for bit, Q, y (against fp64 AND as the fp32 equality
x[rows] + noise Q_kernel), the three sums, the hand-over's hidden layer and tanh values (decoded from the layout ctx_level.hip
documents; every value of its whole tiles finite), dx (equalities, around a pre-loaded constant), dX, d_hyp_rows (an equality with dX,
around a constant), the four weight gradients (accumulated onto a constant) - each element within UNITS_KERNEL_LEVEL units; X, y, Q
and dX are one row longer than n and the extra row keeps its sentinel.

UNITS_KERNEL_LEVEL = 2 max(UNITS_LITERAL_LEVEL, mlp_ref.UNITS_LITERAL) = 2 max(5.6, 6.6) = 13.2 units; both literals are measured on the
CPU (tests/test_ctx_level_ref.py, tests/test_mlp_ref.py), neither number is taken from a kernel's result.

Measured maxima in units (MI355X, 256 CUs; "-": not an output of that entry point; the literals' rows are ctx_level_ref.py's; dX_own:
dX against the cotangent it carries itself, in units of the dX product alone, ctx_level_ref.own_cotangent):
                                        h      t      Q     yf     ys     yo   sums     dX dX_own    dW1    db1   dW2q   db2q
  literal (a) torch, CPU            5.305  1.445  1.053  1.005  0.999  0.995  0.528  1.170  2.353  0.442  0.425  0.442  0.127
  literal (b) sequential            5.580  1.445  1.138  1.058  0.999  0.995  1.906  1.570  2.336  0.461  0.367  0.473  0.288
  literal (c) mlp_frag.h's order    3.880  0.989  0.989  0.992  0.999  0.995  0.141  1.072  1.128  0.581  0.282  0.527  0.119
  fwd_h + bwd_h (20)                5.439  0.771  0.704  0.995  0.999  0.995  0.335  0.974  2.701  0.985  0.946  0.980  0.947
  fwd + bwd2 (10)                       -      -  0.704  0.995  0.999  0.995  0.091  0.974  2.701  0.908  0.804  0.917  0.338
  fwd + bwd (2)                         -      -  0.597  0.902  0.963  0.944  0.030  0.716  1.356  0.622  0.353  0.618  0.228
  optional operands (36)            5.083  0.771  0.642  0.991  0.999  0.995  0.091  0.973  2.688  0.973  0.804  0.962  0.584
The kernels' largest figure is 5.439 (h), 0.14 below the literals' own maximum of 5.580 and 7.8 below the bound of 13.2; every
quantity but dX_own (2.701 against the literals' 2.353) and the weight gradients (0.985 against 0.581: the kernels add workgroup
partials) stays below what the literals need.  No element of any output failed: no kernel had to change.  The slowest test takes
2.3 s (256 CUs + 17 rows, in_dim 71, dense cotangents: the float64 reference of 65 553 rows).

That the tests bite (each alteration built once into a copy of the library outside the source tree, this file and
tests/test_ctx_level_gpu.py run once on it in a call of its own; arithmetic only, no index, bound, address or descriptor changed;
this file has 68 tests, tests/test_ctx_level_gpu.py 14):
  (i)   the backward's ReLU gate `acc1[t][r] >= 0.f`: all 68 fail here; test_ctx_level_gpu.py: 8 of 14 fail
        (test_level_kernels_against_a_torch_statement 4 / 4, test_fused_level_equals_the_separate_launches 4 / 4): `>=` opens every
        closed unit, since the gate reads max(z1, 0).
  (ii)  `(1.f - t0 * t0)` of the first head times 1 + 2^-17: 41 fail here (dX at 14 to 23 units: every case of 65 rows and more
        on every entry point, and one of 17 rows - dyf NULL at in_dim 15); test_ctx_level_gpu.py passes all 14.  The factor is
        128 u on the first head's d qadj, whose own unit is 6 to 8 u: it shows where that head dominates an element of dX, which
        among 17 rows or fewer it rarely does.
  (iii) the W1n4 image staged with its low six mantissa bits cleared: 63 fail here, on dX_own at 14 to 22 units (the 5 that pass:
        1 row at both in_dim, and 15, 16 and 65 rows at in_dim 15); test_ctx_level_gpu.py passes all 14.  A FINDING of the first
        run: judged in dX's unit alone this alteration passed BOTH files (82 / 82), because that unit is mostly the 6 to 8 u |d qadj| the cotangent carries, and up
        to 64 u on each weight of a ~50-term signed sum is 64 / sqrt(50) of the product's own unit, a few of dX's.  The statement was
        sharpened, not the bound: dX_own judges dX against the best cotangent in the span it must lie in, in units of the product
        alone (tests/test_ctx_level_ref.py repeats the alteration on the CPU: 15 to 22 units there).
  (iv)  `aw1` zeroed at the top of a wave's second tile-loop trip (a dropped trip of dW1): 34 fail here, on dW1, exactly the
        cases of 64 CUs + 5 and 256 CUs + 17 rows (hand-over 8 / 8, recompute 8 / 8, optional operands 18 / 18 at 64 CUs + 5), none
        below: the second-trip cases do their job; test_ctx_level_gpu.py: 1 of 14 fails (test_fused_level_equals_the_separate_launches
        at 50 021 anchors).
  ((ii) and (iv) were run once more after dX_own was added: the same 41 and 34 + 1 tests fail.  (i) was run before it only: every
  test of this file already failed there.)
"""
import numpy as np
import pytest
import torch

import ctx_level_ref as lr
import mlp_ref as mr
from ctx_level_ref import NAMES, Q0, SEED, UNITS_KERNEL_LEVEL, WIDTHS

pytestmark = pytest.mark.gpu
SENTINEL, C_DX, C_HYP, C_W = -7.25, 7.0, 9.0, -0.5
HT_FLOATS = 1664                       # CL_HT_BYTES / 4: six 1 KB fragments, 256 B of units 96..99, 256 B of tanh values
KINDS = ("1", "15", "16", "17", "65", "129", "64cu+5", "256cu+17")
MAXIMA = {}


def _cus():
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def _n(kind):
    big = dict(zip(("64cu+5", "256cu+17"), lr.large_counts(_cus())))
    return big[kind] if kind in big else int(kind)


def _np(t):
    return t.detach().cpu().numpy()


def _maxima(entry):
    return MAXIMA.setdefault(entry, mr.Maxima())


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for entry, m in MAXIMA.items():
        print(f"[level-units] {entry:24s}" + "".join(f" {k} {v:.3f}" for k, v in m.m.items()))


# ---- operands and references, one per shape ---------------------------------------------------------------------------------------
_DEV, _FWD, _BWD = {}, {}, {}
ARRAYS = ("anchor", "base_f", "base_s", "hyp", "a_mask", "a_rows", "pos", "W1", "b1", "W2q", "b2q", "xf", "xs", "xo", "rows", "dyf", "dys", "dyo",
          "dQe", "side_map", "side_f", "side_s", "side_o", "side_Q", "dx_sub")


def _case(kind, in_dim, sparse):
    c = lr.draw(_n(kind), in_dim, sparse, _cus())
    key = (c.n, in_dim, sparse)
    if key not in _DEV:
        if c.n > 5000:
            for k in [k for k in _DEV if k[0] > 5000]:
                del _DEV[k]
        _DEV[key] = {k: torch.from_numpy(np.array(getattr(c, k))).cuda() for k in ARRAYS}
    return c, _DEV[key]


def _keep(cache, key, make, big):
    """One reference of a large count at a time (hundreds of MB each); the small ones stay."""
    if key not in cache:
        if big:
            for k in [k for k in cache if k[0] > 5000]:
                del cache[k]
        cache[key] = make()
    return cache[key]


def _fwd_ref(c, mask=True):
    return _keep(_FWD, (c.n, c.in_dim, c.sparse, mask), lambda: lr.Forward(c, mask), c.n > 5000)


def _bwd_ref(c, f, **opt):
    key = (c.n, c.in_dim, c.sparse, f.mask, tuple(sorted(opt.items())))
    return _keep(_BWD, key, lambda: lr.Backward(f, **opt), c.n > 5000)


# ---- the calls --------------------------------------------------------------------------------------------------------------------
def _tail(rows, width):
    """[rows + 1, width] filled with the sentinel: the kernels write rows `rows`, the last one stays."""
    return torch.full((rows + 1, width), SENTINEL, dtype=torch.float32, device="cuda")


def _body(t, rows, what):
    assert bool((t[rows:] == SENTINEL).all()), (what, "the row behind the last one changed")
    return _np(t[:rows])


def _forward(c, d, entry, mask=True, sums=True):
    """cgs_ctx_level_fwd ("fwd") or cgs_ctx_level_fwd_h with a hand-over buffer ("fwd_h") -> the outputs as numpy, H as a tensor."""
    from contextgs_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n, in_dim = c.n, c.in_dim
    ctxl = in_dim == 71
    X = _tail(n, in_dim)
    yf, ys, yo, Q = (_tail(n, w) for w in WIDTHS + (3,))
    acc = torch.zeros(int(L.cgs_means_accum_doubles()), dtype=torch.float64, device="cuda") if sums else None
    head = (in_dim, p(d["anchor"]), c.N, p(d["a_rows"]), p(d["a_mask"]) if (mask and not ctxl) else None, p(d["base_f"]) if ctxl else None,
            p(d["base_s"]) if ctxl else None, c.n_par if ctxl else 0, p(d["pos"]) if ctxl else None, p(d["hyp"]), n, p(d["W1"]), p(d["b1"]),
            p(d["W2q"]), p(d["b2q"]), p(d["xf"]), p(d["xs"]), p(d["xo"]), p(d["rows"]), SEED, *Q0, p(X), p(yf), p(ys), p(yo), p(Q), p(acc))
    H = None
    if entry == "fwd":
        _lib.check(L.cgs_ctx_level_fwd(*head, _lib.current_stream()), "fwd")
    else:
        tiles = (n + 15) // 16
        assert int(L.cgs_ctx_level_hidden_bytes(n)) == tiles * HT_FLOATS * 4
        H = torch.full((tiles * HT_FLOATS + 64,), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(L.cgs_ctx_level_fwd_h(*head, p(H), _lib.current_stream()), "fwd_h")
    out = dict(X=_body(X, n, "X"), Q=_body(Q, n, "Q"), yf=_body(yf, n, "yf"), ys=_body(ys, n, "ys"), yo=_body(yo, n, "yo"))
    if sums:
        out["sums"] = _np(acc.view(-1, 16)[:, :3].sum(0))
        assert bool((acc.view(-1, 16)[:, 3:] == 0).all())
    return out, X, H


def _decode_hand_over(H, n):
    """h [16 tiles, 100] and tanh(qadj) [16 tiles, 3] from the fragment-major layout (ctx_level.hip, CL_HT_BYTES): per tile six 1 KB
    fragments in lane order (lane 16 g + c: units 16 t + 4 g + {0..3} of row c), then units 96..99 of row c at 16 c bytes and
    (tanh 0..2, 0) of row c at 256 + 16 c."""
    tiles = (n + 15) // 16
    assert bool(torch.isnan(H[tiles * HT_FLOATS:]).all()), "the forward wrote behind cgs_ctx_level_hidden_bytes(n)"
    body = H[:tiles * HT_FLOATS]
    assert bool(torch.isfinite(body).all()), "a piece of a whole tile of the hand-over is not finite"
    body = _np(body).reshape(tiles, HT_FLOATS)
    main = body[:, :1536].reshape(tiles, 6, 4, 16, 4).transpose(0, 3, 1, 2, 4).reshape(tiles * 16, 96)
    last = body[:, 1536:1600].reshape(tiles * 16, 4)
    th = body[:, 1600:1664].reshape(tiles * 16, 4)
    assert (th[:, 3] == 0).all()
    return np.concatenate([main, last], axis=1), th[:, :3]


def _judge_forward(c, f, out, H, mx, what, sums=True):
    assert np.array_equal(out["X"].view(np.uint32), f.X.view(np.uint32)), (what, "X is not the gathered row, bit for bit")
    got = {k: out[k] for k in ("Q", "yf", "ys", "yo") + (("sums",) if sums else ())}
    if H is not None:
        h, th = _decode_hand_over(H, c.n)
        got["h"], got["t"] = h[:c.n], th[:c.n]
        assert (h[:c.n][~f.trunk.gate] == 0).all(), (what, "h not 0 behind a closed gate")
    lr.judge(f, got, mx, what)
    for k, y in enumerate(f.y_from(out["Q"])):
        assert np.array_equal(out["y" + NAMES[k]], y), (what, "y" + NAMES[k], "is not x[rows] + noise * Q of the kernel's own Q")
    sat = f.head.flat & (f.head.qadj < 0)
    assert (out["Q"][sat] == np.float32(1e-9)).all(), (what, "Q of a saturated row is not the clamp")


def _backward(c, d, X, H, entry, dy=(True, True, True), dqe=True, side=True, dx_sub=True, dhyp=True):
    """cgs_ctx_level_bwd_h (H given), cgs_ctx_level_bwd2 or cgs_ctx_level_bwd on fresh pre-loaded outputs."""
    from contextgs_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n, N, in_dim = c.n, c.N, c.in_dim
    dx = [torch.full((N, w), C_DX, dtype=torch.float32, device="cuda") for w in WIDTHS]
    dX = _tail(n, in_dim)
    dh = torch.full((N, 12), C_HYP, dtype=torch.float32, device="cuda") if dhyp else None
    dW = [torch.full(s, C_W, dtype=torch.float32, device="cuda") for s in ((100, in_dim), (100,), (3, 100), (3,))]
    ws = torch.empty(int(L.cgs_ctx_level_bwd_scratch_bytes()), dtype=torch.uint8, device="cuda")
    sd = [p(d[k]) if side else None for k in ("side_f", "side_s", "side_o", "side_Q")] + [p(d["dx_sub"]) if (side and dx_sub) else None]
    head = (in_dim, p(X), p(d["W1"]), p(d["b1"]), p(d["W2q"]), p(d["b2q"]), *[p(d["dy" + nm]) if g else None for nm, g in zip(NAMES, dy)],
            p(d["dQe"]) if dqe else None, n, SEED, *Q0, p(d["rows"]), N, *[p(t) for t in dx], p(d["side_map"]) if side else None,
            c.m if side else 0, *sd, p(dX))
    tail = tuple(p(t) for t in dW)
    if entry == "bwd":
        assert not dhyp and H is None
        _lib.check(L.cgs_ctx_level_bwd(*head, *tail, p(ws), ws.numel(), _lib.current_stream()), "bwd")
    elif entry == "bwd2":
        assert H is None
        _lib.check(L.cgs_ctx_level_bwd2(*head, p(dh), *tail, p(ws), ws.numel(), _lib.current_stream()), "bwd2")
    else:
        _lib.check(L.cgs_ctx_level_bwd_h(*head, p(dh), *tail, p(H), p(ws), ws.numel(), _lib.current_stream()), "bwd_h")
    out = dict(dx=[_np(t) for t in dx], dX=_body(dX, n, "dX"), dW1=_np(dW[0]), db1=_np(dW[1]), dW2q=_np(dW[2]), db2q=_np(dW[3]))
    out["d_hyp_rows"] = _np(dh) if dhyp else None
    return out


def _judge_backward(c, b, out, mx, what):
    named = np.zeros(c.N, bool)
    named[c.rows] = True
    for k, nm in enumerate(NAMES):
        got = out["dx"][k]
        assert np.array_equal(got[c.rows], b.dx[k]), (what, "dx" + nm, "is not dy (+ the side row): one fp32 add")
        assert (got[~named] == C_DX).all(), (what, "dx" + nm, "a row no level row names changed")
    lr.judge(b, {k: out[k] for k in ("dX", "dW1", "db1", "dW2q", "db2q")}, mx, what, preload=C_W)
    dead = ~b.trunk.live & (c.side_map < 0)
    assert (out["dX"][dead] == 0).all(), (what, "dX not 0 on a row whose cotangent is 0")
    dh = out["d_hyp_rows"]
    if dh is not None:
        assert np.array_equal(dh[c.rows].view(np.uint32), out["dX"][:, c.in_dim - 12:].view(np.uint32)), (what, "d_hyp_rows is not dX's last 12 columns")
        assert (dh[~named] == C_HYP).all(), (what, "d_hyp_rows: a row no level row names changed")


def _run(kind, in_dim, sparse, fwd_entry, bwd_entry, entry_name, mask=True, sums=True, **opt):
    c, d = _case(kind, in_dim, sparse)
    what = (entry_name, c.n, in_dim, "sparse" if sparse else "dense", mask, sums, tuple(sorted(opt.items())))
    mx = _maxima(entry_name)
    f = _fwd_ref(c, mask)
    out, X, H = _forward(c, d, fwd_entry, mask, sums)
    _judge_forward(c, f, out, H, mx, what, sums)
    ref_opt = {k: v for k, v in opt.items() if k != "dhyp"}
    b = _bwd_ref(c, f, **ref_opt)
    got = _backward(c, d, X, H, bwd_entry, **opt)
    _judge_backward(c, b, got, mx, what)


# ---- a. the hand-over path, every count ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim", [71, 15])
@pytest.mark.parametrize("kind,sparse", [(k, False) for k in KINDS] + [(k, True) for k in KINDS[-2:]])
def test_hand_over_path_every_element(kind, sparse, in_dim):
    _run(kind, in_dim, sparse, "fwd_h", "bwd_h", "fwd_h + bwd_h")


# ---- b. the recompute path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim", [71, 15])
@pytest.mark.parametrize("kind,sparse", [("17", False), ("64cu+5", False), ("256cu+17", False), ("64cu+5", True), ("256cu+17", True)])
def test_recompute_path_every_element(kind, sparse, in_dim):
    _run(kind, in_dim, sparse, "fwd", "bwd2", "fwd + bwd2")


# ---- c. the entry point without d_hyp_rows --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim", [71, 15])
def test_bwd_entry_point_every_element(in_dim):
    _run("129", in_dim, False, "fwd", "bwd", "fwd + bwd", dhyp=False)


# ---- d. the optional operands ---------------------------------------------------------------------------------------------------------
OPTIONAL = {"a_mask": dict(mask=False), "sums": dict(sums=False), "dQ_ext": dict(dqe=False), "side_map": dict(side=False),
            "dx_sub": dict(dx_sub=False), "d_hyp_rows": dict(dhyp=False), "dyf": dict(dy=(False, True, True)),
            "dys": dict(dy=(True, False, True)), "dyo": dict(dy=(True, True, False))}


@pytest.mark.parametrize("in_dim", [71, 15])
@pytest.mark.parametrize("kind", ["17", "64cu+5"])
@pytest.mark.parametrize("null", list(OPTIONAL))
def test_each_optional_operand_null(null, kind, in_dim):
    """A NULL cotangent is zeros, a NULL side map no rate subset, a NULL dx_sub no extra input gradient, NULL sums / d_hyp_rows drop
    the stores, a NULL a_mask (in_dim 15; in_dim 71 ignores the mask: the call passes none either way) the unmasked anchor."""
    _run(kind, in_dim, False, "fwd_h", "bwd_h", "optional operands", **OPTIONAL[null])
