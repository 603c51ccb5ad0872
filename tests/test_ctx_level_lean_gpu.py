"""The fused level kernels (csrc/ctx_level.hip) after they shed work the result does not need: a 32-bit element index for the
noise (ctx_noise_k32) instead of 64-bit index arithmetic whose high word is always zero.  It may not move a bit, and no later
change of these kernels' schedule or descriptors may drop a store or let one through that a descriptor's bounds check drops.

cgs_ctx_level_fwd_h / _bwd_h through the C ABI, in_dim 71 and 15, n = 1, 16, 17, grid + 5 and 2 grid + 5 rows (grid = 16 rows x 4
waves x CU: the last two give every wave of the backward a second trip through its tile loop and a ragged last tile), the rate
side, d_hyp_rows and dQ_ext each given and NULL.

  - the forward's y = x[rows] + u Q with u from oracle.context_ref.ctx_noise (the 64-bit statement), torch.equal, at the largest n:
    element indices up to 50 (2 grid + 5), past 2^20 at 256 CUs;
  - two calls on the same inputs give the same bits (dW1 / db1 / dW2q / db2q included);
  - every output equals the HS = false entry points' (cgs_ctx_level_fwd / _bwd2);
  - n = 17 with NaN-filled outputs one row longer than needed: the rows that exist are written, finite; nothing else is touched.

The operand builder and the launch wrappers of tests/test_ctx_level_hidden_gpu.py are reused where they fit (same shapes, shared cache).
"""
import itertools

import pytest
import torch

from test_ctx_level_hidden_gpu import N_KINDS, Q0, SEED, _bwd, _fwd, _n_rows, _new_h, _operands

pytestmark = pytest.mark.gpu
WIDTHS = (("yf", "xf", 50), ("ys", "xs", 6), ("yo", "xo", 30))


@pytest.mark.parametrize("in_dim", [71, 15])
def test_noise_of_the_forward_is_the_oracles_64_bit_statement(in_dim):
    from oracle.context_ref import ctx_noise
    n = _n_rows("2grid+5")
    assert 50 * n > 1 << 20
    o = _operands(n, in_dim)
    H, _ = _new_h(n)
    f = _fwd(o, H, "fwd_h")
    for k, (y, x, w) in enumerate(WIDTHS):
        u = torch.from_numpy(ctx_noise(SEED, k, n * w).reshape(n, w)).to("cuda")
        assert torch.equal(f[y], o[x][o["rows"]] + u * f["Q"][:, k:k + 1]), y


@pytest.mark.parametrize("in_dim", [71, 15])
@pytest.mark.parametrize("kind", N_KINDS)
def test_same_bits_twice_and_the_bits_of_the_recompute_path(kind, in_dim):
    o = _operands(_n_rows(kind), in_dim)
    ref = _fwd(o, None, "fwd")
    H, H2 = _new_h(o["n"])[0], _new_h(o["n"])[0]
    f, f2 = _fwd(o, H, "fwd_h"), _fwd(o, H2, "fwd_h")
    assert torch.equal(H, H2)
    for k in ("X", "yf", "ys", "yo", "Q"):
        assert torch.equal(f[k], f2[k]), k
        assert torch.equal(f[k], ref[k]), k
    for side, dhyp, dqe in itertools.product((True, False), repeat=3):
        rb = _bwd(o, f["X"], None, side, dhyp, dqe)
        b, b2 = _bwd(o, f["X"], H, side, dhyp, dqe), _bwd(o, f["X"], H, side, dhyp, dqe)
        assert set(b) == set(rb) == set(b2)
        for k in rb:
            assert torch.equal(b[k], b2[k]), ("twice", k, side, dhyp, dqe)
            assert torch.equal(b[k], rb[k]), ("recompute", k, side, dhyp, dqe)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _written_rows_only(buf, rows, name):
    """rows `rows` of buf hold finite values, every other element is still NaN"""
    hit = torch.zeros(buf.shape[0], dtype=torch.bool, device=buf.device)
    hit[rows] = True
    assert bool(torch.isfinite(buf[hit]).all()), name + ": a piece of a valid row was not written"
    assert bool(torch.isnan(buf[~hit]).all()), name + ": a row that does not exist (or is not named) was written"


@pytest.mark.parametrize("in_dim", [71, 15])
def test_valid_rows_are_written_and_the_row_behind_them_is_not(in_dim):
    """n = 17, output buffers one row longer than the kernels are told: the last tile's 15 missing rows and the extra row
    are dropped by the descriptors' bounds checks, the 17 that exist arrive whole."""
    from contextgs_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n = 17
    o = _operands(n, in_dim)
    N, ctxl, st = o["N"], in_dim == 71, _lib.current_stream()
    X, yf, ys, yo, Q = _nan(n + 1, in_dim), _nan(n + 1, 50), _nan(n + 1, 6), _nan(n + 1, 30), _nan(n + 1, 3)
    H, nb = _new_h(n, tail=4096, fill=float("nan"))
    sums = torch.zeros(int(L.cgs_means_accum_doubles()), dtype=torch.float64, device="cuda")
    _lib.check(L.cgs_ctx_level_fwd_h(
        in_dim, p(o["anchor"]), N, p(o["a_rows"]), None if ctxl else p(o["a_mask"]), p(o["base_f"]) if ctxl else None,
        p(o["base_s"]) if ctxl else None, o["n_par"] if ctxl else 0, p(o["pos"]) if ctxl else None, p(o["hyp"]), n, p(o["W1"]), p(o["b1"]),
        p(o["W2q"]), p(o["b2q"]), p(o["xf"]), p(o["xs"]), p(o["xo"]), p(o["rows"]), SEED, *Q0, p(X), p(yf), p(ys), p(yo), p(Q), p(sums),
        p(H[:nb]), st), "fwd_h")
    live = torch.arange(n, device="cuda")
    for name, buf in (("X", X), ("yf", yf), ("ys", ys), ("yo", yo), ("Q", Q)):
        _written_rows_only(buf, live, name)
    assert bool((H[nb:] == 0xA5).all()) and bool(torch.isfinite(H[:nb].view(torch.float32)).all())
    ref = _fwd(o, None, "fwd")
    for name, buf in (("X", X), ("yf", yf), ("ys", ys), ("yo", yo), ("Q", Q)):
        assert torch.equal(buf[:n], ref[name]), name

    dxf, dxs, dxo, dh, dX = _nan(N + 1, 50), _nan(N + 1, 6), _nan(N + 1, 30), _nan(N + 1, 12), _nan(n + 1, in_dim)
    dW1, db1, dW2q, db2q = torch.ones(100, in_dim, device="cuda"), torch.ones(100, device="cuda"), torch.ones(3, 100, device="cuda"), \
        torch.ones(3, device="cuda")
    ws = torch.empty(int(L.cgs_ctx_level_bwd_scratch_bytes()), dtype=torch.uint8, device="cuda")
    _lib.check(L.cgs_ctx_level_bwd_h(
        in_dim, p(X), p(o["W1"]), p(o["b1"]), p(o["W2q"]), p(o["b2q"]), p(o["dyf"]), p(o["dys"]), p(o["dyo"]), p(o["dQe"]), n, SEED, *Q0,
        p(o["rows"]), N, p(dxf), p(dxs), p(dxo), p(o["smap"]), o["m"], p(o["sf"]), p(o["ss"]), p(o["so"]), p(o["sQ"]), p(o["dxsub"]), p(dX),
        p(dh), p(dW1), p(db1), p(dW2q), p(db2q), p(H[:nb]), p(ws), ws.numel(), st), "bwd_h")
    _written_rows_only(dX, live, "dX")
    for name, buf in (("dxf", dxf), ("dxs", dxs), ("dxo", dxo), ("d_hyp_rows", dh)):
        _written_rows_only(buf, o["rows"], name)
    rb = _bwd(o, ref["X"], None, True, True, True)
    got = dict(dX=dX[:n], dxf=dxf[:N], dxs=dxs[:N], dxo=dxo[:N], d_hyp_rows=dh[:N], dW1=dW1, db1=db1, dW2q=dW2q, db2q=db2q)
    named = o["rows"]
    for k, v in got.items():
        assert bool(torch.isfinite(v[named] if k in ("dxf", "dxs", "dxo", "d_hyp_rows") else v).all()), k
        if k in ("dxf", "dxs", "dxo", "d_hyp_rows"):
            assert torch.equal(v[named], rb[k][named]), k
        else:
            assert torch.equal(v, rb[k]), k
