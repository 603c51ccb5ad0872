"""The hidden layer's hand-over of the fused level kernels (csrc/ctx_level.hip): cgs_ctx_level_fwd_h writes relu(W1 X + b1) and the
tanh of the step-size outputs per 16-row tile, cgs_ctx_level_bwd_h reads them instead of recomputing them from X.

The reference is the recompute path — cgs_ctx_level_fwd / cgs_ctx_level_bwd2, whose kernels this change leaves as they were — and
the statement is bit equality: the hand-over carries the very registers the recompute forms, and every product and sum behind them
is the same instruction sequence.  (The recompute path itself is judged per element against float64 in
tests/test_ctx_level_fp64_gpu.py, on every trip of the tile loops; the operands here are built like the C-ABI test of
tests/test_ctx_level_gpu.py, whose builder is inline there, so only its helpers are imported.)

Row counts: every wave of the backward's grid (one workgroup of 4 waves per CU) with zero, one and two tiles, and a ragged last tile.
"""
import itertools

import pytest
import torch

from test_ctx_level_gpu import T  # noqa: F401  (the suite's device helper; keeps the two files on the same import path)

pytestmark = pytest.mark.gpu
SEED, Q0 = 0x5DEECE66D, (1.0, 0.001, 0.2)
N_KINDS = ("one", "tile", "tile+1", "grid+5", "2grid+5")


def _n_rows(kind):
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    return {"one": 1, "tile": 16, "tile+1": 17, "grid+5": 16 * 4 * cu + 5, "2grid+5": 2 * 16 * 4 * cu + 5}[kind]


_OPS = {}


def _operands(n, in_dim):
    """Random operands of one level (shared by the tests of a shape; nothing writes to them)."""
    key = (n, in_dim)
    if key in _OPS:
        return _OPS[key]
    dev = "cuda"
    gen = torch.Generator(device="cpu").manual_seed(7 * n + in_dim)
    R = lambda *s: torch.randn(*s, generator=gen).to(dev)
    N, n_par = n + 11, max(1, n // 3)
    o = dict(n=n, N=N, n_par=n_par, in_dim=in_dim)
    o["anchor"], o["hyp"] = R(N, 3), R(n, 12)
    o["a_rows"] = torch.randperm(N, generator=gen)[:n].to(dev)
    o["a_mask"] = (torch.rand(N, generator=gen) < 0.7).to(dev).view(torch.uint8)
    o["base_f"], o["base_s"] = R(n_par, 50), R(n_par, 6)
    o["pos"] = torch.randint(0, n_par, (n,), generator=gen).to(dev)
    o["W1"], o["b1"], o["W2q"], o["b2q"] = R(100, in_dim) * 0.2, R(100) * 0.1, R(3, 100) * 0.1, R(3) * 0.1
    o["xf"], o["xs"], o["xo"] = R(N, 50), R(N, 6), R(N, 30)
    o["rows"] = torch.randperm(N, generator=gen)[:n].to(dev)
    o["dyf"], o["dys"], o["dyo"], o["dQe"] = R(n, 50), R(n, 6), R(n, 30), R(n, 3)
    m = max(1, int(round(0.15 * n)))                        # the rate side: ~15 % of the rows
    sub = torch.randperm(n, generator=gen)[:m].to(dev)
    smap = torch.full((n,), -1, dtype=torch.int32, device=dev)
    smap[sub] = torch.arange(m, dtype=torch.int32, device=dev)
    o["m"], o["smap"] = m, smap
    o["sf"], o["ss"], o["so"], o["sQ"], o["dxsub"] = R(m, 50), R(m, 6), R(m, 30), R(m, 3), R(m, in_dim)
    _OPS[key] = o
    return o


def _fwd(o, H, entry, mask=True):
    """One forward through `entry` ("fwd": cgs_ctx_level_fwd, "fwd_h": cgs_ctx_level_fwd_h with H, which may be None)."""
    from contextgs_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n, in_dim, dev = o["n"], o["in_dim"], "cuda"
    ctxl = in_dim == 71
    X = torch.empty(n, in_dim, device=dev)
    yf, ys, yo, Q = (torch.empty(n, w, device=dev) for w in (50, 6, 30, 3))
    sums = torch.zeros(int(L.cgs_means_accum_doubles()), dtype=torch.float64, device=dev)
    head = (in_dim, p(o["anchor"]), o["N"], p(o["a_rows"]), p(o["a_mask"]) if (mask and not ctxl) else None,
            p(o["base_f"]) if ctxl else None, p(o["base_s"]) if ctxl else None, o["n_par"] if ctxl else 0, p(o["pos"]) if ctxl else None,
            p(o["hyp"]), n, p(o["W1"]), p(o["b1"]), p(o["W2q"]), p(o["b2q"]), p(o["xf"]), p(o["xs"]), p(o["xo"]), p(o["rows"]), SEED, *Q0,
            p(X), p(yf), p(ys), p(yo), p(Q), p(sums))
    if entry == "fwd":
        _lib.check(L.cgs_ctx_level_fwd(*head, _lib.current_stream()), "fwd")
    else:
        _lib.check(L.cgs_ctx_level_fwd_h(*head, p(H), _lib.current_stream()), "fwd_h")
    return dict(X=X, yf=yf, ys=ys, yo=yo, Q=Q, sums=sums.view(-1, 16)[:, :3].sum(0))


def _new_h(n, tail=0, fill=None):
    from contextgs_amd import _lib
    nb = int(_lib.lib().cgs_ctx_level_hidden_bytes(n))
    assert nb == ((n + 15) // 16) * 6656
    buf = torch.empty(nb + tail, dtype=torch.uint8, device="cuda")
    if fill is not None:
        buf[:nb].view(torch.float32).fill_(fill)
    if tail:
        buf[nb:] = 0xA5
    return buf, nb


def _bwd(o, X, H, side, dhyp, dqe):
    """cgs_ctx_level_bwd_h with the hand-over H, or cgs_ctx_level_bwd2 (H None), on fresh pre-filled outputs."""
    from contextgs_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n, N, in_dim, dev = o["n"], o["N"], o["in_dim"], "cuda"
    dxf, dxs, dxo = (torch.full((N, w), 7.0, device=dev) for w in (50, 6, 30))
    dX = torch.full((n, in_dim), 5.0, device=dev)
    dh = torch.full((N, 12), 9.0, device=dev) if dhyp else None
    dW1, db1, dW2q, db2q = torch.ones(100, in_dim, device=dev), torch.ones(100, device=dev), torch.ones(3, 100, device=dev), \
        torch.ones(3, device=dev)
    ws = torch.empty(int(L.cgs_ctx_level_bwd_scratch_bytes()), dtype=torch.uint8, device=dev)
    sd = [p(o[k]) if side else None for k in ("sf", "ss", "so", "sQ", "dxsub")]
    head = (in_dim, p(X), p(o["W1"]), p(o["b1"]), p(o["W2q"]), p(o["b2q"]), p(o["dyf"]), p(o["dys"]), p(o["dyo"]),
            p(o["dQe"]) if dqe else None, n, SEED, *Q0, p(o["rows"]), N, p(dxf), p(dxs), p(dxo), p(o["smap"]) if side else None,
            o["m"] if side else 0, *sd, p(dX), p(dh), p(dW1), p(db1), p(dW2q), p(db2q))
    if H is None:
        _lib.check(L.cgs_ctx_level_bwd2(*head, p(ws), ws.numel(), _lib.current_stream()), "bwd2")
    else:
        _lib.check(L.cgs_ctx_level_bwd_h(*head, p(H), p(ws), ws.numel(), _lib.current_stream()), "bwd_h")
    out = dict(dxf=dxf, dxs=dxs, dxo=dxo, dX=dX, dW1=dW1, db1=db1, dW2q=dW2q, db2q=db2q)
    if dhyp:
        out["d_hyp_rows"] = dh
    return out


def _sums_close(o, got):
    # (per-lane fp32 partial sums, then double atomics per block: the comparison of tests/test_ctx_level_gpu.py)
    rows = o["rows"]
    ref = torch.stack([o["xf"][rows].double().sum(), o["xs"][rows].double().sum(), o["xo"][rows].double().sum()])
    return torch.allclose(got, ref, rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("in_dim", [71, 15])
@pytest.mark.parametrize("kind", N_KINDS)
def test_forward_with_the_hand_over_writes_what_the_plain_forward_writes(kind, in_dim):
    o = _operands(_n_rows(kind), in_dim)
    for mask in ((True, False) if in_dim == 15 else (True,)):
        ref = _fwd(o, None, "fwd", mask)
        H, _ = _new_h(o["n"])
        for name, got in (("H", _fwd(o, H, "fwd_h", mask)), ("NULL", _fwd(o, None, "fwd_h", mask))):
            for k in ("X", "yf", "ys", "yo", "Q"):
                assert torch.equal(got[k], ref[k]), (name, k, mask)
            assert _sums_close(o, got["sums"]) and _sums_close(o, ref["sums"]), (name, got["sums"], ref["sums"])


@pytest.mark.parametrize("in_dim", [71, 15])
@pytest.mark.parametrize("kind", N_KINDS)
def test_backward_from_the_hand_over_has_the_bits_of_the_recompute(kind, in_dim):
    o = _operands(_n_rows(kind), in_dim)
    H, _ = _new_h(o["n"])
    f = _fwd(o, H, "fwd_h")                 # (a_mask given at in_dim 15)
    for side, dhyp, dqe in itertools.product((True, False), repeat=3):
        ref = _bwd(o, f["X"], None, side, dhyp, dqe)
        got = _bwd(o, f["X"], H, side, dhyp, dqe)
        assert set(got) == set(ref)
        for k in ref:
            assert torch.equal(got[k], ref[k]), (k, side, dhyp, dqe, float((got[k].double() - ref[k].double()).abs().max()))


@pytest.mark.parametrize("in_dim", [71, 15])
def test_whole_tiles_are_written_and_nothing_behind_them(in_dim):
    """n = 17: 15 rows of the second tile do not exist.  They hold what zero input rows give — finite — not what was in the buffer,
    because the backward multiplies them by d qadj = 0 inside an MFMA (0 x NaN = NaN); and the forward stops at the buffer's end."""
    o = _operands(17, in_dim)
    H, nb = _new_h(17, tail=4096, fill=float("nan"))
    f = _fwd(o, H[:nb], "fwd_h")
    assert bool((H[nb:] == 0xA5).all()), "the forward wrote behind cgs_ctx_level_hidden_bytes(n)"
    assert bool(torch.isfinite(H[:nb].view(torch.float32)).all()), "a piece of the last tile was left as it was"
    ref = _bwd(o, f["X"], None, True, True, True)
    got = _bwd(o, f["X"], H[:nb], True, True, True)
    for k in ref:
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k], ref[k]), k
