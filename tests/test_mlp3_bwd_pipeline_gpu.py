"""The fused anchor-MLP backward (csrc/mlp3.hip, mlp3_bwd_wg_kernel) at the row counts where its software pipeline starts and
ends: the kernel requests LDS operands two MFMA groups ahead, hands a head's first weights to the head in front of it and the
next tile's operands across the tile boundary, so a wave's first tile (prologue), a wave's last tile (the hand-over is read for
nothing) and waves with no tile at all are the cases to pin.  W = the number of waves the launcher starts
(min(ceil(tiles / 4), CUs) workgroups of 4 waves, one 16-row tile per wave and trip): n = 1, 15, 16, 17, 16 W - 1, 16 W + 1,
2 * 16 W + 5 give waves with zero, one, two and three tiles and ragged last tiles.

All four forms cgs_anchor_mlp3_backward_rows_t dispatches for the ROWS pair are run through the C-ABI: Hcat row-major or
fragment-major (tiled), input rows kept by the forward (X) or assembled again by the backward (X == NULL).

Reference: torch fp64 autograd over the same three heads on the row [feat_src[src_row] | (a - cam) / |a - cam| | |a - cam|].
The ReLU decision is the forward's — the backward reads it from the sign of Hcat — so the reference masks its fp64 hidden layer
with (Hcat > 0) of the library's forward: a pre-activation within rounding of zero would otherwise turn the comparison into a
test of the forward's rounding.  Tolerances are those of tests/test_mlp_gpu.py for this backward: 2e-5 of the tensor's max for
the data gradients, 2e-4 for the weight and bias gradients (sums over all rows)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = -7.25
PAD = 64
OUTS = (10, 30, 70)
FORMS = [(1, True), (1, False), (0, True), (0, False)]          # (tiled, keep_x)


def _waves():
    return 4 * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _row_counts():
    w = _waves() if torch.cuda.is_available() else 1024
    return [1, 15, 16, 17, 16 * w - 1, 16 * w + 1, 2 * 16 * w + 5]


def _fwd(L, c, tiled, keep_x):
    from contextgs_amd import _lib, mlp
    n, dev = c["n"], "cuda"
    nb = (n + 15) // 16 * 16 if tiled else n
    ys = [torch.empty(n, o, device=dev) for o in OUTS]
    h = torch.empty(nb, 150, device=dev)
    x = torch.empty(n, 54, device=dev) if keep_x else None
    _lib.check(L.cgs_anchor_mlp3_forward_rows_t(_lib.ptr(c["feat"]), _lib.ptr(c["src"]), _lib.ptr(c["anchor"]), _lib.ptr(c["cam"]),
                                                _lib.ptr(x), mlp._ptr_array(c["W1"]), mlp._ptr_array(c["b1"]), mlp._ptr_array(c["W2"]),
                                                mlp._ptr_array(c["b2"]), _lib.ptr(ys[0]), _lib.ptr(ys[1]), _lib.ptr(ys[2]), _lib.ptr(h), n,
                                                tiled, _lib.current_stream()), "fwd rows")
    return ys, h, x


@functools.lru_cache(maxsize=None)
def _case(n):
    """Inputs, the forward's row-major Hcat and the fp64 reference of one row count (computed once, shared by the forms)."""
    from contextgs_amd import _lib
    L = _lib.lib()
    dev = "cuda"
    g = torch.Generator(device="cpu").manual_seed(1000 + n % 997)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    n_src = n + 37
    c = dict(n=n, n_src=n_src)
    c["feat"] = rnd(n_src, 50)
    c["src"] = torch.randperm(n_src, generator=g)[:n].to(dev).contiguous()
    c["anchor"] = (rnd(n, 3) * 2).contiguous()
    c["cam"] = torch.tensor([0.3, -3.0, 0.5], device=dev)
    c["W1"] = [(rnd(50, 54) / 54 ** 0.5).contiguous() for _ in OUTS]
    c["b1"] = [(rnd(50) * 0.1).contiguous() for _ in OUTS]
    c["W2"] = [(rnd(o, 50) / 50 ** 0.5).contiguous() for o in OUTS]
    c["b2"] = [(rnd(o) * 0.1).contiguous() for o in OUTS]
    c["dY"] = [rnd(n, o).contiguous() for o in OUTS]
    _ys, h, _x = _fwd(L, c, 0, False)
    torch.cuda.synchronize()
    d = lambda t: t.double()
    feat, anchor = d(c["feat"]).requires_grad_(True), d(c["anchor"]).requires_grad_(True)
    W1, b1 = [d(t).requires_grad_(True) for t in c["W1"]], [d(t).requires_grad_(True) for t in c["b1"]]
    W2, b2 = [d(t).requires_grad_(True) for t in c["W2"]], [d(t).requires_grad_(True) for t in c["b2"]]
    u = anchor - d(c["cam"])
    dist = u.norm(dim=1, keepdim=True)
    x = torch.cat([feat[c["src"]], u / dist, dist], dim=1)
    loss = 0
    for i, act in enumerate((torch.tanh, torch.sigmoid, lambda t: t)):
        mask = (h[:, 50 * i:50 * i + 50] > 0).double()
        y = act((x @ W1[i].t() + b1[i]) * mask @ W2[i].t() + b2[i])
        loss = loss + (y * d(c["dY"][i])).sum()
    loss.backward()
    c["ref"] = dict(d_feat=feat.grad, d_anchor=anchor.grad, dW1=[t.grad for t in W1], db1=[t.grad for t in b1],
                    dW2=[t.grad for t in W2], db2=[t.grad for t in b2])
    return c


def _bwd(L, c, tiled, keep_x, fwd):
    """One call of the backward into sentinel-padded buffers; returns the flat buffers by name."""
    from contextgs_amd import _lib, mlp
    n, n_src, dev = c["n"], c["n_src"], "cuda"
    ys, h, x = fwd
    gld = mlp._m3_layout()[2]
    sizes = dict(d_feat=n_src * 50, d_anchor=n * 3, dz1=n * gld, dz2_op=n * 10, dz2_color=n * 30, dW1cat=gld * 54, db1cat=gld,
                 dW2_0=10 * 50, dW2_1=30 * 50, dW2_2=70 * 50, db2_0=10, db2_1=30, db2_2=70)
    bufs = {k: torch.full((s + PAD,), SENT, device=dev) for k, s in sizes.items()}
    for k in ("dW1cat", "db1cat", "dW2_0", "dW2_1", "dW2_2", "db2_0", "db2_1", "db2_2"):        # accumulated into: start at zero
        bufs[k][:sizes[k]] = 0
    bufs["d_feat"][:sizes["d_feat"]] = 0                         # (rows no visible anchor reads are the caller's)
    ws_bytes = int(L.cgs_mlp_wgrad_scratch_bytes())
    ws = torch.full((ws_bytes + PAD,), 0x5A, dtype=torch.uint8, device=dev)
    dW2 = [bufs[f"dW2_{i}"] for i in range(3)]
    db2 = [bufs[f"db2_{i}"] for i in range(3)]
    _lib.check(L.cgs_anchor_mlp3_backward_rows_t(
        _lib.ptr(x), _lib.ptr(None if keep_x else c["feat"]), _lib.ptr(c["src"]), _lib.ptr(c["anchor"]), _lib.ptr(c["cam"]),
        mlp._ptr_array(c["W1"]), mlp._ptr_array(c["W2"]), _lib.ptr(ys[0]), _lib.ptr(ys[1]), _lib.ptr(c["dY"][0]), _lib.ptr(c["dY"][1]),
        _lib.ptr(c["dY"][2]), _lib.ptr(h), _lib.ptr(bufs["d_feat"]), _lib.ptr(bufs["d_anchor"]), _lib.ptr(bufs["dz1"]),
        _lib.ptr(bufs["dz2_op"]), _lib.ptr(bufs["dz2_color"]), _lib.ptr(bufs["dW1cat"]), _lib.ptr(bufs["db1cat"]), mlp._ptr_array(dW2),
        mlp._ptr_array(db2), n, tiled, _lib.ptr(ws), ws_bytes, _lib.current_stream()), "bwd rows")
    torch.cuda.synchronize()
    bufs["ws"] = ws
    return bufs, sizes, ws_bytes


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f"tiled{f[0]}-{'x' if f[1] else 'nox'}")
@pytest.mark.parametrize("n", _row_counts())
def test_fused_backward_pipeline_edges(n, form):
    from contextgs_amd import _lib, mlp
    tiled, keep_x = form
    L = _lib.lib()
    c = _case(n)
    fwd = _fwd(L, c, tiled, keep_x)
    a, sizes, ws_bytes = _bwd(L, c, tiled, keep_x, fwd)
    b, _, _ = _bwd(L, c, tiled, keep_x, fwd)
    # two consecutive calls: the same bits everywhere (scratch included)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # nothing behind the end of any buffer the call may write
    for k, s in sizes.items():
        assert bool((a[k][s:] == SENT).all()), k
    assert bool((a["ws"][ws_bytes:] == 0x5A).all())
    # against fp64
    gp = mlp._m3_layout()[3]
    ref = c["ref"]
    got = dict(d_feat=a["d_feat"][:sizes["d_feat"]].view(-1, 50), d_anchor=a["d_anchor"][:sizes["d_anchor"]].view(-1, 3))
    dW1cat, db1cat = a["dW1cat"][:sizes["dW1cat"]].view(-1, 54), a["db1cat"][:sizes["db1cat"]]
    checks = [("d_feat", got["d_feat"], ref["d_feat"], 2e-5), ("d_anchor", got["d_anchor"], ref["d_anchor"], 2e-5)]
    for i, o in enumerate(OUTS):
        checks += [(f"dW1[{i}]", dW1cat[gp * i:gp * i + 50], ref["dW1"][i], 2e-4), (f"db1[{i}]", db1cat[gp * i:gp * i + 50], ref["db1"][i], 2e-4),
                   (f"dW2[{i}]", a[f"dW2_{i}"][:o * 50].view(o, 50), ref["dW2"][i], 2e-4), (f"db2[{i}]", a[f"db2_{i}"][:o], ref["db2"][i], 2e-4)]
    for name, x, r, rel in checks:
        err = float((x.double() - r).abs().max())
        tol = rel * max(1e-6, float(r.abs().max()))
        print(f"{name}: max err {err:.3e} tol {tol:.3e}")
        assert err <= tol, (name, err, tol)
    # the padding rows of the concatenated first-layer gradients (50..63 of each head) stay zero
    for i in range(3):
        assert float(dW1cat[gp * i + 50:gp * (i + 1)].abs().sum()) == 0.0 and float(db1cat[gp * i + 50:gp * (i + 1)].abs().sum()) == 0.0
