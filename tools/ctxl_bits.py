"""Every output of the four level entry points (cgs_ctx_level_fwd / _fwd_h / _bwd2 / _bwd_h, csrc/ctx_level.hip) as .npy, to compare
two builds of the library bit for bit — the test for changes whose old code no longer exists in the tree.

    CGS_LIB_PATH=tools/variants/libcgs_parent.so python tools/ctxl_bits.py dump out/parent
    python tools/ctxl_bits.py dump out/new                    (separate processes: one library per process)
    python tools/ctxl_bits.py compare out/parent out/new      (numpy.array_equal on every array; prints the count, exit 1 on a difference)

Shapes: in_dim 71 and 15, n = 1, 16, 17, 16 * 4 * CU + 5, 2 * 16 * 4 * CU + 5 (CU = multi_processor_count); the backward with the rate
side, d_hyp_rows and dQ_ext all given and all NULL.  Operands from fixed CPU seeds, outputs pre-filled (what a kernel leaves alone
compares equal too).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SEED, Q0 = 0x5DEECE66D, (1.0, 0.001, 0.2)


def operands(n, in_dim):
    import torch
    gen = torch.Generator(device="cpu").manual_seed(7 * n + in_dim)
    R = lambda *s: torch.randn(*s, generator=gen).cuda()
    N, n_par = n + 11, max(1, n // 3)
    o = dict(n=n, N=N, n_par=n_par, in_dim=in_dim)
    o["anchor"], o["hyp"] = R(N, 3), R(n, 12)
    o["a_rows"] = torch.randperm(N, generator=gen)[:n].cuda()
    o["a_mask"] = (torch.rand(N, generator=gen) < 0.7).cuda().view(torch.uint8)
    o["base_f"], o["base_s"] = R(n_par, 50), R(n_par, 6)
    o["pos"] = torch.randint(0, n_par, (n,), generator=gen).cuda()
    o["W1"], o["b1"], o["W2q"], o["b2q"] = R(100, in_dim) * 0.2, R(100) * 0.1, R(3, 100) * 0.1, R(3) * 0.1
    o["xf"], o["xs"], o["xo"] = R(N, 50), R(N, 6), R(N, 30)
    o["rows"] = torch.randperm(N, generator=gen)[:n].cuda()
    o["dyf"], o["dys"], o["dyo"], o["dQe"] = R(n, 50), R(n, 6), R(n, 30), R(n, 3)
    m = max(1, int(round(0.15 * n)))
    sub = torch.randperm(n, generator=gen)[:m].cuda()
    smap = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    smap[sub] = torch.arange(m, dtype=torch.int32, device="cuda")
    o["m"], o["smap"] = m, smap
    o["sf"], o["ss"], o["so"], o["sQ"], o["dxsub"] = R(m, 50), R(m, 6), R(m, 30), R(m, 3), R(m, in_dim)
    return o


def forward(o, with_h):
    import torch
    from contextgs_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n, in_dim, ctxl = o["n"], o["in_dim"], o["in_dim"] == 71
    X = torch.full((n, in_dim), 3.0, device="cuda")
    yf, ys, yo, Q = (torch.full((n, w), 3.0, device="cuda") for w in (50, 6, 30, 3))
    sums = torch.zeros(int(L.cgs_means_accum_doubles()), dtype=torch.float64, device="cuda")
    H = torch.zeros(int(L.cgs_ctx_level_hidden_bytes(n)), dtype=torch.uint8, device="cuda") if with_h else None
    head = (in_dim, p(o["anchor"]), o["N"], p(o["a_rows"]), None if ctxl else p(o["a_mask"]), p(o["base_f"]) if ctxl else None,
            p(o["base_s"]) if ctxl else None, o["n_par"] if ctxl else 0, p(o["pos"]) if ctxl else None, p(o["hyp"]), n, p(o["W1"]), p(o["b1"]),
            p(o["W2q"]), p(o["b2q"]), p(o["xf"]), p(o["xs"]), p(o["xo"]), p(o["rows"]), SEED, *Q0, p(X), p(yf), p(ys), p(yo), p(Q), p(sums))
    if with_h:
        _lib.check(L.cgs_ctx_level_fwd_h(*head, p(H), _lib.current_stream()), "fwd_h")
    else:
        _lib.check(L.cgs_ctx_level_fwd(*head, _lib.current_stream()), "fwd")
    out = dict(X=X, yf=yf, ys=ys, yo=yo, Q=Q)          # (the three sums are atomics over blocks: not a bit-stable output)
    if with_h:
        out["H"] = H
    return out


def backward(o, X, H, full):
    import torch
    from contextgs_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n, N, in_dim = o["n"], o["N"], o["in_dim"]
    dxf, dxs, dxo = (torch.full((N, w), 7.0, device="cuda") for w in (50, 6, 30))
    dX, dh = torch.full((n, in_dim), 5.0, device="cuda"), torch.full((N, 12), 9.0, device="cuda")
    dW1, db1, dW2q, db2q = torch.ones(100, in_dim, device="cuda"), torch.ones(100, device="cuda"), torch.ones(3, 100, device="cuda"), \
        torch.ones(3, device="cuda")
    ws = torch.empty(int(L.cgs_ctx_level_bwd_scratch_bytes()), dtype=torch.uint8, device="cuda")
    sd = [p(o[k]) if full else None for k in ("sf", "ss", "so", "sQ", "dxsub")]
    head = (in_dim, p(X), p(o["W1"]), p(o["b1"]), p(o["W2q"]), p(o["b2q"]), p(o["dyf"]), p(o["dys"]), p(o["dyo"]),
            p(o["dQe"]) if full else None, n, SEED, *Q0, p(o["rows"]), N, p(dxf), p(dxs), p(dxo), p(o["smap"]) if full else None,
            o["m"] if full else 0, *sd, p(dX), p(dh) if full else None, p(dW1), p(db1), p(dW2q), p(db2q))
    if H is None:
        _lib.check(L.cgs_ctx_level_bwd2(*head, p(ws), ws.numel(), _lib.current_stream()), "bwd2")
    else:
        _lib.check(L.cgs_ctx_level_bwd_h(*head, p(H), p(ws), ws.numel(), _lib.current_stream()), "bwd_h")
    return dict(dxf=dxf, dxs=dxs, dxo=dxo, dX=dX, d_hyp_rows=dh, dW1=dW1, db1=db1, dW2q=dW2q, db2q=db2q)


def dump(out_dir):
    import torch
    os.makedirs(out_dir, exist_ok=True)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    count = 0
    for in_dim in (71, 15):
        for n in (1, 16, 17, 16 * 4 * cu + 5, 2 * 16 * 4 * cu + 5):
            o = operands(n, in_dim)
            f, fh = forward(o, False), forward(o, True)
            sets = {"fwd": f, "fwd_h": fh}
            for full in (True, False):
                sets["bwd2_%d" % full] = backward(o, f["X"], None, full)
                sets["bwd_h_%d" % full] = backward(o, fh["X"], fh["H"], full)
            torch.cuda.synchronize()
            for entry, arrays in sets.items():
                for k, v in arrays.items():
                    np.save(os.path.join(out_dir, "in%d_n%d_%s_%s.npy" % (in_dim, n, entry, k)), v.cpu().numpy())
                    count += 1
    print("ctxl_bits: %d arrays written to %s" % (count, out_dir))


def compare(a_dir, b_dir):
    a, b = sorted(os.listdir(a_dir)), sorted(os.listdir(b_dir))
    if a != b or not a:
        print("ctxl_bits: the two dumps hold different (or no) arrays: %d / %d" % (len(a), len(b)))
        return 1
    raw = lambda d, k: np.load(os.path.join(d, k)).reshape(-1).view(np.uint8)        # bytes: -0.0 is not 0.0, a NaN is its payload
    bad = [k for k in a if not np.array_equal(raw(a_dir, k), raw(b_dir, k))]
    print("ctxl_bits: %d arrays compared, %d differ%s" % (len(a), len(bad), "".join("\n  " + k for k in bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
