"""What the fused MLP nodes (contextgs_amd/mlp.py, anchor_gen.py) ask of libcgs_hip.so, call by call: the cases and the writer of
tests/golden/mlp_calls.json, which tests/test_mlp_calls_gpu.py compares the tree under test with.

    python tools/mlp_call_record.py OUT.json       (on the MI355X, at the commit whose behaviour is to be kept)

The fixture is recorded at the PARENT of a change that must keep the host side of the nodes as it is, never from the changed
tree.  Only the public functions of mlp / anchor_gen, their A/B knobs and _lib.lib / _lib.SIGNATURES are used, so the same file
runs on both sides of such a change.  The recording proxy and the notation of a call are tools/raster_call_record.py's: integers
and floats by value, pointers as "ptr" / "null" — the queries (cgs_mlp_wgrad_scratch_bytes, cgs_anchor_mlp3_layout) and the calls
of ctx_ops.zero_unlisted_rows / gather_rows_nograd included.  The one exception is the stamp generation of cgs_mark_rows /
cgs_zero_unmarked_rows, a process-wide counter that depends on what ran before, noted as "gen".

Shapes: n = 37 rows (two full 16-row tiles and a ragged tail) out of n_src = 45, a `loc` of 5 rows; n = 0 once per node.  The
level node's empty case is the empty `loc` (m = 0): an x of no rows is refused by ctx_ops.gather_rows_nograd before any call.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from raster_call_record import CallRecorder  # noqa: E402

N, N_SRC, N_LOC, K = 37, 45, 5, 10
MODES = ("inline", "deferred")
_GEN_ARG = {"cgs_mark_rows": 4, "cgs_zero_unmarked_rows": 2}      # position of the stamp generation in a recorded call


def _seq(i, h, o, act=None):
    import torch.nn as nn
    return nn.Sequential(nn.Linear(i, h), nn.ReLU(True), nn.Linear(h, o), *([act()] if act else [])).to("cuda")


def _heads():
    import torch.nn as nn
    return _seq(54, 50, 10, nn.Tanh), _seq(54, 50, 30, nn.Sigmoid), _seq(54, 50, 70)


def _leaf(*shape):
    import torch
    return torch.randn(*shape, device="cuda").requires_grad_(True)


def _params(*seqs):
    return [p for s in seqs for p in s.parameters()]


# ---- the cases: each returns (run, leaves); run() is one forward, its outputs in a list ----------------------------------------
def _mlp2(shape, n=N, recompute=True):
    from contextgs_amd import mlp
    seq, x = _seq(*shape), _leaf(n, shape[0])

    def run():
        mlp.RECOMPUTE_HIDDEN = recompute
        return [mlp.mlp2(x, seq)]
    return run, [x] + _params(seq)


def _mlp2_nonleaf():
    import torch
    from contextgs_amd import mlp
    seq, x = _seq(71, 100, 175), _leaf(N, 71)
    scale = torch.ones((), device="cuda", requires_grad=True)
    run = lambda: [mlp.mlp2_weights(x, seq[0].weight * scale, seq[0].bias, seq[2].weight, seq[2].bias, 0)]
    return run, [x, scale] + _params(seq)


def _level(read=(0, 1), n=N, n_loc=N_LOC):
    import torch
    from contextgs_amd import mlp
    seq, x = _seq(71, 100, 175), _leaf(n, 71)
    loc = torch.randperm(n, device="cuda")[:n_loc].sort().values

    def run():
        outs = mlp.level_mlp(x, loc, seq, 172)
        return [outs[i] for i in read]
    return run, [x] + _params(seq)


def _anchor_mlp3(n=N):
    from contextgs_amd import mlp
    heads, x = _heads(), _leaf(n, 54)
    return (lambda: list(mlp.anchor_mlp3(x, *heads))), [x] + _params(*heads)


def _rows(keep_x=True, tiled=True, n=N, n_src=N_SRC, pre=False):
    import torch
    from contextgs_amd import mlp
    heads = _heads()
    feat_src = _leaf(n_src, 50)
    src_row = torch.randperm(n_src, device="cuda")[:n].contiguous()
    anchor = (torch.randn(n, 3, device="cuda") * 2).requires_grad_(True)
    cam = torch.tensor([0.3, -3.0, 0.5], device="cuda")

    def run():
        mlp.KEEP_X_OFF, mlp.M3_TILED = not keep_x, tiled
        early = mlp.anchor_mlp3_rows_launch(feat_src, src_row, anchor, cam, *heads) if pre else None
        return list(mlp.anchor_mlp3_rows(feat_src, src_row, anchor, cam, *heads, pre=early))
    return run, [feat_src, anchor] + _params(*heads)


def _anchor_gen(n=N, n_src=N_SRC):
    import torch
    from contextgs_amd import anchor_gen
    heads = _heads()
    feat_src = _leaf(n_src, 50)
    gs_src = (torch.rand(n_src, 6, device="cuda") * 0.1 + 0.01).requires_grad_(True)
    off_src = (torch.randn(n_src, K, 3, device="cuda") * 0.5).requires_grad_(True)
    row = torch.randperm(n_src, device="cuda")[:n].contiguous()
    anchor = (torch.randn(n, 3, device="cuda") * 2).requires_grad_(True)
    cam = torch.tensor([0.3, -3.0, 0.5], device="cuda")
    masks = (torch.rand(n, K, device="cuda") < 0.7).float().requires_grad_(True)

    def run():
        anchor_gen.MODE = "all"
        assert anchor_gen.supported(*heads, K, feat_src, row, anchor, cam, gs_src, off_src, masks)
        return list(anchor_gen.anchor_gen(feat_src, row, anchor, cam, gs_src, off_src, row, masks, *heads)[:6])
    return run, [feat_src, gs_src, off_src, anchor, masks] + _params(*heads)


CASES = {
    "mlp2_stored": lambda: _mlp2((71, 100, 175)),
    "mlp2_recompute": lambda: _mlp2((15, 100, 3)),
    "mlp2_recompute_off": lambda: _mlp2((15, 100, 3), recompute=False),
    "mlp2_weights_nonleaf": _mlp2_nonleaf,
    "level_both": lambda: _level((0, 1)),
    "level_qadj_only": lambda: _level((0,)),
    "level_pred_only": lambda: _level((1,)),
    "level_empty_loc": lambda: _level((0, 1), n_loc=0),
    "anchor_mlp3": _anchor_mlp3,
    **{f"rows_keep{int(k)}_tiled{int(t)}_{'sub' if s > N else 'all'}": (lambda k=k, t=t, s=s: _rows(k, t, n_src=s))
       for k in (True, False) for t in (True, False) for s in (N_SRC, N)},     # n < n_src, n == n_src
    "rows_pre": lambda: _rows(pre=True),
    "anchor_gen": _anchor_gen,
    "mlp2_n0": lambda: _mlp2((71, 100, 175), n=0),
    "mlp2_recompute_n0": lambda: _mlp2((15, 100, 3), n=0),
    "anchor_mlp3_n0": lambda: _anchor_mlp3(n=0),
    "rows_n0": lambda: _rows(n=0),
    "anchor_gen_n0": lambda: _anchor_gen(n=0),
}


def key(case, mode):
    return f"{case}/{mode}"


def run_once(run, leaves):
    """One forward + backward.  Returns the outputs and then the gradient of every leaf (None where it got none)."""
    import torch
    for t in leaves:
        t.grad = None
    outs = run()
    g = torch.Generator(device="cuda").manual_seed(5)
    sum((o * torch.randn(o.shape, device="cuda", generator=g)).sum() for o in outs).backward()
    torch.cuda.synchronize()
    return [o.detach().clone() for o in outs] + [None if t.grad is None else t.grad.clone() for t in leaves]


def record(case, mode):
    """(the calls of two runs in a row, the first with the layout query still to be made; the outputs and gradients of the two)"""
    import torch
    from contextgs_amd import _lib, anchor_gen, mlp
    torch.manual_seed(11)
    knobs = [(mlp, k, getattr(mlp, k)) for k in ("RECOMPUTE_HIDDEN", "KEEP_X_OFF", "M3_TILED", "_M3_LAYOUT")]
    knobs.append((anchor_gen, "MODE", anchor_gen.MODE))
    mlp._M3_LAYOUT = None
    prev = mlp.defer_weight_gradients(mode == "deferred")
    calls, real = [], _lib.lib
    handle = real()
    _lib.lib = lambda: CallRecorder(handle, calls)
    try:
        run, leaves = CASES[case]()
        res = [run_once(run, leaves) for _ in range(2)]
        assert not mlp._Deferred.queue and not mlp._Deferred.armed and not mlp._Deferred.staged
    finally:
        _lib.lib = real
        mlp.defer_weight_gradients(prev)
        for mod, k, v in knobs:
            setattr(mod, k, v)
    for c in calls:
        if c[0] in _GEN_ARG:
            c[_GEN_ARG[c[0]]] = "gen"
    return calls, res


def dump(path, library, calls):
    """JSON with one recorded call per line, so that a difference reads as a line."""
    one = lambda c: "   " + json.dumps(c, separators=(",", ":"))
    body = ",\n".join(f"  {json.dumps(k)}: [\n" + ",\n".join(map(one, v)) + "\n  ]" for k, v in calls.items())
    with open(path, "w") as f:
        f.write(f'{{\n "generator": "tools/mlp_call_record.py (MI355X, gfx950)",\n "library": {json.dumps(library)},\n'
                f' "calls": {{\n{body}\n }}\n}}\n')


def same(res):
    import torch
    a, b = res
    return len(a) == len(b) and all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a, b))


def main():
    from contextgs_amd import _lib
    calls = {}
    for case in CASES:
        for mode in MODES:
            calls[key(case, mode)], res = record(case, mode)
            assert same(res), f"{key(case, mode)}: two runs differ"
    dump(sys.argv[1], (_lib.lib().cgs_build_info() or b"").decode(), calls)
    print(sys.argv[1], {k: len(v) for k, v in calls.items()})


if __name__ == "__main__":
    main()
