"""contextgs_amd.optim.FusedAdam and cgs_adam_step, the parts that need no GPU: argument errors of the entry point, what the
constructor refuses, the refusal of CPU parameters, state dicts in both directions between FusedAdam and torch.optim.Adam,
`training_setup`'s optimizer_type, and how rows="auto" resolves from dist.note_touched_rows."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

ADJ = os.path.join(os.path.dirname(__file__), "golden", "adjust_anchor.npz")
SPARSE_GROUPS = {"anchor", "offset", "anchor_feat", "hyper_latent", "scaling", "rotation"}
TODAY_KEYS = set(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=0.0, eps=1e-15).param_groups[0]) | {"name"}


def _desc(n, numel=8, width=0, ptr=0x1000):
    from contextgs_amd import _lib
    arr = (_lib.AdamTensor * max(n, 1))()
    for k in range(n):        # the pointers are never dereferenced: every call below is refused (or has nothing to do) on the host
        arr[k] = _lib.AdamTensor(ptr, ptr, ptr, ptr, numel, 0.9, 0.999, width, 1e-3, 1.0, 1e-8, 0.0)
    return arr


def test_adam_step_argument_errors_are_return_codes():
    from contextgs_amd import _lib
    lib = _lib.lib()
    assert ctypes.sizeof(_lib.AdamTensor) == 80
    assert lib.cgs_adam_step(0, None, None, 0, None) == 0                      # nt = 0: CGS_OK, nothing launched
    assert lib.cgs_adam_step(3, _desc(3, numel=0, ptr=None), None, 0, None) == 0   # all numel == 0: nothing launched
    for what, call in [
            ("nt", lambda: lib.cgs_adam_step(33, _desc(33), None, 0, None)),
            ("nt", lambda: lib.cgs_adam_step(-1, _desc(1), None, 0, None)),
            ("NULL descriptor", lambda: lib.cgs_adam_step(2, None, None, 0, None)),
            ("numel < 0", lambda: lib.cgs_adam_step(1, _desc(1, numel=-4), None, 0, None)),
            ("NULL pointer", lambda: lib.cgs_adam_step(1, _desc(1, ptr=None), None, 0, None)),
            ("numel", lambda: lib.cgs_adam_step(1, _desc(1, numel=12, width=3), 0x1000, 5, None)),        # 5 rows of 3 != 12
            ("numel", lambda: lib.cgs_adam_step(1, _desc(1, numel=13, width=3), 0x1000, 4, None)),        # 13 is no multiple of 3
            ("rows is NULL", lambda: lib.cgs_adam_step(1, _desc(1, numel=12, width=3), None, 4, None))]:
        assert call() == 1, what                                                # CGS_ERR_ARG
        assert what.encode() in lib.cgs_last_error(), (what, lib.cgs_last_error())


@pytest.mark.parametrize("kw", [dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True),
                                dict(foreach=True), dict(fused=True)])
def test_constructor_refuses_what_the_kernel_does_not_do(kw):
    from contextgs_amd.optim import FusedAdam
    with pytest.raises(ValueError, match=next(iter(kw))):
        FusedAdam([torch.nn.Parameter(torch.zeros(3))], lr=1e-3, **kw)


def test_constructor_accepts_weight_decay_and_is_an_adam():
    from contextgs_amd.optim import FusedAdam
    opt = FusedAdam([torch.nn.Parameter(torch.zeros(3))], lr=1e-3, weight_decay=0.01, foreach=False, fused=False)
    assert isinstance(opt, torch.optim.Adam) and opt.param_groups[0]["weight_decay"] == 0.01


def test_step_on_a_cpu_parameter_raises():
    from contextgs_amd.optim import FusedAdam
    p = torch.nn.Parameter(torch.ones(5))
    opt = FusedAdam([p], lr=1e-3)
    opt.step()                                   # no gradient anywhere: nothing to do, nothing to refuse
    assert len(opt.state[p]) == 0
    p.grad = torch.ones(5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert len(opt.state[p]) == 0 and torch.equal(p.detach(), torch.ones(5))


def _two_groups(seed=0):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.nn.Parameter(torch.randn(6, 3, generator=g)), torch.nn.Parameter(torch.randn(4, generator=g))
    return a, b, [{"params": [a], "lr": 1e-2, "name": "a", "row_sparse": True}, {"params": [b], "lr": 3e-3, "name": "b", "eps": 1e-10}]


def test_state_dicts_round_trip_both_ways():
    from contextgs_amd.optim import FusedAdam
    a, b, groups = _two_groups()
    ref = torch.optim.Adam([{k: v for k, v in g.items() if k != "row_sparse"} for g in groups], lr=0.0, eps=1e-15)
    gen = torch.Generator().manual_seed(1)
    for _ in range(2):
        a.grad, b.grad = torch.randn(6, 3, generator=gen), torch.randn(4, generator=gen)
        ref.step()
    sd = ref.state_dict()
    opt = FusedAdam(groups, lr=0.0, eps=1e-15)
    opt.load_state_dict(sd)
    for p in (a, b):
        assert float(opt.state[p]["step"]) == 2.0 and not opt.state[p]["step"].is_cuda
        assert torch.equal(opt.state[p]["exp_avg"], ref.state[p]["exp_avg"])
        assert torch.equal(opt.state[p]["exp_avg_sq"], ref.state[p]["exp_avg_sq"])
    assert [g["lr"] for g in opt.param_groups] == [1e-2, 3e-3] and opt.param_groups[1]["eps"] == 1e-10
    # a checkpoint of torch.optim.Adam carries no row_sparse key: the flags of the optimizer that loads it survive
    assert [g.get("row_sparse", False) for g in opt.param_groups] == [True, False]
    back = torch.optim.Adam([{"params": [a]}, {"params": [b]}], lr=0.5)
    back.load_state_dict(opt.state_dict())
    for p in (a, b):
        assert set(back.state[p]) == {"step", "exp_avg", "exp_avg_sq"}
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(back.state[p][k], ref.state[p][k]), k
    assert [g["lr"] for g in back.param_groups] == [1e-2, 3e-3]
    a.grad, b.grad = torch.randn(6, 3, generator=gen), torch.randn(4, generator=gen)
    back.step()                                  # torch steps on from FusedAdam's state dict
    assert float(back.state[a]["step"]) == 3.0


def _model(monkeypatch, env=None, attr=None):
    from contextgs_amd.model import GaussianModel
    z = np.load(ADJ)
    args = types.SimpleNamespace(**{str(k): float(v) for k, v in zip(z["args_names"], z["args_values"])})
    if attr is not None:
        args.optimizer_type = attr
    if env is None:
        monkeypatch.delenv("CGS_OPTIMIZER", raising=False)
    else:
        monkeypatch.setenv("CGS_OPTIMIZER", env)
    pc = GaussianModel(device="cpu")
    n, K = 7, pc.n_offsets
    pc.set_state(torch.zeros(n, 3), torch.zeros(n, K, 3), torch.zeros(n, K, 1), torch.zeros(n, 50), torch.zeros(n, 12), torch.zeros(n, 6))
    pc.spatial_lr_scale = 1.7
    pc.training_setup(args)
    return pc


def test_training_setup_default_is_todays_optimizer(monkeypatch):
    from contextgs_amd.optim import FusedAdam
    for attr in (None, "default"):
        opt = _model(monkeypatch, attr=attr).optimizer
        assert type(opt) is torch.optim.Adam and not isinstance(opt, FusedAdam)
        assert len(opt.param_groups) == 13
        for g in opt.param_groups:
            assert set(g) == TODAY_KEYS, set(g) ^ TODAY_KEYS
        assert opt.defaults["eps"] == 1e-15


@pytest.mark.parametrize("kind", ["fused_adam", "sparse_adam"])
def test_training_setup_fused_and_sparse(monkeypatch, kind):
    from contextgs_amd.optim import FusedAdam
    ref = _model(monkeypatch).optimizer
    opt = _model(monkeypatch, attr=kind).optimizer
    assert type(opt) is FusedAdam
    flagged = {g["name"] for g in opt.param_groups if g.get("row_sparse", False)}
    assert flagged == (SPARSE_GROUPS if kind == "sparse_adam" else set())
    assert [g["name"] for g in opt.param_groups] == [g["name"] for g in ref.param_groups]
    for g, r in zip(opt.param_groups, ref.param_groups):
        assert {k: v for k, v in g.items() if k not in ("params", "row_sparse")} == {k: v for k, v in r.items() if k != "params"}
        assert [tuple(p.shape) for p in g["params"]] == [tuple(p.shape) for p in r["params"]]


def test_training_setup_unknown_type_and_environment_override(monkeypatch):
    from contextgs_amd.optim import FusedAdam
    with pytest.raises(ValueError, match="optimizer_type"):
        _model(monkeypatch, attr="adamw")
    with pytest.raises(ValueError, match="optimizer_type"):
        _model(monkeypatch, env="nonsense")
    opt = _model(monkeypatch, env="sparse_adam", attr="default").optimizer          # the environment wins over the attribute
    assert type(opt) is FusedAdam and sum(bool(g.get("row_sparse")) for g in opt.param_groups) == 6
    opt = _model(monkeypatch, env="default", attr="fused_adam").optimizer
    assert type(opt) is torch.optim.Adam
    opt = _model(monkeypatch, env="", attr="fused_adam").optimizer                  # an empty variable is no choice
    assert type(opt) is FusedAdam


def test_auto_rows_resolve_from_the_renderers_note(monkeypatch):
    from contextgs_amd import dist
    from contextgs_amd.optim import FusedAdam
    a, b, groups = _two_groups()
    mask = torch.tensor([True, False, True, False, False, True])
    dist.note_touched_rows(mask, 3)               # a render BEFORE the optimizer exists does not count
    opt = FusedAdam(groups, lr=0.0)
    got, count = dist.touched_rows()
    assert got is mask
    assert opt.resolve_rows("auto") is None       # counter + 0 since construction
    dist.note_touched_rows(mask, 3)
    assert dist.touched_rows()[1] == count + 1
    assert opt.resolve_rows("auto") is mask       # + 1: the note
    assert opt.resolve_rows("auto") is None       # + 0 again: already consumed
    dist.note_touched_rows(mask, 3)
    dist.note_touched_rows(mask, 3)
    assert opt.resolve_rows("auto") is None       # + 2 (gradient accumulation): the union is unknown
    dist.note_touched_rows(None, 0)
    assert opt.resolve_rows("auto") is None       # + 1 but "every row"
    dist.note_touched_rows(mask, 3)
    monkeypatch.setattr(dist, "world", lambda: 2)
    assert opt.resolve_rows("auto") is None       # + 1, a mask, but two ranks
    monkeypatch.setattr(dist, "world", lambda: 1)
    dist.note_touched_rows(mask, 3)
    assert opt.resolve_rows(None) is None         # an explicit dense step consumes the note too ...
    assert opt.resolve_rows("auto") is None       # ... (+ 0)
    dist.note_touched_rows(mask, 3)
    dist.note_touched_rows(mask, 3)
    other = torch.zeros(6, dtype=torch.bool)
    assert opt.resolve_rows(other) is other       # an explicit mask does not depend on the counter
    # no row_sparse group: always dense
    dense = FusedAdam([{"params": [b]}], lr=0.0)
    dist.note_touched_rows(mask, 3)
    assert dense.resolve_rows("auto") is None and dense.resolve_rows(other) is None
    with pytest.raises(ValueError):
        opt.resolve_rows("visible")
