"""The weight-gradient hand-off of the fused MLP nodes (contextgs_amd/mlp.py, _WeightGrads) on CPU tensors: no library, no GPU.
A toy autograd node (y = x W^T + b) goes through the same helper as _MLP2, _LevelMLP, _AnchorMLP3 and _AnchorMLP3Rows: its
decision, its pointers, and what it returns inline and with the products left for the end of the backward."""
import pytest
import torch

from contextgs_amd import mlp


class _Toy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b, log, name, also):
        ctx.save_for_backward(x, W.detach())
        ctx.params, ctx.log, ctx.name, ctx.also = (W, b), log, name, also
        return x @ W.detach().t() + b.detach()

    @staticmethod
    def backward(ctx, g):
        x, Wd = ctx.saved_tensors
        log, name = ctx.log, ctx.name
        wg = mlp._WeightGrads(ctx.params, ctx.also)
        dW, db = torch.zeros_like(Wd), torch.zeros(Wd.shape[0])
        log.append(("node", name, wg.deferred, wg.ptr(dW), wg.ptr(dW, keep=True), wg.ptr([dW, db])))

        def launch():
            log.append(("launch", name))
            dW.add_(g.t() @ x)
            db.add_(g.sum(0))
        if not wg.deferred:         # (a real node: its C call writes them when it is handed the pointers)
            launch()
        left = wg.leave((dW, db), launch)
        log.append(("left", name, left))
        return (g @ Wd, *left, None, None, None)


@pytest.fixture
def deferral():
    """Switches the deferral; leaves the module as it found it."""
    prev = mlp._Deferred.on
    yield mlp.defer_weight_gradients
    mlp.defer_weight_gradients(prev)
    mlp._drop_stale_deferred()


def _run(defer, backwards, log=None):
    torch.manual_seed(3)
    W, b = torch.randn(5, 7, requires_grad=True), torch.randn(5, requires_grad=True)
    x = torch.randn(11, 7, requires_grad=True)
    w = torch.randn(11, 5)
    log = [] if log is None else log
    mlp.defer_weight_gradients(defer)
    for _ in range(backwards):
        (_Toy.apply(x, W, b, log, "a", True) * w).sum().backward()
        assert not mlp._Deferred.queue and not mlp._Deferred.armed and not mlp._Deferred.staged
    return [W.grad, b.grad, x.grad], log


@pytest.mark.parametrize("backwards", [1, 2])
def test_deferred_and_inline_leave_equal_grads(backwards, deferral):
    a, log_a = _run(False, backwards)
    b, log_b = _run(True, backwards)
    assert all(t is not None for t in a + b)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert [e[2] for e in log_a if e[0] == "node"] == [False] * backwards
    assert [e[2] for e in log_b if e[0] == "node"] == [True] * backwards
    # against autograd's own gradients of the same expression
    torch.manual_seed(3)
    W, bias = torch.randn(5, 7, requires_grad=True), torch.randn(5, requires_grad=True)
    x = torch.randn(11, 7, requires_grad=True)
    w = torch.randn(11, 5)
    for _ in range(backwards):
        ((x @ W.t() + bias) * w).sum().backward()
    for u, v in zip(a, [W.grad, bias.grad, x.grad]):
        assert torch.allclose(u, v, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("defer", [False, True])
def test_two_nodes_on_one_parameter_are_summed_in_node_order_before_the_add(defer, deferral):
    """fp32 at 1e8 has a spacing of 8: 1e8 + (3 + 3) = 1e8 + 8, while (1e8 + 3) + 3 = 1e8.  The contributions of one backward
    are summed first, in the order the nodes ran, and only then added to an existing .grad, as the engine does inline."""
    W, b = torch.ones(1, 1, requires_grad=True), torch.zeros(1, requires_grad=True)
    W.grad, b.grad = torch.full((1, 1), 1e8), torch.zeros(1)
    x = torch.full((1, 1), 3.0)
    log = []
    deferral(defer)
    (_Toy.apply(x, W, b, log, "a", True) + _Toy.apply(x, W, b, log, "b", True)).sum().backward()
    assert float(W.grad) == 1e8 + 8 and float(b.grad) == 2.0
    ran = [e[1] for e in log if e[0] == "node"]
    assert sorted(ran) == ["a", "b"]
    assert [e[1] for e in log if e[0] == "launch"] == ran                       # queued launches: node order
    if defer:
        assert [e[0] for e in log] == ["node", "left", "node", "left", "launch", "launch"]
    assert not mlp._Deferred.queue and not mlp._Deferred.armed and not mlp._Deferred.staged


def test_a_non_leaf_parameter_is_never_deferred(deferral):
    W0, b = torch.randn(5, 7, requires_grad=True), torch.randn(5, requires_grad=True)
    scale = torch.ones((), requires_grad=True)
    x = torch.randn(4, 7)
    log, hooked = [], []
    hook = mlp.add_before_flush_hook(lambda: hooked.append(1))
    deferral(True)
    try:
        _Toy.apply(x, W0 * scale, b, log, "a", True).sum().backward()
    finally:
        mlp.remove_before_flush_hook(hook)
    node, left = log[0], log[-1]
    assert node[2] is False and node[3] is not None and all(g is not None for g in left[2])
    assert [e[0] for e in log] == ["node", "launch", "left"] and hooked == []      # nothing queued: no flush
    assert W0.grad is not None and scale.grad is not None and b.grad is not None
    assert torch.equal(W0.grad, torch.ones(4, 5).t() @ x)
    assert not mlp._Deferred.queue and not mlp._Deferred.armed and not mlp._Deferred.staged


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("also", [False, True])
def test_ptr_is_null_exactly_when_deferred_and_not_kept_and_leave_returns_a_none_per_gradient(on, also, deferral):
    W, b = torch.randn(5, 7, requires_grad=True), torch.randn(5, requires_grad=True)
    log = []
    deferral(on)
    _Toy.apply(torch.randn(4, 7), W, b, log, "a", also).sum().backward()
    (_, _, deferred, p, p_keep, p_list), left = log[0], next(e for e in log if e[0] == "left")[2]
    assert deferred is (on and also)            # the node's own condition on top of _can_defer
    assert (p is None) is deferred and (p_list is None) is deferred and p_keep is not None
    if deferred:
        assert left == (None, None)
    else:
        assert len(left) == 2 and all(isinstance(g, torch.Tensor) for g in left)
    assert W.grad is not None and b.grad is not None
    wg = mlp._WeightGrads((W, b), also)         # outside a backward: the decision alone, nothing queued
    assert wg.deferred is deferred
    if not deferred:
        grads = (1, 2, 3)
        assert wg.leave(grads, None) is grads   # inline: handed back unchanged


def test_the_hook_runs_before_the_queued_launch_and_the_flush_leaves_nothing(deferral):
    W, b = torch.randn(5, 7, requires_grad=True), torch.randn(5, requires_grad=True)
    log = []
    hook = mlp.add_before_flush_hook(lambda: log.append(("hook",)))
    deferral(True)
    try:
        y = _Toy.apply(torch.randn(4, 7), W, b, log, "a", True)
        assert not mlp._Deferred.queue and not mlp._Deferred.armed
        y.sum().backward()
    finally:
        mlp.remove_before_flush_hook(hook)
    assert [e[0] for e in log] == ["node", "left", "hook", "launch"]
    assert mlp._Deferred.queue == [] and mlp._Deferred.armed is False and mlp._Deferred.staged == {}
    assert hook not in mlp._Deferred.before_flush
    assert torch.equal(b.grad, torch.full((5,), 4.0))
