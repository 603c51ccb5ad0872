"""The per-step ledger of gradients handed between autograd nodes outside autograd (contextgs_amd/ctx_ops.py: JoinedGrads,
RateSide, the anchor counting of RowSource) on CPU tensors: what a lookup may match, what taking clears, what a step's end checks.
The routes themselves run in tests/test_ctx_level_gpu.py."""
import pytest
import torch

from contextgs_amd import ctx_ops

SIZES = [3, 4, 5]      # rows of three levels, side by side in one gradient


def _join_backward(record, g):
    """What context_model._JoinRows.backward does with the gradient of the joined tensor."""
    g = g.contiguous()
    if record is not None:
        record.note(g)
    return torch.split(g, SIZES)


def test_a_part_finds_the_prefix_right_in_front_of_it():
    rec = ctx_ops.JoinedGrads()
    g = torch.arange(12 * 6, dtype=torch.float32).reshape(12, 6)
    parts = _join_backward(rec, g)
    for part, n_prefix in ((parts[1], 3), (parts[2], 7)):
        v = rec.prefix(part, n_prefix, 6)
        assert v is not None and tuple(v.shape) == (n_prefix, 6)
        assert v.data_ptr() == g.data_ptr() and v.storage_offset() == g.storage_offset()
        assert torch.equal(v, g[:n_prefix])
        v[n_prefix - 1, 5] += 1000.0
        assert float(g[n_prefix - 1, 5]) == 1000.0 + (n_prefix - 1) * 6 + 5
    # a gradient that is itself a row range of a larger buffer: the offsets are the storage's
    whole = torch.zeros(20, 6)
    parts = _join_backward(rec, whole[8:])
    v = rec.prefix(parts[1], 3, 6)
    assert v is not None and v.storage_offset() == 8 * 6 and v.data_ptr() == whole[8:].data_ptr()


def test_nothing_else_is_taken_for_a_prefix():
    rec, other_step = ctx_ops.JoinedGrads(), ctx_ops.JoinedGrads()
    g = torch.zeros(12, 6)
    parts = _join_backward(rec, g)
    assert rec.prefix(parts[1], 3, 6) is not None
    assert other_step.prefix(parts[1], 3, 6) is None                             # another step's record
    never_noted = torch.split(torch.zeros(12, 6), SIZES)
    assert rec.prefix(never_noted[1], 3, 6) is None                              # equal shape, never noted
    assert _join_backward(None, torch.zeros(12, 6))[1] is not None               # (a join without a record notes nowhere)
    assert rec.prefix(parts[1] + never_noted[1], 3, 6) is None                   # a fresh tensor, as the engine's sum would be
    assert rec.prefix(parts[1], 4, 6) is None                                    # more rows than lie in front
    assert rec.prefix(parts[2], 3, 6) is None                                    # the prefix does not start the gradient
    assert rec.prefix(parts[0], 0, 6) is None
    assert rec.prefix(parts[1], 3, 5) is None                                    # the wrong width
    assert rec.prefix(parts[1][:, :5], 3, 5) is None and rec.prefix(parts[1][::2], 3, 6) is None      # not contiguous
    g64 = torch.zeros(12, 6, dtype=torch.float64)
    assert rec.prefix(_join_backward(rec, g64)[1], 3, 6) is None                 # fp64
    assert rec.prefix(parts[1].requires_grad_(), 3, 6) is None                   # requires_grad
    assert rec.prefix(None, 3, 6) is None
    rec.clear()
    assert rec.prefix(torch.split(g, SIZES)[1], 3, 6) is None                    # the same record, emptied


def test_rate_side_gives_once_and_takes_once():
    side = ctx_ops.RateSide()
    assert side.take() == (None,) * 5 and side.take_branch() == (None, None) and not side.lazy
    smap = torch.tensor([-1, 0, 1, -1], dtype=torch.int32)
    given = (smap, torch.ones(2, 50), torch.ones(2, 6), torch.ones(2, 30), torch.ones(2, 3))
    side.give(*given)
    with pytest.raises(AssertionError):
        side.give(*given)
    taken = side.take()
    assert len(taken) == 5 and all(a is b for a, b in zip(taken, given))
    assert side.take() == (None,) * 5
    # a level without a chosen row: an all -1 map and zero-row arrays count as absent
    side.give(torch.full((4,), -1, dtype=torch.int32), torch.ones(0, 50), torch.ones(0, 6), torch.ones(0, 30), torch.ones(0, 3))
    assert side.take() == (None,) * 5
    # a lazy level: the loan, the branch gradients with the rate gradients, the loan's end
    with pytest.raises(AssertionError):
        side.loan()
    X, W = torch.ones(4, 71), (torch.ones(100, 71), torch.ones(100), torch.ones(175, 100), torch.ones(175))
    side.lend(X, W)
    assert side.lazy and side.loan()[0] is X and side.loan()[1] is W
    dx, dW = torch.ones(2, 71), tuple(torch.zeros_like(w) for w in W)
    side.give(*given, dx=dx, dW=dW)
    with pytest.raises(AssertionError):
        side.give(*given, dx=dx, dW=dW)
    b = side.take_branch()
    assert b[0] is dx and b[1] is dW and side.take()[0] is smap
    assert side.take_branch() == (None, None) and not side.lazy
    with pytest.raises(AssertionError):
        side.loan()


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0), (1, 2, 0)])
def test_the_last_release_hands_the_anchor_buffer_on(order):
    led = ctx_ops._AnchorLedger()
    assert issubclass(ctx_ops.RowSource, ctx_ops._AnchorLedger)
    led.anchor_finish()
    for _ in range(3):
        led.anchor_register()
    with pytest.raises(RuntimeError, match="shared anchor gradient"):
        led.anchor_finish()                                      # a step that ended with registrations open
    out = []
    for k in order:
        t = led.anchor_target((7, 3), "cpu")
        assert tuple(t.shape) == (7, 3) and (k != order[0] or float(t.abs().sum()) == 0.0)
        t[k] += 1.0
        if k != order[-1]:
            with pytest.raises(RuntimeError, match="shared anchor gradient"):
                led.anchor_finish()
        out.append(led.anchor_release())
    assert out[0] is None and out[1] is None and out[2] is not None
    assert torch.equal(out[2][:3], torch.ones(3, 3)) and float(out[2][3:].abs().sum()) == 0.0
    led.anchor_finish()
