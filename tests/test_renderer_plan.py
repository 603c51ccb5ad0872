"""The two decisions the renderer makes once per call, on plain values: what generate_neural_gaussians runs
(renderer._gen_plan: phase, rate, anchor-bound update; gaussian_renderer/__init__.py:54-63, :83) and whether render() may take the
fused expand + raster node (renderer._view_fusion).  No tensor on a device, no library call."""
import pytest
import torch

from contextgs_amd import renderer
from contextgs_amd.renderer import _gen_plan, _view_fusion


@pytest.mark.parametrize("step, decoded, phase, rate, bound", [
    (0, False, "plain", False, False),
    (3000, False, "plain", False, False),
    (3001, False, "noise", False, False),
    (10000, False, "noise", False, True),
    (10001, False, "context", True, False),
    (10001, True, "context", True, False),          # (training does not look at decoded_version, :63)
])
def test_training_plan(step, decoded, phase, rate, bound):
    plan = _gen_plan(True, step, decoded)
    assert (plan.phase, plan.predict_rate, plan.update_bound) == (phase, rate, bound)
    assert plan.predict_rate is rate and plan.update_bound is bound


@pytest.mark.parametrize("step", [0, 3000, 3001, 5000, 10000, 10001, 20000])
@pytest.mark.parametrize("decoded", [False, True])
def test_eval_plan(step, decoded):
    plan = _gen_plan(False, step, decoded)
    assert plan.phase == ("plain" if decoded else "context")        # never "noise"
    assert plan.predict_rate is False and plan.update_bound is False


def test_the_plan_is_immutable():
    with pytest.raises(AttributeError):
        _gen_plan(True, 0, False).phase = "context"


_PLAIN = dict(is_training=True, return_aux=False, return_geometry=False, antialiasing=False, cam_grad=False,
              anchor_features=None, contrib=None)


def test_a_plain_training_call_may_fuse():
    assert renderer.FUSE_VIEW, "CGS_FUSE_VIEW=0 in the environment: the default is what this test is about"
    settings = object()
    view = _view_fusion(**_PLAIN, raster_settings=settings, retain_grad=True, absgrad=True, deterministic=False)
    assert isinstance(view, renderer.ViewFusion) and view.done is None
    assert view.raster_settings is settings and view.retain_grad is True and view.absgrad is True and view.deterministic is False


@pytest.mark.parametrize("reason", [
    dict(return_aux=True), dict(return_geometry=True), dict(antialiasing=True), dict(cam_grad=True),
    dict(anchor_features=torch.zeros(4, 3)), dict(contrib=object())], ids=lambda d: next(iter(d)))
def test_each_reason_alone_refuses_the_fused_node(reason):
    assert _view_fusion(**{**_PLAIN, **reason}) is None


def test_eval_refuses_the_fused_node():
    assert _view_fusion(**{**_PLAIN, "is_training": False}) is None


def test_the_knob_and_no_grad_refuse_the_fused_node(monkeypatch):
    with torch.no_grad():
        assert _view_fusion(**_PLAIN) is None
    monkeypatch.setattr(renderer, "FUSE_VIEW", False)       # (read at call time: tests and the benchmark set it)
    assert _view_fusion(**_PLAIN) is None
