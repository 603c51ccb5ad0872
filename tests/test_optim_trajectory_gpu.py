"""The 28-iteration training trajectory of tests/test_trajectory_gpu.py, replayed with CGS_OPTIMIZER=fused_adam: the same test,
imported and not edited, must pass with its own tolerances (loss, rate, checksums, bit-equal grown anchors, one densification
round with optimizer surgery) when every optimizer step of the replay is FusedAdam's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_trajectory_with_fused_adam(monkeypatch):
    import test_trajectory_gpu as ttg
    import trajectory_common as tc
    from contextgs_amd.optim import FusedAdam
    monkeypatch.setenv("CGS_OPTIMIZER", "fused_adam")
    calls = []
    real = FusedAdam.step

    def counted(self, *args, **kwargs):
        calls.append(type(self))
        return real(self, *args, **kwargs)

    monkeypatch.setattr(FusedAdam, "step", counted)
    ttg.test_training_trajectory_matches_the_reference_loop(monkeypatch)
    g = np.load(ttg.GOLD)
    iterations = int(dict(zip((str(k) for k in g["args_names"]), g["args_values"]))["iterations"])
    expected = sum(1 for it in tc.ITERATIONS if it < iterations)          # the loop steps only while it < opt.iterations
    assert len(tc.ITERATIONS) == 28 and expected >= 27
    assert len(calls) == expected and all(c is FusedAdam for c in calls), (len(calls), expected)
