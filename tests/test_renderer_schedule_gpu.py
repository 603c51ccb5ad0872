"""The launch ORDER of a training view (renderer.generate_neural_gaussians): which work is in the queue before which host
read-back.  Host call order on the one stream is queue order, so the order in which a step asks the library for its entry points
is the order of the launches.  The second step=20000 step of a 12 000-anchor scene (cached plan, default knobs) with
contextgs_amd._lib.lib replaced by a proxy that notes every entry point it hands out; only the forward (render()) is recorded.
Nothing is provoked: names are noted around calls the step makes anyway."""
import pytest
import torch

from test_training_gpu import _ctx_step, _setup

pytestmark = pytest.mark.gpu


class _Recorder:
    def __init__(self, handle, names):
        self._handle, self._names = handle, names

    def __getattr__(self, name):
        self._names.append(name)
        return getattr(self._handle, name)


def _recorded_forward(early_mlp3=True):
    """(entry-point names of the second step's render() in call order, number of non-empty levels)"""
    from contextgs_amd import _lib, renderer
    pc, cams, pipe, bg = _setup(N=12000, W=256, H=144, seed=7)
    _ctx_step(pc, cams[0], pipe, bg)                     # builds the plan
    for p in pc.parameters():
        p.grad = None
    vis = renderer.prefilter_voxel(cams[1], pc, pipe, bg)
    names, real = [], _lib.lib
    handle = real()
    prev, renderer.EARLY_MLP3 = renderer.EARLY_MLP3, early_mlp3
    _lib.lib = lambda: _Recorder(handle, names)
    try:
        pkg = renderer.render(cams[1], pc, pipe, bg, visible_mask=vis, step=20000)
    finally:
        _lib.lib, renderer.EARLY_MLP3 = real, prev
    loss = (1.0 - pkg["render"]).abs().mean() + 0.001 * pkg["bit_per_param"]
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    return names, sum(1 for s in pc._level_cache["sizes"] if s > 0)


def _first(names, pred):
    pred_ = pred if callable(pred) else (lambda n: n == pred)
    hits = [i for i, n in enumerate(names) if pred_(n)]
    assert hits, f"{pred} was not called; recorded: {sorted(set(names))}"
    return hits[0]


def _in_order(names, *preds):
    at = [_first(names, p) for p in preds]
    assert at == sorted(at) and len(set(at)) == len(at), list(zip([p if isinstance(p, str) else p.__name__ for p in preds], at))


def level_forward(n):
    return n.startswith("cgs_ctx_level_fwd")


def rate_entry(n):
    return n.startswith("cgs_rate_") or n.startswith("cgs_level_rate_")


MLP3 = "cgs_anchor_mlp3_forward_rows_t"


def test_launch_order_of_a_training_view():
    names, levels = _recorded_forward()
    print("[schedule]", " ".join(names))
    # everything that does not need the visible list is in the queue before its count is read
    _in_order(names, "cgs_nonzero_launch", "cgs_ctx_choose_flags_slots", "cgs_hyper_noise_gather", level_forward, "cgs_nonzero_wait")
    # the anchor MLPs are in the queue before the context model's read-back
    _in_order(names, "cgs_nonzero_wait", MLP3, "cgs_ctx_choose_compact")
    assert names.count(MLP3) == 1, "the early launch was dropped and repeated"
    assert levels >= 2 and sum(level_forward(n) for n in names) == levels
    # the rate model goes between the expansion's count launch and its wait; the fused node follows
    first_rate = names[_first(names, rate_entry)]
    print("[schedule] first rate entry:", first_rate)
    _in_order(names, "cgs_expand_count_launch", first_rate, "cgs_expand_count_wait", "cgs_raster_preprocess_expand_launch")


def test_without_the_early_mlp_launch_the_mlps_follow_the_read_back():
    names, _levels = _recorded_forward(early_mlp3=False)
    _in_order(names, "cgs_ctx_choose_compact", MLP3)
    assert names.count(MLP3) == 1
