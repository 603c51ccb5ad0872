"""The fused MLP nodes ask the library for exactly what they asked before: every call of libcgs_hip.so that a forward + backward
of _MLP2, _LevelMLP, _AnchorMLP3, _AnchorMLP3Rows and _AnchorGen makes, with its integer arguments by value and its pointers as
"ptr" / "null", against tests/golden/mlp_calls.json.

The fixture was recorded on the MI355X by tools/mlp_call_record.py AT THE PARENT of the change that gave the four MLP nodes one
weight-gradient hand-off (mlp._WeightGrads) and one carve of the anchor heads' gradient buffers; the cases are that file's and
the recording proxy is tools/raster_call_record.py's, so both sides run the same code around the nodes.  What is pinned: the
entry points and their order (the data-only backward + cgs_*_wgrad at the end of the backward when deferred, one fused call
inline), which gradient pointers are NULL, every size, stride and flag, the workspace bytes, the queries
(cgs_mlp_wgrad_scratch_bytes, cgs_anchor_mlp3_layout) and the calls of zero_unlisted_rows / gather_rows_nograd — at 37 rows
(two 16-row tiles and a ragged tail) out of 45, a `loc` of 5 rows, and at n = 0.  A change that is MEANT to alter a call
records the fixture again at its own parent and says which lines moved.  Nothing is provoked: the proxy notes calls the nodes
make anyway."""
import importlib.util
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_TOOLS = os.path.join(os.path.dirname(_HERE), "tools")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_TOOLS, name + ".py"))
    mod = sys.modules[name] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_load("raster_call_record")         # (mlp_call_record imports the proxy from it)
rec = _load("mlp_call_record")

with open(os.path.join(_HERE, "golden", "mlp_calls.json")) as _f:
    GOLDEN = json.load(_f)["calls"]


def test_the_fixture_holds_every_case():
    assert set(GOLDEN) == {rec.key(c, m) for c in rec.CASES for m in rec.MODES}
    want = {"mlp2_stored", "mlp2_recompute", "mlp2_recompute_off", "mlp2_weights_nonleaf", "level_both", "level_qadj_only",
            "level_pred_only", "level_empty_loc", "anchor_mlp3", "rows_pre", "anchor_gen", "mlp2_n0", "anchor_mlp3_n0", "rows_n0",
            "anchor_gen_n0"} | {f"rows_keep{k}_tiled{t}_{s}" for k in (0, 1) for t in (0, 1) for s in ("sub", "all")}
    assert want <= set(rec.CASES)
    names = lambda k: [c[0] for c in GOLDEN[k]]
    # deferred: the weight-gradient products are launches of their own; a non-leaf weight and an empty node never defer
    assert names("mlp2_stored/deferred").count("cgs_mlp2_wgrad") == 2 and "cgs_mlp2_wgrad" not in names("mlp2_stored/inline")
    assert names("level_both/deferred").count("cgs_mlp2_wgrad") == 4
    assert names("anchor_mlp3/deferred").count("cgs_anchor_mlp3_wgrad") == 2
    for k in ("mlp2_weights_nonleaf", "mlp2_n0", "anchor_mlp3_n0", "rows_n0", "anchor_gen"):
        assert GOLDEN[k + "/deferred"] == GOLDEN[k + "/inline"], k
    # the recomputing kernel is handed dW2 / db2 even when deferred; the kernel with a stored hidden layer is not
    grads = lambda k: next(c for c in GOLDEN[k] if c[0] == "cgs_mlp2_backward")[19:23]
    assert grads("mlp2_recompute/deferred") == ["null", "null", "ptr", "ptr"]
    assert grads("mlp2_recompute_off/deferred") == ["null"] * 4 and grads("mlp2_recompute/inline") == ["ptr"] * 4


@pytest.mark.parametrize("mode", rec.MODES)
@pytest.mark.parametrize("case", list(rec.CASES))
def test_calls_are_the_recorded_ones(case, mode):
    calls, res = rec.record(case, mode)
    want = GOLDEN[rec.key(case, mode)]
    names = [c[0] for c in calls]
    assert names == [c[0] for c in want], f"entry points differ: {names} vs {[c[0] for c in want]}"
    for i, (got, ref) in enumerate(zip(calls, want)):
        assert got == ref, f"call {i} ({got[0]}): argument(s) {[j for j, (a, b) in enumerate(zip(got, ref)) if a != b]} differ"
    # no atomics on these paths: two runs give the same bits in every output and every gradient
    assert len(res[0]) == len(res[1])
    for i, (u, v) in enumerate(zip(*res)):
        assert (u is None and v is None) or torch.equal(u, v), i
