"""The drop-in rasterizer asks the library for exactly what it asked before: every call of libcgs_hip.so that a forward +
backward makes, with its integer arguments by value and its pointers as "ptr" / "null", against tests/golden/raster_calls.json.

The fixture was recorded on the MI355X by tools/raster_call_record.py AT THE PARENT of the change that introduced RasterRequest
(the node's flags as one record, outputs and gradients by name); the cases, the scenes and the recording proxy are that file's, so
both sides run the same code around the rasterizer.  What is pinned: the choice of cgs_raster_backward* entry point, the
pattern of NULL gradients and optional inputs, P, R, D, M, opts, C, means2D_cols and every byte size, on the non-speculative
and on the speculative path of bin_and_blend (each case runs twice from an empty pair capacity), with 64 Gaussians in view,
with all of them behind the camera (R = 0) and with none (P = 0).  A change that is MEANT to alter a call records the fixture
again at its own parent and says which lines moved.  Nothing is provoked: the proxy notes calls the rasterizer makes anyway."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("raster_call_record",
                                               os.path.join(os.path.dirname(_HERE), "tools", "raster_call_record.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(os.path.join(_HERE, "golden", "raster_calls.json")) as _f:
    GOLDEN = json.load(_f)["calls"]


def test_the_fixture_holds_every_case():
    assert set(GOLDEN) == {rec.key(c, s) for c in rec.CASES for s in rec.SCENES}
    want = {"plain", "return_aux", "features", "contrib", "contrib_slots", "absgrad", "deterministic", "return_geometry",
            "return_normals", "antialiasing", "shs_cov", "combined", "combined_distortion_only", "combined_features_only",
            "viewmatrix_grad"}
    assert want <= set(rec.CASES)
    # the three losses of the combined case end in three different backward calls
    ends = {c: [call[0] for call in GOLDEN[rec.key(c, "visible")] if call[0].startswith("cgs_raster_backward")]
            for c in ("combined", "combined_distortion_only", "combined_features_only")}
    assert all(len(v) == 2 for v in ends.values()), ends
    null_patterns = {c: tuple(a for a in next(call for call in GOLDEN[rec.key(c, "visible")] if call[0] == ends[c][0])
                              if a in ("ptr", "null")) for c in ends}
    assert len(set(null_patterns.values())) == 3, "the three losses do not differ in which gradients are NULL"


@pytest.mark.parametrize("scene", rec.SCENES)
@pytest.mark.parametrize("case", list(rec.CASES))
def test_calls_are_the_recorded_ones(case, scene):
    calls, outs = rec.record(case, scene)
    want = GOLDEN[rec.key(case, scene)]
    names = [c[0] for c in calls]
    assert names == [c[0] for c in want], f"entry points differ: {names} vs {[c[0] for c in want]}"
    for i, (got, ref) in enumerate(zip(calls, want)):
        assert got == ref, f"call {i} ({got[0]}): argument(s) {[j for j, (a, b) in enumerate(zip(got, ref)) if a != b]} differ"
    if scene == "visible":      # the first run took the non-speculative render, the second the speculative one
        assert names.count("cgs_raster_render") == 1 and names.count("cgs_raster_render_spec") == 1
    # the forward has no atomics: two runs give the same bits in every output
    assert set(outs[0]) == set(outs[1])
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
