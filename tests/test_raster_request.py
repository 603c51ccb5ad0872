"""The drop-in rasterizer's request record and its name tables (contextgs_amd/rasterizer.py: RasterRequest, output_names,
named_extras, NON_DIFFERENTIABLE, INPUT_NAMES) against the index arithmetic they replaced, which is spelled out here.  No
tensor on a device, no library call."""
import inspect
import itertools

import pytest

from contextgs_amd import rasterizer as rz

FLAGS = list(itertools.product((False, True), repeat=5))        # aux, contrib, geometry, features, normals: 32 combinations


def _request(aux, contrib, geometry, normals):
    return rz.RasterRequest(aux=aux, contrib=object() if contrib else None, geometry=geometry, normals=3 if normals else 0)


@pytest.mark.parametrize("aux, contrib, geometry, features, normals", FLAGS)
def test_every_output_sits_where_the_old_arithmetic_put_it(aux, contrib, geometry, features, normals):
    request = _request(aux, contrib, geometry, normals)
    has_features = features or normals          # the normals ride on the feature walk: the node then has a feature matrix
    names = rz.output_names(request, has_features)
    assert rz.output_names(request.flags(), has_features) == names      # the backward's view of the same request
    assert names[:2] == ("color", "radii")
    if aux:
        assert names[2:5] == ("depth", "invdepth", "alpha")
    k = 5 if aux else 2
    if contrib:
        assert names[k:k + 3] == ("top_id", "top_weight", "count")
    k = 2 + (3 if aux else 0) + (3 if contrib else 0)
    if geometry:
        assert names[k:k + 3] == ("distortion", "median_depth", "median_id")
        geom_at = k - 2     # the old ctx.geom_at = len(outs) - 2, an index into the backward's *grad_rest (behind color, radii)
        assert names[2:][geom_at:geom_at + 2] == ("distortion", "median_depth")
    if has_features:
        assert names[-1] == "features" and names.count("features") == 1
    assert len(names) == 2 + 3 * aux + 3 * contrib + 3 * geometry + bool(has_features)
    assert len(set(names)) == len(names)
    for absent, given in ((("depth", "invdepth", "alpha"), aux), (("top_id", "top_weight", "count"), contrib),
                          (("distortion", "median_depth", "median_id"), geometry), (("features",), has_features)):
        assert all((n in names) == bool(given) for n in absent)


@pytest.mark.parametrize("aux, contrib, geometry, features, normals", FLAGS)
def test_extras_by_name_are_the_old_slices(aux, contrib, geometry, features, normals):
    request = _request(aux, contrib, geometry, normals)
    has_features = features or normals
    names = rz.output_names(request, has_features)
    out = tuple(f"out{i}" for i in range(len(names)))       # stand-ins: only identity matters
    if has_features:        # the feature map as a list of channels, user channels first
        out = out[:-1] + ([f"c{i}" for i in range((2 if features else 0) + (3 if normals else 0))],)
    if len(names) == 2:
        assert not (aux or contrib or geometry or has_features)     # the call that returns (color, radii) alone
        return
    extras = rz.named_extras(request, features, dict(zip(names, out)))
    want = {}
    if aux:
        want.update(depth=out[2], invdepth=out[3], alpha=out[4])
    if contrib:
        k = 5 if aux else 2
        want.update(contrib=request.contrib, top_id=out[k], top_weight=out[k + 1], count=out[k + 2])
    if geometry:
        k = 2 + (3 if aux else 0) + (3 if contrib else 0)
        want.update(distortion=out[k], median_depth=out[k + 1], median_id=out[k + 2])
    if features:
        want["features"] = out[-1][:-3] if normals else out[-1]
    if normals:
        want["normals"] = out[-1][-3:]
    assert extras == want and list(extras) == list(want)
    if contrib:
        assert extras["contrib"] is request.contrib
    if features and normals:
        assert extras["features"] == ["c0", "c1"] and extras["normals"] == ["c2", "c3", "c4"]


def test_the_non_differentiable_outputs():
    assert rz.NON_DIFFERENTIABLE == {"radii", "top_id", "top_weight", "count", "median_id"}
    everything = rz.output_names(rz.RasterRequest(aux=True, contrib=object(), geometry=True), True)
    assert rz.NON_DIFFERENTIABLE < set(everything)
    assert [n for n in everything if n not in rz.NON_DIFFERENTIABLE] == [
        "color", "depth", "invdepth", "alpha", "distortion", "median_depth", "features"]


def test_every_field_of_the_request_defaults_to_off():
    assert rz.RasterRequest._fields == ("aux", "contrib", "contrib_slots", "absgrad", "deterministic", "geometry", "normals")
    assert set(rz.RasterRequest._field_defaults) == set(rz.RasterRequest._fields)
    assert all(v is None or v is False or (v == 0 and type(v) is int) for v in rz.RasterRequest._field_defaults.values())
    assert rz.output_names(rz.RasterRequest(), False) == ("color", "radii")


def test_the_kept_flags_hold_no_object():
    slots, contrib = object(), object()
    kept = rz.RasterRequest(True, contrib, slots, True, False, True, 3).flags()
    assert kept == rz.RasterRequest(True, True, None, True, False, True, 3)
    assert rz.RasterRequest().flags() == rz.RasterRequest()


def test_keywords_are_those_of_the_rasterizer():
    request = rz.RasterRequest(True, "c", "s", True, True, True, 3)
    kw = request.keywords()
    assert kw == dict(return_aux=True, contrib="c", contrib_slots="s", absgrad=True, deterministic=True, return_geometry=True,
                      return_normals=True)
    params = inspect.signature(rz.GaussianRasterizer.forward).parameters
    assert set(kw) <= set(params)
    off = rz.RasterRequest().keywords()
    assert all(off[k] == params[k].default for k in off if k != "deterministic") and off["deterministic"] is False


def test_input_names_are_the_forward_s_parameters():
    params = list(inspect.signature(rz._RasterizeGaussians.forward).parameters)
    assert params[0] == "ctx" and tuple(params[1:]) == rz.INPUT_NAMES
    assert len(rz.INPUT_NAMES) == len(params) - 1 == 14
    # the one non-tensor argument that replaced the flags comes first, features (a tensor: it gets a gradient) stays an input
    assert rz.INPUT_NAMES[0] == "request" and rz.INPUT_NAMES[-1] == "features"
    assert rz.INPUT_NAMES[10:13] == ("viewmatrix", "projmatrix", "campos")      # the old ctx.needs_input_grad[10:13]
