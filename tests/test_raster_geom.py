"""The rasterizer's depth-distortion and median-depth maps without a GPU: the fp64 reference (tests/raster_geom_ref.py) against
itself (the running sum equals the O(n^2) double sum; e_i and the z-term equal central differences); the two C-ABI entry
points are declared and exported and their argument errors come back with their code and a message naming the function (nothing
is launched); `check_deterministic` refuses return_geometry by name and leaves the old call forms as they were; the keyword is
off by default on every surface and the existing ValueErrors still come first."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import raster_geom_ref as ref
from raster_harness import fake_cfg

CGS_OK = 0
CGS_ERR_ARG = 1
CGS_ERR_WORKSPACE = 3

NEW_SYMBOLS = ("cgs_raster_render_geom", "cgs_raster_backward_geom")
P1 = C.c_void_p(4096)      # a non-NULL stand-in: the checks only look at which pointers are given
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against itself ----------------------------------------------------------------------------------------------
def _lists(n_lists=40, seed=0):
    rng = np.random.default_rng(seed)
    for k in range(n_lists):
        n = int(rng.integers(1, 60))
        alpha = np.minimum(0.99, rng.uniform(1 / 255, 1.0, n) ** (1 + k % 3))
        z = np.sort(rng.uniform(0.3, 7.0, n))
        if n > 3 and k % 4 == 0:
            z[2] = z[1]                 # a tie in depth
        yield alpha, z


def test_running_sum_equals_the_double_sum():
    for alpha, z in _lists():
        w = ref.list_weights(alpha)
        a, b = ref.list_distortion(w, z), ref.list_distortion_pairs(w, z)
        assert a >= 0 and abs(a - b) <= 1e-12 * max(1.0, b), (a, b)
        assert math.isclose(float(w.sum()), 1.0 - float(np.prod(1.0 - alpha)), rel_tol=1e-12)


def test_view_form_equals_the_list_form():
    """geom_maps() on a matrix whose columns are shuffled lists (rows in any order, zeros for non-contributors)."""
    rng = np.random.default_rng(3)
    P, N = 50, 12
    z = rng.uniform(0.5, 5.0, P)
    w = np.zeros((P, N))
    want_d, want_m, want_id = [], [], []
    order = np.lexsort((np.arange(P), z))
    for p in range(N):
        rows = order[np.sort(rng.choice(P, size=int(rng.integers(0, 30)), replace=False))]
        alpha = rng.uniform(0.01, 0.6 if p % 3 else 0.02, rows.size)      # every third list is too faint to reach one half
        wl = ref.list_weights(alpha) if rows.size else np.zeros(0)
        w[rows, p] = wl
        want_d.append(ref.list_distortion(wl, z[rows]))
        T_after = np.cumprod(1.0 - alpha)
        m = np.nonzero(T_after < 0.5)[0]
        want_id.append(int(rows[m[0]]) if m.size else -1)
        want_m.append(float(z[rows[m[0]]]) if m.size else 0.0)
    got = ref.geom_maps(w, z)
    assert np.allclose(got["distortion"], want_d, rtol=1e-12, atol=1e-15)
    assert (got["median_id"] == np.array(want_id)).all() and np.array_equal(got["median_depth"], np.array(want_m))
    assert -1 in want_id and max(want_id) >= 0
    assert (got["margin"] > 0).all() and (got["margin"] <= 0.5).all()
    assert (got["e"][w == 0] != 0).any()        # e_i is defined for every row; only w_i e_i vanishes off the list
    assert np.allclose((w * got["e"]).sum(0), 2.0 * got["distortion"], rtol=1e-12, atol=1e-15)      # degree 2 in w


def test_e_and_zterm_equal_central_differences():
    h = 1e-6
    for alpha, z in _lists(12, seed=1):
        z = z + np.arange(z.size) * 1e-3          # strictly increasing by more than the step: the order is fixed
        w = ref.list_weights(alpha)
        e, zt = ref.list_terms(w, z)
        scale_e, scale_z = max(np.abs(e).max(), 1e-300), max(np.abs(zt).max(), 1e-300)
        for i in range(w.size):
            d = np.zeros(w.size)
            d[i] = h
            fd_w = (ref.list_distortion(w + d, z) - ref.list_distortion(w - d, z)) / (2 * h)
            fd_z = (ref.list_distortion(w, z + d) - ref.list_distortion(w, z - d)) / (2 * h)
            assert abs(fd_w - e[i]) <= 1e-6 * scale_e, (i, fd_w, e[i])
            assert abs(fd_z - zt[i]) <= 1e-6 * scale_z, (i, fd_z, zt[i])


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------
def _render_geom(cfg=None, P=1, R=1, geom=P1, bin_ws=P1, img=P1, img_bytes=1 << 30, geom_bytes=1 << 30, bin_bytes=1 << 30,
                 dist=P1, med=P1, mid=P1, mom=P1):
    from contextgs_amd import _lib
    L = _lib.lib()
    rc = L.cgs_raster_render_geom(C.byref(cfg or fake_cfg()), P, R, geom, geom_bytes, bin_ws, bin_bytes, img, img_bytes, dist, med,
                                  mid, mom, None)
    return rc, L.cgs_last_error().decode()


def _backward_geom(P=1, R=0, geom=P1, img=P1, scratch=P1, scratch_bytes=1 << 40, m2=P1, opts=0, moments=P1, median_id=P1,
                   g_dist=P1, g_med=P1, bin_ws=None):
    """colours + scales / rotations, no features, every other pointer given"""
    from contextgs_amd import _lib
    L = _lib.lib()
    rc = L.cgs_raster_backward_geom(C.byref(fake_cfg()), P, R, P1, P1, None, 0, 0, P1, P1, P1, None, P1, geom, 1 << 30, bin_ws,
                                    1 << 40 if bin_ws else 0, img, 1 << 30, None, None, None, None, P1, m2, P1, P1, None, P1, P1,
                                    None, scratch, scratch_bytes, None, opts, None, 0, None, None, moments, median_id, g_dist, g_med)
    return rc, L.cgs_last_error().decode()


def test_entry_points_are_declared_and_exported():
    from contextgs_amd import _lib
    L = _lib.lib()
    src = open(os.path.join(ROOT, "include", "cgs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), n
        assert hasattr(L, n) and n in _lib.SIGNATURES
    # cgs_raster_render_aux's workspaces, then four outputs and the stream; cgs_raster_backward_abs's arguments, then four more
    assert len(_lib.SIGNATURES["cgs_raster_render_geom"][1]) == len(_lib.SIGNATURES["cgs_raster_render_aux"][1]) + 1
    assert _lib.SIGNATURES["cgs_raster_backward_geom"][1][:-4] == _lib.SIGNATURES["cgs_raster_backward_abs"][1]


def test_render_geom_argument_errors():
    fn = "cgs_raster_render_geom"
    for kw in (dict(dist=None), dict(med=None), dict(mid=None), dict(mom=None), dict(img=None), dict(geom=None), dict(bin_ws=None)):
        rc, msg = _render_geom(**kw)
        assert rc == CGS_ERR_ARG and "NULL" in msg and fn in msg, (kw, msg)
    for kw in (dict(P=-1), dict(R=-1)):
        rc, msg = _render_geom(**kw)
        assert rc == CGS_ERR_ARG and "P < 0 or R < 0" in msg and fn in msg, (kw, msg)
    rc, msg = _render_geom(cfg=fake_cfg(H=0))
    assert rc == CGS_ERR_ARG and "image size" in msg
    for kw, needle in ((dict(img_bytes=16), "image workspace too small"), (dict(geom_bytes=16), "geometry workspace too small"),
                       (dict(bin_bytes=16), "binning workspace too small")):
        rc, msg = _render_geom(**kw)
        assert rc == CGS_ERR_WORKSPACE and needle in msg and fn in msg, (kw, msg)
    rc, msg = _render_geom(P=0, R=0, geom=None, bin_ws=None)          # nothing to walk, nothing enqueued
    assert rc == CGS_OK, msg


def test_backward_geom_argument_errors():
    fn = "cgs_raster_backward_geom"
    for kw in (dict(moments=None), dict(median_id=None), dict(moments=None, g_med=None), dict(median_id=None, g_dist=None)):
        rc, msg = _backward_geom(**kw)
        assert rc == CGS_ERR_ARG and "needs moments" in msg and "needs median_id" in msg and fn in msg, (kw, msg)
    for kw in (dict(geom=None), dict(img=None), dict(scratch=None), dict(m2=None)):
        rc, msg = _backward_geom(**kw)
        assert rc == CGS_ERR_ARG and "NULL" in msg and fn in msg, (kw, msg)
    rc, msg = _backward_geom(R=1)           # pairs without a binning workspace
    assert rc == CGS_ERR_ARG and "NULL" in msg and fn in msg, msg
    for kw in (dict(P=-1), dict(R=-1)):
        rc, msg = _backward_geom(**kw)
        assert rc == CGS_ERR_ARG and "P < 0 or R < 0" in msg and fn in msg, (kw, msg)
    for opts in (4, 2, 1 << 31):
        rc, msg = _backward_geom(opts=opts)
        assert rc == CGS_ERR_ARG and "unknown option bits" in msg and fn in msg, (opts, msg)
    from contextgs_amd import _lib
    L = _lib.lib()
    # the scratch is cgs_raster_backward_abs's: the aux layout is too small
    rc, msg = _backward_geom(P=1000, scratch_bytes=L.cgs_raster_bwd_aux_scratch_bytes(1000))
    assert rc == CGS_ERR_WORKSPACE and "scratch too small" in msg and fn in msg, msg
    rc, msg = _backward_geom(P=1000, scratch_bytes=L.cgs_raster_bwd_abs_scratch_bytes(1000) - 1)
    assert rc == CGS_ERR_WORKSPACE and "scratch too small" in msg and fn in msg, msg
    rc, msg = _backward_geom(P=0, geom=None, img=None, scratch=None, m2=None)
    assert rc == CGS_OK, msg
    # a gradient's own map missing is an error even where the other pair is complete; no gradient: neither map is looked at
    rc, msg = _backward_geom(P=0, moments=None, median_id=None, g_dist=None, g_med=None)
    assert rc == CGS_OK, msg


# ---- Python ------------------------------------------------------------------------------------------------------------------
def test_check_deterministic_refuses_return_geometry_by_name(monkeypatch):
    from contextgs_amd.rasterizer import check_deterministic
    monkeypatch.delenv("CGS_RASTER_DETERMINISTIC", raising=False)
    with pytest.raises(ValueError, match="return_geometry"):
        check_deterministic(True, return_geometry=True)
    with pytest.raises(ValueError, match="deterministic=True does not cover return_geometry"):
        check_deterministic(True, False, None, None, True)
    assert check_deterministic(False, return_geometry=True) is False and check_deterministic(None, return_geometry=True) is False
    monkeypatch.setenv("CGS_RASTER_DETERMINISTIC", "1")
    with pytest.raises(ValueError, match="return_geometry"):
        check_deterministic(None, return_geometry=True)
    assert check_deterministic(False, return_geometry=True) is False


def test_check_deterministic_old_call_forms_are_unchanged(monkeypatch):
    from contextgs_amd.rasterizer import check_deterministic
    monkeypatch.delenv("CGS_RASTER_DETERMINISTIC", raising=False)
    assert inspect.signature(check_deterministic).parameters["return_geometry"].default is False
    assert list(inspect.signature(check_deterministic).parameters)[:4] == ["deterministic", "return_aux", "features", "contrib"]
    assert check_deterministic(True) is True and check_deterministic(True, False, None, None) is True
    assert check_deterministic(True, return_aux=False, features=None, contrib=False, return_geometry=False) is True
    assert check_deterministic(False) is False and check_deterministic(None) is False
    old = "the depth / alpha map blends, the feature blend and GaussianContrib.weight sum with float atomics (not covered: " \
          "return_aux, features, contrib)"
    for kw, name in ((dict(return_aux=True), "return_aux"), (dict(features=torch.zeros(3, 2)), "features"),
                     (dict(contrib=True), "contrib")):
        with pytest.raises(ValueError) as ei:
            check_deterministic(True, **kw)
        assert str(ei.value) == f"deterministic=True does not cover {name}: {old}"
        with pytest.raises(ValueError, match=name):          # the earlier refusals come first
            check_deterministic(True, return_geometry=True, **kw)


def test_keyword_surfaces():
    from contextgs_amd import renderer
    from contextgs_amd.dropin import diff_gaussian_rasterization as shim
    from contextgs_amd.rasterizer import GaussianRasterizer, RasterRequest
    assert inspect.signature(GaussianRasterizer.forward).parameters["return_geometry"].default is False
    assert inspect.signature(shim.GaussianRasterizer.forward).parameters["return_geometry"].default is False
    p = inspect.signature(renderer.render).parameters["return_geometry"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert RasterRequest._field_defaults["geometry"] is False
    for needle in ("return_geometry", "distortion[p]", "median_depth[p]", "median_id[p]"):
        import contextgs_amd.rasterizer as rz
        assert needle in rz.__doc__, needle


def _rasterizer(sh_degree=1):
    from contextgs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    eye = torch.eye(4)
    rs = GaussianRasterizationSettings(16, 16, math.tan(0.5), math.tan(0.5), torch.zeros(3), 1.0, eye, eye, sh_degree,
                                       torch.zeros(3), False, False)
    return GaussianRasterizer(rs)


@pytest.mark.parametrize("kw, needle", [
    (dict(scales=(5, 3), rotations=(5, 4)), "SHs or precomputed colors"),
    (dict(colors_precomp=(5, 3)), "scale/rotation pair"),
    (dict(colors_precomp=(5, 3), scales=(5, 3), rotations=(5, 4), cov3D_precomp=(5, 6)), "scale/rotation pair"),
    (dict(shs=(5, 3, 3), scales=(5, 3), rotations=(5, 4)), "SH coefficients"),
    (dict(colors_precomp=(5, 3), cov3D_precomp=(5, 5)), r"cov3D_precomp must be \[P, 6\]"),
    (dict(colors_precomp=(5, 3), scales=(5, 3), rotations=(5, 4), features=(4, 2)), "rows for 5 Gaussians"),
    (dict(colors_precomp=(5, 3), scales=(5, 3), rotations=(5, 4), means2D=(5, 4)), "absgrad=True, which was not given"),
    (dict(colors_precomp=(5, 3), scales=(5, 3), rotations=(5, 4), deterministic=True), "return_geometry"),
])
def test_existing_value_errors_come_before_any_device(kw, needle):
    kw = dict(kw)
    args = {k: (torch.zeros(v) if isinstance(v, tuple) else v) for k, v in kw.items()}
    m2 = args.pop("means2D", torch.zeros(5, 3))
    with pytest.raises(ValueError, match=needle):       # (CPU tensors: a device check would raise RuntimeError)
        _rasterizer()(means3D=torch.zeros(5, 3), means2D=m2, opacities=torch.zeros(5, 1), return_geometry=True, **args)


def test_return_geometry_has_no_cpu_path():
    P = 5
    with pytest.raises(RuntimeError, match="no CPU path"):
        _rasterizer()(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.zeros(P, 1), return_geometry=True,
                      colors_precomp=torch.zeros(P, 3), scales=torch.zeros(P, 3), rotations=torch.zeros(P, 4))
