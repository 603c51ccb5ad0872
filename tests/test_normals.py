"""Normal maps and the normal-consistency regulariser without a GPU: the numpy restatement (tests/normals_ref.py) against the
reference's own outputs (tests/golden/depth_normals.npz, written by tools/make_normals_golden.py) and against central
differences; the fp32 restatement against the fp64 one at HALF of every cap the GPU tests apply, on exactly their inputs (the
run that admits those inputs: change a seed, never a cap); the hemisphere scene on the raster oracle; the six C-ABI entry
points declared and exported, with their argument errors by name (nothing is launched); every ValueError of the keyword."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import normals_ref as ref

CGS_OK = 0
CGS_ERR_ARG = 1
NEW_SYMBOLS = ("cgs_gaussian_normals_fwd", "cgs_gaussian_normals_bwd", "cgs_depth_normals_fwd", "cgs_depth_normals_bwd",
               "cgs_normal_consistency_fwd", "cgs_normal_consistency_bwd")
P1 = C.c_void_p(4096)      # a non-NULL stand-in: the checks only look at which pointers are given
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX, TY = ref.TAN


# ---- the restatement against the reference's outputs ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "depth_normals.npz"))


@pytest.mark.parametrize("kind", ["smooth", "rough", "constant"])
def test_restatement_matches_the_reference_at_its_eps(golden, kind):
    depth = golden[kind + "_depth"]
    assert depth.shape == (1, 24, 40) and np.array_equal(depth, ref.depth_case(kind, 24, 40))
    if kind != "constant":
        assert (depth[0][ref.HOLE] == 0).all() and (depth > 0).sum() == 24 * 40 - 40
    tx, ty = float(golden["tanfovx"]), float(golden["tanfovy"])
    want = golden[kind + "_normals"]
    assert want.shape == (3, 24, 40) and np.isfinite(want).all()
    ref.check_map(ref.depth_normals(depth, tx, ty, 1e-5), want, f"{kind}, fp64 restatement vs the reference")
    ref.check_map(ref.depth_normals(depth, tx, ty, 1e-5, np.float32), want, f"{kind}, fp32 restatement vs the reference")
    if kind != "constant":      # the undrawn region: 0, where a sqrt-of-squares restatement has NaN gradients
        assert (want[:, 6:8, 11:19] == 0).all() and (ref.depth_normals(depth, tx, ty, 1e-5)[:, 6:8, 11:19] == 0).all()


def test_constant_depth_gives_plus_z(golden):
    """The hemisphere: a fronto-parallel plane has the normal (0, 0, +z), in the reference and in the restatement."""
    for N in (golden["constant_normals"], ref.depth_normals(golden["constant_depth"], TX, TY, 1e-5),
              ref.depth_normals(golden["constant_depth"], TX, TY, 0.0, np.float32)):
        assert (N[:2] == 0).all() and (N[2] > 0.99).all()
    assert np.allclose(ref.depth_normals(golden["constant_depth"], TX, TY, 0.0)[2], 1.0, rtol=0, atol=1e-12)


# ---- the restatement against itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 1e-5])
def test_depth_gradients_equal_central_differences(eps):
    H, W = 9, 11
    x = ref.pixel_inputs("smooth", H, W)
    d = x["depth"].astype(np.float64)         # (float32 values: the restatement reads its inputs as float32)
    g_n = ref.depth_normals_bwd(d, TX, TY, eps, x["gN"])
    dn, g_e = ref.normal_consistency_bwd(x["normals"], d, TX, TY, x["weight"], eps, x["gE"])
    h = 2.0 ** -10                            # a float32 step at depth ~2
    fd_n, fd_e = np.zeros((H, W)), np.zeros((H, W))
    for v in range(H):
        for u in range(W):
            lo, hi = d.copy(), d.copy()
            lo[0, v, u] -= h
            hi[0, v, u] += h
            fd_n[v, u] = ((ref.depth_normals(hi, TX, TY, eps) - ref.depth_normals(lo, TX, TY, eps)) * x["gN"]).sum() / (2 * h)
            fd_e[v, u] = ((ref.normal_consistency(x["normals"], hi, TX, TY, x["weight"], eps)
                           - ref.normal_consistency(x["normals"], lo, TX, TY, x["weight"], eps)) * x["gE"][0]).sum() / (2 * h)
    assert np.abs(fd_n - g_n).max() <= 2e-3 * np.abs(g_n).max(), np.abs(fd_n - g_n).max() / np.abs(g_n).max()
    assert np.abs(fd_e - g_e).max() <= 2e-3 * np.abs(g_e).max(), np.abs(fd_e - g_e).max() / np.abs(g_e).max()
    N = ref.depth_normals(d, TX, TY, eps)
    k = -(x["weight"][0].astype(np.float64) * x["gE"][0])
    assert np.allclose(dn, k * N, rtol=0, atol=1e-15)       # E is linear in `normals`


def test_gaussian_gradient_equals_central_differences():
    V = ref.view_matrix()
    x = ref.gaussian_inputs(40, seed=3)
    got = ref.gaussian_normals_bwd(x["means3D"], x["scales"], x["rotations"], V, x["g"])
    h = 2.0 ** -12
    fd = np.zeros_like(got)
    for j in range(4):
        lo, hi = x["rotations"].astype(np.float64), x["rotations"].astype(np.float64)
        lo[:, j] -= h
        hi[:, j] += h
        # (steps that stay float32 values: the restatement rounds its inputs to float32 first)
        lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
        a = ref.gaussian_normals(x["means3D"], x["scales"], lo32, V)["n"]
        b = ref.gaussian_normals(x["means3D"], x["scales"], hi32, V)["n"]
        fd[:, j] = ((b - a) * x["g"]).sum(1) / (hi32[:, j].astype(np.float64) - lo32[:, j])
    assert np.abs(fd - got).max() <= 1e-4 * np.abs(got).max(), np.abs(fd - got).max() / np.abs(got).max()
    # through the normalisation: the gradient is orthogonal to q
    assert np.abs((got * x["rotations"]).sum(1)).max() <= 1e-12 * np.abs(got).max() * 3.0


def test_gaussian_normals_definition():
    V = ref.view_matrix()
    x = ref.gaussian_inputs(257, seed=257)
    f = ref.gaussian_normals(x["means3D"], x["scales"], x["rotations"], V)
    assert np.allclose(np.linalg.norm(f["n"], axis=1), 1.0, atol=1e-12)                 # unnormalised quaternions: unit normals
    t = x["means3D"].astype(np.float64) @ V.astype(np.float64)[:3, :3] + V[3, :3]
    assert ((f["n"] * t).sum(1) >= 0).all() and (t[:, 2] < 0).sum() > 20                # away from the camera, also behind it
    s = x["scales"]
    assert (s[np.arange(257), f["k"]] == s.min(1)).all()
    assert (f["k"][::11] == 0).all()                                                     # ties go to the lowest index
    two_small = (s[:, 1] == s[:, 2]) & (s[:, 0] > s[:, 1])
    assert two_small.sum() > 20 and (f["k"][two_small] == 1).all()
    assert set(np.unique(f["k"])) == {0, 1, 2}
    assert ref.gaussian_normals(x["means3D"][:0], x["scales"][:0], x["rotations"][:0], V)["n"].shape == (0, 3)


@pytest.mark.parametrize("H, W", ref.THIN)
def test_one_pixel_wide_or_high_is_exactly_zero(H, W):
    x = ref.pixel_inputs("rough", H, W)
    for eps in (0.0, 1e-5):
        for dt in (np.float32, np.float64):
            assert (ref.depth_normals(x["depth"], TX, TY, eps, dt) == 0).all()
            assert (ref.depth_normals_bwd(x["depth"], TX, TY, eps, x["gN"], dt) == 0).all()
            assert (ref.normal_consistency(x["normals"], x["depth"], TX, TY, x["weight"], eps, dt) == 1).all()
            dn, dd = ref.normal_consistency_bwd(x["normals"], x["depth"], TX, TY, x["weight"], eps, x["gE"], dt)
            assert (dn == 0).all() and (dd == 0).all()


# ---- the run that admits the GPU tests' inputs: fp32 alone stays within half of every cap ---------------------------------------
@pytest.mark.parametrize("kind", ["smooth", "rough"])
@pytest.mark.parametrize("H, W", ref.SHAPES)
def test_fp32_restatement_within_half_caps_per_pixel(H, W, kind):
    x = ref.pixel_inputs(kind, H, W)
    for eps in (0.0, 1e-5):
        what = f"{H}x{W} {kind} eps {eps:g}, fp32 vs fp64"
        a, b = (ref.depth_normals(x["depth"], TX, TY, eps, dt) for dt in (np.float32, np.float64))
        assert a.dtype == np.float32 and np.isfinite(b).all()
        ref.check_map(a, b, f"depth normals {what}", cap=0.5)
        a, b = (ref.depth_normals_bwd(x["depth"], TX, TY, eps, x["gN"], dt) for dt in (np.float32, np.float64))
        assert a.dtype == np.float32 and np.isfinite(b).all()
        ref.check_grad(a, b, f"dL/ddepth of the normals {what}", cap=0.5)
        for w in (None, x["weight"]):
            a, b = (ref.normal_consistency(x["normals"], x["depth"], TX, TY, w, eps, dt) for dt in (np.float32, np.float64))
            ref.check_map(a, b, f"E {what}", cap=0.5)
            a, b = (ref.normal_consistency_bwd(x["normals"], x["depth"], TX, TY, w, eps, x["gE"], dt)
                    for dt in (np.float32, np.float64))
            assert a[0].dtype == np.float32 and a[1].dtype == np.float32
            ref.check_grad(a[0], b[0], f"dL/dnormals {what}", cap=0.5)
            ref.check_grad(a[1], b[1], f"dL/ddepth of E {what}", cap=0.5)


@pytest.mark.parametrize("P", [1, 200, 257])
def test_fp32_restatement_within_half_caps_per_gaussian(P):
    V = ref.view_matrix()
    x = ref.gaussian_inputs(P, seed=P)
    a, b = (ref.gaussian_normals(x["means3D"], x["scales"], x["rotations"], V, dt) for dt in (np.float32, np.float64))
    ok = b["margin"] >= 1e-4
    assert (~ok).sum() <= 0.01 * P * 0.5 and (a["k"] == b["k"]).all()
    ref.check_map(a["n"][ok], b["n"][ok], f"P = {P}, fp32 vs fp64", cap=0.5)
    ga, gb = (ref.gaussian_normals_bwd(x["means3D"], x["scales"], x["rotations"], V, x["g"], dt) for dt in (np.float32, np.float64))
    assert ga.dtype == np.float32
    ref.check_grad(ga[ok], gb[ok], f"dL/drotations P = {P}, fp32 vs fp64", cap=0.5)


def test_hemispheres_agree_on_the_oracle(oracle64):
    """The scene of the GPU test, on the CPU: the raster oracle blends the restated per-Gaussian normals and (z, 1) as colours
    over a zero background; against the restated depth normals of depth / alpha the mean cosine is near +1.  With the other
    hemisphere for either side it is near -1: the scene tells the two apart."""
    cam, g = ref.plane_scene()
    V = np.asarray(cam.world_view_transform, np.float32)
    f = ref.gaussian_normals(g["means3D"], g["scales"], g["rotations"], V)
    stored = ref._columns(g["rotations"].astype(np.float64))[np.arange(len(f["k"])), f["k"]] @ V.astype(np.float64)[:3, :3]
    flipped = (stored * f["n"]).sum(1) < 0
    assert 0.3 < flipped.mean() < 0.7 and set(np.unique(f["k"])) == {0, 1, 2}       # the axes as stored point to either side
    z = g["means3D"].astype(np.float64) @ V.astype(np.float64)[:3, 2] + V[3, 2]
    cd = cam.oracle_dict(bg=(0.0, 0.0, 0.0))
    nm = oracle64.render(cd, g["means3D"], f["n"], g["opacities"], g["scales"], g["rotations"])["color"]
    da = oracle64.render(cd, g["means3D"], np.stack([z, np.ones_like(z), np.zeros_like(z)], 1), g["opacities"], g["scales"],
                         g["rotations"])["color"]
    tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    mean, n = ref.hemisphere_agreement(nm, da[0:1], da[1:2], tx, ty)
    print(f"[hemisphere] oracle + restatement: mean cosine {mean:.4f} over {n} pixels")
    assert n > 1500 and mean > 0.9
    assert ref.hemisphere_agreement(-nm, da[0:1], da[1:2], tx, ty)[0] < -0.9


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------
def _view_cfg(view=P1):
    from contextgs_amd import _lib
    return _lib.RasterCfg(image_height=16, image_width=16, tanfovx=0.5, tanfovy=0.5, scale_modifier=1.0, prefiltered=0,
                          debug=0, viewmatrix=view, projmatrix=P1, campos=P1, bg=P1)


def _call(name, *args):
    from contextgs_amd import _lib
    L = _lib.lib()
    rc = getattr(L, name)(*args)
    return rc, L.cgs_last_error().decode()


def test_entry_points_are_declared_and_exported():
    from contextgs_amd import _lib
    L = _lib.lib()
    src = open(os.path.join(ROOT, "include", "cgs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), n
        assert hasattr(L, n) and n in _lib.SIGNATURES
    # the per-pixel entry points take H, W, tanfovx, tanfovy, eps and not the whole cgs_raster_cfg
    for n in NEW_SYMBOLS[2:]:
        assert _lib.SIGNATURES[n][1][:5] == [C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float], n
    assert len(_lib.SIGNATURES["cgs_normal_consistency_bwd"][1]) == 5 + 7


def test_gaussian_normals_argument_errors():
    for fn, n_ptr in (("cgs_gaussian_normals_fwd", 4), ("cgs_gaussian_normals_bwd", 5)):
        full = [P1] * n_ptr
        rc, msg = _call(fn, None, 1, *full, None)
        assert rc == CGS_ERR_ARG and "cfg is NULL" in msg and fn in msg, msg
        rc, msg = _call(fn, C.byref(_view_cfg()), -1, *full, None)
        assert rc == CGS_ERR_ARG and "P < 0" in msg and fn in msg, msg
        rc, msg = _call(fn, C.byref(_view_cfg()), 1 << 39, *full, None)
        assert rc == CGS_ERR_ARG and "beyond one launch" in msg and fn in msg, msg
        rc, msg = _call(fn, C.byref(_view_cfg(view=None)), 1, *full, None)
        assert rc == CGS_ERR_ARG and "viewmatrix is NULL" in msg and fn in msg, msg
        for i in range(n_ptr):
            args = list(full)
            args[i] = None
            rc, msg = _call(fn, C.byref(_view_cfg()), 1, *args, None)
            assert rc == CGS_ERR_ARG and "NULL" in msg and fn in msg, (i, msg)
        rc, msg = _call(fn, C.byref(_view_cfg()), 0, *([None] * n_ptr), None)         # nothing to do, nothing enqueued
        assert rc == CGS_OK, msg


@pytest.mark.parametrize("fn, n_ptr, optional", [("cgs_depth_normals_fwd", 2, ()), ("cgs_depth_normals_bwd", 3, ()),
                                                 ("cgs_normal_consistency_fwd", 4, (2,)),
                                                 ("cgs_normal_consistency_bwd", 6, (2, 4, 5))])
def test_per_pixel_argument_errors(fn, n_ptr, optional):
    """Every path below fails its checks before anything is enqueued (the pointers are stand-ins)."""
    full = [P1] * n_ptr
    for H, W in ((0, 4), (4, 0), (-1, 4), (65536, 4), (4, 65536)):
        rc, msg = _call(fn, H, W, 0.5, 0.5, 0.0, *full, None)
        assert rc == CGS_ERR_ARG and "image size" in msg and fn in msg, msg
    for tx, ty in ((0.0, 0.5), (0.5, -1.0), (float("nan"), 0.5), (0.5, float("inf"))):
        rc, msg = _call(fn, 4, 4, tx, ty, 0.0, *full, None)
        assert rc == CGS_ERR_ARG and "tanfovx, tanfovy" in msg and fn in msg, msg
    for eps in (-1e-6, float("nan"), float("inf")):
        rc, msg = _call(fn, 4, 4, 0.5, 0.5, eps, *full, None)
        assert rc == CGS_ERR_ARG and "eps" in msg and fn in msg, msg
    for i in range(n_ptr):
        if i in optional:       # weight, or one of the loss backward's two outputs: the call would launch, so it is not made here
            continue
        args = list(full)
        args[i] = None
        rc, msg = _call(fn, 4, 4, 0.5, 0.5, 0.0, *args, None)
        assert rc == CGS_ERR_ARG and "NULL" in msg and fn in msg, (i, msg)
    if fn == "cgs_normal_consistency_bwd":      # either output may be NULL, not both
        rc, msg = _call(fn, 4, 4, 0.5, 0.5, 0.0, P1, P1, P1, P1, None, None, None)
        assert rc == CGS_ERR_ARG and "no output given" in msg and fn in msg, msg


# ---- Python ------------------------------------------------------------------------------------------------------------------
def _rasterizer(view=None):
    from contextgs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    eye = torch.eye(4)
    rs = GaussianRasterizationSettings(16, 16, math.tan(0.5), math.tan(0.5), torch.zeros(3), 1.0, eye if view is None else view,
                                       eye, 1, torch.zeros(3), False, False)
    return GaussianRasterizer(rs)


def _forward(rast=None, P=5, **kw):
    args = dict(colors_precomp=torch.zeros(P, 3), scales=torch.zeros(P, 3), rotations=torch.zeros(P, 4))
    args.update(kw)
    return (rast or _rasterizer())(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.zeros(P, 1),
                                   return_normals=True, **args)


def test_return_normals_value_errors_come_before_any_device(monkeypatch):
    monkeypatch.delenv("CGS_RASTER_DETERMINISTIC", raising=False)
    # (CPU tensors: a device check would raise RuntimeError)
    with pytest.raises(ValueError, match="return_normals=True needs scales and rotations"):
        _forward(scales=None, rotations=None, cov3D_precomp=torch.zeros(5, 6))
    with pytest.raises(ValueError, match="features has 30 columns, more than 29"):
        _forward(features=torch.zeros(5, 30))
    with pytest.raises(ValueError, match="deterministic=True does not cover return_normals"):
        _forward(deterministic=True)
    with pytest.raises(ValueError, match="viewmatrix that requires a gradient"):
        _forward(_rasterizer(view=torch.eye(4, requires_grad=True)))
    monkeypatch.setenv("CGS_RASTER_DETERMINISTIC", "1")
    with pytest.raises(ValueError, match="return_normals"):
        _forward()
    monkeypatch.delenv("CGS_RASTER_DETERMINISTIC")
    # the existing errors still come first
    with pytest.raises(ValueError, match="SHs or precomputed colors"):
        _forward(colors_precomp=None)
    with pytest.raises(ValueError, match="outside 1..32"):
        _forward(features=torch.zeros(5, 33))
    with pytest.raises(ValueError, match="deterministic=True does not cover features"):
        _forward(features=torch.zeros(5, 2), deterministic=True)
    # 29 user columns pass every check: the next thing in the way is the device
    with pytest.raises(RuntimeError, match="no CPU path"):
        _forward(features=torch.zeros(5, 29))
    with pytest.raises(RuntimeError, match="no CPU path"):
        _forward()


def test_check_deterministic_names_return_normals(monkeypatch):
    from contextgs_amd.rasterizer import check_deterministic
    monkeypatch.delenv("CGS_RASTER_DETERMINISTIC", raising=False)
    assert inspect.signature(check_deterministic).parameters["return_normals"].default is False
    assert check_deterministic(False, return_normals=True) is False and check_deterministic(None, return_normals=True) is False
    with pytest.raises(ValueError, match="return_geometry"):          # the earlier refusals come first
        check_deterministic(True, return_geometry=True, return_normals=True)


def test_keyword_surfaces():
    from contextgs_amd import normals, renderer
    from contextgs_amd.dropin import diff_gaussian_rasterization as shim
    from contextgs_amd.rasterizer import GaussianRasterizer
    import contextgs_amd.rasterizer as rz
    assert inspect.signature(GaussianRasterizer.forward).parameters["return_normals"].default is False
    assert inspect.signature(shim.GaussianRasterizer.forward).parameters["return_normals"].default is False
    p = inspect.signature(renderer.render).parameters["return_normals"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(renderer._view_fusion).parameters["return_normals"].default is False
    assert renderer._view_fusion(True, False, False, False, False, None, None, return_normals=True) is None      # the unfused path
    assert inspect.signature(normals.depth_normals).parameters["eps"].default == 0.0
    assert inspect.signature(normals.normal_consistency).parameters["weight"].default is None
    for needle in ("return_normals", "normals[c, p]", "AWAY from", "opposite of 2DGS"):
        assert needle in rz.__doc__, needle
    assert "AWAY from the camera" in normals.__doc__ and "opposite of 2DGS" in normals.__doc__


def test_python_shape_errors_and_no_cpu_path():
    from contextgs_amd import normals
    rs = _rasterizer().raster_settings
    with pytest.raises(ValueError, match=r"depth must be \[1, H, W\] or \[H, W\]"):
        normals.depth_normals(torch.zeros(1, 16, 15), rs)
    with pytest.raises(ValueError, match="eps must be >= 0"):
        normals.depth_normals(torch.zeros(16, 16), rs, eps=-1.0)
    with pytest.raises(ValueError, match=r"normals must be \[3, H, W\]"):
        normals.normal_consistency(torch.zeros(1, 16, 16), torch.zeros(1, 16, 16), rs)
    with pytest.raises(ValueError, match="weight must be"):
        normals.normal_consistency(torch.zeros(3, 16, 16), torch.zeros(1, 16, 16), rs, weight=torch.zeros(3, 16, 16))
    with pytest.raises(ValueError, match=r"rotations must be \[P, 4\]"):
        normals.gaussian_normals(torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(5, 3), rs)
    with pytest.raises(ValueError, match=r"scales must be \[P, 3\]"):
        normals.gaussian_normals(torch.zeros(5, 3), torch.zeros(4, 3), torch.zeros(5, 4), rs)
    for call in (lambda: normals.depth_normals(torch.zeros(1, 16, 16), rs),
                 lambda: normals.normal_consistency(torch.zeros(3, 16, 16), torch.zeros(16, 16), rs),
                 lambda: normals.gaussian_normals(torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(5, 4), rs)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
