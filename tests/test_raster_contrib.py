"""The rasterizer's per-Gaussian contribution statistics without a GPU: the C-ABI entry point exists and its argument errors
come back with their code and a message (nothing is launched); the drop-in's `contrib` / `contrib_slots` keywords are off by
default, their shape, dtype and length rules raise ValueError before a device is touched in all four argument forms, and a
CPU call has no path; render() takes `contrib` as a keyword-only argument; GaussianContrib and densify.anchor_importance on
hand-made tensors."""
import ctypes as C
import inspect
import math
import types

import pytest
import torch

from raster_harness import fake_cfg

CGS_ERR_ARG = 1
CGS_ERR_WORKSPACE = 3

P1 = C.c_void_p(4096)      # a non-NULL stand-in: the checks only look at which pointers are given


def _contrib(P=1, R=1, geom=P1, bin_ws=P1, img=P1, img_bytes=1 << 30, slot=None, n_slots=None, accs=(P1,) * 4, maps=(P1,) * 3):
    from contextgs_amd import _lib
    L = _lib.lib()
    rc = L.cgs_raster_contrib(C.byref(fake_cfg()), P, R, geom, 1 << 30, bin_ws, 1 << 30, img, img_bytes, slot,
                              P if n_slots is None else n_slots, *accs, *maps, None)
    return rc, L.cgs_last_error().decode()


def test_new_symbol_resolves():
    from contextgs_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "cgs_raster_contrib") and "cgs_raster_contrib" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["cgs_raster_contrib"][1]) == 19


def test_argument_errors():
    rc, msg = _contrib(P=-1)
    assert rc == CGS_ERR_ARG and "P < 0" in msg, (rc, msg)
    rc, msg = _contrib(accs=(None,) * 4, maps=(None,) * 3)
    assert rc == CGS_ERR_ARG and "no output" in msg, (rc, msg)
    for kw in (dict(img=None), dict(geom=None), dict(bin_ws=None)):
        rc, msg = _contrib(**kw)
        assert rc == CGS_ERR_ARG and "NULL workspace" in msg, (kw, rc, msg)
    for n in (0, -3):
        rc, msg = _contrib(slot=P1, n_slots=n)
        assert rc == CGS_ERR_ARG and "n_slots" in msg and "<= 0" in msg, (n, rc, msg)
    for n in (0, 2):
        rc, msg = _contrib(P=1, n_slots=n)
        assert rc == CGS_ERR_ARG and "without a slot table" in msg, (n, rc, msg)
    for m in ("cgs_raster_contrib",):
        assert m in msg
    rc, msg = _contrib(R=0, img_bytes=16)
    assert rc == CGS_ERR_WORKSPACE and "workspace too small" in msg, (rc, msg)


def test_a_single_output_is_enough_to_pass_the_output_check():
    """Any of the seven may be NULL: with one given the call goes on to the next check (here the short image workspace)."""
    for k in range(7):
        ptrs = [None] * 7
        ptrs[k] = P1
        rc, msg = _contrib(R=0, img_bytes=16, accs=tuple(ptrs[:4]), maps=tuple(ptrs[4:]))
        assert rc == CGS_ERR_WORKSPACE, (k, rc, msg)


def _rasterizer(sh_degree=1):
    from contextgs_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    eye = torch.eye(4)
    rs = GaussianRasterizationSettings(16, 16, math.tan(0.5), math.tan(0.5), torch.zeros(3), 1.0, eye, eye, sh_degree,
                                       torch.zeros(3), False, False)
    return GaussianRasterizer(rs)


def test_contrib_defaults_to_none():
    from contextgs_amd import renderer
    from contextgs_amd.rasterizer import GaussianContrib, GaussianRasterizer
    sig = inspect.signature(GaussianRasterizer.forward).parameters
    assert sig["contrib"].default is None and sig["contrib_slots"].default is None
    p = inspect.signature(renderer.render).parameters["contrib"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    from contextgs_amd.dropin import diff_gaussian_rasterization as shim
    assert shim.GaussianContrib is GaussianContrib


def _form(form, P=5):
    return dict(plain=dict(colors_precomp=torch.zeros(P, 3), scales=torch.zeros(P, 3), rotations=torch.zeros(P, 4)),
                shs=dict(shs=torch.zeros(P, 4, 3), scales=torch.zeros(P, 3), rotations=torch.zeros(P, 4)),
                shs_cov=dict(shs=torch.zeros(P, 4, 3), cov3D_precomp=torch.zeros(P, 6)),
                cov=dict(colors_precomp=torch.zeros(P, 3), cov3D_precomp=torch.zeros(P, 6)))[form]


def _bad(kind, P=5):
    from contextgs_amd.rasterizer import GaussianContrib
    c = GaussianContrib.zeros(P)
    i32 = torch.zeros(P, dtype=torch.int32)
    if kind == "length":
        return dict(contrib=GaussianContrib.zeros(P - 1)), "rows for 5 Gaussians"
    if kind == "empty with slots":
        return dict(contrib=GaussianContrib.zeros(0), contrib_slots=i32), "at least one row"
    if kind == "dtype":
        c.pixels = torch.zeros(P, dtype=torch.int32)
        return dict(contrib=c), r"contrib.pixels must be torch.int64"
    if kind == "dtype float":
        c.max_weight = torch.zeros(P, dtype=torch.float64)
        return dict(contrib=c), r"contrib.max_weight must be torch.float32"
    if kind == "ragged":
        c.top_pixels = torch.zeros(P + 1, dtype=torch.int64)
        return dict(contrib=c), r"contrib.top_pixels must be \[n\]"
    if kind == "strided":
        c.weight = torch.zeros(2 * P)[::2]
        return dict(contrib=c), "contrib.weight must be contiguous"
    if kind == "type":
        return dict(contrib=torch.zeros(P)), "must be a GaussianContrib or True"
    if kind == "slots alone":
        return dict(contrib_slots=i32), "without contrib"
    if kind == "slots dtype":
        return dict(contrib=True, contrib_slots=torch.zeros(P, dtype=torch.int64)), "int32"
    if kind == "slots shape":
        return dict(contrib=c, contrib_slots=torch.zeros(P + 1, dtype=torch.int32)), r"contrib_slots must be \[P\]"
    if kind == "slots 2-D":
        return dict(contrib=c, contrib_slots=torch.zeros(P, 1, dtype=torch.int32)), r"contrib_slots must be \[P\]"
    if kind == "device":
        c.weight = torch.zeros(P, device="meta")
        return dict(contrib=c), "contrib.weight is on meta, means3D on cpu"
    if kind == "slots device":
        return dict(contrib=c, contrib_slots=torch.zeros(P, dtype=torch.int32, device="meta")), "contrib_slots is on meta"
    assert kind == "slots strided"
    return dict(contrib=c, contrib_slots=torch.zeros(2 * P, dtype=torch.int32)[::2]), "contrib_slots must be contiguous"


@pytest.mark.parametrize("form", ["plain", "shs", "shs_cov", "cov"])
@pytest.mark.parametrize("kind", ["length", "empty with slots", "dtype", "dtype float", "ragged", "strided", "type", "slots alone",
                                  "slots dtype", "slots shape", "slots 2-D", "slots strided", "device", "slots device"])
def test_errors_come_before_any_device(form, kind):
    P = 5
    kw, needle = _bad(kind, P)
    with pytest.raises(ValueError, match=needle):       # (CPU tensors: a device check would raise RuntimeError instead)
        _rasterizer()(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.zeros(P, 1), **kw, **_form(form))


@pytest.mark.parametrize("form", ["plain", "shs", "shs_cov", "cov"])
def test_contrib_has_no_cpu_path(form):
    from contextgs_amd.rasterizer import GaussianContrib
    P = 5
    for kw in (dict(contrib=True), dict(contrib=GaussianContrib.zeros(P)),
               dict(contrib=GaussianContrib.zeros(3), contrib_slots=torch.zeros(P, dtype=torch.int32))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            _rasterizer()(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.zeros(P, 1), **kw, **_form(form))


def test_gaussian_contrib_zeros_and_reset():
    from contextgs_amd.rasterizer import GaussianContrib
    c = GaussianContrib.zeros(7, "cpu")
    assert len(c) == 7 and c.views == 0
    assert [t.dtype for t in c.tensors()] == [torch.float32, torch.float32, torch.int64, torch.int64]
    assert all(t.shape == (7,) and t.device.type == "cpu" and not t.requires_grad and bool((t == 0).all()) for t in c.tensors())
    assert c.tensors()[0] is c.weight and c.tensors()[3] is c.top_pixels
    c.weight += 1.5
    c.max_weight[2] = 0.25
    c.pixels += 3
    c.top_pixels[0] = 9
    c.views = 4
    kept = c.tensors()
    assert c.reset() is c and c.views == 0
    assert all(a is b for a, b in zip(kept, c.tensors()))         # zeroed in place: the caller's tensors stay the caller's
    assert all(bool((t == 0).all()) for t in c.tensors())
    assert len(GaussianContrib.zeros(0)) == 0


def test_anchor_importance():
    from contextgs_amd.densify import anchor_importance
    from contextgs_amd.rasterizer import GaussianContrib
    K = 3
    c = GaussianContrib.zeros(4 * K)
    c.max_weight.copy_(torch.tensor([0.1, 0.7, 0.2, 0, 0, 0, 0.3, 0.3, 0.05, 0, 0.9, 0]))
    c.weight.copy_(torch.arange(12, dtype=torch.float32))
    c.pixels.copy_(torch.arange(12) * 2)
    c.top_pixels.copy_(torch.tensor([1, 0, 0, 0, 0, 0, 2, 3, 0, 0, 0, 7]))
    imp = anchor_importance(c, K)
    assert imp.dtype == torch.float32 and torch.equal(imp, torch.tensor([0.7, 0.0, 0.3, 0.9]))
    assert torch.equal(anchor_importance(c, K, reduce="max_weight"), imp)
    assert torch.equal(anchor_importance(c, K, reduce="weight"), torch.tensor([3.0, 12.0, 21.0, 30.0]))
    assert torch.equal(anchor_importance(c, K, reduce="pixels"), torch.tensor([6, 24, 42, 60]))
    assert torch.equal(anchor_importance(c, K, reduce="top_pixels"), torch.tensor([1, 0, 5, 7]))
    assert anchor_importance(c, 1).shape == (12,) and anchor_importance(c, 12).shape == (1,)
    with pytest.raises(ValueError, match="reduce"):
        anchor_importance(c, K, reduce="mean")
    with pytest.raises(ValueError, match="multiple"):
        anchor_importance(c, 5)


def test_render_checks_the_length_before_anything_runs():
    from contextgs_amd import renderer
    from contextgs_amd.rasterizer import GaussianContrib

    class _PC:      # render() reads the mode, the anchors and K before it generates anything
        n_offsets = 4
        get_anchor = torch.zeros(6, 3)

        class get_color_mlp:
            training = False

    cam = types.SimpleNamespace(world_view_transform=None, full_proj_transform=None, camera_center=None)
    with pytest.raises(ValueError, match="6 anchors x 4 offsets"):
        renderer.render(cam, _PC(), None, None, contrib=GaussianContrib.zeros(23))
    with pytest.raises(ValueError, match="GaussianContrib or True"):
        renderer.render(cam, _PC(), None, None, contrib=torch.zeros(24))
