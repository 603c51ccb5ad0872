"""The depth-prior kernels (csrc/depth_prior.hip, contextgs_amd/depth_prior.py) against the fp64 reference of
tests/depth_prior_ref.py, whose docstring derives every budget from the reference alone; tests/test_depth_prior.py shows that the
budgets have teeth.  Every buffer a kernel writes through the C ABI (outputs, coefficients and scratch) sits between two guards of
64 sentinel floats that are checked afterwards, and starts as NaN so that an element left unwritten shows.  No pixel is excluded
from a comparison.  Each check prints `[depth-prior-ratio] <what> | <case> | <quantity> | <max |hip - fp64| / budget>` (pytest -s).
Shapes: 1x1, 1x63, 17x33 (vector tail, less than a wave, one workgroup), 16x64 (one full tile), 3x1025 (four workgroups, no
multiple of 4) and 257x1024 = 263168 pixels, which needs 257 workgroup records: one more than the finishing workgroup's 256
threads, so a thread adds two.  The kernels have two instances each: 16-byte accesses (4-byte for a byte mask) for every full
quad of pixels when every plane is aligned, with the last partial quad pixel by pixel; scalar accesses of the same four pixels per
lane when a plane is not aligned.  Every aligned call here runs the vector instances — against the reference, for every shape,
mode and mask type, through the C ABI and through the nodes (16x64 and 257x1024 are multiples of 4, the others end in a partial
quad, 1x1 is one) — and the `shift=1` calls run the scalar instances, all planes shifted and one plane at a time; their outputs
must be the same bytes.
Where the reference's L1 budget is the subgradient interval (depth_prior_ref: the fit is exact in exact arithmetic, so rounding
alone decides sign(r)), d x of the selected pixels is checked for its magnitude bound |g| m / N only, not for its sign.  These are
the `l1-lstsq-mask` and `l1-lstsq-image` modes of: every 1x1 case (one pixel), `17-33-one_pixel-*` (one selected pixel),
`17-33-same-*` (x = y) and `17-33-const_render-*` (a constant x).  Their values, their pixels of m = 0, every other mode of these
cases and `l1-lstsq` on every other case are checked in full.
Measured on an MI355X: the tests of this file take 5.1 s together.  Largest ratios: d x 0.999 (L1 and L2; Pearson 0.922), values
0.985 (L1), 0.949 (L2), 0.354 (Pearson), d a 0.926, d b 0.954, scale_shift a 0.518, b 0.993; with an fp16 render (budget plus half a
spacing of fp16) d x 0.968; trainable affine tensors d a 0.200, d b 0.822.  The ratios sit close under 1 because nearly all of an
output's budget is its own rounding to fp32 (2^-24 |value|, which half a unit in the last place reaches for a value just above a
power of two); the fitted a and b of the fp64 coefficient record agree with the reference to less than 0.0005 of their budgets.
"""
import numpy as np
import pytest
import torch

import depth_prior_ref as dr

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -24681.5
KIND = {"l1": 0, "l2": 1, "pearson": 2}
FP16_HALF, FP16_SUB = 2.0 ** -11, 2.0 ** -25     # half a spacing of fp16: relative for normal numbers, absolute for subnormal ones


def _L():
    from contextgs_amd import _lib
    return _lib, _lib.lib()


class Guarded:
    """n floats with GUARD sentinel floats on each side; `shift` floats off the 16-byte alignment of the allocation."""

    def __init__(self, n, shift=0):
        self.n, self.lo = n, GUARD + shift
        self.buf = torch.full((n + 2 * GUARD + shift,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.buf[self.lo:self.lo + n]
        self.t.fill_(float("nan"))

    def numpy(self, dtype=np.float32):
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == np.float32(SENTINEL)).all() and (b[self.lo + self.n:] == np.float32(SENTINEL)).all(), "write outside the buffer"
        return b[self.lo:self.lo + self.n].copy().view(dtype)


def _dev(a, shift=0):
    """The array on the device; `shift` elements off the alignment of the allocation (16 bytes for floats, 4 for bytes)."""
    if a is None:
        return None
    t = torch.tensor(np.ascontiguousarray(a), device="cuda")
    if shift:
        big = torch.zeros(t.numel() + shift, dtype=t.dtype, device="cuda")
        big[shift:] = t.reshape(-1)
        t = big[shift:].reshape(t.shape)
        assert t.data_ptr() % (16 if t.element_size() == 4 else 4) != 0
    return t


def _mask_dev(m, shift=0):
    if m is None:
        return None, 0
    if m.dtype == np.float32:
        return _dev(m, shift), 1
    return _dev(m.view(np.uint8), shift), 2


def _report(what, case, ratios):
    for k, v in ratios.items():
        print(f"[depth-prior-ratio] {what} | {dr.case_id(case)} | {k} | {v:.3f}")
    return {k: v for k, v in ratios.items() if not v <= 1.0}


def _abi(case, mode, shift=0, mask=None, only="xymd"):
    """Every output of the C entries for one (case, mode), through guarded buffers: {'loss', 'dx', 'coef', 'da', 'db'} or
    {'a', 'b'}.  mask: another mask array in place of the case's.  shift: elements off the alignment, for the planes named in
    `only` (x, y, m = the mask, d = dx): one misaligned plane is enough to send a call to the scalar instances."""
    _lib, L = _L()
    H, W = case[:2]
    inp = dr.inputs(*case)
    sx, sy, sm, sd = (shift if c in only else 0 for c in "xymd")
    x, y = _dev(inp.x, sx), _dev(inp.y, sy)
    m, mt = _mask_dev(inp.m if mask is None else mask, sm)
    st = _lib.current_stream()
    nbytes = int(L.cgs_depth_prior_scratch_bytes(H, W))
    assert nbytes > 0 and nbytes % 64 == 0
    scratch = Guarded(nbytes // 4)
    if mode == "scale_shift":
        ab = Guarded(2)
        _lib.check(L.cgs_depth_prior_scale_shift(_lib.ptr(x), _lib.ptr(y), _lib.ptr(m), mt, H, W, ab.t.data_ptr(), scratch.t.data_ptr(),
                                                 nbytes, st), "cgs_depth_prior_scale_shift")
        torch.cuda.synchronize()
        scratch.numpy()
        a, b = ab.numpy()
        return {"a": a, "b": b}
    if mode == "pearson":
        kind, align, mean, a, b = 2, 0, 0, 0.0, 0.0
    else:
        k, al, mo = mode.split("-")
        kind, align, mean = KIND[k], int(al == "lstsq"), int(mo == "image")
        a, b = dr.given_affine(case[2]) if al == "affine" else (1.0, 0.0)
    out, coef, dx = Guarded(1), Guarded(16), Guarded(H * W, sd)
    g = torch.tensor([dr.G], dtype=torch.float32, device="cuda")
    _lib.check(L.cgs_depth_prior_fwd(_lib.ptr(x), _lib.ptr(y), _lib.ptr(m), mt, H, W, kind, align, mean, a, b, None, None, out.t.data_ptr(),
                                     coef.t.data_ptr(), scratch.t.data_ptr(), nbytes, st), "cgs_depth_prior_fwd")
    _lib.check(L.cgs_depth_prior_bwd(_lib.ptr(x), _lib.ptr(y), _lib.ptr(m), mt, H, W, kind, coef.t.data_ptr(), _lib.ptr(g), dx.t.data_ptr(), st),
               "cgs_depth_prior_bwd")
    res = {}
    if mode != "pearson" and align == 0:
        dab = Guarded(2)
        _lib.check(L.cgs_depth_prior_dab(_lib.ptr(x), _lib.ptr(y), _lib.ptr(m), mt, H, W, kind, coef.t.data_ptr(), _lib.ptr(g), dab.t.data_ptr(),
                                         scratch.t.data_ptr(), nbytes, st), "cgs_depth_prior_dab")
        torch.cuda.synchronize()
        res["da"], res["db"] = dab.numpy()
    torch.cuda.synchronize()
    scratch.numpy()
    res.update(loss=out.numpy()[0], dx=dx.numpy().reshape(H, W), coef=coef.numpy(np.float64))
    assert np.isfinite(res["coef"]).all()                                  # all eight written
    return res


def _check(what, case, mode, got):
    """The ratios of one (case, mode) and what must hold exactly; returns the ratios beyond 1."""
    ref = dr.reference(case, mode)
    inp, r64 = ref.inp, ref.r64
    if mode == "scale_shift":
        return _report(f"{what} {mode}", case, {"a": ref.ratio("a", got["a"]), "b": ref.ratio("b", got["b"])})
    r = {"loss": ref.ratio("loss", got["loss"]), "dx": ref.ratio("dx", got["dx"])}
    off = ~inp.sel
    assert not got["dx"][off].any() and not np.signbit(got["dx"][off]).any(), "a pixel selected out has gradient +0"
    if mode != "pearson":
        if "da" in got:
            r["da"], r["db"] = ref.ratio("da", got["da"]), ref.ratio("db", got["db"])
        if "coef" in got:
            r["a"] = dr.ratio(got["coef"][4], r64["a"], r64["b_a"])
            r["b"] = dr.ratio(got["coef"][5], r64["b"], r64["b_b"])
        if ref.kind == "l1" and not (ref.align == "lstsq" and inp.fit_exact):
            assert r64["sign_stable"]                                      # min |r| beyond the device's error in r: no sign differs
    return _report(f"{what} {mode}", case, r)


# ---- C ABI: the matrix on every shape, the value cases -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", dr.CASES, ids=dr.case_id)
def test_abi_matrix(case):
    """Every mode through the C entries: against fp64, twice (the same bytes), and with every plane off its alignment (the same
    bytes again)."""
    bad = {}
    for mode in dr.MODES:
        got = _abi(case, mode)
        for k, v in _check("abi", case, mode, got).items():
            bad[f"{mode} {k}"] = v
        runs = [_abi(case, mode), _abi(case, mode, shift=1)]
        runs += [_abi(case, mode, shift=1, only=c) for c in ("xmd" if case[3] != "none" else "xd")]      # one plane sends the call there
        for again in runs:
            assert all(np.asarray(again[k]).tobytes() == np.asarray(got[k]).tobytes() for k in got), mode
    assert not bad, bad


def test_exact_values():
    """x = y under the default affine, an all-zero mask, constant planes: exact values and exactly zero gradients."""
    for mk in ("none", "float"):
        for mode in ("l1-default-mask", "l2-default-image", "l2-default-mask"):
            got = _abi((17, 33, "same", mk), mode)
            assert got["loss"] == 0.0 and not got["dx"].any() and got["da"] == 0.0 and got["db"] == 0.0, mode
    for mk in ("float", "bool"):
        case = (17, 33, "zero_mask", mk)
        for mode in dr.MODES[:-2]:
            got = _abi(case, mode)
            assert got["loss"] == 0.0 and not got["dx"].any() and not np.signbit(got["dx"]).any(), mode
            assert got.get("da", 0.0) == 0.0 and got.get("db", 0.0) == 0.0
        got = _abi(case, "pearson")
        assert got["loss"] == 1.0 and not got["dx"].any()
        ab = _abi(case, "scale_shift")
        assert ab["a"] == 0.0 and ab["b"] == 0.0
    for values in ("const_prior", "const_render", "one_pixel"):
        mk = "bool" if values == "one_pixel" else "none"
        got = _abi((17, 33, values, mk), "pearson")
        assert got["loss"] == 1.0 and not got["dx"].any(), values
    ab = _abi((17, 33, "const_prior", "none"), "scale_shift")
    assert ab["a"] == 0.0 and abs(ab["b"] - dr.reference((17, 33, "const_prior", "none"), "scale_shift").r64["b"]) < 1e-6
    ab = _abi((17, 33, "const_render", "none"), "scale_shift")
    assert abs(ab["a"]) < 1e-12 and ab["b"] == 3.25


@pytest.mark.parametrize("shape", [(17, 33), (16, 64), (3, 1025), dr.BIG], ids=lambda s: f"{s[0]}x{s[1]}")
def test_float_mask_of_zeros_and_ones_is_the_bool_mask(shape):
    case = (*shape, "offset", "bool")
    keep = dr.inputs(*case).m
    for mode in ("l1-lstsq-mask", "l2-affine-image", "l2-lstsq-mask", "pearson", "scale_shift"):
        as_bool = _abi(case, mode)
        as_float = _abi(case, mode, mask=keep.astype(np.float32))
        assert all(np.asarray(as_bool[k]).tobytes() == np.asarray(as_float[k]).tobytes() for k in as_bool), mode


def test_scratch_size_is_checked_before_anything_is_enqueued():
    _lib, L = _L()
    case = (3, 1025, "offset", "none")
    inp = dr.inputs(*case)
    x, y = _dev(inp.x), _dev(inp.y)
    need = int(L.cgs_depth_prior_scratch_bytes(3, 1025))
    assert need == 4 * 64
    out, coef, sc = torch.zeros(1, device="cuda"), torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros(need // 8, dtype=torch.float64, device="cuda")
    rc = L.cgs_depth_prior_fwd(_lib.ptr(x), _lib.ptr(y), None, 0, 3, 1025, 2, 0, 0, 1.0, 0.0, None, None, _lib.ptr(out), _lib.ptr(coef),
                               _lib.ptr(sc), need - 8, _lib.current_stream())
    assert rc == 3 and b"scratch" in L.cgs_last_error()
    torch.cuda.synchronize()
    assert not out.any() and not coef.any() and not sc.any()


# ---- through autograd --------------------------------------------------------------------------------------------------------------
def _call(mode, x, y, m, values, affine=None):
    from contextgs_amd.depth_prior import depth_prior_loss, pearson_depth_loss
    if mode == "pearson":
        return pearson_depth_loss(x, y, m)
    kind, align, mean_over = mode.split("-")
    kw = {"affine": affine or dr.given_affine(values)} if align == "affine" else ({"align": "lstsq"} if align == "lstsq" else {})
    return depth_prior_loss(x, y, m, kind=kind, mean_over=mean_over, **kw)


def _mask_tensor(m):
    return None if m is None else torch.tensor(m, device="cuda")


@pytest.mark.parametrize("case", [(17, 33, "offset", "float"), (3, 1025, "offset", "bool"), (17, 33, "nonfinite", "uint8"),
                                  (17, 33, "neg", "none"), (16, 64, "offset", "uint8"), (16, 64, "offset", "float"),
                                  (*dr.BIG, "offset", "bool")], ids=dr.case_id)
def test_nodes_with_an_upstream_gradient(case):
    """Every mode through the Python surface with the upstream gradient G != 1; [1,H,W] gives the bytes of [H,W]."""
    from contextgs_amd.depth_prior import scale_shift
    inp = dr.inputs(*case)
    y, m = _dev(inp.y), _mask_tensor(inp.m)
    up = torch.tensor(dr.G, device="cuda")
    bad = {}
    for mode in dr.MODES[:-1]:
        x = _dev(inp.x).requires_grad_()
        loss = _call(mode, x, y, m, case[2])
        assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
        (dx,) = torch.autograd.grad(loss, [x], up)
        assert dx.shape == x.shape and dx.dtype == torch.float32
        got = {"loss": loss.detach().cpu().numpy(), "dx": dx.cpu().numpy()}
        for k, v in _check("node", case, mode, got).items():
            bad[f"{mode} {k}"] = v
        x3 = _dev(inp.x)[None].requires_grad_()
        loss3 = _call(mode, x3, y[None], None if m is None else m[None], case[2])
        (dx3,) = torch.autograd.grad(loss3, [x3], up)
        assert dx3.shape == (1, *x.shape)
        assert loss3.detach().cpu().numpy().tobytes() == got["loss"].tobytes() and dx3[0].cpu().numpy().tobytes() == got["dx"].tobytes(), mode
        assert not _call(mode, _dev(inp.x), y, m, case[2]).requires_grad
    a, b = scale_shift(_dev(inp.x), y, m)
    assert a.shape == () and b.shape == () and a.dtype == torch.float32 and a.is_cuda and not a.requires_grad
    bad.update(_check("node", case, "scale_shift", {"a": a.cpu().numpy(), "b": b.cpu().numpy()}))
    assert not bad, bad


@pytest.mark.parametrize("route", ["fp16", "transposed"])
def test_input_routes(route):
    """Other float types and layouts are converted first; the gradient comes back in the input's own type and shape."""
    case = (17, 33, "neg", "float")
    base = dr.inputs(*case)
    if route == "fp16":
        x16 = base.x.astype(np.float16)
        inp = dr.Inputs(*case, x=x16.astype(np.float32))                  # what the kernels will see
        leaf = _dev(x16).requires_grad_()
        x = leaf
        half, sub = FP16_HALF, FP16_SUB
    else:
        inp = base
        leaf = _dev(np.ascontiguousarray(base.x.T)).requires_grad_()
        x = leaf.t()
        assert not x.is_contiguous()
        half, sub = 0.0, 0.0
    y, m = _dev(inp.y).double(), _mask_tensor(inp.m)                       # a prior of another float type as well
    r = {}
    for mode in ("l1-lstsq-mask", "l2-affine-image", "l2-lstsq-mask", "pearson"):
        ref = dr.Reference(case, mode, inp)
        if mode.startswith("l1"):
            assert ref.r64["sign_stable"]
        loss = _call(mode, x, y, m, case[2])
        (dl,) = torch.autograd.grad(loss, [leaf], torch.tensor(dr.G, device="cuda"))
        assert dl.dtype == leaf.dtype and dl.shape == leaf.shape and loss.dtype == torch.float32
        dx = (dl if route == "fp16" else dl.t()).float().cpu().numpy()
        r[f"{mode} loss"] = ref.ratio("loss", loss.detach().cpu().numpy())
        r[f"{mode} dx"] = dr.ratio(dx, ref.r64["dx"], ref.r64["b_dx"] + half * np.abs(ref.r64["dx"]) + sub)
    bad = _report(f"route-{route}", case, r)
    assert not bad, bad


@pytest.mark.parametrize("shape", [(17, 33), (16, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["l1", "l2"])
def test_trainable_affine(kind, shape):
    """a and b as device tensors that require grad: d L / d a and d L / d b against the reference, next to d x; either alone too."""
    from contextgs_amd.depth_prior import depth_prior_loss
    case = (*shape, "offset", "float")
    mode = f"{kind}-affine-mask"
    ref = dr.reference(case, mode)
    inp = ref.inp
    a0, b0 = dr.given_affine(case[2])
    x, y, m = _dev(inp.x).requires_grad_(), _dev(inp.y), _mask_tensor(inp.m)
    a = torch.tensor(a0, device="cuda", requires_grad=True)
    b = torch.tensor([b0], device="cuda", dtype=torch.float64, requires_grad=True)
    loss = depth_prior_loss(x, y, m, kind=kind, affine=(a, b))
    dx, da, db = torch.autograd.grad(loss, [x, a, b], torch.tensor(dr.G, device="cuda"), retain_graph=True)
    assert da.shape == () and da.dtype == torch.float32 and db.shape == (1,) and db.dtype == torch.float64
    r = {"loss": ref.ratio("loss", loss.detach().cpu().numpy()), "dx": ref.ratio("dx", dx.cpu().numpy()),
         "da": ref.ratio("da", da.cpu().numpy()), "db": ref.ratio("db", db.cpu().numpy()[0])}
    (da2,) = torch.autograd.grad(loss, [a], torch.tensor(dr.G, device="cuda"))
    assert da2.cpu().numpy().tobytes() == da.cpu().numpy().tobytes()
    only_b = depth_prior_loss(x.detach(), y, m, kind=kind, affine=(a0, b))
    (db2,) = torch.autograd.grad(only_b, [b], torch.tensor(dr.G, device="cuda"))
    assert db2.cpu().numpy().tobytes() == db.cpu().numpy().tobytes()
    assert only_b.cpu().detach().numpy().tobytes() == loss.detach().cpu().numpy().tobytes()
    bad = _report(f"trainable-{kind}", case, r)
    assert not bad, bad


def test_a_second_derivative_is_refused():
    from contextgs_amd.depth_prior import depth_prior_loss, pearson_depth_loss
    inp = dr.inputs(16, 64, "offset", "bool")
    y, m = _dev(inp.y), _mask_tensor(inp.m)
    for fn in (lambda x: depth_prior_loss(x, y, m, kind="l2", align="lstsq"), lambda x: pearson_depth_loss(x, y, m)):
        x = _dev(inp.x).requires_grad_()
        (dx,) = torch.autograd.grad(fn(x), [x], create_graph=True)
        assert not dx.requires_grad                                        # a constant, visibly: nothing to differentiate again
        up = torch.ones((), device="cuda", requires_grad=True)
        (dx,) = torch.autograd.grad(fn(x), [x], up, create_graph=True)
        assert dx.requires_grad
        with pytest.raises(RuntimeError, match="once_differentiable"):
            dx.sum().backward()


def test_gradient_reaches_the_gaussians_of_a_render():
    """render -> invdepth -> the three losses -> means3D: finite and not all zero, on a 64x64 view with empty pixels masked."""
    import raster_harness as rh
    from contextgs_amd.depth_prior import depth_prior_loss, pearson_depth_loss
    from contextgs_amd.rasterizer import GaussianRasterizer
    cam, g = rh.scene(400, 64, 64, 3, 1.0, (0.02, 0.12))
    t = {k: rh.leaf(v) for k, v in g.items()}
    m2 = torch.zeros(400, 3, device="cuda", requires_grad=True)
    res = GaussianRasterizer(rh.settings(cam))(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], colors_precomp=t["colors"],
                                               scales=t["scales"], rotations=t["rotations"], return_aux=True)
    inv, alpha = res[2]["invdepth"], res[2]["alpha"]
    assert inv.shape == (1, 64, 64)
    gen = torch.Generator(device="cuda").manual_seed(1)
    prior = 2.5 * inv.detach() + 0.1 + 0.01 * torch.randn(inv.shape, device="cuda", generator=gen)
    prior[alpha.detach() < 0.5] = float("nan")                             # "sky"
    mask = alpha.detach() >= 0.5
    assert 64 < int(mask.sum()) < 64 * 64
    loss = depth_prior_loss(inv, prior, mask, align="lstsq") + depth_prior_loss(inv, prior, mask, kind="l2", affine=(0.4, -0.04)) \
        + pearson_depth_loss(inv, prior, mask)
    assert torch.isfinite(loss)
    loss.backward()
    d = t["means3D"].grad
    assert d is not None and torch.isfinite(d).all() and d.abs().max() > 0
