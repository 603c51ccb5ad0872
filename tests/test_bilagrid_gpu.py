"""The bilateral grid kernels (csrc/bilagrid.hip, contextgs_amd/bilagrid.py) per element against the fp64 reference of
tests/bilagrid_ref.py, whose docstring derives every budget from the reference alone; tests/test_bilagrid.py shows that the
budgets have teeth.  Every buffer a kernel writes through the C ABI (outputs and scratch) sits between two guards of 64 sentinel
floats that are checked afterwards, and starts as NaN so that an element left unwritten shows.  No pixel is excluded from a
comparison.  Each check prints `[bilagrid-ratio] <what> | <case> | <quantity> | <max |hip - fp64| / budget>` (pytest -s).
Measured on an MI355X: the 57 tests of this file take 3.4 s together.  Largest ratios: out 0.31, d image 0.29, d grid 0.35, TV
gradient 0.37, TV scalar 0.005; with an fp16 image (budget plus half a spacing of fp16) out 0.95, d image 0.85.
"""
import numpy as np
import pytest
import torch

import bilagrid_ref as br

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -24681.5


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

    def numpy(self, shape=None):
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == np.float32(SENTINEL)).all() and (b[self.lo + self.n:] == np.float32(SENTINEL)).all(), "write outside the buffer"
        return b[self.lo:self.lo + self.n].reshape(shape if shape is not None else (self.n,)).copy()


def _dev(a, shift=0):
    t = torch.tensor(np.ascontiguousarray(a), device="cuda")
    if shift:
        big = torch.zeros(t.numel() + shift, dtype=t.dtype, device="cuda")
        big[shift:] = t.reshape(-1)
        t = big[shift:].reshape(t.shape)
        assert t.data_ptr() % 16 != 0
    return t


def _report(what, case, ratios):
    for k, v in ratios.items():
        print(f"[bilagrid-ratio] {what} | {br.case_id(case)} | {k} | {v:.3f}")
    return {k: v for k, v in ratios.items() if not v <= 1.0}


def _fwd(ref, shift=0):
    _lib, L = _L()
    Lz, Gh, Gw, H, W, _ = ref.case
    g, x = _dev(ref.grid), _dev(ref.img, shift)
    out = Guarded(3 * H * W, shift)
    _lib.check(L.cgs_bilagrid_slice_fwd(_lib.ptr(g), Lz, Gh, Gw, _lib.ptr(x), H, W, out.t.data_ptr(), _lib.current_stream()),
               "cgs_bilagrid_slice_fwd")
    torch.cuda.synchronize()
    return out.numpy((3, H, W))


def _bwd(ref, dimg=True, dgrid=True, shift=0):
    """(dimg, dgrid) of cgs_bilagrid_slice_bwd; the scratch is guarded as well."""
    _lib, L = _L()
    Lz, Gh, Gw, H, W, _ = ref.case
    g, x, d = _dev(ref.grid), _dev(ref.img, shift), _dev(ref.dout, shift)
    nbytes = int(L.cgs_bilagrid_bwd_scratch_bytes(Lz, Gh, Gw, H, W))
    assert nbytes > 0 and nbytes % 4 == 0
    di = Guarded(3 * H * W, shift) if dimg else None
    dg = Guarded(12 * Lz * Gh * Gw) if dgrid else None
    sc = Guarded(nbytes // 4) if dgrid else None
    _lib.check(L.cgs_bilagrid_slice_bwd(_lib.ptr(g), Lz, Gh, Gw, _lib.ptr(x), _lib.ptr(d), H, W, di.t.data_ptr() if di else None,
                                        dg.t.data_ptr() if dg else None, sc.t.data_ptr() if sc else None, nbytes if sc else 0,
                                        _lib.current_stream()), "cgs_bilagrid_slice_bwd")
    torch.cuda.synchronize()
    if sc:
        assert np.isfinite(sc.numpy()).all()                    # every partial written
    return (di.numpy((3, H, W)) if di else None), (dg.numpy((12, Lz, Gh, Gw)) if dg else None)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", br.CASES, ids=br.case_id)
def test_abi_slice_forward(case):
    ref = br.reference(case)
    out = _fwd(ref)
    assert np.isfinite(out).all()
    bad = _report("abi-fwd", case, {"out": ref.ratio("out", out)})
    assert not bad, bad
    assert _fwd(ref, shift=1).tobytes() == out.tobytes()           # planes off the 16-byte alignment: the same values


@pytest.mark.parametrize("case", br.CASES, ids=br.case_id)
def test_abi_slice_backward(case):
    ref = br.reference(case)
    dimg, dgrid = _bwd(ref)
    assert np.isfinite(dimg).all() and np.isfinite(dgrid).all()
    bad = _report("abi-bwd", case, {"dimg": ref.ratio("dimg", dimg), "dgrid": ref.ratio("dgrid", dgrid)})
    assert not bad, bad
    d1, none = _bwd(ref, dgrid=False)
    none2, g2 = _bwd(ref, dimg=False)
    assert none is None and none2 is None
    assert d1.tobytes() == dimg.tobytes() and g2.tobytes() == dgrid.tobytes()      # either alone: the same bytes; dgrid reproducible
    d3, g3 = _bwd(ref, shift=1)
    assert d3.tobytes() == dimg.tobytes() and g3.tobytes() == dgrid.tobytes()
    if case[5] == "dark":                                       # gz = 0 everywhere: the upper level is reached by no pixel
        assert not dgrid[:, 1:].any() and dgrid[:, 0].all()
        assert (ref.r64["b_dgrid"][:, 1:] == 0).all()


def test_scratch_size_is_checked_on_the_device_too():
    _lib, L = _L()
    ref = br.reference(br.CASES[1])
    Lz, Gh, Gw, H, W, _ = ref.case
    g, x, d = _dev(ref.grid), _dev(ref.img), _dev(ref.dout)
    dg = torch.zeros(12, Lz, Gh, Gw, device="cuda")
    need = int(L.cgs_bilagrid_bwd_scratch_bytes(Lz, Gh, Gw, H, W))
    sc = torch.zeros(need, dtype=torch.uint8, device="cuda")
    rc = L.cgs_bilagrid_slice_bwd(_lib.ptr(g), Lz, Gh, Gw, _lib.ptr(x), _lib.ptr(d), H, W, None, _lib.ptr(dg), _lib.ptr(sc), need - 4,
                                  _lib.current_stream())
    assert rc != 0 and b"scratch" in L.cgs_last_error()
    torch.cuda.synchronize()
    assert not dg.any() and not sc.any()


# ---- the autograd node -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrt", ["grid", "image", "both"])
@pytest.mark.parametrize("case", br.CASES, ids=br.case_id)
def test_node(case, wrt):
    from contextgs_amd.bilagrid import bilagrid_slice
    ref = br.reference(case)
    g, x, d = _dev(ref.grid), _dev(ref.img), _dev(ref.dout)
    g.requires_grad_(wrt in ("grid", "both"))
    x.requires_grad_(wrt in ("image", "both"))
    out = bilagrid_slice(g, x)
    assert out.requires_grad and type(out.grad_fn).__name__ == "_SliceBackward"
    r = {"out": ref.ratio("out", out.detach().cpu().numpy())}
    runs = []
    for _ in range(2):
        grads = torch.autograd.grad(out, [t for t in (g, x) if t.requires_grad], d, retain_graph=True)
        runs.append([t.cpu().numpy() for t in grads])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
    got = dict(zip([n for n, t in (("dgrid", g), ("dimg", x)) if t.requires_grad], runs[0]))
    for name, v in got.items():
        assert v.shape == ref.r64[name].shape and v.dtype == np.float32
        r[name] = ref.ratio(name, v)
    bad = _report(f"node-{wrt}", case, r)
    assert not bad, bad


def test_node_without_grad_is_one_launch_that_keeps_nothing():
    from contextgs_amd.bilagrid import bilagrid_slice
    case = br.CASES[5]
    ref = br.reference(case)
    g, x = _dev(ref.grid), _dev(ref.img)
    bilagrid_slice(g, x)                                                   # (the library, the stream and the allocator are warm)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = bilagrid_slice(g, x)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    assert not out.requires_grad and out.grad_fn is None
    assert grown < 2 * ref.img.size * 4, grown                             # the output and nothing of its size beside it
    bad = _report("node-nograd", case, {"out": ref.ratio("out", out.cpu().numpy())})
    assert not bad, bad


@pytest.mark.parametrize("route", ["fp16", "permuted", "crop"])
def test_input_routes(route):
    """Other float types and layouts are converted first; the gradients come back in the inputs' own type and shape."""
    from contextgs_amd.bilagrid import bilagrid_slice
    case = br.CASES[1]
    grid, img, dout = br.make_inputs(case)
    if route == "fp16":
        img16 = img.astype(np.float16)
        img, dout = img16.astype(np.float32), dout.astype(np.float16).astype(np.float32)       # what the kernels will see
        zs = br.luminance_scaled(img, case[0])
        assert np.abs(zs - np.round(zs)).min() >= br.GZ_MARGIN / 4         # rounding to fp16 left the kinks at a distance
        leaf = _dev(img16).requires_grad_()
        x = leaf
    elif route == "permuted":
        leaf = _dev(np.ascontiguousarray(img.transpose(1, 2, 0))).requires_grad_()
        x = leaf.permute(2, 0, 1)
        assert not x.is_contiguous()
    else:
        leaf = torch.rand(3, case[3] + 4, case[4] + 3, device="cuda")
        leaf[:, 1:1 + case[3], 2:2 + case[4]] = _dev(img)
        leaf.requires_grad_()
        x = leaf[:, 1:1 + case[3], 2:2 + case[4]]
    r64 = br.slice_all(grid, img, dout, np.float64, budgets=True)
    g = _dev(grid).double().requires_grad_()                               # a grid of another float type as well
    out = bilagrid_slice(g, x)
    assert out.dtype == x.dtype and out.shape == x.shape
    dg, dl = torch.autograd.grad(out, [g, leaf], _dev(dout).to(out.dtype))
    assert dg.dtype == torch.float64 and dl.dtype == leaf.dtype and dl.shape == leaf.shape
    dx = {"fp16": lambda t: t, "permuted": lambda t: t.permute(2, 0, 1), "crop": lambda t: t[:, 1:1 + case[3], 2:2 + case[4]]}[route](dl)
    # half a spacing of the format the results come back in: relative for normal numbers, 2^-25 in fp16's subnormal range
    half, sub = (2.0 ** -11, 2.0 ** -25) if route == "fp16" else (0.0, 0.0)
    r = {"out": br.ratio(out.detach().float().cpu().numpy(), r64["out"], r64["b_out"] + half * np.abs(r64["out"]) + sub),
         "dimg": br.ratio(dx.float().cpu().numpy(), r64["dimg"], r64["b_dimg"] + half * np.abs(r64["dimg"]) + sub),
         "dgrid": br.ratio(dg.cpu().numpy(), r64["dgrid"], r64["b_dgrid"])}
    if route == "crop":
        outside = dl.clone()
        outside[:, 1:1 + case[3], 2:2 + case[4]] = 0
        assert not outside.any()
    bad = _report(f"route-{route}", case, r)
    assert not bad, bad


# ---- TV ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tv_case", br.TV_CASES, ids=br.case_id)
def test_tv_abi_and_node(tv_case):
    from contextgs_amd.bilagrid import bilagrid_tv
    _lib, L = _L()
    grids, ref = br.tv_reference(tv_case)
    N, Lz, Gh, Gw = tv_case
    G = _dev(grids)
    nbytes = int(L.cgs_bilagrid_tv_scratch_bytes(N, Lz, Gh, Gw))
    assert nbytes >= 4 and nbytes % 4 == 0
    out, sc, dG = Guarded(1), Guarded(nbytes // 4), Guarded(grids.size)
    gout = torch.tensor([br.TV_G], dtype=torch.float32, device="cuda")
    st = _lib.current_stream()
    _lib.check(L.cgs_bilagrid_tv_fwd(_lib.ptr(G), N, Lz, Gh, Gw, out.t.data_ptr(), sc.t.data_ptr(), st), "cgs_bilagrid_tv_fwd")
    _lib.check(L.cgs_bilagrid_tv_bwd(_lib.ptr(G), N, Lz, Gh, Gw, _lib.ptr(gout), dG.t.data_ptr(), st), "cgs_bilagrid_tv_bwd")
    torch.cuda.synchronize()
    tv, d = out.numpy()[0], dG.numpy(grids.shape)
    assert np.isfinite(sc.numpy()).all()
    r = {"tv": br.ratio(tv, ref["tv"], ref["b_tv"]), "dgrids": br.ratio(d, ref["dgrids"], ref["b_dgrids"])}
    if float(ref["tv"]) == 0.0:                                            # one node per axis: nothing to differ from
        assert tv == 0.0 and not d.any()
    Gp = _dev(grids).requires_grad_()
    node = bilagrid_tv(Gp)
    assert node.shape == () and node.detach().cpu().numpy().tobytes() == tv.tobytes()
    (dn,) = torch.autograd.grad(node, [Gp], torch.tensor(br.TV_G, device="cuda"))
    assert dn.cpu().numpy().tobytes() == d.tobytes()
    assert not bilagrid_tv(_dev(grids)).requires_grad
    bad = _report("tv", tv_case, r)
    assert not bad, bad


# ---- the parameter holder ----------------------------------------------------------------------------------------------------------
def test_bilateral_grid_module():
    from contextgs_amd.bilagrid import BilateralGrid
    case = br.CASES[0]
    _, img, dout = br.make_inputs(case)
    Lz, Gh, Gw, H, W, _ = case
    bg = BilateralGrid(3, grid_x=Gw, grid_y=Gh, grid_w=Lz).cuda()
    assert bg.grids.shape == (3, 12, Lz, Gh, Gw)
    eye = np.broadcast_to(np.eye(3, 4, dtype=np.float32).reshape(12, 1, 1, 1), (12, Lz, Gh, Gw))
    r64 = br.slice_all(eye, img, dout, np.float64, budgets=True)
    assert np.abs(r64["out"] - img).max() < 1e-12                          # the identity grid returns the image
    x = _dev(img).requires_grad_()
    out = bg(x, 1)
    tv = bg.tv_loss()
    assert float(tv.detach()) == 0.0
    (out * _dev(dout)).sum().backward()
    r = {"out": br.ratio(out.detach().cpu().numpy(), img.astype(np.float64), r64["b_out"]),
         "dimg": br.ratio(x.grad.cpu().numpy(), r64["dimg"], r64["b_dimg"]),
         "dgrid": br.ratio(bg.grids.grad[1].cpu().numpy(), r64["dgrid"], r64["b_dgrid"])}
    assert not bg.grids.grad[0].any() and not bg.grids.grad[2].any()       # only the used view's slab
    assert bg.grids.grad[1].any()
    tv.backward()                                                          # flat grids: an exactly zero TV gradient everywhere
    assert not bg.grids.grad[0].any() and not bg.grids.grad[2].any()
    with pytest.raises(IndexError):
        bg(x, 3)
    with pytest.raises(ValueError, match="image on cpu"):
        bg(x.detach().cpu(), 0)
    bad = _report("module", case, r)
    assert not bad, bad
