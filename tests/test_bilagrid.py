"""The bilateral grid without a device: the numpy reference of tests/bilagrid_ref.py against torch's grid_sample in fp64 (values and
both gradients, every case), that the budgets have teeth (four wrong variants each exceed them) and are attainable (the reference
run in float32 stays inside), and what of the feature itself needs no GPU: the symbols, the argument checks of the C entries and of
the Python surface, and the refusal of CPU tensors."""
import numpy as np
import pytest
import torch

import bilagrid_ref as br
from contextgs_amd.bilagrid import BilateralGrid, bilagrid_slice, bilagrid_tv


def _torch_composition(grid, img, dout):
    """(out, dgrid, dimg) of grid_sample + the affine map, fp64 on the CPU through autograd."""
    G = torch.tensor(grid, dtype=torch.float64, requires_grad=True)
    I = torch.tensor(img, dtype=torch.float64, requires_grad=True)
    _, L, Gh, Gw = G.shape
    _, H, W = I.shape
    gx = (torch.arange(W, dtype=torch.float64) + 0.5) / W
    gy = (torch.arange(H, dtype=torch.float64) + 0.5) / H
    z = (0.299 * I[0] + 0.587 * I[1] + 0.114 * I[2])
    # grid_sample's coordinates are in [-1, 1]; with align_corners -1 and 1 are the first and last nodes.  An axis of one node maps
    # everything onto it.  Border padding clamps the coordinate, which is the definition's clamp of gz with no gradient outside.
    coords = torch.stack([(gx * 2 - 1)[None, :].expand(H, W), (gy * 2 - 1)[:, None].expand(H, W), z * 2 - 1], dim=-1)
    A = torch.nn.functional.grid_sample(G[None], coords[None, None], mode="bilinear", align_corners=True, padding_mode="border")[0, :, 0]
    A = A.reshape(3, 4, H, W)
    out = (A[:, :3] * I[None]).sum(dim=1) + A[:, 3]
    dgrid, dimg = torch.autograd.grad(out, [G, I], torch.tensor(dout, dtype=torch.float64))
    return out.detach().numpy(), dgrid.numpy(), dimg.numpy()


@pytest.mark.parametrize("case", br.CASES, ids=br.case_id)
def test_reference_is_grid_sample_and_the_affine_map(case):
    ref = br.reference(case)
    out, dgrid, dimg = _torch_composition(ref.grid, ref.img, ref.dout)
    for name, got in (("out", out), ("dgrid", dgrid), ("dimg", dimg)):
        want = ref.r64[name]
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), name


@pytest.mark.parametrize("case", br.CASES, ids=br.case_id)
def test_cases_saturate_at_both_ends_and_keep_clear_of_the_kinks(case):
    ref = br.reference(case)
    L, Gh, Gw, H, W, kind = case
    zs = ref.r64["gz_raw"]
    if L > 1:
        assert np.abs(zs - np.round(zs)).min() >= br.GZ_MARGIN
    assert ref.img.min() >= -0.3 - 1e-6 and ref.img.max() <= 1.3 + 1e-2
    if H * W >= 100 and kind == "wide":
        lum = zs / max(L - 1, 1) if L > 1 else br.luminance_scaled(ref.img, 2)
        assert (lum < 0).mean() >= 0.01 and (lum > 1).mean() >= 0.01
    if kind == "dark":
        assert (zs < 0).all() and not ref.r64["dgrid"][:, 1:].any() and not ref.r64["b_dgrid"][:, 1:].any()
        assert ref.r64["dgrid"][:, 0].all()


@pytest.mark.parametrize("case", br.CASES, ids=br.case_id)
def test_float32_reference_stays_inside_the_budgets(case):
    ref = br.reference(case)
    r32 = br.slice_all(ref.grid, ref.img, ref.dout, np.float32)
    for name in ("out", "dimg", "dgrid"):
        assert r32[name].dtype == np.float32
        assert ref.ratio(name, r32[name]) <= 1.0, name


@pytest.mark.parametrize("variant", br.VARIANTS)
def test_budgets_have_teeth(variant):
    """Each wrong variant, computed in fp64, is outside the budget of some output on at least one case."""
    worst = 0.0
    for case in br.CASES:
        ref = br.reference(case)
        bad = br.slice_all(ref.grid, ref.img, ref.dout, np.float64, variant=variant)
        worst = max(worst, max(ref.ratio(name, bad[name]) for name in ("out", "dimg", "dgrid")))
    assert worst > 1.0, (variant, worst)


@pytest.mark.parametrize("tv_case", br.TV_CASES, ids=br.case_id)
def test_tv_reference_against_torch(tv_case):
    grids, ref = br.tv_reference(tv_case)
    G = torch.tensor(grids, dtype=torch.float64, requires_grad=True)
    tv = torch.zeros((), dtype=torch.float64)
    for axis in (2, 3, 4):
        if G.shape[axis] > 1:
            tv = tv + torch.diff(G, dim=axis).pow(2).mean(dim=(1, 2, 3, 4)).sum() / G.shape[0]
    if tv.requires_grad:
        (d,) = torch.autograd.grad(tv, [G], torch.tensor(br.TV_G, dtype=torch.float64))
    else:
        d = torch.zeros_like(G)
    assert abs(float(tv.detach()) - float(ref["tv"])) <= 1e-13 * max(1.0, float(tv.detach()))
    assert np.abs(d.numpy() - ref["dgrids"]).max() <= 1e-13 * max(1.0, np.abs(ref["dgrids"]).max())
    r32 = br.tv_all(grids, br.TV_G, np.float32)
    assert br.ratio(r32["tv"], ref["tv"], ref["b_tv"]) <= 1.0 and br.ratio(r32["dgrids"], ref["dgrids"], ref["b_dgrids"]) <= 1.0
    wrong = br.tv_all(grids * 1.01, br.TV_G, np.float64)                   # a 1 % error is outside, unless there is nothing to miss
    if float(ref["tv"]) > 0:
        assert br.ratio(wrong["tv"], ref["tv"], ref["b_tv"]) > 1.0 and br.ratio(wrong["dgrids"], ref["dgrids"], ref["b_dgrids"]) > 1.0


# ---- the feature itself, as far as it goes without a device ------------------------------------------------------------------------
NAMES = ("cgs_bilagrid_slice_fwd", "cgs_bilagrid_slice_bwd", "cgs_bilagrid_bwd_scratch_bytes", "cgs_bilagrid_tv_fwd",
         "cgs_bilagrid_tv_bwd", "cgs_bilagrid_tv_scratch_bytes")


def test_symbols_resolve():
    from contextgs_amd import _lib
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(L, n), n


def test_library_entries_reject_bad_arguments_before_a_launch():
    """Every call below fails an argument check, so nothing is launched (P is never dereferenced)."""
    from contextgs_amd import _lib
    L = _lib.lib()
    P = 4096

    def rejected(rc, word=b"bilagrid"):
        assert rc != 0
        msg = L.cgs_last_error()
        assert msg and word in msg, msg

    good = (8, 16, 16)
    big = 1 << 30
    for bad in ((0, 16, 16), (8, 0, 16), (8, 16, 0), (-1, 16, 16)):
        rejected(L.cgs_bilagrid_slice_fwd(P, *bad, P, 5, 7, P, None))
        rejected(L.cgs_bilagrid_slice_bwd(P, *bad, P, P, 5, 7, P, P, P, big, None))
        rejected(L.cgs_bilagrid_tv_fwd(P, 2, *bad, P, P, None))
        rejected(L.cgs_bilagrid_tv_bwd(P, 2, *bad, P, P, None))
        assert L.cgs_bilagrid_bwd_scratch_bytes(*bad, 5, 7) == 0 and L.cgs_bilagrid_tv_scratch_bytes(2, *bad) == 0
    for hw in ((0, 7), (5, 0), (5, -3)):
        rejected(L.cgs_bilagrid_slice_fwd(P, *good, P, *hw, P, None))
        rejected(L.cgs_bilagrid_slice_bwd(P, *good, P, P, *hw, P, P, P, big, None))
        assert L.cgs_bilagrid_bwd_scratch_bytes(*good, *hw) == 0
    rejected(L.cgs_bilagrid_tv_fwd(P, 0, *good, P, P, None))
    rejected(L.cgs_bilagrid_tv_bwd(P, 0, *good, P, P, None))
    for args in ((None, P, P), (P, None, P), (P, P, None)):
        rejected(L.cgs_bilagrid_slice_fwd(args[0], *good, args[1], 5, 7, args[2], None), b"NULL")
        rejected(L.cgs_bilagrid_slice_bwd(args[0], *good, args[1], args[2], 5, 7, P, P, P, big, None), b"NULL")
        rejected(L.cgs_bilagrid_tv_fwd(args[0], 2, *good, args[1], args[2], None), b"NULL")
        rejected(L.cgs_bilagrid_tv_bwd(args[0], 2, *good, args[1], args[2], None), b"NULL")
    rejected(L.cgs_bilagrid_slice_bwd(P, *good, P, P, 5, 7, None, None, P, big, None), b"neither")
    need = int(L.cgs_bilagrid_bwd_scratch_bytes(*good, 5, 7))
    assert need > 0 and need % 192 == 0                                    # whole [4 corners][12] records
    rejected(L.cgs_bilagrid_slice_bwd(P, *good, P, P, 5, 7, P, P, P, need - 1, None), b"scratch")
    rejected(L.cgs_bilagrid_slice_bwd(P, *good, P, P, 5, 7, None, P, None, need, None), b"scratch")
    assert int(L.cgs_bilagrid_tv_scratch_bytes(200, *good)) > 0
    assert int(L.cgs_bilagrid_bwd_scratch_bytes(8, 16, 16, 1080, 1920)) == 2 * 15 * 15 * 8 * 192
    assert int(L.cgs_bilagrid_bwd_scratch_bytes(2, 2, 3, 70, 90)) == 6 * 1 * 2 * 2 * 192     # the split case of bilagrid_ref.CASES


def test_python_arguments_are_checked_before_a_device_is_touched():
    grid, img = torch.zeros(12, 2, 3, 4), torch.rand(3, 5, 7)
    for bad in (torch.zeros(11, 2, 3, 4), torch.zeros(2, 3, 4), torch.zeros(1, 12, 2, 3, 4), torch.zeros(12, 2, 3, 4, dtype=torch.int32),
                torch.zeros(12, 0, 3, 4), "grid"):
        with pytest.raises(ValueError, match="grid"):
            bilagrid_slice(bad, img)
    for bad in (torch.rand(5, 7), torch.rand(1, 3, 5, 7), torch.zeros(3, 5, 7, dtype=torch.int64), torch.rand(3, 0, 7), None):
        with pytest.raises(ValueError, match="image"):
            bilagrid_slice(grid, bad)
    for c in (1, 2, 4):
        with pytest.raises(ValueError, match="three-channel"):
            bilagrid_slice(grid, torch.rand(c, 5, 7))
    with pytest.raises(ValueError, match="image on cpu, grid on meta"):
        bilagrid_slice(grid.to("meta"), img)
    for bad in (torch.zeros(12, 2, 3, 4), torch.zeros(2, 11, 2, 3, 4)):
        with pytest.raises(ValueError, match="grid"):
            bilagrid_tv(bad)
    for kw in ({"n_views": 0}, {"n_views": 2, "grid_x": 0}, {"n_views": 2, "grid_w": 0}):
        with pytest.raises(ValueError):
            BilateralGrid(**kw)
    bg = BilateralGrid(3, grid_x=4, grid_y=3, grid_w=2)
    assert [tuple(p.shape) for p in bg.parameters()] == [(3, 12, 2, 3, 4)]
    eye = torch.eye(3, 4).reshape(12)
    assert torch.equal(bg.grids.detach(), eye.reshape(1, 12, 1, 1, 1).expand(3, 12, 2, 3, 4))
    assert bg.grids.detach()[:, [0, 5, 10]].eq(1).all() and bg.grids.detach().sum() == 3 * 3 * 2 * 3 * 4
    for i in (-1, 3, 1.0, True):
        with pytest.raises(IndexError, match="view index"):
            bg(img, i)
    with pytest.raises(ValueError, match="three-channel"):
        bg(torch.rand(2, 5, 7), 0)


def test_cpu_tensors_are_refused():
    bg = BilateralGrid(2, grid_x=4, grid_y=3, grid_w=2)
    img = torch.rand(3, 5, 7, requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bg(img, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bg.tv_loss()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bilagrid_slice(torch.zeros(12, 2, 3, 4), img.detach())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bilagrid_tv(torch.zeros(1, 12, 2, 3, 4))
