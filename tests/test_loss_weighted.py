"""CPU: the reference of the weighted / exposed image loss (tests/loss_weighted_ref.py) is the maths the node documents, and its
budget has teeth, before anything runs on a card.

  - with w = 1 and E = [I | 0] it is loss_cases.outputs, exactly, in fp64
  - its dL/dx and dL/dE are the derivatives of its own forward (central differences, fp64, relative 1e-6 of the largest entry)
  - five deliberately wrong variants each break the budget on at least one of TEETH_CASES
  - S = 0 gives (0, 0, 1) and zeros; the correct fp32 oracle passes every case with factor 1
and what of the feature itself needs no device: the four `cgs_l1_ssim_w_*` entries exist and reject bad arguments before a launch,
`training_image_loss` refuses bad keywords before a device is touched (and has no CPU path behind good ones), `ViewExposure`.
"""
import numpy as np
import pytest

import loss_cases as lc
import loss_weighted_ref as wr


@pytest.mark.parametrize("shape", [(3, 6, 7), (3, 33, 65), (3, 38, 31)])
@pytest.mark.parametrize("explicit", [False, True])
def test_unit_weight_and_identity_exposure_are_the_plain_loss(shape, explicit):
    img, gt = lc.images(shape, "noise")
    w, E = (wr.weight(shape, "ones"), wr.exposure("identity")) if explicit else (None, None)
    a, b = wr.outputs(img, gt, w, E, np.float64), lc.outputs(img, gt, np.float64)
    for q in ("ssim", "absdiff", "tile_l1", "tile_ssim") + lc.MAPS:
        assert np.array_equal(a[q], b[q]), q
    assert np.array_equal(a["tile_w"], lc.tile_pixels(shape))
    assert a["l1"] == b["l1"] and a["ssim_mean"] == b["ssim_mean"]
    assert np.array_equal(a["G_l1"], b["g_l1"]) and np.array_equal(a["G_ssim"], b["g_ssim"])
    for g in lc.G_PAIRS:
        dx, dE, _ = wr.grads(a, *g)
        assert np.array_equal(dx, lc.combine(b, *g))
        assert (dE is None) == (not explicit)


def _separated(shape, E, seed):
    """(x, y, w) in fp64 with |x' - y| >= 0.05: sign(x' - y) does not move under the step."""
    r = np.random.default_rng(seed)
    x = r.random(shape)
    xp = wr.expose(x, E.astype(np.float64))
    y = xp - np.where(r.random(shape) < 0.5, -1.0, 1.0) * (0.05 + 0.2 * r.random(shape))
    w = 0.1 + r.random(shape[1:])
    return x, y, w


@pytest.mark.parametrize("shape", [(3, 6, 7), (3, 12, 13)])
def test_gradients_are_the_derivatives_of_the_forward(shape):
    E = wr.exposure("generic").astype(np.float64)
    x, y, w = _separated(shape, E, 7)
    g0, g1, h = 0.7, -0.4, 1e-5

    def f(xv, Ev):
        o = wr.outputs(xv, y, w, Ev, np.float64)
        return g0 * o["l1"] + g1 * o["ssim_mean"]

    dx, dE, _ = wr.grads(wr.outputs(x, y, w, E, np.float64), g0, g1)
    num_x = np.zeros(shape)
    for i in np.ndindex(*shape):
        d = np.zeros(shape)
        d[i] = h
        num_x[i] = (f(x + d, E) - f(x - d, E)) / (2 * h)
    num_E = np.zeros((3, 4))
    for i in np.ndindex(3, 4):
        d = np.zeros((3, 4))
        d[i] = h
        num_E[i] = (f(x, E + d) - f(x, E - d)) / (2 * h)
    ex, eE = np.abs(dx - num_x).max() / np.abs(num_x).max(), np.abs(dE - num_E).max() / np.abs(num_E).max()
    print(f"[loss-weighted] central differences {shape}: dx {ex:.2e}, dE {eE:.2e}")
    assert ex <= 1e-6 and eE <= 1e-6, (ex, eE)
    assert np.abs(num_E).min() > 0


@pytest.mark.parametrize("name", wr.WRONG)
def test_wrong_variant_breaks_the_budget(name):
    worst = {}
    for case in wr.TEETH_CASES:
        ref = wr.reference(*case)
        r = ref.ratios(wr.outputs(ref.img, ref.gt, ref.w, ref.Em, np.float32, wrong=name))
        print(f"[loss-weighted] wrong {name} {wr.case_id(case)}: {r}")
        worst[wr.case_id(case)] = max(r.values())
    assert max(worst.values()) > 1.0, (name, worst)


@pytest.mark.parametrize("case", wr.CASES + wr.BIG_CASES, ids=wr.case_id)
def test_correct_fp32_oracle_passes_with_factor_one(case):
    ref = wr.reference(*case)
    r = ref.ratios(ref.o32, factor=1.0)
    for g in lc.G_PAIRS:
        dx, dE, _ = wr.grads(ref.o32, *g)
        r[f"grad{g}"] = ref.ratio(g, dx, factor=1.0)
        if dE is not None:
            r[f"dE{g}"] = ref.dE_ratio(g, dE, factor=1.0)
    assert max(r.values()) <= 1.0, r
    for o in (ref.o32, ref.o64):
        assert all(np.isfinite(v).all() for v in o.values() if isinstance(v, np.ndarray))


@pytest.mark.parametrize("ename", [None, "generic"])
def test_zero_weight_sum(ename):
    shape = (3, 33, 38)
    img, gt = lc.images(shape, "noise")
    for dtype in (np.float32, np.float64):
        o = wr.outputs(img, gt, wr.weight(shape, "zero"), None if ename is None else wr.exposure(ename), dtype)
        assert (o["l1"], o["ssim_mean"], wr.loss_value(o)) == (0.0, 1.0, 0.0)
        dx, dE, _ = wr.grads(o, 0.8, -0.2)
        assert not dx.any() and (dE is None or not dE.any())
        assert not o["tile_w"].any() and not o["dmu1"].any()


def test_left0_keeps_the_ssim_gradient_beside_the_weighted_pixels():
    """Weight 0 for columns < 32: no L1 gradient there, an SSIM gradient exactly for the columns within the window's reach (27..31)."""
    ref = wr.reference((3, 33, 65), "noise", "left0", None)
    g_l1, g_s = ref.o64["G_l1"], ref.o64["G_ssim"]
    assert not g_l1[:, :, :32].any() and g_l1[:, :, 32:].all()
    assert not g_s[:, :, :27].any() and np.abs(g_s[:, :, 27:32]).min() > 0
    assert not ref.o64["tile_w"][:, :, 0].any()


# ---- the feature itself, as far as it goes without a device ------------------------------------------------------------------------
def test_library_entries_exist_and_reject_bad_arguments_before_a_launch():
    """Every call below fails an argument check, so nothing is launched (P is never dereferenced)."""
    from contextgs_amd import _lib
    L = _lib.lib()
    P = 4096                                                               # a non-NULL pointer value

    def rejected(rc, word=b"l1_ssim_w"):
        assert rc != 0
        msg = L.cgs_last_error()
        assert msg and word in msg, msg

    for shape in ((0, 5, 7), (3, 0, 7), (3, 5, 0)):
        rejected(L.cgs_l1_ssim_w_fwd(P, P, P, None, *shape, P, P, None))
        rejected(L.cgs_l1_ssim_w_finish(P, *shape, 0.2, P, P, None))
        rejected(L.cgs_l1_ssim_w_bwd(P, P, P, None, P, P, P, P, 0.2, *shape, P, None, None))
    rejected(L.cgs_l1_ssim_w_fwd(P, P, P, P, 2, 5, 7, P, P, None), b"C == 3")                  # an exposure with C != 3
    rejected(L.cgs_l1_ssim_w_bwd(P, P, P, P, P, P, P, P, 0.2, 4, 5, 7, P, P, None), b"C == 3")
    rejected(L.cgs_l1_ssim_w_fwd(None, P, P, P, 3, 5, 7, P, P, None))
    rejected(L.cgs_l1_ssim_w_fwd(P, None, P, P, 3, 5, 7, P, P, None))
    rejected(L.cgs_l1_ssim_w_fwd(P, P, P, P, 3, 5, 7, P, None, None))
    rejected(L.cgs_l1_ssim_w_finish(None, 3, 5, 7, 0.2, P, P, None))
    rejected(L.cgs_l1_ssim_w_finish(P, 3, 5, 7, 0.2, None, P, None))
    rejected(L.cgs_l1_ssim_w_finish(P, 3, 5, 7, 0.2, P, None, None))
    rejected(L.cgs_l1_ssim_w_bwd(P, P, P, P, None, P, P, P, 0.2, 3, 5, 7, P, P, None))          # no maps
    rejected(L.cgs_l1_ssim_w_bwd(P, P, P, P, P, None, P, P, 0.2, 3, 5, 7, P, P, None))          # no 1 / (C S)
    rejected(L.cgs_l1_ssim_w_bwd(P, P, P, P, P, P, None, None, 0.2, 3, 5, 7, P, P, None))       # no upstream gradient
    rejected(L.cgs_l1_ssim_w_bwd(P, P, P, P, P, P, P, P, 0.2, 3, 5, 7, None, None, None))       # nothing to write
    rejected(L.cgs_l1_ssim_w_bwd(P, P, P, None, P, P, P, P, 0.2, 3, 5, 7, P, P, None))          # dE partials without an exposure
    rejected(L.cgs_l1_ssim_w_dexposure(None, 5, 7, P, None))
    rejected(L.cgs_l1_ssim_w_dexposure(P, 5, 7, None, None))
    rejected(L.cgs_l1_ssim_w_dexposure(P, 0, 7, P, None))
    assert int(L.cgs_l1_ssim_partials(1, 33, 4100)) == 258 and int(L.cgs_l1_ssim_partials(3, 289, 321)) == 330     # BIG_CASES' second trips


def test_keywords_are_checked_before_a_device_is_touched():
    import torch
    from contextgs_amd.loss_utils import training_image_loss
    x, gt = torch.rand(3, 9, 12, requires_grad=True), torch.rand(3, 9, 12)
    w, E = torch.rand(9, 12), torch.eye(3, 4)
    for bad in (torch.rand(12, 9), torch.rand(3, 9, 12), torch.rand(9), torch.ones(9, 12, dtype=torch.int64)):
        with pytest.raises(ValueError, match="weight"):
            training_image_loss(x, gt, 0.2, weight=bad)
    with pytest.raises(NotImplementedError, match="weight"):
        training_image_loss(x, gt, 0.2, weight=w.clone().requires_grad_())
    with pytest.raises(ValueError, match="three-channel"):
        training_image_loss(torch.rand(2, 9, 12), torch.rand(2, 9, 12), 0.2, exposure=E)
    for bad in (torch.eye(4, 3), torch.eye(3), torch.rand(1, 3, 4), torch.ones(3, 4, dtype=torch.int32)):
        with pytest.raises(ValueError, match="exposure"):
            training_image_loss(x, gt, 0.2, exposure=bad)
    with pytest.raises(ValueError, match="same shape"):
        training_image_loss(x, torch.rand(3, 9, 11), 0.2, weight=w)
    # good keywords on CPU tensors: an error, not a torch fallback
    for kw in ({"weight": w}, {"exposure": E}, {"weight": w[None].bool(), "exposure": E.requires_grad_()}):
        with pytest.raises(RuntimeError, match="no CPU path"):
            training_image_loss(x, gt, 0.2, **kw)


def test_view_exposure_holds_one_row_per_view():
    import torch
    from contextgs_amd.exposure import ViewExposure
    ve = ViewExposure(4)
    assert [tuple(p.shape) for p in ve.parameters()] == [(4, 3, 4)]
    assert torch.equal(ve.exposure.detach(), torch.eye(3, 4).expand(4, 3, 4))
    img = torch.tensor(lc.images((3, 6, 7), "noise")[0])
    assert torch.equal(ve.apply(img, 2), img)                              # [I | 0]
    E = wr.exposure("generic")
    with torch.no_grad():
        ve.exposure[1] = torch.tensor(E)
    want = wr.expose(img.numpy().astype(np.float64), E.astype(np.float64))
    assert np.abs(ve.apply(img, 1).detach().numpy() - want).max() <= 8 * wr.EPS32 * np.abs(want).max()
    row = ve(1)
    assert row.shape == (3, 4) and row.requires_grad
    opt = torch.optim.SGD(ve.parameters(), lr=0.5)
    (row * torch.arange(1.0, 13.0).reshape(3, 4)).sum().backward()         # every entry of the row gets a gradient
    opt.step()
    after, eye = ve.exposure.detach(), torch.eye(3, 4)
    assert all(torch.equal(after[i], eye) for i in (0, 2, 3)) and (after[1] != torch.tensor(E)).all()
    seen = []
    assert ve.apply(lambda m: seen.append(m)) is ve and seen == [ve]       # nn.Module.apply(fn) is still nn.Module's
    with pytest.raises(ValueError):
        ViewExposure(0)
