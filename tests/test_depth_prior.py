"""The depth-prior losses without a device: the gradients of the numpy reference (tests/depth_prior_ref.py) against central
differences of the reference's own values, that its budgets have teeth (float32-accumulated moments exceed them on the offset
case; a sign-flipped gradient and 1 / n for 1 / M exceed them on every case they can differ on), that the L1 signs of every case
are stable, and what of the feature itself needs no GPU: the symbols, the argument and workspace checks of the C entries (stand-in
pointers that are never dereferenced) and the refusals of the Python surface."""
import numpy as np
import pytest
import torch

import depth_prior_ref as dr
from contextgs_amd.depth_prior import depth_prior_loss, pearson_depth_loss, scale_shift

SMALL = [(17, 33, "offset", "float"), (17, 33, "neg", "none"), (1, 63, "offset", "uint8")]


def _value(case, mode, x, affine=None):
    inp = dr.Inputs(*case, x=x)
    if mode == "pearson":
        return dr.pearson_mode(inp)["loss"]
    kind, align, mean_over = mode.split("-")
    return dr.affine_mode(inp, kind, align, mean_over, affine=affine)["loss"]


@pytest.mark.parametrize("mode", ["l1-affine-mask", "l1-default-image", "l2-affine-image", "l2-default-mask", "l2-lstsq-mask",
                                  "l2-lstsq-image", "pearson"])
@pytest.mark.parametrize("case", SMALL, ids=dr.case_id)
def test_reference_gradient_is_the_central_difference_of_the_reference(case, mode):
    """d / d x_p of the reference's value, refitting (a, b) for lstsq: for L2 the detached fit IS the total derivative."""
    ref = dr.reference(case, mode)
    x0 = ref.inp.x.astype(np.float64)
    # rho's value cancels (its own budget is ~1e-11 here) and curves over the render's 3e-3 of spread: a wider step and tolerance
    h, tol = (1e-5, 2e-4) if mode == "pearson" else (1e-6, 2e-6)
    pix =[0, x0.size // 3, x0.size - 1] + list(np.flatnonzero(~ref.inp.sel.ravel())[:1])
    for p in pix:
        xp, xm = x0.copy(), x0.copy()
        xp.flat[p] += h
        xm.flat[p] -= h
        fd = dr.G * (_value(case, mode, xp) - _value(case, mode, xm)) / (2 * h)
        want = ref.r64["dx"].flat[p]
        scale = np.abs(ref.r64["dx"]).max()
        assert abs(fd - want) <= tol * scale + 1e-9, (p, fd, want)
        if not ref.inp.sel.flat[p]:
            assert want == 0.0 and not np.signbit(want)


@pytest.mark.parametrize("kind", ["l1", "l2"])
@pytest.mark.parametrize("case", SMALL, ids=dr.case_id)
def test_reference_affine_gradients_are_central_differences(case, kind):
    mode = f"{kind}-affine-mask"
    ref = dr.reference(case, mode)
    a, b = dr.given_affine(case[2])
    x0 = ref.inp.x.astype(np.float64)
    h = 1e-7
    da = dr.G * (_value(case, mode, x0, (a + h, b)) - _value(case, mode, x0, (a - h, b))) / (2 * h)
    db = dr.G * (_value(case, mode, x0, (a, b + h)) - _value(case, mode, x0, (a, b - h))) / (2 * h)
    tol = 1e-2 if kind == "l1" else 1e-5            # L1: a kink or two inside +-h of a few hundred pixels
    assert abs(da - ref.r64["da"]) <= tol * max(1.0, abs(ref.r64["da"])), (da, ref.r64["da"])
    assert abs(db - ref.r64["db"]) <= tol * max(1.0, abs(ref.r64["db"])), (db, ref.r64["db"])


def test_least_squares_fit_satisfies_the_normal_equations():
    for case in SMALL:
        inp = dr.inputs(*case)
        a, b = inp.lstsq
        r = inp.xs - (a.val * inp.ys + b.val)
        scale = dr.fsum(inp.w * np.abs(inp.xs))
        assert abs(dr.fsum(inp.w * r)) <= 1e-12 * scale and abs(dr.fsum(inp.w * r * inp.ys)) <= 1e-12 * scale


# ---- the budgets have teeth --------------------------------------------------------------------------------------------------------
def test_float32_moments_exceed_the_budgets_on_the_offset_case():
    """x = 4 + 0.01 (...): Vx, Vy and C cancel; moments accumulated in float32 are far outside every budget that depends on them."""
    case = (17, 33, "offset", "none")
    inp = dr.inputs(*case)
    m32 = dr.moments(inp.x, inp.y, inp.w, np.float32)
    wrong = dr.pearson_mode(inp, moments_override=m32)
    ref = dr.reference(case, "pearson")
    assert abs(wrong["loss"] - ref.r64["loss"]) > 0.01                   # rho itself is off in the second digit
    assert ref.ratio("loss", wrong["loss"]) > 1000 and ref.ratio("dx", wrong["dx"]) > 1000
    a32, b32 = dr.lstsq_plain(m32)
    ss = dr.reference(case, "scale_shift")
    assert ss.ratio("a", a32) > 1000 and ss.ratio("b", b32) > 10          # (b's budget is mostly its own fp32 rounding)
    for mode in ("l2-lstsq-mask", "l1-lstsq-image"):
        ref = dr.reference(case, mode)
        kind, align, mean_over = mode.split("-")
        wrong = dr.affine_mode(inp, kind, align, mean_over, moments_override=m32)
        assert ref.ratio("loss", wrong["loss"]) > 1.0, mode              # (the summed value is flat in (a, b) at the fit)
    ref = dr.reference(case, "l2-lstsq-mask")
    M, Sx, Sy, Sxx, Syy, Sxy = m32
    assert ref.ratio("loss", ((M * Sxx - Sx * Sx) - a32 * (M * Sxy - Sx * Sy)) / M / M) > 1000     # the closed form of the value
    assert ref.ratio("dx", dr.affine_mode(inp, "l2", "lstsq", "mask", moments_override=m32)["dx"]) > 1000


def test_reference_in_float64_order_stays_inside_the_budgets():
    """The budgets are attainable: plain fp64 running sums (the worst order a kernel could use) stay inside them."""
    for case in [c for c in dr.CASES if c[2] in ("offset", "neg")]:
        inp = dr.inputs(*case)
        sel = inp.sel
        ws, xs, ys = inp.w[sel], inp.xs[sel], inp.ys[sel]
        m64 = tuple(float(np.cumsum(t)[-1]) for t in (ws, ws * xs, ws * ys, ws * xs * xs, ws * ys * ys, ws * xs * ys))
        ref = dr.reference(case, "pearson")
        got = dr.pearson_mode(inp, moments_override=m64)
        assert ref.ratio("loss", got["loss"]) <= 1.0 and ref.ratio("dx", got["dx"]) <= 1.0, case
        ss = dr.reference(case, "scale_shift")
        a, b = dr.lstsq_plain(m64)
        assert ss.ratio("a", a) <= 1.0 and ss.ratio("b", b) <= 1.0, case
        M, Sx, Sy, Sxx, Syy, Sxy = m64
        closed = ((M * Sxx - Sx * Sx) - a * (M * Sxy - Sx * Sy)) / M / M if inp.n > 1 else 0.0
        assert dr.reference(case, "l2-lstsq-mask").ratio("loss", closed) <= 1.0, case


@pytest.mark.parametrize("case", dr.CASES, ids=dr.case_id)
def test_wrong_gradients_exceed_the_budgets(case):
    """A sign-flipped gradient on every case with a gradient; 1 / n for 1 / M (and back) on every case where M != n."""
    inp = dr.inputs(*case)
    for mode in ("l1-affine-mask", "l2-affine-image", "l2-lstsq-mask", "pearson"):
        ref = dr.reference(case, mode)
        if not np.any(ref.r64["dx"]) or (mode == "l2-lstsq-mask" and inp.fit_exact):
            continue                                                   # nothing to flip: the gradient is 0 (exactly, or but for rounding)
        if mode == "pearson":
            flipped = dr.pearson_mode(inp, flip="sign")
        else:
            kind, align, mean_over = mode.split("-")
            flipped = dr.affine_mode(inp, kind, align, mean_over, flip="sign")
            if inp.mom[0] != inp.n:
                swapped = dr.affine_mode(inp, kind, align, mean_over, flip="n_for_m")
                assert ref.ratio("dx", swapped["dx"]) > 1.0, mode
                if "da" in swapped:
                    assert ref.ratio("da", swapped["da"]) > 1.0 and ref.ratio("loss", swapped["loss"]) > 1.0, mode
        assert ref.ratio("dx", flipped["dx"]) > 1.0, mode
        if "da" in flipped and ref.r64["da"] != 0:
            assert ref.ratio("da", flipped["da"]) > 1.0, mode


@pytest.mark.parametrize("case", dr.CASES, ids=dr.case_id)
def test_l1_signs_are_stable(case):
    """min |r| over the masked pixels exceeds the bound on the device's error in r, so no sign can differ — except where the fit
    is exact in exact arithmetic and rounding alone decides (depth_prior_ref's docstring): there the reference says so."""
    inp = dr.inputs(*case)
    for mode in [m for m in dr.MODES if m.startswith("l1")]:
        ref = dr.reference(case, mode)
        if ref.align == "lstsq" and inp.fit_exact:
            continue
        assert ref.r64["sign_stable"], mode


def test_exact_cases_of_the_reference():
    same = dr.reference((17, 33, "same", "none"), "l1-default-mask")
    assert same.r64["loss"] == 0.0 and not same.r64["dx"].any() and same.r64["b_loss"] == 0.0 and not same.r64["b_dx"].any()
    zero = dr.inputs(17, 33, "zero_mask", "bool")
    for mode in dr.MODES[:-2]:
        r = dr.reference((17, 33, "zero_mask", "bool"), mode).r64
        assert r["loss"] == 0.0 and not r["dx"].any() and r["b_loss"] == 0.0, mode
    assert zero.mom[0] == 0 and dr.reference((17, 33, "zero_mask", "bool"), "pearson").r64["loss"] == 1.0
    flat = dr.reference((17, 33, "const_prior", "none"), "scale_shift").r64
    assert flat["a"] == 0.0 and flat["b_a"] == 0.0 and abs(flat["b"] - 4.0) < 0.01
    for v in ("const_prior", "const_render", "one_pixel"):
        r = dr.reference((17, 33, v, "float"), "pearson").r64
        assert r["loss"] == 1.0 and not r["dx"].any()
    nf = dr.inputs(17, 33, "nonfinite", "bool")
    assert not np.isfinite(nf.x).all() and not np.isfinite(nf.y).all() and np.isfinite(nf.x[nf.sel]).all()
    for mode in dr.MODES:
        r = dr.reference((17, 33, "nonfinite", "bool"), mode).r64
        assert all(np.isfinite(v).all() for k, v in r.items() if k != "sign_stable"), mode


# ---- the feature itself, as far as it goes without a device ------------------------------------------------------------------------
NAMES = ("cgs_depth_prior_scratch_bytes", "cgs_depth_prior_fwd", "cgs_depth_prior_bwd", "cgs_depth_prior_dab",
         "cgs_depth_prior_scale_shift")


def test_symbols_resolve():
    from contextgs_amd import _lib
    L = _lib.lib()
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(L, n), n


def test_library_entries_reject_bad_arguments_before_a_launch():
    """Every call below fails an argument or workspace check, so nothing is launched (P is never dereferenced)."""
    from contextgs_amd import _lib
    L = _lib.lib()
    P, big = 4096, 1 << 20
    ARG, WORKSPACE = 1, 3

    def rejected(rc, who, word=None, code=ARG):
        assert rc == code, rc
        msg = L.cgs_last_error()
        assert msg and who in msg and (word is None or word in msg), msg

    def fwd(x=P, y=P, mask=None, mt=0, H=5, W=7, kind=0, align=0, mean=0, out=P, coef=P, scratch=P, nbytes=big):
        return L.cgs_depth_prior_fwd(x, y, mask, mt, H, W, kind, align, mean, 1.0, 0.0, None, None, out, coef, scratch, nbytes, None)

    def bwd(x=P, y=P, mask=None, mt=0, H=5, W=7, kind=0, coef=P, g=P, dx=P):
        return L.cgs_depth_prior_bwd(x, y, mask, mt, H, W, kind, coef, g, dx, None)

    def dab(x=P, y=P, mask=None, mt=0, H=5, W=7, kind=0, coef=P, g=P, out=P, scratch=P, nbytes=big):
        return L.cgs_depth_prior_dab(x, y, mask, mt, H, W, kind, coef, g, out, scratch, nbytes, None)

    def ss(x=P, y=P, mask=None, mt=0, H=5, W=7, out=P, scratch=P, nbytes=big):
        return L.cgs_depth_prior_scale_shift(x, y, mask, mt, H, W, out, scratch, nbytes, None)

    entries = ((fwd, b"depth_prior_fwd"), (bwd, b"depth_prior_bwd"), (dab, b"depth_prior_dab"), (ss, b"depth_prior_scale_shift"))
    for call, who in entries:
        for hw in ((0, 7), (5, 0), (5, -3), (-1, 7)):
            rejected(call(H=hw[0], W=hw[1]), who, b"positive")
        rejected(call(H=1 << 16, W=1 << 15), who, b"2^30")
        rejected(call(x=None), who, b"NULL")
        rejected(call(y=None), who, b"NULL")
        for mt in (-1, 3, 99):
            rejected(call(mask=P, mt=mt), who, b"mask type")
        rejected(call(mask=None, mt=1), who, b"mask")
        rejected(call(mask=None, mt=2), who, b"mask")
        rejected(call(mask=P, mt=0), who, b"mask")
    for call, who in entries[:3]:
        for kind in (-1, 3, 7):
            rejected(call(kind=kind), who, b"kind")
        rejected(call(coef=None), who, b"coef")
        rejected(call(coef=P + 4), who, b"coef")
    rejected(dab(kind=2), b"depth_prior_dab", b"kind")
    rejected(fwd(align=2), b"depth_prior_fwd", b"align")
    rejected(fwd(mean=2), b"depth_prior_fwd", b"mean_over")
    rejected(fwd(mean=-1), b"depth_prior_fwd", b"mean_over")
    rejected(fwd(out=None), b"depth_prior_fwd", b"NULL")
    rejected(bwd(g=None), b"depth_prior_bwd", b"NULL")
    rejected(bwd(dx=None), b"depth_prior_bwd", b"NULL")
    rejected(dab(g=None), b"depth_prior_dab", b"NULL")
    rejected(dab(out=None), b"depth_prior_dab", b"NULL")
    rejected(ss(out=None), b"depth_prior_scale_shift", b"NULL")
    need = int(L.cgs_depth_prior_scratch_bytes(5, 7))
    assert need == 8 * 8                                                   # one workgroup record of 8 doubles
    for call, who in (entries[0], entries[2], entries[3]):
        rejected(call(nbytes=need - 1), who, b"scratch", WORKSPACE)
        rejected(call(scratch=None, nbytes=need), who, b"scratch", WORKSPACE)
        rejected(call(scratch=P + 4), who, b"aligned")
    for hw in ((0, 7), (5, 0), (-2, 3), (1 << 16, 1 << 15)):
        assert L.cgs_depth_prior_scratch_bytes(*hw) == 0
    # a record per 1024 pixels up to the cap of 1024 workgroups
    assert int(L.cgs_depth_prior_scratch_bytes(*dr.BIG)) == (dr.DP_THREADS + 1) * 64
    assert int(L.cgs_depth_prior_scratch_bytes(1080, 1920)) == 1024 * 64
    assert int(L.cgs_depth_prior_scratch_bytes(1, 1024)) == 64 and int(L.cgs_depth_prior_scratch_bytes(1, 1025)) == 128


def test_python_arguments_are_checked_before_a_device_is_touched():
    x, y = torch.rand(5, 7), torch.rand(5, 7)
    for fn in (depth_prior_loss, pearson_depth_loss, scale_shift):
        for bx, by in ((torch.rand(5, 7), torch.rand(7, 5)), (torch.rand(1, 5, 7), torch.rand(5, 7))):
            with pytest.raises(ValueError, match="shape mismatch"):
                fn(bx, by)
        for bad in (torch.rand(35), torch.rand(2, 5, 7), torch.rand(1, 1, 5, 7), torch.rand(0, 7)):
            with pytest.raises(ValueError, match=r"\[H,W\] or \[1,H,W\]"):
                fn(bad, bad.clone())
        for bad in (torch.zeros(5, 7, dtype=torch.int64), "x", None):
            with pytest.raises(ValueError, match="float"):
                fn(bad, y)
        with pytest.raises(ValueError, match="shape mismatch"):
            fn(x, y, torch.ones(7, 5))
        with pytest.raises(ValueError, match="mask"):
            fn(x, y, torch.ones(5, 7, dtype=torch.int32))
    with pytest.raises(ValueError, match="not both"):
        depth_prior_loss(x, y, affine=(1.0, 0.0), align="lstsq")
    for kw in ({"kind": "huber"}, {"kind": "L1"}, {"align": "midas"}, {"mean_over": "all"}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            depth_prior_loss(x, y, **kw)
    for bad in ((1.0,), 1.0, (1.0, "b"), (torch.ones(2), 0.0), (True, 0.0), (torch.ones(1, dtype=torch.int32), 0.0)):
        with pytest.raises(ValueError, match="affine"):
            depth_prior_loss(x, y, affine=bad)


def test_cpu_tensors_are_refused():
    x, y = torch.rand(5, 7, requires_grad=True), torch.rand(5, 7)
    for call in (lambda: depth_prior_loss(x, y), lambda: depth_prior_loss(x, y, align="lstsq", kind="l2"),
                 lambda: depth_prior_loss(x, y, torch.ones(5, 7, dtype=torch.bool)), lambda: pearson_depth_loss(x, y),
                 lambda: scale_shift(x.detach(), y),
                 lambda: depth_prior_loss(x, y, affine=(torch.ones((), requires_grad=True), 0.0))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_a_prior_or_mask_that_requires_grad_is_refused():
    x, y = torch.rand(5, 7), torch.rand(5, 7, requires_grad=True)
    for call in (lambda: depth_prior_loss(x, y), lambda: pearson_depth_loss(x, y),
                 lambda: depth_prior_loss(x, y.detach(), torch.ones(5, 7, requires_grad=True)),
                 lambda: pearson_depth_loss(x, y.detach(), torch.ones(5, 7, requires_grad=True))):
        with pytest.raises(NotImplementedError, match="requires grad"):
            call()
