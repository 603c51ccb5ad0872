"""The weighted / exposed image loss (`cgs_l1_ssim_w_*` of csrc/loss.hip, `training_image_loss(..., weight=, exposure=)`) per pixel
against the fp64 oracle, at the shapes where a tiled kernel goes wrong.

Cases, weight patterns, exposure matrices and every budget (measured from the oracle, never from the kernel) are
tests/loss_weighted_ref.py; that the budget has teeth is tests/test_loss_weighted.py.  Every buffer a kernel writes through the
C ABI sits between two guards of 64 sentinel floats that are checked afterwards.  The backward through the C ABI runs on the
ORACLE's fp32 weighted maps and its 1 / (C S): the backward on its own; the Python node runs the whole chain.
Each check prints `[loss-ratio] <what> | <case> | <quantity> | <max |hip - fp64| / budget>` (pytest -s).
Measured on an MI355X: the 248 tests of this file take 5.4 s together.  Largest ratios: weighted maps 0.37, per-workgroup
partials 0.25, scalars 0.25, dimg / dE from the oracle's maps 0.27 / 0.28, through the node gradients 0.29 and dE 0.75 (flat,
left0, generic E); 16-bit images (budget plus half a spacing of the gradient's format): fp16 0.93, bf16 0.99.
"""
import numpy as np
import pytest
import torch

import loss_cases as lc
import loss_weighted_ref as wr

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -24681.5
LAM = 0.2
ROUTE_CASE = ((3, 33, 65), "noise", "soft", "generic")
DET_CASES = [ROUTE_CASE, wr.BIG_CASES[0]]
# (g2, g_loss) of a backward call and the pair (g0, g1) of d(g0 L1 + g1 SSIM) it amounts to at LAM = 0.2
BWD_CALLS = [((1.0, 0.0), None, (1.0, 0.0)), ((0.0, 1.0), None, (0.0, 1.0)), ((0.5, -0.25), None, (0.5, -0.25)),
             (None, 1.0, (0.8, -0.2)), (None, 2.5, (2.5 * 0.8, -2.5 * 0.2)), ((0.5, -0.25), 1.5, (0.5 + 1.5 * 0.8, -0.25 - 1.5 * 0.2))]


def _L():
    from contextgs_amd import _lib
    return _lib, _lib.lib()


class Guarded:
    """n floats with GUARD sentinel floats on each side."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]
        self.t.fill_(float("nan"))                    # an element the kernel should have written and did not stays nan

    def numpy(self, shape):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == np.float32(SENTINEL)).all() and (b[GUARD + self.n:] == np.float32(SENTINEL)).all(), "write outside the buffer"
        return b[GUARD:GUARD + self.n].reshape(shape).copy()


def _dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device="cuda")


def _report(what, case, ratios):
    for k, v in ratios.items():
        print(f"[loss-ratio] {what} | {wr.case_id(case)} | {k} | {v:.3f}")
    return {k: v for k, v in ratios.items() if not v <= 1.0}


def _forward(ref, with_maps=True):
    """(maps [3,C,H,W] or None, partials [np,3], out3, inv_cs) of cgs_l1_ssim_w_fwd + cgs_l1_ssim_w_finish, guards checked."""
    _lib, L = _L()
    C, H, W = ref.shape
    n_part = int(L.cgs_l1_ssim_partials(C, H, W))
    x, y, w, E = _dev(ref.img), _dev(ref.gt), _dev(ref.w), _dev(ref.Em)
    maps = Guarded(3 * C * H * W) if with_maps else None
    part, out3, inv = Guarded(3 * n_part), Guarded(3), Guarded(1)
    st, p = _lib.current_stream(), _lib.ptr
    _lib.check(L.cgs_l1_ssim_w_fwd(p(x), p(y), p(w), p(E), C, H, W, p(maps.t) if maps else None, p(part.t), st), "cgs_l1_ssim_w_fwd")
    _lib.check(L.cgs_l1_ssim_w_finish(p(part.t), C, H, W, LAM, p(out3.t), p(inv.t), st), "cgs_l1_ssim_w_finish")
    torch.cuda.synchronize()
    return (maps.numpy((3, C, H, W)) if maps else None), part.numpy((n_part, 3)), out3.numpy((3,)), inv.numpy((1,))


def _inv_cs(ref):
    cs = ref.o64["cs"]
    return np.float32(1.0 / cs if cs > 0 else 0.0)


def _backward(ref, g2=None, g_loss=None, dimg=True, dE=True):
    """(dimg, dE partials [tiles,3,4], dE [3,4]) of cgs_l1_ssim_w_bwd (+ cgs_l1_ssim_w_dexposure) from the ORACLE's fp32 maps."""
    _lib, L = _L()
    C, H, W = ref.shape
    x, y, w, E = _dev(ref.img), _dev(ref.gt), _dev(ref.w), _dev(ref.Em)
    maps, inv = _dev(np.stack([ref.o32[q] for q in wr.MAPS])), _dev(np.array([_inv_cs(ref)]))
    gd = None if g2 is None else torch.tensor(g2, dtype=torch.float32, device="cuda")
    gl = None if g_loss is None else torch.tensor([g_loss], dtype=torch.float32, device="cuda")
    nt = int(L.cgs_l1_ssim_partials(1, H, W))
    d = Guarded(C * H * W) if dimg else None
    part = Guarded(12 * nt) if (dE and E is not None) else None
    out = Guarded(12) if part else None
    st, p = _lib.current_stream(), _lib.ptr
    _lib.check(L.cgs_l1_ssim_w_bwd(p(x), p(y), p(w), p(E), p(maps), p(inv), p(gl), p(gd), LAM, C, H, W, p(d.t) if d else None,
                                   p(part.t) if part else None, st), "cgs_l1_ssim_w_bwd")
    if part:
        _lib.check(L.cgs_l1_ssim_w_dexposure(p(part.t), H, W, p(out.t), st), "cgs_l1_ssim_w_dexposure")
    torch.cuda.synchronize()
    return (d.numpy((C, H, W)) if d else None), (part.numpy((nt, 3, 4)) if part else None), (out.numpy((3, 4)) if out else None)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wr.CASES + wr.BIG_CASES, ids=wr.case_id)
def test_abi_forward_maps_partials_and_scalars(case):
    ref = wr.reference(*case)
    C, H, W = ref.shape
    maps, part, out3, inv = _forward(ref)
    assert np.isfinite(maps).all() and np.isfinite(part).all() and np.isfinite(out3).all() and np.isfinite(inv).all()
    r = {q: ref.ratio(q, maps[i]) for i, q in enumerate(wr.MAPS)}
    for i, q in enumerate(("tile_l1", "tile_ssim", "tile_w")):
        r[q] = ref.tile_ratio(q, part[:, i])
    r["l1"], r["ssim_mean"] = ref.l1_ratio(out3[1]), ref.ssim_ratio(out3[2])
    cs = ref.o64["cs"]
    if cs > 0:
        # 1 / (C S): what the weight partials' own budget allows for C S, and the rounding of the quotient
        d_cs = float((wr.FACTOR * np.abs(ref.o32["tile_w"].astype(np.float64) - ref.o64["tile_w"]) + 1e-6 * ref.npix).sum())
        r["inv_cs"] = abs(float(inv[0]) - 1.0 / cs) / (d_cs / cs ** 2 + wr.EPS32 / cs)
        assert abs(part[:, 2].sum(dtype=np.float64) - cs) <= d_cs
    else:
        assert out3.tolist() == [0.0, 0.0, 1.0] and inv[0] == 0.0 and not maps.any() and not part.any()
    assert abs(float(out3[0]) - ((1.0 - LAM) * float(out3[1]) + LAM * (1.0 - float(out3[2])))) < 2e-6
    bad = _report("w-fwd", case, r)
    assert not bad, bad
    none, part2, out3b, invb = _forward(ref, with_maps=False)
    assert none is None and part2.tobytes() == part.tobytes() and out3b.tobytes() == out3.tobytes() and invb.tobytes() == inv.tobytes()


@pytest.mark.parametrize("case", wr.CASES + wr.BIG_CASES, ids=wr.case_id)
def test_abi_backward_from_the_oracle_maps(case):
    ref = wr.reference(*case)
    shape, cls, wname, ename = case
    r, got = {}, {}
    for g2, g_loss, pair in BWD_CALLS:
        d, part, dE = _backward(ref, g2=g2, g_loss=g_loss)
        key = f"g2={g2} g_loss={g_loss}"
        got[key] = (pair, d)
        assert np.isfinite(d).all(), key
        r[f"dimg {key}"] = ref.ratio(pair, d)
        if ename is None:
            assert part is None and dE is None
            continue
        assert np.isfinite(part).all() and np.isfinite(dE).all(), key
        r[f"dE {key}"] = ref.dE_ratio(pair, dE)
        assert (np.abs(part.sum(axis=0, dtype=np.float64) - dE) <= wr.EPS32 * np.abs(part).sum(axis=0, dtype=np.float64)).all()
    if ename is not None:            # either output alone is the same bytes
        g2, g_loss, pair = BWD_CALLS[-1]
        d, part, dE = _backward(ref, g2=g2, g_loss=g_loss)
        d1, p1, e1 = _backward(ref, g2=g2, g_loss=g_loss, dE=False)
        d2, p2, e2 = _backward(ref, g2=g2, g_loss=g_loss, dimg=False)
        assert p1 is None and e1 is None and d2 is None
        assert d1.tobytes() == d.tobytes() and p2.tobytes() == part.tobytes() and e2.tobytes() == dE.tobytes()
    bad = _report("w-bwd", case, r)
    assert not bad, bad
    if wname == "zero":
        assert all(not d.any() for _, d in got.values())
    if wname == "left0" and shape[2] > 32:
        d_l1, d_ssim = got["g2=(1.0, 0.0) g_loss=None"][1], got["g2=(0.0, 1.0) g_loss=None"][1]
        assert not d_l1[:, :, :32].any()                   # weight 0: exactly nothing from L1 ...
        assert not d_ssim[:, :, :27].any() and (d_ssim[:, :, 27:32] != 0).all()       # ... and the window's reach of SSIM


def test_abi_rejects_bad_arguments_without_launching():
    _lib, L = _L()
    C, H, W = 3, 5, 7
    x, y, w, E = (torch.rand(*s, device="cuda") for s in ((C, H, W), (C, H, W), (H, W), (3, 4)))
    x2, y2 = torch.rand(2, H, W, device="cuda"), torch.rand(2, H, W, device="cuda")
    maps, part, d = torch.zeros(3, C, H, W, device="cuda"), torch.zeros(C, 3, device="cuda"), torch.zeros(C, H, W, device="cuda")
    dpart, dE, out3, inv = (torch.zeros(n, device="cuda") for n in (12, 12, 3, 1))
    g, gl, one = torch.ones(2, device="cuda"), torch.ones(1, device="cuda"), torch.ones(1, device="cuda")
    st, p = _lib.current_stream(), _lib.ptr

    def rejected(rc):
        assert rc != 0
        msg = L.cgs_last_error()
        assert msg and b"l1_ssim_w" in msg, msg

    for shape in ((0, H, W), (C, 0, W), (C, H, 0)):
        rejected(L.cgs_l1_ssim_w_fwd(p(x), p(y), p(w), None, *shape, p(maps), p(part), st))
        rejected(L.cgs_l1_ssim_w_finish(p(part), *shape, LAM, p(out3), p(inv), st))
        rejected(L.cgs_l1_ssim_w_bwd(p(x), p(y), p(w), None, p(maps), p(one), p(gl), p(g), LAM, *shape, p(d), None, st))
    rejected(L.cgs_l1_ssim_w_dexposure(p(dpart), 0, W, p(dE), st))
    rejected(L.cgs_l1_ssim_w_dexposure(p(dpart), H, 0, p(dE), st))
    rejected(L.cgs_l1_ssim_w_dexposure(None, H, W, p(dE), st))
    rejected(L.cgs_l1_ssim_w_dexposure(p(dpart), H, W, None, st))
    rejected(L.cgs_l1_ssim_w_fwd(None, p(y), p(w), p(E), C, H, W, p(maps), p(part), st))
    rejected(L.cgs_l1_ssim_w_fwd(p(x), None, p(w), p(E), C, H, W, p(maps), p(part), st))
    rejected(L.cgs_l1_ssim_w_fwd(p(x), p(y), p(w), p(E), C, H, W, p(maps), None, st))
    rejected(L.cgs_l1_ssim_w_fwd(p(x2), p(y2), p(w), p(E), 2, H, W, p(maps), p(part), st))            # an exposure with C != 3
    rejected(L.cgs_l1_ssim_w_finish(None, C, H, W, LAM, p(out3), p(inv), st))
    rejected(L.cgs_l1_ssim_w_finish(p(part), C, H, W, LAM, None, p(inv), st))
    rejected(L.cgs_l1_ssim_w_finish(p(part), C, H, W, LAM, p(out3), None, st))
    rejected(L.cgs_l1_ssim_w_bwd(p(x), p(y), p(w), p(E), None, p(one), p(gl), p(g), LAM, C, H, W, p(d), p(dpart), st))
    rejected(L.cgs_l1_ssim_w_bwd(p(x), p(y), p(w), p(E), p(maps), None, p(gl), p(g), LAM, C, H, W, p(d), p(dpart), st))
    rejected(L.cgs_l1_ssim_w_bwd(p(x), p(y), p(w), p(E), p(maps), p(one), None, None, LAM, C, H, W, p(d), p(dpart), st))
    rejected(L.cgs_l1_ssim_w_bwd(p(x), p(y), p(w), p(E), p(maps), p(one), p(gl), p(g), LAM, C, H, W, None, None, st))
    rejected(L.cgs_l1_ssim_w_bwd(p(x), p(y), p(w), None, p(maps), p(one), p(gl), p(g), LAM, C, H, W, p(d), p(dpart), st))   # dE without E
    rejected(L.cgs_l1_ssim_w_bwd(p(x), p(y), p(w), None, p(maps), p(one), p(gl), p(g), LAM, C, H, W, None, None, st))
    rejected(L.cgs_l1_ssim_w_bwd(p(x2), p(y2), p(w), p(E), p(maps), p(one), p(gl), p(g), LAM, 2, H, W, p(d), p(dpart), st))
    torch.cuda.synchronize()
    for t in (maps, part, d, dpart, dE, out3, inv):
        assert not t.any()                                                # nothing ran


# ---- the Python node -------------------------------------------------------------------------------------------------------------
def _node(ref, x, gt, w, E):
    """training_image_loss on device tensors: the three values and the gradients of loss, L1, SSIM and a mixture, against `ref`."""
    from contextgs_amd.loss_utils import training_image_loss
    loss, l1, s = training_image_loss(x, gt, LAM, weight=w, exposure=E)
    vals = tuple(float(t.detach()) for t in (loss, l1, s))
    r = {"l1": ref.l1_ratio(vals[1]), "ssim_mean": ref.ssim_ratio(vals[2])}
    assert abs(vals[0] - ((1.0 - LAM) * vals[1] + LAM * (1.0 - vals[2]))) < 2e-6
    wrt =[x] + ([E] if E is not None and E.requires_grad else [])
    heads = {"loss": (loss, (0.8, -0.2)), "L1": (l1, (1.0, 0.0)), "SSIM": (s, (0.0, 1.0)),
             "mixed": (2.0 * loss + 0.5 * l1 - 0.25 * s, (2.0 * 0.8 + 0.5, -2.0 * 0.2 - 0.25))}
    grads = {}
    for name, (head, pair) in heads.items():
        gs = torch.autograd.grad(head, wrt, retain_graph=True)
        assert gs[0].shape == x.shape and gs[0].dtype == x.dtype
        gx = gs[0].detach().float().cpu().numpy().reshape(ref.shape)
        assert np.isfinite(gx).all()
        r[f"grad {name}"] = ref.ratio(pair, gx)
        grads[name] = [gx]
        if len(gs) > 1:
            assert gs[1].shape == (3, 4) and gs[1].dtype == E.dtype
            ge = gs[1].detach().float().cpu().numpy()
            r[f"dE {name}"] = ref.dE_ratio(pair, ge)
            grads[name].append(ge)
    return vals, grads, r


@pytest.mark.parametrize("case", wr.CASES + wr.BIG_CASES, ids=wr.case_id)
def test_python_node_per_pixel(case):
    ref = wr.reference(*case)
    shape, cls, wname, ename = case
    x, gt, w = _dev(ref.img).requires_grad_(), _dev(ref.gt), _dev(ref.w)
    E = None if ename is None else _dev(ref.Em).requires_grad_()
    vals, grads, r = _node(ref, x, gt, w, E)
    # what the unweighted reference of loss_cases says where the keywords change nothing, or only the order of the channels
    plain = None
    if (wname in (None, "ones")) and ename in (None, "identity"):
        plain = lc.reference(shape, cls)
    elif wname is None and ename == "perm":                     # x'_c = x_PERM[c] exactly: the plain loss of the permuted image
        plain = lc.Reference(np.ascontiguousarray(ref.img[list(wr.PERM)]), ref.gt)
    if plain is not None:
        r["plain l1"], r["plain ssim_mean"] = plain.l1_ratio(vals[1]), plain.ssim_ratio(vals[2])
        for name, pair in (("loss", (0.8, -0.2)), ("L1", (1.0, 0.0)), ("SSIM", (0.0, 1.0))):
            gx = grads[name][0]
            r[f"plain grad {name}"] = plain.ratio(pair, gx[list(wr.PERM)] if ename == "perm" else gx)      # dx_PERM[c] = G_c
    if wname == "zero":
        assert vals == (0.0, 0.0, 1.0) and all(not g.any() for gs in grads.values() for g in gs)
    bad = _report("w-node", case, r)
    assert not bad, bad


def test_keywords_left_at_none_are_the_plain_call():
    from contextgs_amd.loss_utils import training_image_loss
    ref = lc.reference((3, 33, 65), "noise")
    out = []
    for kw in ({}, {"weight": None, "exposure": None}):
        x, gt = _dev(ref.img).requires_grad_(), _dev(ref.gt)
        vals = training_image_loss(x, gt, LAM, **kw)
        assert type(vals[0].grad_fn).__name__ == "_TrainImageLossBackward"      # the plain node, not the weighted one
        (g,) = torch.autograd.grad(2.0 * vals[0] + 0.5 * vals[1] - 0.25 * vals[2], [x])
        out.append([t.detach().cpu().numpy().tobytes() for t in vals + (g,)])
    assert out[0] == out[1]


@pytest.mark.parametrize("case", DET_CASES, ids=wr.case_id)
def test_two_runs_are_bit_identical(case):
    ref = wr.reference(*case)
    runs = []
    for _ in range(2):
        maps, part, out3, inv = _forward(ref)
        d, dpart, dE = _backward(ref, g2=(0.5, -0.25), g_loss=1.5)
        x, gt, w, E = _dev(ref.img).requires_grad_(), _dev(ref.gt), _dev(ref.w), _dev(ref.Em).requires_grad_()
        vals, grads, _ = _node(ref, x, gt, w, E)
        runs.append([maps, part, out3, inv, d, dpart, dE, np.array(vals)] + [g for gs in grads.values() for g in gs])
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()


# ---- input routes ----------------------------------------------------------------------------------------------------------------
def _route(name, a):
    """A device tensor that holds the values of the [C,H,W] array `a` in the form `name`; and the [C,H,W] view of it."""
    C, H, W = a.shape
    t = _dev(a)
    if name == "batch1":
        t = t[None].contiguous()
        return t, lambda v: v[0]
    if name == "permuted":
        t = t.permute(1, 2, 0).contiguous()                    # stored [H,W,C]
        return t, lambda v: v.permute(2, 0, 1)
    if name == "crop":
        big = torch.rand(C, H + 7, W + 5, device="cuda")
        big[:, 3:3 + H, 2:2 + W] = t
        return big, lambda v: v[:, 3:3 + H, 2:2 + W]
    return t.to({"fp16": torch.float16, "bf16": torch.bfloat16}[name]), lambda v: v


# A 16-bit image gets its gradient back in its own format: half a spacing of that format (relative for normal numbers, 2^-25 in
# fp16's subnormal range, which a gradient of 1 / (C S) reaches) comes on top of the budget (as in tests/test_loss_edges_gpu.py).
SLACK = {"fp16": (2.0 ** -11, 2.0 ** -25), "bf16": (2.0 ** -8, 0.0)}


@pytest.mark.parametrize("name", ["batch1", "permuted", "crop", "fp16", "bf16"])
def test_image_routes(name):
    from contextgs_amd.loss_utils import training_image_loss
    shape, cls, wname, ename = ROUTE_CASE
    img, gt = lc.images(shape, cls)
    store_x, view = _route(name, img)
    store_y, _ = _route(name, gt)
    seen_x, seen_y = view(store_x).float().cpu().numpy(), view(store_y).float().cpu().numpy()     # what the kernel sees
    assert np.array_equal(seen_x, img) == (name not in SLACK)
    ref = wr.WeightedReference(np.ascontiguousarray(seen_x), np.ascontiguousarray(seen_y), wr.weight(shape, wname), wr.exposure(ename))
    leaf, E = store_x.clone().requires_grad_(), _dev(ref.Em).requires_grad_()
    x, y = (leaf, store_y) if name == "batch1" else (view(leaf), view(store_y))
    if name in ("permuted", "crop"):
        assert not x.is_contiguous()
    loss, l1, s = training_image_loss(x, y, LAM, weight=_dev(ref.w), exposure=E)
    r = {"l1": ref.l1_ratio(l1.item()), "ssim_mean": ref.ssim_ratio(s.item())}
    loss.backward()
    g = leaf.grad
    assert g.shape == leaf.shape and g.dtype == leaf.dtype and E.grad.dtype == torch.float32
    gv = view(g).float().cpu().numpy()
    pair = (0.8, -0.2)
    tol = ref.budget(pair)
    if name in SLACK:
        tol = tol + SLACK[name][0] * np.abs(ref._pair(pair)[1]) + SLACK[name][1]
    r["grad"] = float((ref.error(pair, gv) / tol).max())
    r["dE"] = ref.dE_ratio(pair, E.grad.cpu().numpy())
    if name == "crop":                                        # nothing flows to the pixels outside the crop
        outside = g.clone()
        outside[:, 3:3 + shape[1], 2:2 + shape[2]] = 0
        assert not outside.any()
    bad = _report(f"w-route-{name}", ROUTE_CASE, r)
    assert not bad, bad


@pytest.mark.parametrize("name", ["bool", "fp16", "1hw", "strided"])
def test_weight_routes(name):
    shape, cls, _, ename = ROUTE_CASE
    H, W = shape[1:]
    w = wr.weight(shape, "binary" if name == "bool" else "soft")
    if name == "bool":
        wt = _dev(w).bool()
    elif name == "fp16":
        wt = _dev(w).half()
        w = wt.float().cpu().numpy()
    elif name == "1hw":
        wt = _dev(w)[None]
    else:
        wt = _dev(np.ascontiguousarray(w.T)).t()              # [H,W], stored [W,H]
        assert not wt.is_contiguous()
    img, gt = lc.images(shape, cls)
    ref = wr.WeightedReference(img, gt, w, wr.exposure(ename))
    _, _, r = _node(ref, _dev(img).requires_grad_(), _dev(gt), wt, _dev(ref.Em).requires_grad_())
    bad = _report(f"w-weight-{name}", ROUTE_CASE, r)
    assert not bad, bad


def test_exposure_without_grad_and_image_without_grad():
    """Either operand alone may ask for a gradient; the values do not depend on who asks."""
    from contextgs_amd.loss_utils import training_image_loss
    ref = wr.reference(*ROUTE_CASE)
    gt, w = _dev(ref.gt), _dev(ref.w)
    x, E = _dev(ref.img).requires_grad_(), _dev(ref.Em)
    loss, _, _ = training_image_loss(x, gt, LAM, weight=w, exposure=E)
    (gx,) = torch.autograd.grad(loss, [x])
    x2, E2 = _dev(ref.img), _dev(ref.Em).requires_grad_()
    loss2, _, _ = training_image_loss(x2, gt, LAM, weight=w, exposure=E2)
    (ge,) = torch.autograd.grad(loss2, [E2])
    assert loss.item() == loss2.item()
    r = {"grad": ref.ratio((0.8, -0.2), gx.cpu().numpy()), "dE": ref.dE_ratio((0.8, -0.2), ge.cpu().numpy())}
    bad = _report("w-one-sided", ROUTE_CASE, r)
    assert not bad, bad


def test_nothing_to_differentiate_allocates_no_maps():
    from contextgs_amd.loss_utils import training_image_loss
    case = wr.BIG_CASES[0]
    ref = wr.reference(*case)
    x, gt, w, E = _dev(ref.img), _dev(ref.gt), _dev(ref.w), _dev(ref.Em)
    training_image_loss(x, gt, LAM, weight=w, exposure=E)                  # (the library, the stream and the allocator are warm)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss, l1, s = training_image_loss(x, gt, LAM, weight=w, exposure=E)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    assert grown < 3 * ref.img.size * 4, grown
    assert not loss.requires_grad and not l1.requires_grad and not s.requires_grad
    assert ref.l1_ratio(l1.item()) <= 1.0 and ref.ssim_ratio(s.item()) <= 1.0


# ---- argument checks ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    from contextgs_amd.loss_utils import training_image_loss
    x, gt = torch.rand(3, 9, 12, device="cuda", requires_grad=True), torch.rand(3, 9, 12, device="cuda")
    x2, gt2 = torch.rand(2, 9, 12, device="cuda"), torch.rand(2, 9, 12, device="cuda")
    w, E = torch.rand(9, 12, device="cuda"), torch.eye(3, 4, device="cuda")
    for bad in (torch.rand(12, 9, device="cuda"), torch.rand(3, 9, 12, device="cuda"), torch.rand(9, device="cuda")):
        with pytest.raises(ValueError, match="weight"):
            training_image_loss(x, gt, LAM, weight=bad)
    with pytest.raises(NotImplementedError, match="weight"):
        training_image_loss(x, gt, LAM, weight=w.clone().requires_grad_())
    with pytest.raises(ValueError, match="three-channel"):
        training_image_loss(x2, gt2, LAM, exposure=E)
    for bad in (torch.eye(4, 3, device="cuda"), torch.eye(3, device="cuda"), torch.rand(1, 3, 4, device="cuda")):
        with pytest.raises(ValueError, match="exposure"):
            training_image_loss(x, gt, LAM, exposure=bad)
    with pytest.raises(ValueError, match="weight on cpu"):
        training_image_loss(x, gt, LAM, weight=w.cpu())
    with pytest.raises(ValueError, match="exposure on cpu"):
        training_image_loss(x, gt, LAM, exposure=E.cpu())
    with pytest.raises(ValueError, match="gt on cpu"):
        training_image_loss(x, gt.cpu(), LAM, weight=w)
    with pytest.raises(NotImplementedError, match="first image only"):
        training_image_loss(x, gt.clone().requires_grad_(), LAM, weight=w, exposure=E)
    assert training_image_loss(x, gt, LAM, weight=w, exposure=E)[0].requires_grad


# ---- the parameter holder ----------------------------------------------------------------------------------------------------------
def test_view_exposure():
    from contextgs_amd.exposure import ViewExposure
    from contextgs_amd.loss_utils import training_image_loss
    ref = lc.reference((3, 33, 65), "noise")
    x, gt = _dev(ref.img).requires_grad_(), _dev(ref.gt)
    ve = ViewExposure(4).cuda()
    assert ve.exposure.shape == (4, 3, 4) and torch.equal(ve.exposure.detach().cpu(), torch.eye(3, 4).expand(4, 3, 4))
    loss, l1, s = training_image_loss(x, gt, LAM, exposure=ve(2))          # the identity row: the call without an exposure
    r = {"l1": ref.l1_ratio(l1.item()), "ssim_mean": ref.ssim_ratio(s.item())}
    opt = torch.optim.SGD(ve.parameters(), lr=0.1)
    loss.backward()
    r["grad"] = ref.ratio(lc.G_DEFAULT, x.grad.cpu().numpy())
    bad = _report("view-exposure", ((3, 33, 65), "noise", None, "identity"), r)
    assert not bad, bad
    opt.step()
    after = ve.exposure.detach().cpu()
    eye = torch.eye(3, 4)
    assert all(torch.equal(after[i], eye) for i in (0, 1, 3)) and (after[2] != eye).all()
    # apply() is the same transform in plain torch
    E = torch.tensor(wr.exposure("generic"), device="cuda")
    with torch.no_grad():
        ve.exposure[1] = E
    want = wr.expose(ref.img.astype(np.float64), wr.exposure("generic").astype(np.float64))
    got = ve.apply(x.detach(), 1)
    assert got.requires_grad                                               # through autograd too, for whoever wants it
    assert np.abs(got.detach().cpu().numpy() - want).max() <= 8 * wr.EPS32 * np.abs(want).max()
    ve.apply(lambda m: None)                                               # nn.Module.apply(fn) still works
