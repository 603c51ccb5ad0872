"""The fused L1 / SSIM kernels of csrc/loss.hip per pixel against the fp64 oracle, at the shapes where a tiled kernel goes wrong.

Cases, contents and the error budget (measured from the oracle, never from the kernel) are tests/loss_cases.py; that the budget
has teeth is tests/test_loss_edges.py.  Every buffer a kernel writes through the C ABI sits between two guards of 64 sentinel
floats that are checked afterwards: an edge tile that writes outside its image shows here without faulting.
Measured on an MI355X: the 175 tests of this file take 3.3 s together.  Largest |hip - fp64| / budget: derivative maps 0.29,
per-tile partials 0.25, scalars 0.25 (flat; 0.08 elsewhere), backward from the oracle's maps 0.25, gradients through the Python
nodes 0.38 (same) and 0.50 (eq_px 1x1x1: one pixel); most maxima sit at 0.25 = 1 / FACTOR, i.e. the kernel's worst pixel is the
fp32 oracle's worst pixel.  16-bit inputs (budget plus half a spacing of the gradient's format): fp16 0.75, bf16 0.98.
Each check prints `[loss-ratio] <what> | <case> | <quantity> | <max |hip - fp64| / budget>` (pytest -s): the share of the factor 4 used.
"""
import numpy as np
import pytest
import torch

import loss_cases as lc

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -24681.5
DET_CASES = [((3, 33, 65), "noise"), ((3, 289, 321), "noise")]
ROUTE_SHAPE = (3, 33, 65)


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
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _report(what, case, ratios):
    for k, v in ratios.items():
        print(f"[loss-ratio] {what} | {lc.case_id(case)} | {k} | {v:.3f}")
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    return bad


def _forward(ref, with_maps=True):
    """(maps [3,C,H,W] or None, partials [np,2]) of cgs_l1_ssim_fwd, guards checked."""
    _lib, L = _L()
    C, H, W = ref.shape
    n_part = int(L.cgs_l1_ssim_partials(C, H, W))
    assert n_part == C * -(-H // lc.TILE) * -(-W // lc.TILE)
    x, y = _dev(ref.img), _dev(ref.gt)
    maps = Guarded(3 * C * H * W) if with_maps else None
    part = Guarded(2 * n_part)
    _lib.check(L.cgs_l1_ssim_fwd(_lib.ptr(x), _lib.ptr(y), C, H, W, _lib.ptr(maps.t) if maps else None, _lib.ptr(part.t),
                                 _lib.current_stream()), "cgs_l1_ssim_fwd")
    torch.cuda.synchronize()
    return (maps.numpy((3, C, H, W)) if maps else None), part.numpy((n_part, 2))


def _oracle_maps(ref):
    return _dev(np.stack([ref.o32[q] for q in lc.MAPS]))


def _backward(ref, g=None, g_loss=None, lam=None):
    """dimg of cgs_l1_ssim_bwd (lam None) or cgs_l1_ssim_bwd_loss from the ORACLE's fp32 maps: the backward on its own."""
    _lib, L = _L()
    C, H, W = ref.shape
    x, y, maps = _dev(ref.img), _dev(ref.gt), _oracle_maps(ref)
    gd = None if g is None else torch.tensor(g, dtype=torch.float32, device="cuda")
    gl = None if g_loss is None else torch.tensor([g_loss], dtype=torch.float32, device="cuda")
    d = Guarded(C * H * W)
    if lam is None:
        _lib.check(L.cgs_l1_ssim_bwd(_lib.ptr(x), _lib.ptr(y), _lib.ptr(maps), _lib.ptr(gd), C, H, W, _lib.ptr(d.t),
                                     _lib.current_stream()), "cgs_l1_ssim_bwd")
    else:
        _lib.check(L.cgs_l1_ssim_bwd_loss(_lib.ptr(x), _lib.ptr(y), _lib.ptr(maps), _lib.ptr(gl), _lib.ptr(gd), float(lam), C, H, W,
                                          _lib.ptr(d.t), _lib.current_stream()), "cgs_l1_ssim_bwd_loss")
    torch.cuda.synchronize()
    return d.numpy((C, H, W))


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_abi_forward_maps_and_partials(case):
    ref = lc.reference(*case)
    maps, part = _forward(ref)
    assert np.isfinite(maps).all() and np.isfinite(part).all()
    r = {q: ref.ratio(q, maps[i]) for i, q in enumerate(lc.MAPS)}
    r["tile_l1"], r["tile_ssim"] = ref.tile_ratio("tile_l1", part[:, 0]), ref.tile_ratio("tile_ssim", part[:, 1])
    n = ref.img.size
    r["l1"] = ref.l1_ratio(part[:, 0].sum(dtype=np.float64) / n)
    r["ssim_mean"] = ref.ssim_ratio(part[:, 1].sum(dtype=np.float64) / n)
    bad = _report("fwd", case, r)
    assert not bad, (bad, {q: ref.where(q, maps[i]) for i, q in enumerate(lc.MAPS) if q in bad})
    none, part2 = _forward(ref, with_maps=False)
    assert none is None and part2.tobytes() == part.tobytes()
    if case[1] == "same":
        assert (part[:, 0] == 0.0).all()


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_abi_backward_from_the_oracle_maps(case):
    ref = lc.reference(*case)
    r, got = {}, {}
    for g in lc.G_PAIRS:
        got[f"bwd{g}"] = (g, _backward(ref, g=g))
    f32 = np.float32
    for lam in (0.2, 0.0, 1.0):
        pair = (float(f32(1) - f32(lam)), float(-f32(lam)))
        d = _backward(ref, g_loss=1.0, lam=lam)
        got[f"loss(1,lam={lam})"] = (pair, d)
        assert d.tobytes() == _backward(ref, g=pair, lam=lam).tobytes(), lam             # (g_loss = 1, lam) IS g2 = (1 - lam, -lam)
        assert d.tobytes() == _backward(ref, g=pair).tobytes(), lam
    got["loss(2.5,lam=0.2)"] = ((2.5 * 0.8, -2.5 * 0.2), _backward(ref, g_loss=2.5, lam=0.2))
    got["g2 only"] = ((0.5, -0.25), _backward(ref, g=(0.5, -0.25), lam=0.2))
    got["loss and g2"] = ((0.5 + 1.5 * 0.8, -0.25 - 1.5 * 0.2), _backward(ref, g=(0.5, -0.25), g_loss=1.5, lam=0.2))
    for k, (pair, d) in got.items():
        assert np.isfinite(d).all(), k
        r[k] = ref.ratio(pair, d)
    bad = _report("bwd", case, r)
    assert not bad, (bad, {k: ref.where(got[k][0], got[k][1]) for k in bad})
    if case[1] == "same":                                    # sign(0) = 0: the L1 term gives exactly nothing
        assert not got[f"bwd{lc.G_PAIRS[0]}"][1].any()


# ---- Python nodes ----------------------------------------------------------------------------------------------------------------
def _grad(out, x, **kw):
    (g,) = torch.autograd.grad(out, [x], **kw)
    return g


def _nodes(ref, case, what, x, gt):
    """l1_ssim / ssim / l1_loss / training_image_loss on (x, gt) against `ref`, and against each other."""
    from contextgs_amd.loss_utils import l1_loss, l1_ssim, ssim, training_image_loss
    r = {}

    def grad_ratio(pair, g):
        assert g.shape == x.shape and g.dtype == x.dtype
        g = g.detach().float().cpu().numpy().reshape(ref.shape)
        assert np.isfinite(g).all()
        return ref.ratio(pair, g)

    l1, s = l1_ssim(x, gt)
    r["l1"], r["ssim_mean"] = ref.l1_ratio(float(l1)), ref.ssim_ratio(float(s))
    ga = _grad(0.8 * l1 + 0.2 * (1.0 - s), x)
    r["grad l1_ssim"] = grad_ratio(lc.G_DEFAULT, ga)
    s1, a1 = ssim(x, gt), l1_loss(x, gt)
    assert float(s1) == float(s) and float(a1) == float(l1)
    r["grad ssim"] = grad_ratio((0.0, 1.0), _grad(s1, x))                   # only SSIM: no gradient arrives for L1
    r["grad l1_loss"] = grad_ratio((1.0, 0.0), _grad(a1, x))                # only L1
    loss, l1t, st = training_image_loss(x, gt, 0.2)
    r["t l1"], r["t ssim_mean"] = ref.l1_ratio(float(l1t)), ref.ssim_ratio(float(st))
    assert abs(float(l1t) - float(l1)) < 1e-6 and abs(float(st) - float(s)) < 2e-6
    assert abs(float(loss) - (0.8 * float(l1t) + 0.2 * (1.0 - float(st)))) < 2e-6
    gb = _grad(loss, x, retain_graph=True)
    r["grad training"] = grad_ratio(lc.G_DEFAULT, gb)
    assert float((gb - ga).abs().max()) <= 1e-6 * float(ga.abs().max()) + 1e-12
    r["grad t.l1"] = grad_ratio((1.0, 0.0), _grad(l1t, x, retain_graph=True))
    r["grad t.ssim"] = grad_ratio((0.0, 1.0), _grad(st, x, retain_graph=True))
    r["grad t.mixed"] = grad_ratio((2.0 * 0.8 + 0.5, -2.0 * 0.2 - 0.25), _grad(2.0 * loss + 0.5 * l1t - 0.25 * st, x))
    bad = _report(what, case, r)
    assert not bad, bad


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_python_nodes_per_pixel(case):
    ref = lc.reference(*case)
    _nodes(ref, case, "nodes", _dev(ref.img).requires_grad_(), _dev(ref.gt))


@pytest.mark.parametrize("case", lc.BIG_CASES, ids=lc.case_id)
def test_finish_kernel_beyond_one_trip(case):
    """330 partials (no multiple of 256) and two rows of 257 tiles (514): l1_ssim_finish_kernel's stride loop goes round."""
    _lib, L = _L()
    ref = lc.reference(*case)
    assert int(L.cgs_l1_ssim_partials(*ref.shape)) == {(3, 289, 321): 330, (1, 33, 8200): 514}[ref.shape]
    _nodes(ref, case, "finish", _dev(ref.img).requires_grad_(), _dev(ref.gt))


def test_finish_partial_counts():
    _lib, L = _L()
    assert int(L.cgs_l1_ssim_partials(3, 289, 321)) == 330 and int(L.cgs_l1_ssim_partials(1, 33, 8200)) == 514
    assert int(L.cgs_l1_ssim_partials(1, 32, 8200)) == 257


@pytest.mark.parametrize("case", DET_CASES, ids=lc.case_id)
def test_two_runs_are_bit_identical(case):
    from contextgs_amd.loss_utils import l1_ssim, training_image_loss
    ref = lc.reference(*case)
    runs = []
    for _ in range(2):
        maps, part = _forward(ref)
        d = _backward(ref, g=lc.G_DEFAULT)
        dl = _backward(ref, g=(0.5, -0.25), g_loss=1.5, lam=0.2)
        x, gt = _dev(ref.img).requires_grad_(), _dev(ref.gt)
        l1, s = l1_ssim(x, gt)
        ga = _grad(0.8 * l1 + 0.2 * (1.0 - s), x)
        out3 = training_image_loss(x, gt, 0.2)
        gb = _grad(out3[0], x)
        runs.append([maps, part, d, dl] + [t.detach().cpu().numpy() for t in (l1, s, ga, gb) + tuple(out3)])
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
# fp16's subnormal range, which a gradient of 1 / (C H W) reaches) comes on top of the budget.
SLACK = {"fp16": (2.0 ** -11, 2.0 ** -25), "bf16": (2.0 ** -8, 0.0)}


@pytest.mark.parametrize("name", ["batch1", "permuted", "crop", "fp16", "bf16"])
def test_input_routes(name):
    from contextgs_amd.loss_utils import l1_ssim, training_image_loss
    img, gt = lc.images(ROUTE_SHAPE, "noise")
    store_x, view = _route(name, img)
    store_y, _ = _route(name, gt)
    seen_x, seen_y = view(store_x).float().cpu().numpy(), view(store_y).float().cpu().numpy()     # what the kernel sees
    if name in SLACK:
        assert not np.array_equal(seen_x, img)
    else:
        assert np.array_equal(seen_x, img)
    ref = lc.Reference(np.ascontiguousarray(seen_x), np.ascontiguousarray(seen_y))
    case = (ROUTE_SHAPE, name)
    for node in ("l1_ssim", "training"):
        leaf = store_x.clone().requires_grad_()
        x, y = view(leaf), view(store_y)
        if name == "batch1":
            x, y = leaf, store_y                              # the nodes take [1,C,H,W] themselves
        elif name != "crop" and name not in SLACK:
            assert not x.is_contiguous()
        if name == "crop":
            assert x.storage_offset() > 0 and not x.is_contiguous()
        if node == "l1_ssim":
            l1, s = l1_ssim(x, y)
            loss = 0.8 * l1 + 0.2 * (1.0 - s)
        else:
            loss, l1, s = training_image_loss(x, y, 0.2)
        r = {"l1": ref.l1_ratio(float(l1)), "ssim_mean": ref.ssim_ratio(float(s))}
        loss.backward()
        g = leaf.grad
        assert g.shape == leaf.shape and g.dtype == leaf.dtype
        gv = view(g).float().cpu().numpy()
        tol = ref.budget(lc.G_DEFAULT)
        if name in SLACK:
            tol = tol + SLACK[name][0] * np.abs(lc.combine(ref.o64, *lc.G_DEFAULT)) + SLACK[name][1]
        r["grad"] = float((ref.error(lc.G_DEFAULT, gv) / tol).max())
        if name == "crop":                                    # nothing flows to the pixels outside the crop
            outside = g.clone()
            outside[:, 3:3 + ROUTE_SHAPE[1], 2:2 + ROUTE_SHAPE[2]] = 0
            assert not outside.any()
        bad = _report(f"route-{node}", case, r)
        assert not bad, bad


def test_image_without_grad_allocates_no_maps():
    from contextgs_amd.loss_utils import l1_ssim, training_image_loss
    case = lc.BIG_CASES[0]
    ref = lc.reference(*case)
    x, gt = _dev(ref.img), _dev(ref.gt)
    l1_ssim(x, gt), training_image_loss(x, gt, 0.2)                        # (the library, the stream and the allocator are warm)
    for node in (lambda: l1_ssim(x, gt), lambda: training_image_loss(x, gt, 0.2)[1:]):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        l1, s = node()
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - before
        assert grown < 3 * ref.img.size * 4, grown
        assert not l1.requires_grad and not s.requires_grad
        assert ref.l1_ratio(float(l1)) <= 1.0 and ref.ssim_ratio(float(s)) <= 1.0


# ---- argument checks ---------------------------------------------------------------------------------------------------------------
def test_abi_rejects_bad_arguments_without_launching():
    _lib, L = _L()
    C, H, W = 2, 5, 7
    x, y = torch.rand(C, H, W, device="cuda"), torch.rand(C, H, W, device="cuda")
    maps, part, d = torch.zeros(3, C, H, W, device="cuda"), torch.zeros(C, 2, device="cuda"), torch.zeros(C, H, W, device="cuda")
    g, gl = torch.ones(2, device="cuda"), torch.ones(1, device="cuda")
    st, p = _lib.current_stream(), _lib.ptr

    def rejected(rc):
        assert rc != 0
        msg = L.cgs_last_error()
        assert msg and b"l1_ssim" in msg, msg

    for shape in ((0, H, W), (C, 0, W), (C, H, 0)):
        rejected(L.cgs_l1_ssim_fwd(p(x), p(y), *shape, p(maps), p(part), st))
        rejected(L.cgs_l1_ssim_bwd(p(x), p(y), p(maps), p(g), *shape, p(d), st))
        rejected(L.cgs_l1_ssim_bwd_loss(p(x), p(y), p(maps), p(gl), p(g), 0.2, *shape, p(d), st))
        rejected(L.cgs_l1_ssim_finish(p(part), *shape, 0.2, p(d), st))
    rejected(L.cgs_l1_ssim_fwd(None, p(y), C, H, W, p(maps), p(part), st))
    rejected(L.cgs_l1_ssim_fwd(p(x), None, C, H, W, p(maps), p(part), st))
    rejected(L.cgs_l1_ssim_fwd(p(x), p(y), C, H, W, p(maps), None, st))
    rejected(L.cgs_l1_ssim_bwd(p(x), p(y), None, p(g), C, H, W, p(d), st))
    rejected(L.cgs_l1_ssim_bwd_loss(p(x), p(y), None, p(gl), p(g), 0.2, C, H, W, p(d), st))
    rejected(L.cgs_l1_ssim_bwd_loss(p(x), p(y), p(maps), None, None, 0.2, C, H, W, p(d), st))
    torch.cuda.synchronize()
    assert not maps.any() and not part.any() and not d.any()             # nothing ran


@pytest.mark.parametrize("fn", ["l1_ssim", "ssim", "l1_loss", "training_image_loss"])
def test_a_target_that_requires_grad_is_refused(fn):
    """The fused loss differentiates its first image only; a second argument that asks for a gradient is an error, not zeros."""
    from contextgs_amd import loss_utils
    x = torch.rand(3, 9, 12, device="cuda", requires_grad=True)
    gt = torch.rand(3, 9, 12, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="first image only"):
        getattr(loss_utils, fn)(x, gt)
    with pytest.raises(NotImplementedError, match="first image only"):
        getattr(loss_utils, fn)(x.detach(), gt)                            # swapped arguments
    out = getattr(loss_utils, fn)(x, gt.detach())                          # a detached target is the way out
    assert (out[0] if isinstance(out, tuple) else out).requires_grad
