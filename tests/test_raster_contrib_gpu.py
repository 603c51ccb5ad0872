"""GPU checks of the rasterizer's per-Gaussian contribution statistics and top-contributor maps (csrc/raster_contrib.hip)
against the existing oracle, unchanged, used as a per-pixel decomposition.

`oracle.render(colors = ones, bg = 0, dL_dout = one-hot at pixel p on channel 0)` returns dL_dcolors[:, 0] = w_i(p) for every
Gaussian i, so a loop over all pixels of a tiny image gives the whole matrix w[i, p] from the fp64 oracle; the sums, maxima,
counts (w > 0), the per-pixel argmax and the top counts follow from it in numpy.  One call with dL_dout = ones gives
sum_p w_i(p) for a scene of any size.

Tolerances.  `weight` and `max_weight`: `check_grad` of tests/raster_harness.py: at most a 2e-3 share of entries beyond 2e-4
of the tensor's maximum.  `top_weight`: `check_map`: RMSE <= 1e-5 of the map's maximum and at most a 1e-4 share of values
beyond 2e-5.  `pixels`, `top_pixels`, `count` and `top_id` are discrete, and a pair whose alpha sits at
1/255 or whose two largest weights nearly tie may fall either way in fp32, so: sum_i |pixels - ref| <= 1e-3 sum_i ref, the same
for top_pixels; count equal on >= 99.8 % of the pixels and never off by more than 2; top_id equal on every pixel whose two
largest reference weights differ by more than 1e-4 relative (and on every pixel without a contributor), and at most 1 % of the
pixels may be excluded that way.  These caps are conditions, not measurements: every decomposed scene below was first run on
the CPU with the fp32 oracle's decomposition against the fp64 oracle's under the same checks (`_check_stats(..., cap=0.5)`), and
kept only because the fp32 oracle alone stays within HALF of every cap; a scene that does not gets another seed, never
another cap.  Sums that float atomics build in an unspecified order are compared with the rigorous bound of a sum of n
non-negative fp32 addends, n 2^-24 relative, n counted from the call (`_sum_tol`).
References are computed once per scene and shared; nobody writes into them.
"""
import itertools

import numpy as np
import pytest
import torch

from contextgs_amd.synth import look_at_camera, random_gaussians
from raster_harness import (check_grad, check_map, cov6_torch, leaf, memo, model, named_scene, np_of, run, scene, settings,
                            sh_eval_torch, shs)

pytestmark = pytest.mark.gpu

FIELDS = ("weight", "max_weight", "pixels", "top_pixels")
DECOMPOSED = ("ragged", "long", "saturated", "single")


# ---- the oracle as a per-pixel decomposition ---------------------------------------------------------------------------------
def decompose(oracle, cam, g):
    """{"w": [P, H*W] in the oracle's precision, "final_T", "radii", "stats"}"""
    P = g["means3D"].shape[0]
    H, W = cam.image_height, cam.image_width
    ones = np.ones((P, 3), np.float32)
    cd = cam.oracle_dict(bg=(0.0, 0.0, 0.0))
    w = np.zeros((P, H * W), oracle.dtype)
    d = np.zeros((3, H, W), np.float32)
    r = None
    for p in range(H * W):
        d[0].flat[p] = 1.0
        r = oracle.render(cd, g["means3D"], ones, g["opacities"], g["scales"], g["rotations"], dL_dout=d)
        d[0].flat[p] = 0.0
        w[:, p] = r["dL_dcolors"][:, 0]
    return {"w": w, "final_T": r["final_T"], "radii": r["radii"], "stats": r["stats"]}


def stats_of(w, H, W):
    """Everything the kernel reports, from the matrix w[i, p] (ties in an exactly computed w do not occur in these scenes)."""
    P = w.shape[0]
    hit = w > 0
    top = np.where(hit.any(0), w.argmax(0), -1)
    srt = np.sort(w, axis=0)
    w1 = srt[-1]
    w2 = srt[-2] if P > 1 else np.zeros_like(w1)
    return {"weight": w.sum(1), "max_weight": w.max(1), "pixels": hit.sum(1).astype(np.int64),
            "top_pixels": np.bincount(top[top >= 0], minlength=P).astype(np.int64),
            "top_id": top.reshape(H, W).astype(np.int32), "top_weight": w1.reshape(1, H, W), "count": hit.sum(0).reshape(H, W),
            "w1": w1, "w2": w2}


def _check_stats(got, ref, what, cap=1.0):
    """`got`: the seven results as arrays; `ref`: stats_of() of the fp64 decomposition.  cap = 0.5: the fp32 oracle's own test."""
    check_grad(got["weight"], ref["weight"], f"weight {what}", allow_frac=2e-3 * cap)
    check_grad(got["max_weight"], ref["max_weight"], f"max_weight {what}", allow_frac=2e-3 * cap)
    check_map(got["top_weight"], ref["top_weight"], f"top_weight {what}", cap=cap)
    for k in ("pixels", "top_pixels"):
        a, b = np_of(got[k]).astype(np.int64), ref[k]
        off, tot = int(np.abs(a - b).sum()), int(b.sum())
        print(f"[allowance] {k} {what}: sum |got - ref| = {off} of {tot}")
        assert off <= 1e-3 * cap * tot, (k, what, off, tot)
    a, b = np_of(got["count"]).astype(np.int64), ref["count"]
    diff = np.abs(a - b)
    print(f"[allowance] count {what}: {int((diff != 0).sum())} of {diff.size} pixels differ, worst {int(diff.max())}")
    assert (diff == 0).mean() >= 1 - 2e-3 * cap and diff.max() <= 2, (what, int((diff != 0).sum()), int(diff.max()))
    decided = ((ref["w1"] - ref["w2"]) > 1e-4 * ref["w1"]) | (ref["w1"] == 0)
    print(f"[allowance] top_id {what}: {int((~decided).sum())} of {decided.size} pixels are near ties")
    assert (~decided).mean() <= 1e-2 * cap, (what, int((~decided).sum()))
    a, b = np_of(got["top_id"]).reshape(-1), ref["top_id"].reshape(-1)
    assert (a[decided] == b[decided]).all(), (what, int((a[decided] != b[decided]).sum()))


# ---- running the rasterizer --------------------------------------------------------------------------------------------------
def _run(rs, g, contrib=None, slots=None, F=None, **kw):
    """raster_harness.run with the accumulators' four fields next to the maps."""
    o = run(rs, g, features=F, contrib=contrib, contrib_slots=slots, **kw)
    if "contrib" in o:
        o.update({k: getattr(o["contrib"], k) for k in FIELDS})
    return o


def _check_shapes(out, P, H, W):
    assert out["top_id"].shape == (H, W) and out["top_id"].dtype == torch.int32
    assert out["top_weight"].shape == (1, H, W) and out["top_weight"].dtype == torch.float32
    assert out["count"].shape == (H, W) and out["count"].dtype == torch.int32
    # the arrays hold exact integers
    assert int(out["pixels"].sum()) == int(out["count"].sum())
    assert int(out["top_pixels"].sum()) == int((out["top_id"] >= 0).sum())
    assert bool(((out["top_id"] >= 0) == (out["count"] > 0)).all())
    assert bool(((out["top_id"] >= -1) & (out["top_id"] < max(P, 1))).all())


def _sum_tol(n):
    """Relative bound on a sum of n non-negative fp32 addends taken in any order."""
    return n * 2.0 ** -24


def _row_addends(cam):
    """Addends of one row of `weight` in one call: the 16 rows of a workgroup meet in LDS, then one flush per tile."""
    return _tiles(cam) + 16


def _tiles(cam):
    return ((cam.image_height + 15) // 16) * ((cam.image_width + 15) // 16)


# ---- the decomposed scenes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DECOMPOSED)
def test_matches_the_fp64_decomposition(oracle64, name):
    cam, g = named_scene(name)
    P, H, W = g["means3D"].shape[0], cam.image_height, cam.image_width
    dec = memo(("contrib", "dec", name), lambda: decompose(oracle64, cam, g))
    ref = memo(("contrib", "stats", name), lambda: stats_of(dec["w"], H, W))
    if name == "long":
        assert int(dec["stats"][0]) / _tiles(cam) > 512        # more than two 256-entry batches in the tile
        assert int(dec["stats"][1]) / _tiles(cam) > 256        # and the walk goes beyond the first
    if name == "saturated":
        assert float(dec["final_T"].min()) < 1e-3              # pixels stop early: later entries must count nothing
    if name == "single":
        assert int(ref["pixels"][0]) > 0
    rs = settings(cam, debug=(name == "single"))
    out = _run(rs, g, contrib=True)
    plain = _run(rs, g)
    assert torch.equal(out["color"], plain["color"]) and torch.equal(out["radii"], plain["radii"])
    assert (out["radii"].cpu().numpy() == dec["radii"]).all()
    assert out["contrib"].views == 1 and len(out["contrib"]) == P
    _check_shapes(out, P, H, W)
    _check_stats(out, ref, name)


# ---- a larger scene, one oracle call -----------------------------------------------------------------------------------------
LARGE = (4000, 256, 256, 4000)


def _large_ref(oracle64):
    cam, g = scene(*LARGE)
    P, H, W = g["means3D"].shape[0], cam.image_height, cam.image_width

    def make():
        d = np.zeros((3, H, W), np.float32)
        d[0] = 1.0
        return oracle64.render(cam.oracle_dict(bg=(0.0, 0.0, 0.0)), g["means3D"], np.ones((P, 3), np.float32), g["opacities"],
                               g["scales"], g["rotations"], dL_dout=d)["dL_dcolors"][:, 0].copy()
    return memo(("contrib", "large",), make)


def test_larger_scene(oracle64):
    cam, g = scene(*LARGE)
    P, H, W = g["means3D"].shape[0], cam.image_height, cam.image_width
    rs = settings(cam)
    out = _run(rs, g, contrib=True, return_aux=True)
    plain = _run(rs, g)
    assert torch.equal(out["color"], plain["color"]) and torch.equal(out["radii"], plain["radii"])
    _check_shapes(out, P, H, W)
    check_grad(out["weight"], _large_ref(oracle64), "weight vs the fp64 oracle's dL_dcolors[:, 0]")
    feat = _run(rs, g, F=np.ones((P, 1), np.float32), loss_w={"features": np.ones((1, H, W), np.float32)})
    check_grad(out["weight"], feat["grad"]["features"].cpu().numpy(), "weight vs the gradient of features = ones")
    total, want = float(out["weight"].double().sum()), float(out["alpha"].double().sum())
    print(f"[contrib] sum of weight {total:.6f} vs sum of the alpha map {want:.6f}")
    assert abs(total - want) <= 1e-4 * want
    assert bool((out["max_weight"] <= out["weight"]).all())
    assert bool(((out["max_weight"] > 0) == (out["pixels"] > 0)).all())
    assert bool((out["top_pixels"] <= out["pixels"]).all())
    assert bool((out["pixels"][out["radii"] <= 0] == 0).all()) and int((out["pixels"] > 0).sum()) > P // 10
    # top_weight is the weight of top_id at that pixel: never above that Gaussian's maximum
    ids = out["top_id"].long().reshape(-1)
    tw = out["top_weight"].reshape(-1)
    cover = ids >= 0
    assert bool((tw[cover] <= out["max_weight"][ids[cover]]).all()) and bool((tw[~cover] == 0).all())


# ---- accumulation ------------------------------------------------------------------------------------------------------------
def test_two_calls_into_one_accumulator():
    from contextgs_amd.rasterizer import GaussianContrib
    cam, g = scene(*LARGE)
    P = g["means3D"].shape[0]
    rs = settings(cam)
    one = _run(rs, g, contrib=True)
    acc = GaussianContrib.zeros(P, "cuda")
    _run(rs, g, contrib=acc)
    two = _run(rs, g, contrib=acc)
    assert two["contrib"] is acc and acc.views == 2
    assert torch.equal(acc.pixels, 2 * one["pixels"]) and torch.equal(acc.top_pixels, 2 * one["top_pixels"])
    assert torch.equal(acc.max_weight, one["max_weight"])
    assert torch.equal(two["top_id"], one["top_id"]) and torch.equal(two["top_weight"], one["top_weight"])
    tol = _sum_tol(3 * _row_addends(cam))          # two calls on one side, one on the other
    assert bool(((acc.weight - 2 * one["weight"]).abs() <= tol * 2 * one["weight"]).all())
    acc.reset()
    assert acc.views == 0 and all(bool((getattr(acc, k) == 0).all()) for k in FIELDS)


def test_maximum_over_two_cameras():
    from contextgs_amd.rasterizer import GaussianContrib
    P, W, H, seed = 2000, 128, 96, 7
    cam_a, g = scene(P, W, H, seed)
    cam_b, _ = scene(P, W, H, seed, eye=(-1.5, -1.8, 0.9))
    a = _run(settings(cam_a), g, contrib=True)
    b = _run(settings(cam_b), g, contrib=True)
    assert not torch.equal(a["pixels"], b["pixels"])
    acc = GaussianContrib.zeros(P, "cuda")
    _run(settings(cam_a), g, contrib=acc)
    _run(settings(cam_b), g, contrib=acc)
    assert torch.equal(acc.max_weight, torch.maximum(a["max_weight"], b["max_weight"]))
    assert torch.equal(acc.pixels, a["pixels"] + b["pixels"]) and torch.equal(acc.top_pixels, a["top_pixels"] + b["top_pixels"])
    want = a["weight"] + b["weight"]
    assert bool(((acc.weight - want).abs() <= _sum_tol(4 * _row_addends(cam_a)) * want).all())


def test_slot_tables():
    from contextgs_amd import rasterizer
    from contextgs_amd.rasterizer import GaussianContrib
    cam, g = scene(*LARGE)
    P = g["means3D"].shape[0]
    rs = settings(cam)
    one = _run(rs, g, contrib=True)
    pairs = int(rasterizer.last_call["num_rendered"])
    row_tol = _sum_tol(2 * _row_addends(cam))       # one call on either side

    # a random permutation permutes the rows; top_id stays a Gaussian index
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(3)).to(torch.int32).cuda()
    acc = GaussianContrib.zeros(P, "cuda")
    out = _run(rs, g, contrib=acc, slots=perm)
    idx = perm.long()
    assert torch.equal(acc.pixels[idx], one["pixels"]) and torch.equal(acc.top_pixels[idx], one["top_pixels"])
    assert torch.equal(acc.max_weight[idx], one["max_weight"])
    assert bool(((acc.weight[idx] - one["weight"]).abs() <= row_tol * one["weight"]).all())
    assert torch.equal(out["top_id"], one["top_id"]) and torch.equal(out["count"], one["count"])

    # all-zeros: every sum lands in row 0 of an accumulator of any length
    acc = GaussianContrib.zeros(3, "cuda")
    _run(rs, g, contrib=acc, slots=torch.zeros(P, dtype=torch.int32, device="cuda"))
    assert int(acc.pixels[0]) == int(one["pixels"].sum()) and int(acc.top_pixels[0]) == int(one["top_pixels"].sum())
    assert float(acc.max_weight[0]) == float(one["max_weight"].max())
    want = float(one["weight"].double().sum())
    # row 0 takes one flush per (tile, Gaussian) pair at the most, in any order; the other side is the rows of `one`
    assert abs(float(acc.weight[0]) - want) <= _sum_tol(pairs + 16 + _row_addends(cam)) * want
    assert all(bool((getattr(acc, k)[1:] == 0).all()) for k in FIELDS)

    # a longer accumulator: rows that no slot names, and rows of Gaussians that contributed nowhere, stay as they were
    acc = GaussianContrib(torch.full((P + 7,), 5.0, device="cuda"), torch.full((P + 7,), 0.5, device="cuda"),
                          torch.full((P + 7,), 11, dtype=torch.int64, device="cuda"),
                          torch.full((P + 7,), 13, dtype=torch.int64, device="cuda"))
    shift = (torch.arange(P, dtype=torch.int32, device="cuda") + 7)
    _run(rs, g, contrib=acc, slots=shift)
    idle = torch.ones(P + 7, dtype=torch.bool, device="cuda")
    idle[7:] = one["pixels"] == 0
    assert int(idle.sum()) > 7          # the scene has Gaussians behind the near plane
    assert bool((acc.weight[idle] == 5.0).all()) and bool((acc.max_weight[idle] == 0.5).all())
    assert bool((acc.pixels[idle] == 11).all()) and bool((acc.top_pixels[idle] == 13).all())
    assert torch.equal(acc.pixels[7:], one["pixels"] + 11) and torch.equal(acc.top_pixels[7:], one["top_pixels"] + 13)
    assert torch.equal(acc.max_weight[7:], torch.clamp(one["max_weight"], min=0.5))


# ---- the four argument forms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["shs+scales", "shs+cov", "colors+cov"])
def test_all_forms_match_colors_precomp_scales_rotations(form):
    from contextgs_amd.rasterizer import GaussianRasterizer
    P, W, H, D, M = 4000, 256, 256, 2, 9
    cam, g = scene(P, W, H, P + 3)
    sh = shs(P, M, seed=P)
    rs = settings(cam, D=D)
    campos = rs.campos.float()

    def run(use_shs, use_cov):
        t = {k: torch.tensor(g[k], device="cuda") for k in ("means3D", "opacities", "scales", "rotations", "colors")}
        t["shs"] = torch.tensor(sh, device="cuda")
        kw = dict(means3D=t["means3D"], means2D=torch.zeros(P, 3, device="cuda"), opacities=t["opacities"], contrib=True)
        if use_shs:
            kw["shs"] = t["shs"]
        else:         # the reference form: torch's SH into colors_precomp when the other side uses shs
            kw["colors_precomp"] = sh_eval_torch(t["shs"], t["means3D"], campos, D) if "shs" in form else t["colors"]
        if use_cov:
            kw["cov3D_precomp"] = cov6_torch(t["scales"], t["rotations"], 1.0)
        else:
            kw["scales"], kw["rotations"] = t["scales"], t["rotations"]
        color, radii, ex = GaussianRasterizer(rs)(**kw)
        torch.cuda.synchronize()
        o = {k: getattr(ex["contrib"], k) for k in FIELDS}
        o.update(radii=radii, top_id=ex["top_id"], top_weight=ex["top_weight"], count=ex["count"])
        return o

    ref = run(False, False)
    new = run("shs" in form, "cov" in form)
    same = (ref["radii"] == new["radii"])
    assert float(same.float().mean()) >= 1 - 1e-4
    _check_shapes(new, P, H, W)
    rows = same.cpu().numpy()
    for k in ("weight", "max_weight"):
        check_grad(np_of(new[k])[rows], np_of(ref[k])[rows], f"{k} {form}")
    check_map(new["top_weight"], np_of(ref["top_weight"]), f"top_weight {form}")
    for k in ("pixels", "top_pixels"):       # the discrete results under the caps of the decomposed scenes
        a, b = np_of(new[k])[rows], np_of(ref[k])[rows]
        assert int(np.abs(a - b).sum()) <= 1e-3 * int(b.sum()), (k, form)
    diff = (new["count"] - ref["count"]).abs()
    assert float((diff == 0).float().mean()) >= 1 - 2e-3 and int(diff.max()) <= 2
    assert float((new["top_id"] == ref["top_id"]).float().mean()) >= 1 - 1e-2


# ---- antialiasing ------------------------------------------------------------------------------------------------------------
def test_antialiasing_reads_the_compensated_opacity():
    P, W, H = 2000, 128, 96
    cam, g = scene(P, W, H, 7)
    aa = _run(settings(cam, aa=True), g, contrib=True, return_aux=True)
    no = _run(settings(cam), g, contrib=True)
    assert not torch.equal(aa["weight"], no["weight"]) and not torch.equal(aa["top_weight"], no["top_weight"])
    _check_shapes(aa, P, H, W)
    total, want = float(aa["weight"].double().sum()), float(aa["alpha"].double().sum())
    print(f"[contrib] antialiasing: sum of weight {total:.6f} vs sum of the alpha map {want:.6f}")
    assert abs(total - want) <= 1e-4 * want


# ---- one walk with and without the per-entry reduction -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged", "long"])
def test_maps_are_the_same_bits_without_the_accumulators(name):
    """top_id / top_weight / count of a call that also asks for the accumulators (the kernel instance with the per-entry
    reduction) against a maps-only call on the same workspaces (the instance without it; only the C entry point can ask for
    that): bit-identical.  Ragged tiles (40x24), and more than two 256-entry batches in a tile."""
    from contextgs_amd import _lib, rasterizer
    cam, g = named_scene(name)
    P, H, W = g["means3D"].shape[0], cam.image_height, cam.image_width
    out = _run(settings(cam), g, contrib=True)
    assert int(out["count"].sum()) > 0 and int(out["pixels"].sum()) == int(out["count"].sum())
    lc = dict(rasterizer.last_call)
    geom, binws, img = lc["geom_ws"], lc["bin_ws"], lc["img_ws"]
    top_id = torch.full((H, W), -7, dtype=torch.int32, device="cuda")
    top_w = torch.full((1, H, W), -7.0, device="cuda")
    count = torch.full((H, W), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().cgs_raster_contrib(lc["cfg"].ref, P, lc["bin_R"], _lib.ptr(geom), geom.numel(), _lib.ptr(binws),
                                             binws.numel(), _lib.ptr(img), img.numel(), None, P, None, None, None, None,
                                             _lib.ptr(top_id), _lib.ptr(top_w), _lib.ptr(count), _lib.current_stream()),
               "cgs_raster_contrib")
    torch.cuda.synchronize()
    assert torch.equal(top_id, out["top_id"])
    assert torch.equal(top_w, out["top_weight"])
    assert torch.equal(count, out["count"])


# ---- empty views -------------------------------------------------------------------------------------------------------------
def test_empty_view_and_no_gaussians():
    from contextgs_amd.rasterizer import GaussianContrib
    cam = look_at_camera((0.0, -3.0, 0.0), (0, 0, 0), 80, 64, fovx_deg=50.0)
    rs = settings(cam)
    g = random_gaussians(64, seed=6)
    g["means3D"][:, 1] -= 20.0                        # everything behind the camera
    for gg in (g, {k: v[:0] for k, v in g.items()}):
        P = gg["means3D"].shape[0]
        for slots in (None, torch.zeros(P, dtype=torch.int32, device="cuda")):
            n = P if slots is None else 3
            acc = GaussianContrib(torch.full((n,), 5.0, device="cuda"), torch.full((n,), 0.5, device="cuda"),
                                  torch.full((n,), 11, dtype=torch.int64, device="cuda"),
                                  torch.full((n,), 13, dtype=torch.int64, device="cuda"))
            out = _run(rs, gg, contrib=acc, slots=slots)
            assert out["top_id"].shape == (64, 80) and bool((out["top_id"] == -1).all())
            assert bool((out["top_weight"] == 0).all()) and bool((out["count"] == 0).all())
            assert bool((acc.weight == 5.0).all()) and bool((acc.max_weight == 0.5).all())
            assert bool((acc.pixels == 11).all()) and bool((acc.top_pixels == 13).all())
            assert acc.views == 1
        out = _run(rs, gg, contrib=True)
        assert len(out["contrib"]) == P and bool((out["top_id"] == -1).all())


# ---- behind a voided speculative render --------------------------------------------------------------------------------------
def test_after_a_voided_speculative_render():
    from contextgs_amd import rasterizer
    P, W, H = 20000, 320, 240
    cam, g = scene(P, W, H, 9)
    rs = settings(cam)
    rasterizer._pair_capacity[(H, W)] = 1 << 10       # far below the view's pair count: the speculative render is voided
    out = _run(rs, g, contrib=True)
    assert rasterizer.last_call["num_rendered"] > (1 << 10)
    assert rasterizer.last_call["bin_R"] == rasterizer.last_call["num_rendered"]     # re-rendered with the true count
    _check_shapes(out, P, H, W)
    assert int(out["pixels"].sum()) > H * W
    again = _run(rs, g, contrib=True)                     # now with a capacity that holds: the speculative render stands
    for k in ("pixels", "top_pixels", "max_weight", "top_id", "top_weight", "count"):
        assert torch.equal(again[k], out[k]), k
    assert bool(((again["weight"] - out["weight"]).abs() <= _sum_tol(2 * _row_addends(cam)) * out["weight"]).all())


# ---- the backward does not see it --------------------------------------------------------------------------------------------
def test_backward_with_contrib():
    """The gradients of a call with `contrib` against those of a call without.  The blend backward sums dL/d(pixel mean), which
    feeds means2D as every other geometry gradient, with float atomics (raster_blend_rows.hip), so no gradient of this node is
    bit-reproducible by construction; bit-equality is asserted for every gradient that two plain calls reproduce bit for bit,
    and all of them stay within `_check_grad`."""
    P, W, H = 3000, 256, 256
    cam, g = scene(P, W, H, 1, 1.0, (0.003, 0.04))
    rs = settings(cam)
    gC = np.random.default_rng(18).normal(size=(3, H, W)).astype(np.float32)
    a = _run(rs, g, contrib=True, loss_w={"color": gC})
    b = _run(rs, g, loss_w={"color": gC})
    b2 = _run(rs, g, loss_w={"color": gC})
    assert torch.equal(a["color"], b["color"])
    assert float(a["grad"]["means2D"].abs().sum()) > 0
    for k in ("means2D", "means3D", "opacities", "scales", "rotations", "colors"):
        # bit-equal wherever the backward is bit-reproducible at all, i.e. where two calls without contrib agree bit for bit
        fixed = torch.equal(b["grad"][k], b2["grad"][k])
        print(f"[contrib] d{k}: two plain calls bit-equal: {fixed}; with contrib bit-equal: {torch.equal(a['grad'][k], b['grad'][k])}")
        if fixed:
            assert torch.equal(a["grad"][k], b["grad"][k]), k
        check_grad(a["grad"][k], b["grad"][k].cpu().numpy(), f"d{k} with contrib vs without")
    # and with the maps and the features in the same call
    F = np.ones((P, 1), np.float32)
    c = _run(rs, g, contrib=True, F=F, return_aux=True, loss_w={"color": gC, "features": np.ones((1, H, W), np.float32)})
    for k in ("top_id", "count", "pixels", "max_weight"):
        assert torch.equal(c[k], a[k]), k
    assert c["features"].shape == (1, H, W) and c["depth"].shape == (1, H, W)
    check_grad(a["weight"], c["grad"]["features"].cpu().numpy(), "weight vs dL/dfeatures of the same call")


def _raw_call(g, **kw):
    """The node's raw outputs (nothing detached) of a call whose inputs all require a gradient."""
    from contextgs_amd.rasterizer import GaussianRasterizer
    cam, _ = scene(2000, 128, 96, 7)
    P = g["means3D"].shape[0]
    t = {k: leaf(v) for k, v in g.items()}
    m2 = torch.zeros(P, 3, device="cuda", requires_grad=True)
    return GaussianRasterizer(settings(cam))(means3D=t["means3D"], means2D=m2, opacities=t["opacities"],
                                              colors_precomp=t["colors"], scales=t["scales"], rotations=t["rotations"], **kw)


@pytest.mark.parametrize("return_aux, with_features", [(False, False), (True, False), (False, True), (True, True)])
def test_outputs_are_marked_non_differentiable(return_aux, with_features):
    _, g = scene(2000, 128, 96, 7)
    P = g["means3D"].shape[0]
    kw = dict(features=leaf(np.ones((P, 2), np.float32))) if with_features else {}
    color, radii, ex = _raw_call(g, contrib=True, return_aux=return_aux, **kw)
    assert color.requires_grad and color.grad_fn is not None
    for k in ("top_id", "top_weight", "count"):
        assert ex[k].requires_grad is False and ex[k].grad_fn is None, k
    assert radii.requires_grad is False and radii.grad_fn is None
    for t in ex["contrib"].tensors():
        assert t.requires_grad is False and t.grad_fn is None
    for k in (("depth", "invdepth", "alpha") if return_aux else ()) + (("features",) if with_features else ()):
        assert ex[k].requires_grad and ex[k].grad_fn is color.grad_fn, k      # the differentiable outputs stay so
    assert ex["top_id"].dtype == torch.int32 and ex["top_weight"].shape == (1, 96, 128) and ex["count"].dtype == torch.int32


def test_the_backward_saves_nothing_new():
    _, g = scene(2000, 128, 96, 7)
    plain = _raw_call(g)
    color, _, ex = _raw_call(g, contrib=True)
    saved_plain, saved = plain[0].grad_fn.saved_tensors, color.grad_fn.saved_tensors
    assert len(saved) == len(saved_plain) == 12
    for a, b in zip(saved, saved_plain):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.shape == b.shape and a.dtype == b.dtype
    kept = {t.data_ptr() for t in saved if t is not None and t.numel()}
    new = [ex["top_id"], ex["top_weight"], ex["count"], *ex["contrib"].tensors()]
    assert all(t.data_ptr() not in kept for t in new)
    assert not any(isinstance(v, type(ex["contrib"])) for v in getattr(color.grad_fn, "__dict__", {}).values())


# ---- render() ----------------------------------------------------------------------------------------------------------------
def _render(pc, cam, pipe, bg, **kw):
    from contextgs_amd import ctx_ops
    from contextgs_amd.renderer import prefilter_voxel, render
    torch.manual_seed(0)
    ctx_ops._seed_counter = itertools.count(1)       # the same noise streams in every call
    vis = prefilter_voxel(cam, pc, pipe, bg)
    return render(cam, pc, pipe, bg, visible_mask=vis, step=1000, **kw), vis


@pytest.mark.parametrize("training", [False, True])
def test_render_accumulates_per_anchor_and_offset(training):
    from contextgs_amd.densify import anchor_importance
    from contextgs_amd.rasterizer import GaussianContrib
    pc, cams, pipe, bg = model()
    pc.train(training)
    N, K = pc.get_anchor.shape[0], pc.n_offsets
    with (torch.enable_grad() if training else torch.no_grad()):
        plain, _ = _render(pc, cams[1], pipe, bg)
        aux, _ = _render(pc, cams[1], pipe, bg, return_aux=True)
        pkg, vis = _render(pc, cams[1], pipe, bg, return_aux=True, contrib=True)
    con = pkg["contrib"]
    for k in ("top_id", "top_weight", "count"):       # the raw outputs, in training mode of a call whose inputs require grad
        assert pkg[k].requires_grad is False and pkg[k].grad_fn is None, k
    assert pkg["render"].requires_grad == training
    assert isinstance(con, GaussianContrib) and len(con) == N * K and con.views == 1
    # the plain call (in training mode: the fused path) gives the same image; the unfused call gives every key bit for bit
    assert torch.equal(pkg["render"].detach(), plain["render"].detach()) and torch.equal(pkg["radii"], plain["radii"])
    for k in plain:
        assert k in pkg, k
    for k, v in aux.items():
        if torch.is_tensor(v):
            assert pkg[k].shape == v.shape and pkg[k].dtype == v.dtype, k
            if k.startswith(("bit_", "bpp_")):      # the rate sums use float atomics
                assert torch.allclose(pkg[k].detach(), v.detach(), rtol=1e-5), k
            else:
                assert torch.equal(pkg[k].detach(), v.detach()), k
    assert pkg["top_id"].shape == (180, 320) and pkg["top_id"].dtype == torch.int32
    assert pkg["top_weight"].shape == (1, 180, 320) and pkg["count"].shape == (180, 320)
    # rows of anchors outside visible_mask, and of offsets the selection mask dropped, are all zero
    touched = torch.zeros(N, K, dtype=torch.bool, device="cuda")
    touched[vis] = True
    if training:
        touched[vis] = pkg["selection_mask"].reshape(-1, K)
    idle = ~touched.reshape(-1)
    assert int(idle.sum()) > 0
    assert all(bool((getattr(con, k)[idle] == 0).all()) for k in FIELDS)
    total, want = float(con.weight.double().sum()), float(pkg["alpha"].double().sum())
    print(f"[render] sum of weight {total:.6f} vs sum of the alpha map {want:.6f}, training={training}")
    assert want > 0 and abs(total - want) <= 1e-4 * want
    ids = pkg["top_id"].long()
    assert int(ids.min()) >= -1 and int(ids.max()) < N * K and int(ids.max()) >= 0
    assert bool((con.pixels[ids[ids >= 0]] > 0).all()) and bool((con.top_pixels[ids[ids >= 0]] > 0).all())
    assert int(con.top_pixels.sum()) == int((ids >= 0).sum()) and int(con.pixels.sum()) == int(pkg["count"].sum())
    assert bool((ids >= 0).eq(pkg["count"] > 0).all())
    # two orbit cameras into one object
    with (torch.enable_grad() if training else torch.no_grad()):
        other, _ = _render(pc, cams[2], pipe, bg, contrib=True)
        acc = GaussianContrib.zeros(N * K, "cuda")
        _render(pc, cams[1], pipe, bg, contrib=acc)
        both, _ = _render(pc, cams[2], pipe, bg, contrib=acc)
    assert both["contrib"] is acc and acc.views == 2
    assert torch.equal(acc.pixels, con.pixels + other["contrib"].pixels)
    assert torch.equal(acc.top_pixels, con.top_pixels + other["contrib"].top_pixels)
    assert torch.equal(acc.max_weight, torch.maximum(con.max_weight, other["contrib"].max_weight))
    imp = anchor_importance(acc, K)
    assert imp.shape == (N,) and torch.equal(imp, acc.max_weight.view(N, K).max(1).values) and float(imp.max()) > 0
    with pytest.raises(ValueError, match="anchors x"):
        _render(pc, cams[1], pipe, bg, contrib=GaussianContrib.zeros(N * K + 1, "cuda"))
