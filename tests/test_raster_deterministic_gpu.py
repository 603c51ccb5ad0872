"""GPU checks of the rasterizer's bit-reproducible backward (`deterministic=True`, cgs_raster_backward_det: the DET instances of
csrc/raster_blend_rows.hip and det_sum_kernel).

Two kinds of assertion.  Equality: gradients of two runs on the same input bits are torch.equal, whatever varied between them
(fresh leaves and workspaces, the binning, a speculative pair capacity, the fused or the unfused node).  Values: the flag's
gradients against the UNCHANGED fp32 oracle and against the default (float-atomic) path, with `check_grad` of
tests/raster_harness.py (at most a 2e-3 share of entries beyond 2e-4 of the tensor's maximum; on the CPU, on all five
scenes, the fp32 oracle against the fp64 oracle leaves no entry of any of the six gradient tensors beyond it, worst 1.3e-5).

Scenes: those of tests/test_raster_absgrad_gpu.py plus `giant` (64 Gaussians of which 47 have a radius beyond the
width of the 416 x 320 image, hundreds of tiles each: the per-Gaussian sum kernel's wave path with several passes), bg = (0.1, 0.25, 0.4), normal loss
weights from default_rng(5).  The oracle's backward of a scene is computed once and shared."""
import itertools

import numpy as np
import pytest
import torch

from contextgs_amd.synth import look_at_camera, random_gaussians
from raster_harness import BG, check_grad, cov6_torch, leaf, loss_weights, memo, model, run, scene, settings, shs, stack_scene

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-4         # tests/test_raster_camera_gpu.py: of the tensor's maximum
GRADS = (("dL_dmeans3D", "means3D"), ("dL_dmeans2D", "means2D"), ("dL_dopacities", "opacities"), ("dL_dscales", "scales"),
         ("dL_drotations", "rotations"), ("dL_dcolors", "colors"))
SCENES = ("s300", "sat", "long", "wide", "giant")


def _giant():
    cam = look_at_camera((0.3, -3.0, 0.5), (0, 0, 0), 416, 320, fovx_deg=55)
    g = random_gaussians(64, seed=64, extent=1.0, scale_lo=0.5, scale_hi=2.0)
    g["opacities"][:] = np.random.default_rng(13).uniform(0.02, 0.1, size=g["opacities"].shape).astype(np.float32)
    return cam, g


def _named(name):
    return {"s300": lambda: scene(300, 40, 24, 7, srange=(0.01, 0.12)),     # 565 pairs, near-plane culls
            "sat": lambda: stack_scene("saturated", 32, 16),                # every pixel stops early, occluded Gaussians
            "long": lambda: stack_scene("long", 24, 16),                    # 700-entry lists, three staged batches
            "wide": lambda: scene(2000, 128, 96, 7),                        # 48 tiles, thousands of pairs
            "giant": _giant}[name]()


def _ref(oracle, name):
    """The fp32 oracle's forward and backward of a scene: computed once, nobody writes into it."""
    def make():
        cam, g = _named(name)
        w = loss_weights(cam.image_height, cam.image_width)
        return oracle.render(cam.oracle_dict(bg=BG), g["means3D"], g["colors"], g["opacities"], g["scales"], g["rotations"],
                             dL_dout=w)
    return memo(("deterministic", name), make)


def _run(rs, g, w, deterministic=True, absgrad=False):
    """Forward + backward of sum(color * w) on fresh leaves (and, the allocator willing, fresh workspaces)."""
    return run(rs, g, loss_w={"color": w}, means2D_cols=4 if absgrad else 3, deterministic=deterministic,
               **(dict(absgrad=True) if absgrad else {}))


def _assert_same_bits(a, b, what):
    for _, k in GRADS:
        assert torch.equal(a["grad"][k], b["grad"][k]), (what, k, float((a["grad"][k] - b["grad"][k]).abs().max()))


def _scene_run(name, **kw):
    cam, g = _named(name)
    return _run(settings(cam), g, loss_weights(cam.image_height, cam.image_width), **kw)


# ---- 1: run-to-run equality ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_three_runs_give_the_same_bits(name):
    runs = []
    for i in range(3):
        runs.append(_scene_run(name))
        junk = torch.full((1 << 22,), float("nan"), device="cuda")       # recycled blocks do not come back as they were left
        del junk
    for i in (1, 2):
        assert torch.equal(runs[0]["color"], runs[i]["color"])
        _assert_same_bits(runs[0], runs[i], f"{name} run 0 vs run {i}")
    assert float(runs[0]["grad"]["means3D"].abs().max()) > 0
    a, b = _scene_run(name, deterministic=False), _scene_run(name, deterministic=False)
    differ = [k for _, k in GRADS if not torch.equal(a["grad"][k], b["grad"][k])]
    print(f"[deterministic] {name}: two DEFAULT-path runs differed in {differ or 'nothing'} (information, not asserted)")


# ---- 2: the oracle and the default path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_matches_the_oracle_and_the_default_path(oracle32, name):
    ref = _ref(oracle32, name)
    det, plain = _scene_run(name), _scene_run(name, deterministic=False)
    assert torch.equal(det["color"], plain["color"]) and torch.equal(det["radii"], plain["radii"])
    assert (det["radii"].cpu().numpy() == ref["radii"]).all()
    for k, tname in GRADS:
        a = det["grad"][tname]
        assert float(np.abs(ref[k]).max()) > 0
        r = ref[k].reshape(ref[k].shape[0], -1)[:, :a.reshape(a.shape[0], -1).shape[1]]
        check_grad(a, r, f"{k} {name} vs oracle32")
        check_grad(a, plain["grad"][tname].cpu().numpy(), f"{k} {name} vs the default path")
    culled = det["radii"] <= 0
    for _, tname in GRADS:
        assert bool((det["grad"][tname][culled] == 0).all()), tname
    if name == "s300":
        assert int(culled.sum()) > 0
    if name == "sat":       # Gaussians behind the saturated stack: in the lists, reached by no pixel, slots nobody writes
        occluded = (~culled) & (torch.as_tensor(np.abs(ref["dL_dcolors"]).max(axis=1) == 0, device="cuda"))
        assert int(occluded.sum()) == 7
        assert bool((det["grad"]["colors"][occluded] == 0).all())
    if name == "giant":
        # 47 radii >= the image width; the oracle's square rectangles make 33 160 pairs, the library's (the tighter boxes of its
        # preprocess) fewer, but far beyond 64 slots per Gaussian on average: the sum kernel's wave path, several passes
        from contextgs_amd import rasterizer as rz
        assert int((det["radii"] >= 416).sum()) == 47 and int(ref["stats"][0]) == 33160
        assert int(rz.last_call["num_rendered"]) > 64 * 64 * 4


# ---- 3: binning and pair-count independence --------------------------------------------------------------------------------------
@pytest.fixture
def restore_bin_mode():
    from contextgs_amd import _lib
    yield
    _lib.check(_lib.lib().cgs_debug_set_bin_mode(0), "cgs_debug_set_bin_mode")


@pytest.mark.parametrize("name", ["wide", "giant"])
def test_binning_and_pair_count_do_not_change_a_bit(name, restore_bin_mode):
    from contextgs_amd import _lib
    from contextgs_amd import rasterizer as rz
    L = _lib.lib()
    cam, _ = _named(name)
    H, W = cam.image_height, cam.image_width
    base = _scene_run(name)
    for mode in (1, 2):
        _lib.check(L.cgs_debug_set_bin_mode(mode), "cgs_debug_set_bin_mode")
        other = _scene_run(name)
        assert torch.equal(base["color"], other["color"])
        _assert_same_bits(base, other, f"{name} default binning vs mode {mode}")
    _lib.check(L.cgs_debug_set_bin_mode(0), "cgs_debug_set_bin_mode")
    if name != "wide":
        return
    saved = rz._pair_capacity.get((H, W))
    try:
        rz._pair_capacity.pop((H, W), None)
        host = _scene_run(name)                         # no capacity known: the pair count is read on the host first
        R = int(rz.last_call["num_rendered"])
        assert R > 1000 and rz.last_call["bin_R"] == R
        rz._pair_capacity[(H, W)] = rz.pair_capacity_for(R)
        spec = _scene_run(name)                         # speculative: workspaces and slot array carved for the capacity
        assert rz.last_call["bin_R"] == rz.pair_capacity_for(R) > R
        _assert_same_bits(host, spec, "host count vs speculative capacity")
        _assert_same_bits(host, base, "host count vs the first run")
    finally:
        rz._pair_capacity.pop((H, W), None)
        if saved is not None:
            rz._pair_capacity[(H, W)] = saved


# ---- 4: forms and options --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form, aa", [pytest.param(f, a, id=f + ("-aa" if a else "")) for a in (False, True)
                                      for f in ("shs+scales", "shs+cov", "colors+cov")])
def test_every_form_with_and_without_antialiasing(form, aa):
    from contextgs_amd.rasterizer import GaussianRasterizer
    P, W, H, D, M = 2000, 128, 96, 2, 9
    cam, g = scene(P, W, H, P + 3)
    sh = shs(P, M, seed=P)
    rs = settings(cam, D=D, aa=aa)
    w = torch.tensor(loss_weights(H, W), device="cuda")

    def run(deterministic):
        t = {k: leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
        t["shs"] = leaf(sh)
        m2 = torch.zeros(P, 3, device="cuda", requires_grad=True)
        kw = dict(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], deterministic=deterministic)
        used = ["means3D", "opacities"]
        if "shs" in form:
            kw["shs"] = t["shs"]
            used.append("shs")
        else:
            kw["colors_precomp"] = t["colors"]
            used.append("colors")
        if "cov" in form:
            cov = cov6_torch(t["scales"], t["rotations"], 1.0).detach().requires_grad_(True)
            kw["cov3D_precomp"] = t["cov"] = cov
            used.append("cov")
        else:
            kw["scales"], kw["rotations"] = t["scales"], t["rotations"]
            used += ["scales", "rotations"]
        color, radii = GaussianRasterizer(rs)(**kw)
        (color * w).sum().backward()
        torch.cuda.synchronize()
        out = {k: t[k].grad for k in used}
        out["means2D"] = m2.grad
        return color.detach(), radii, out

    c1, r1, a = run(True)
    c2, r2, b = run(True)
    c0, r0, ref = run(False)
    assert torch.equal(c1, c2) and torch.equal(c1, c0) and torch.equal(r1, r0)
    for k in a:
        assert torch.equal(a[k], b[k]), (form, aa, k)
        assert float(ref[k].abs().max()) > 0, k
        check_grad(a[k], ref[k].cpu().numpy(), f"{k} {form}{' aa' if aa else ''} vs the default path")


# ---- 5: absgrad ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s300", "sat", "long"])
def test_absgrad_columns(name):
    cam, g = _named(name)
    P = g["means3D"].shape[0]
    a, b = _scene_run(name, absgrad=True), _scene_run(name, absgrad=True)
    ref = _scene_run(name, deterministic=False, absgrad=True)
    m2 = a["grad"]["means2D"]
    assert m2.shape == (P, 4)
    _assert_same_bits(a, b, f"{name} absgrad")
    assert float(ref["grad"]["means2D"][:, 2:4].max()) > 0
    check_grad(m2[:, 2:4], ref["grad"]["means2D"][:, 2:4].cpu().numpy(), f"absolute columns {name} vs the default path")
    check_grad(m2[:, 0:2], ref["grad"]["means2D"][:, 0:2].cpu().numpy(), f"signed columns {name} vs the default path")
    assert bool((m2[:, 2:4] >= 0).all())
    # the other gradients are those of the flag without absgrad, bit for bit (the same sums in the same order)
    plain = _scene_run(name)
    for _, k in GRADS:
        if k != "means2D":
            assert torch.equal(a["grad"][k], plain["grad"][k]), k
    assert torch.equal(m2[:, 0:2], plain["grad"]["means2D"][:, 0:2])


# ---- 6: camera gradients ---------------------------------------------------------------------------------------------------------
def test_camera_gradients():
    from contextgs_amd.rasterizer import GaussianRasterizer
    P, W, H = 2000, 160, 120
    cam, g = scene(P, W, H, 13)
    w = torch.tensor(loss_weights(H, W), device="cuda")
    c = cam.to_torch("cuda")

    def run(deterministic):
        V, PM = c.world_view_transform.clone().requires_grad_(True), c.full_proj_transform.clone().requires_grad_(True)
        rs = settings(cam, view=V, proj=PM)
        t = {k: leaf(g[k]) for k in ("means3D", "opacities", "scales", "rotations", "colors")}
        m2 = torch.zeros(P, 3, device="cuda", requires_grad=True)
        img, _ = GaussianRasterizer(rs)(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], colors_precomp=t["colors"],
                                        scales=t["scales"], rotations=t["rotations"], deterministic=deterministic)
        (img * w).sum().backward()
        torch.cuda.synchronize()
        return V.grad, PM.grad

    (aV, aPM), (bV, bPM), (rV, rPM) = run(True), run(True), run(False)
    assert torch.equal(aV, bV) and torch.equal(aPM, bPM)
    for name, a, r in (("viewmatrix", aV, rV), ("projmatrix", aPM, rPM)):
        rel = float((a - r).abs().max()) / max(float(r.abs().max()), 1e-30)
        print(f"[camera] dL/d{name}: deterministic vs default {rel:.3e} of the tensor maximum")
        assert float(r.abs().max()) > 0 and rel <= GRAD_TOL, (name, rel)


# ---- 7: nothing uninitialised reaches a result -----------------------------------------------------------------------------------
def test_poisoned_workspaces_change_nothing():
    """One direct call of cgs_raster_backward_det on the workspaces the node's forward left, with det_ws, the scratch, dL_dcolors
    and dL_dopacities filled with 0xFF bytes (NaN as floats, 2^32 - 1 as integers) beforehand."""
    from contextgs_amd import _lib
    from contextgs_amd import rasterizer as rz
    L = _lib.lib()
    cam, g = _named("s300")
    H, W = cam.image_height, cam.image_width
    P = g["means3D"].shape[0]
    w = torch.tensor(loss_weights(H, W), device="cuda")
    node = _run(settings(cam), g, w)
    lc = dict(rz.last_call)
    t = node["leaves"]
    R = int(lc["bin_R"])

    def poison(nbytes):
        return torch.full((max(int(nbytes), 256),), 0xFF, dtype=torch.uint8, device="cuda")

    scratch = poison(L.cgs_raster_bwd_abs_scratch_bytes(P))
    det_ws = poison(L.cgs_raster_bwd_det_bytes(P, R, 3))
    out = {k: poison(4 * P * n).view(torch.float32)[:P * n].view(P, n)
           for k, n in (("means3D", 3), ("means2D", 3), ("colors", 3), ("opacities", 1), ("scales", 3), ("rotations", 4))}
    p = _lib.ptr
    geom, binws, img = lc["geom_ws"], lc["bin_ws"], lc["img_ws"]
    rc = L.cgs_raster_backward_det(
        lc["cfg"].ref, P, R, p(t["means3D"].detach()), p(t["colors"].detach()), None, 0, 0, p(t["opacities"].detach()),
        p(t["scales"].detach()), p(t["rotations"].detach()), None, p(node["radii"]), p(geom), geom.numel(), p(binws), binws.numel(),
        p(img), img.numel(), p(w), None, None, None, p(out["means3D"]), p(out["means2D"]), p(out["colors"]), p(out["opacities"]),
        None, p(out["scales"]), p(out["rotations"]), None, p(scratch), scratch.numel(), _lib.current_stream(), 0, 3, p(det_ws),
        det_ws.numel())
    _lib.check(rc, "cgs_raster_backward_det")
    torch.cuda.synchronize()
    for k, v in out.items():
        assert not bool(torch.isnan(v).any()), k
        assert torch.equal(v, node["grad"][k].reshape(v.shape)), k


# ---- 8: render() and the fused training node -------------------------------------------------------------------------------------
def _train_view(pc, cam, pipe, bg, fuse, **kw):
    from contextgs_amd import ctx_ops, renderer
    from contextgs_amd.renderer import prefilter_voxel, render
    torch.manual_seed(0)
    ctx_ops._seed_counter = itertools.count(1)       # the same noise streams in every call
    seen = []
    prev, renderer.FUSE_VIEW = renderer.FUSE_VIEW, fuse
    orig = renderer._ExpandRasterize.apply
    renderer._ExpandRasterize.apply = staticmethod(lambda *a: (seen.append(1), orig(*a))[1])
    for q in pc.parameters():
        q.grad = None
    try:
        vis = prefilter_voxel(cam, pc, pipe, bg)
        pkg = render(cam, pc, pipe, bg, visible_mask=vis, retain_grad=True, step=1000, **kw)
        w = torch.randn(pkg["render"].shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
        (pkg["render"] * w).sum().backward()
        torch.cuda.synchronize()
    finally:
        renderer.FUSE_VIEW = prev
        renderer._ExpandRasterize.apply = orig
    assert bool(seen) == fuse           # the flag does not push a training view off the fused node
    pkg["param_grads"] = {n: q.grad.detach().clone() for n, q in pc.named_parameters() if q.grad is not None}
    return pkg


def test_render_and_the_fused_node():
    pc, cams, pipe, bg = model()
    pc.train()
    a = _train_view(pc, cams[1], pipe, bg, True, deterministic=True)
    b = _train_view(pc, cams[1], pipe, bg, True, deterministic=True)
    u = _train_view(pc, cams[1], pipe, bg, False, deterministic=True)
    plain = _train_view(pc, cams[1], pipe, bg, True)
    ga, gb, gu, gp = (p["viewspace_points"].grad for p in (a, b, u, plain))
    assert ga.shape == gp.shape and float(ga.abs().max()) > 0
    assert torch.equal(a["render"], b["render"]) and torch.equal(a["render"], u["render"]) and torch.equal(a["render"], plain["render"])
    assert torch.equal(ga, gb)
    assert torch.equal(ga, gu)          # same records and same lists in, same bits out
    check_grad(ga, gp.cpu().numpy(), "viewspace_points.grad, with vs without the flag")
    same = sorted(n for n in a["param_grads"] if n in b["param_grads"] and torch.equal(a["param_grads"][n], b["param_grads"][n]))
    other = sorted(set(a["param_grads"]) - set(same))
    print(f"[deterministic] fused training view, parameter gradients bit-equal between two calls: {same}; not: {other} "
          "(information, not asserted: other launches of the step still sum with float atomics)")


# ---- 9: refusals and empties -----------------------------------------------------------------------------------------------------
def test_refusals():
    from contextgs_amd import _lib
    from contextgs_amd import rasterizer as rz
    from contextgs_amd.rasterizer import GaussianRasterizer
    L = _lib.lib()
    cam, g = _named("s300")
    H, W = cam.image_height, cam.image_width
    P = g["means3D"].shape[0]
    rs = settings(cam)
    t = {k: torch.tensor(v, device="cuda") for k, v in g.items()}
    args = dict(means3D=t["means3D"], means2D=torch.zeros(P, 3, device="cuda"), opacities=t["opacities"], colors_precomp=t["colors"],
                scales=t["scales"], rotations=t["rotations"], deterministic=True)
    for kw, name in ((dict(return_aux=True), "return_aux"), (dict(features=torch.zeros(P, 2, device="cuda")), "features"),
                     (dict(contrib=True), "contrib")):
        with pytest.raises(ValueError, match=name):
            GaussianRasterizer(rs)(**args, **kw)
    # the C level, on a real view's workspaces
    w = torch.tensor(loss_weights(H, W), device="cuda")
    node = _run(rs, g, w)
    lc = dict(rz.last_call)
    R = int(lc["bin_R"])
    p = _lib.ptr
    geom, binws, img = lc["geom_ws"], lc["bin_ws"], lc["img_ws"]
    scratch = torch.empty(L.cgs_raster_bwd_abs_scratch_bytes(P), dtype=torch.uint8, device="cuda")
    det_ws = torch.empty(L.cgs_raster_bwd_det_bytes(P, R, 3), dtype=torch.uint8, device="cuda")
    out = {k: torch.empty(P, n, device="cuda") for k, n in (("means3D", 3), ("means2D", 3), ("colors", 3), ("opacities", 1),
                                                            ("scales", 3), ("rotations", 4))}

    def call(d_depth=None, det_bytes=det_ws.numel()):
        rc = L.cgs_raster_backward_det(
            lc["cfg"].ref, P, R, p(t["means3D"]), p(t["colors"]), None, 0, 0, p(t["opacities"]), p(t["scales"]), p(t["rotations"]),
            None, p(node["radii"]), p(geom), geom.numel(), p(binws), binws.numel(), p(img), img.numel(), p(w), d_depth, None, None,
            p(out["means3D"]), p(out["means2D"]), p(out["colors"]), p(out["opacities"]), None, p(out["scales"]), p(out["rotations"]),
            None, p(scratch), scratch.numel(), _lib.current_stream(), 0, 3, p(det_ws), det_bytes)
        return rc, L.cgs_last_error().decode()

    rc, msg = call(d_depth=p(torch.zeros(1, H, W, device="cuda")))
    assert rc == 1 and "must be NULL" in msg, msg                        # CGS_ERR_ARG
    rc, msg = call(det_bytes=L.cgs_raster_bwd_det_bytes(P, R, 3) - 1)         # one byte short
    assert rc == 3 and "det_ws too small" in msg, msg                    # CGS_ERR_WORKSPACE
    rc, msg = call()
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert torch.equal(out["means3D"], node["grad"]["means3D"])


def test_empty_inputs_give_zero_gradients():
    cam = look_at_camera((0.0, -3.0, 0.0), (0, 0, 0), 80, 64, fovx_deg=50.0)
    rs = settings(cam)
    g = random_gaussians(64, seed=6)
    g["means3D"][:, 1] -= 20.0                        # everything behind the camera
    for gg in (g, {k: v[:0] for k, v in g.items()}):
        P = gg["means3D"].shape[0]
        for absgrad in (False, True):
            out = _run(rs, gg, torch.ones(3, 64, 80, device="cuda"), absgrad=absgrad)
            assert int((out["radii"] > 0).sum()) == 0
            assert out["grad"]["means2D"].shape == (P, 4 if absgrad else 3)
            for _, k in GRADS:
                if k != "means2D":
                    assert out["grad"][k].shape == out["leaves"][k].shape, k
                assert bool((out["grad"][k] == 0).all()), k
