"""End-to-end sanity of the drop-in path as a TRAINING step consumer would use it (train.py:158-256):
prefilter_voxel -> render -> loss -> backward -> Adam, for both training phases.  The loss must go
down, the render dict must carry what train.py / training_statis read, and BASELINE-size inputs
(c4/c5-scale anchor counts) must run."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _setup(N=20000, W=320, H=180, seed=0):
    from contextgs_amd.synth import SynthPipe, make_scene, orbit_cameras
    pc = make_scene(N, seed=seed)
    pc.train()
    cams = [c.to_torch("cuda") for c in orbit_cameras(4, W, H)]
    return pc, cams, SynthPipe(), torch.zeros(3, device="cuda")


@pytest.mark.parametrize("step", [1000, 5000, 20000])
def test_render_dict_and_gradients_reach_every_parameter(step):
    from contextgs_amd.renderer import prefilter_voxel, render
    pc, cams, pipe, bg = _setup()
    vis = prefilter_voxel(cams[0], pc, pipe, bg)
    assert vis.dtype == torch.bool and vis.shape[0] == pc._anchor.shape[0] and 0 < int(vis.sum())
    pkg = render(cams[0], pc, pipe, bg, visible_mask=vis, retain_grad=True, step=step)
    for k in ("render", "viewspace_points", "visibility_filter", "radii", "selection_mask", "neural_opacity", "scaling",
              "bit_per_param", "bit_per_anchor_param", "bit_per_feat_param", "bit_per_scaling_param",
              "bit_per_offsets_param", "bpp_per_level"):
        assert k in pkg, k                                   # gaussian_renderer/__init__.py:209-222
    assert pkg["render"].shape == (3, 180, 320)
    P = pkg["radii"].shape[0]
    assert pkg["viewspace_points"].shape == (P, 3) and pkg["scaling"].shape == (P, 3)
    assert pkg["selection_mask"].shape[0] == int(vis.sum()) * pc.n_offsets and int(pkg["selection_mask"].sum()) == P
    loss = (1.0 - pkg["render"]).abs().mean() + 0.01 * pkg["scaling"].prod(dim=1).mean()      # train.py:199-204
    if step > 10000:
        assert pkg["bit_per_anchor_param"] == 16 and len(pkg["bpp_per_level"]) == 2 + pc.level_num
        loss = loss + 0.001 * pkg["bit_per_param"] + 5e-4 * torch.mean(torch.sigmoid(pc._mask))  # :206-209
    else:
        assert pkg["bit_per_param"] is None
    loss.backward()
    g = pkg["viewspace_points"].grad                        # consumed by training_statis (scene/gaussian_model.py:710)
    assert g is not None and g.shape == (P, 3) and float(g[:, :2].abs().sum()) > 0 and float(g[:, 2].abs().sum()) == 0
    expect = ["_anchor", "_offset", "_mask", "_anchor_feat", "_scaling"] + (["_hyper_latent"] if step > 10000 else [])
    for name in expect:
        gr = getattr(pc, name).grad
        assert gr is not None and torch.isfinite(gr).all() and float(gr.abs().sum()) > 0, name
    mlps = [pc.mlp_opacity, pc.mlp_cov, pc.mlp_color] + ([pc.mlp_grid, pc.latent_codec] if step > 10000 else [])
    for m in mlps:
        for n_, p in m.named_parameters():
            if n_ == "quantiles":
                continue
            assert p.grad is not None and torch.isfinite(p.grad).all(), n_


def test_loss_decreases_under_adam():
    from contextgs_amd.renderer import prefilter_voxel, render
    pc, cams, pipe, bg = _setup(N=15000, W=256, H=144, seed=3)
    with torch.no_grad():                       # target: the same scene 40 % darker (reachable: colours / opacities down)
        pc.eval()
        pc.decoded_version = False
        targets = []
        for c in cams:
            vis = prefilter_voxel(c, pc, pipe, bg)
            pc.train()
            targets.append(render(c, pc, pipe, bg, visible_mask=vis, step=1000)["render"] * 0.6)
    pc.train()
    opt = torch.optim.Adam([{"params": [pc._anchor_feat, pc._offset, pc._scaling], "lr": 5e-3},
                            {"params": list(pc.mlp_color.parameters()) + list(pc.mlp_opacity.parameters()) +
                             list(pc.mlp_cov.parameters()), "lr": 2e-3}])
    losses = []
    for it in range(40):
        c, tgt = cams[it % 4], targets[it % 4]
        vis = prefilter_voxel(c, pc, pipe, bg)
        pkg = render(c, pc, pipe, bg, visible_mask=vis, step=1000)
        loss = (pkg["render"] - tgt).abs().mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert sum(losses[-8:]) / 8 < 0.7 * sum(losses[:8]) / 8, (losses[:8], losses[-8:])


@pytest.mark.parametrize("N", [1_500_000, 3_000_000])
def test_baseline_scale_anchor_counts_run(N):
    """c4 / c5 anchor counts (BASELINE.json configs) at 1920x1080: one full training-phase step each."""
    from contextgs_amd.renderer import prefilter_voxel, render
    from contextgs_amd.synth import SynthPipe, make_scene, orbit_cameras
    pc = make_scene(N, seed=1)
    pc.train()
    cam = orbit_cameras(8, 1920, 1080)[2].to_torch("cuda")
    bg = torch.zeros(3, device="cuda")
    vis = prefilter_voxel(cam, pc, SynthPipe(), bg)
    pkg = render(cam, pc, SynthPipe(), bg, visible_mask=vis, step=20000)
    (pkg["render"].mean() + 0.001 * pkg["bit_per_param"]).backward()
    torch.cuda.synchronize()
    assert torch.isfinite(pkg["render"]).all() and 0.0 <= float(pkg["render"].min()) and float(pkg["render"].max()) <= 1.0 + 1e-4
    assert torch.isfinite(pc._anchor_feat.grad).all() and float(pc._anchor_feat.grad.abs().sum()) > 0
    assert math.isfinite(float(pkg["bit_per_param"])) and 0 < float(pkg["bit_per_param"]) < 32
    del pc, pkg
    torch.cuda.empty_cache()


@pytest.mark.parametrize("loss_kind", ["render+rate", "rate_only", "render_only"])
def test_row_source_and_rate_side_equal_the_autograd_formulation(monkeypatch, loss_kind):
    """The two backward short-cuts of the fused level loop — parameter rows read / gradients scattered through the
    coding-order permutation inside the level kernels (ctx_ops.RowSource) and the rate gradients handed to the
    noise_quant backward in compact form (ctx_ops.RateSide) — against the plain autograd formulation they replace
    (gather -> split -> ... -> cat -> index_copy, N-row rate gradients + adds), same seeds: the same sums in another
    order, so gradients agree to rounding, also when one of the two loss branches is absent."""
    from contextgs_amd import context_model as cm
    from contextgs_amd import ctx_ops
    from contextgs_amd.renderer import prefilter_voxel, render
    pc, cams, pipe, bg = _setup(N=30000)
    vis = prefilter_voxel(cams[2], pc, pipe, bg)
    params = [p for p in pc.parameters() if p.requires_grad]
    names = [n for n, p in pc.named_parameters() if p.requires_grad]

    def run(short_cuts):
        for p in params:
            p.grad = None
        torch.manual_seed(9)
        it = iter(range(100, 200))
        monkeypatch.setattr(ctx_ops, "next_seed", lambda: next(it))
        monkeypatch.setattr(cm, "ROW_SOURCE", short_cuts)
        monkeypatch.setattr(cm, "RATE_SIDE", short_cuts)
        # both runs on the separate level launches: the fused level kernels (csrc/ctx_level.hip, the default) only exist on the
        # RowSource path and form the step sizes in another summation order — their comparison with these launches, with and
        # without the rate side, is tests/test_ctx_level_gpu.py
        monkeypatch.setattr(cm, "LEVEL_FUSED", False)
        pkg = render(cams[2], pc, pipe, bg, visible_mask=vis, step=20000)
        loss = 0.0
        if loss_kind != "rate_only":
            loss = loss + (1.0 - pkg["render"]).abs().mean()
        if loss_kind != "render_only":
            loss = loss + 0.05 * pkg["bit_per_param"]
        loss.backward()
        return pkg["render"].detach().clone(), [None if p.grad is None else p.grad.clone() for p in params]

    img_a, g_a = run(True)
    img_b, g_b = run(False)
    assert torch.equal(img_a, img_b)
    for n, a, b in zip(names, g_a, g_b):
        assert (a is None) == (b is None), n
        if a is not None:
            scale = float(b.abs().max()) + 1e-20
            assert float((a - b).abs().max()) <= 1e-5 * scale, (n, float((a - b).abs().max()) / scale)


def test_bench_scene_full_size_properties(tmp_path):
    """The bench workload itself (1 M anchors, 1920x1080) through properties that need no oracle:
    * the deterministic phase (step <= 3000) renders bit-identically twice and its backward is LINEAR in dL/dimage
      (grad(w1) + grad(w2) == grad(w1 + w2) for every per-anchor parameter, relative 1e-4 of the largest entry);
    * the training phase (step > 10000) gives every per-anchor parameter a finite, non-zero gradient through the
      RowSource / RateSide backward, and the three rate terms are positive;
    * conduct_encoding -> conduct_decoding at this size round-trips anchors and masks bit-exactly and fills every
      decoded tensor (value-level equality of the decoded attributes is pinned at 3 k / 12 k anchors in
      tests/test_codec_gpu.py::test_container_encode_decode_roundtrip)."""
    from contextgs_amd.renderer import prefilter_voxel, render
    from contextgs_amd.synth import SynthPipe, make_scene, orbit_cameras
    pc = make_scene(1_000_000, seed=0)
    pc.train()
    pipe, bg = SynthPipe(), torch.zeros(3, device="cuda")
    cam = orbit_cameras(8, 1920, 1080)[0].to_torch("cuda")
    names = ("_anchor_feat", "_offset", "_scaling")
    g = torch.Generator(device="cuda").manual_seed(5)
    w1, w2 = (torch.randn(3, 1080, 1920, device="cuda", generator=g) for _ in range(2))

    def grads(w, step):
        for p in pc.parameters():
            p.grad = None
        vis = prefilter_voxel(cam, pc, pipe, bg)
        pkg = render(cam, pc, pipe, bg, visible_mask=vis, step=step)
        loss = (pkg["render"] * w).sum()
        if pkg["bit_per_param"] is not None:
            loss = loss + 1000.0 * pkg["bit_per_param"]
        loss.backward()
        return pkg, {n: getattr(pc, n).grad.clone() for n in names}

    pa, ga = grads(w1, 1000)
    pb, gb = grads(w2, 1000)
    pab, gab = grads(w1 + w2, 1000)
    assert torch.equal(pa["render"], pb["render"]) and torch.equal(pa["render"], pab["render"])
    for n in names:
        scale = float(gab[n].abs().max())
        assert scale > 0 and float((ga[n] + gb[n] - gab[n]).abs().max()) <= 1e-4 * scale, n
    pkg, gt = grads(w1, 20000)
    for k in ("bit_per_feat_param", "bit_per_scaling_param", "bit_per_offsets_param"):
        assert 0 < float(pkg[k].detach()) < 64
    for n in names + ("_hyper_latent", "_mask"):
        gr = getattr(pc, n).grad
        assert gr is not None and torch.isfinite(gr).all() and float(gr.abs().sum()) > 0, n
    del pa, pb, pab, ga, gb, gab, pkg, gt

    pc.eval()
    d = str(tmp_path / "bits")
    pc.conduct_encoding(d)
    dec = make_scene(1_000_000, seed=0, requires_grad=False)
    dec.eval()
    dec.conduct_decoding(d)
    m = pc.get_mask_anchor
    nv = int(m.sum())
    assert torch.equal(dec._anchor[:nv], pc.get_anchor[m]) and torch.equal(dec._mask[:nv], pc.get_mask[m])
    sizes = {f: (tmp_path / "bits" / f).stat().st_size for f in ("feat0.b", "scaling0.b", "offsets0.b", "masks.b")}
    assert all(v > 0 for v in sizes.values())
    assert dec._anchor_feat.shape == (1_000_000, 50) and torch.isfinite(dec._anchor_feat).all()


def test_mid_phase_noise_is_one_launch_with_the_reference_distribution(monkeypatch):
    """3000 < step <= 10000 (gaussian_renderer/__init__.py:54-58): feat / scaling / offsets of the visible anchors get
    U(-1/2, 1/2) * (1, 0.001, 0.2) added — by one fused launch; the values that reach the anchor MLPs / the expansion
    differ from the parameters by exactly such noise, and the gradients pass through unchanged."""
    from contextgs_amd import ctx_ops, renderer
    pc, cams, pipe, bg = _setup(N=30000)
    seen = {}
    real = ctx_ops.noise_quant

    def spy(xf, xs, xo, qadj, q0, **kw):
        out = real(xf, xs, xo, qadj, q0, **kw)
        seen.update(x=(xf.detach().clone(), xs.detach().clone(), xo.detach().clone()), y=tuple(t.detach().clone() for t in out[:3]),
                    q0=q0, calls=seen.get("calls", 0) + 1)
        return out

    monkeypatch.setattr(ctx_ops, "noise_quant", spy)
    vis = renderer.prefilter_voxel(cams[0], pc, pipe, bg)
    pkg = renderer.render(cams[0], pc, pipe, bg, visible_mask=vis, retain_grad=True, step=5000)
    assert seen["calls"] == 1 and tuple(seen["q0"]) == (1, 0.001, 0.2)
    for x, y, q in zip(seen["x"], seen["y"], seen["q0"]):
        u = (y - x) / q
        # x + u q in fp32: the quotient carries the rounding of the sum (|x| up to ~10 against q down to 1e-3)
        assert float(u.abs().max()) <= 0.5 + 1e-2 and abs(float(u.mean())) < 5e-3
        assert abs(float(u.var()) - 1.0 / 12.0) < 5e-3
    pkg["render"].sum().backward()
    for name in ("_anchor_feat", "_scaling", "_offset"):
        g = getattr(pc, name).grad
        assert g is not None and torch.isfinite(g).all() and float(g.abs().sum()) > 0, name


def test_miniature_training_run_with_densification_encodes_and_decodes():
    """tools/train_loop.py: the reference's train.py loop in miniature on contextgs_amd.model.GaussianModel alone —
    training_setup, learning-rate schedule, three phases, training_statis, adjust_anchor (grow + prune + optimizer
    surgery) several times, then conduct_encoding / conduct_decoding of the trained model."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "train_loop.py"), "180", "30000"], capture_output=True,
                       text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "finite True" in r.stdout and r.stdout.count("adjust_anchor") >= 3
    losses = [float(l.split("loss")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("it ")]
    assert losses[-1] < 0.7 * losses[0], losses
    dec = [l for l in r.stdout.splitlines() if l.startswith("decoded anchors")][0].split()
    assert dec[2] == dec[4], dec


@pytest.mark.parametrize("n,p", [(1, 1.0), (1000, 0.0), (4097, 0.5), (1_000_003, 0.995)])
def test_visible_list_equals_torch_nonzero(n, p):
    from contextgs_amd.renderer import VisibleList
    g = torch.Generator(device="cuda").manual_seed(n)
    mask = torch.rand(n, device="cuda", generator=g) < p
    pending = VisibleList(mask)
    filler = torch.ones(1000, device="cuda").cumsum(0)          # work enqueued between the two halves
    got = pending.wait()
    assert got.dtype == torch.int64 and torch.equal(got, torch.nonzero(mask)[:, 0]) and float(filler[-1]) == 1000.0


@pytest.mark.parametrize("step", [5000, 20000])
def test_training_steps_do_not_accumulate_device_memory(step):
    """Live device memory after step k is what it was after step 2, for both training phases: no autograd node keeps one of
    its own outputs (a cycle through the C++ node that Python's collector cannot break).  Round 5's fused level node did —
    ~350 MB per step at 1 M anchors, every level node and RowSource of every step — until the device was full and each step
    paid an allocator retry (tools/leak_probe.py)."""
    import gc
    from contextgs_amd.renderer import prefilter_voxel, render
    pc, cams, pipe, bg = _setup(N=60000)
    params = [p for p in pc.parameters() if p.requires_grad]
    live = []
    for i in range(7):
        for p in params:
            p.grad = None
        cam = cams[i % len(cams)]
        pkg = render(cam, pc, pipe, bg, visible_mask=prefilter_voxel(cam, pc, pipe, bg), step=step)
        loss = pkg["render"].mean() + (0.001 * pkg["bit_per_param"] if pkg["bit_per_param"] is not None else 0.0)
        loss.backward()
        del pkg, loss
        torch.cuda.synchronize()
        live.append(torch.cuda.memory_allocated())
    gc.collect()
    ctxs = [type(o).__name__ for o in gc.get_objects() if type(o).__name__ in ("_LevelFusedBackward", "_RowSourceFnBackward", "_NoiseQuantBackward")]
    print(f"[leak] live bytes after steps 2..6: {live[2:]}, context nodes alive: {len(ctxs)}")
    assert max(live[3:]) - live[2] <= 8 << 20, live          # (views differ by a few thousand Gaussians: a few MB either way)
    assert len(ctxs) <= 4, ctxs                              # at most the last step's nodes (3 levels + the token node), not 7 steps' worth


def _ctx_step(pc, cam, pipe, bg):
    from contextgs_amd.renderer import prefilter_voxel, render
    for p in pc.parameters():
        p.grad = None
    vis = prefilter_voxel(cam, pc, pipe, bg)
    pkg = render(cam, pc, pipe, bg, visible_mask=vis, step=20000)
    loss = (1.0 - pkg["render"]).abs().mean() + 0.001 * pkg["bit_per_param"]
    loss.backward()
    return pkg, float(loss)


def test_early_launches_fall_back_when_the_plan_turns_out_stale():
    """The level kernels / anchor MLPs are enqueued ahead of the read-back that validates the cached level plan
    (context_model._early_levels).  Moving anchors between two steps makes the plan stale AFTER they were enqueued: the step must
    rebuild the plan and run the plain way (context_model._EarlyMismatch), with finite results and gradients everywhere."""
    from contextgs_amd import context_model as cm
    if not cm.EARLY_LEVELS:
        pytest.skip("CGS_EARLY_LEVELS=0: nothing is enqueued early")
    pc, cams, pipe, bg = _setup(N=12000, W=256, H=144, seed=7)
    _ctx_step(pc, cams[0], pipe, bg)                     # builds the plan
    _ctx_step(pc, cams[1], pipe, bg)                     # a step on the cached plan: the early path
    cache = pc._level_cache
    seen = {"n": 0}
    orig = cm._early_levels

    def counting(*a, **k):
        r = orig(*a, **k)
        seen["n"] += r is not None
        return r
    cm._early_levels = counting
    try:
        with torch.no_grad():
            pc._anchor.add_(3.0 * float(pc.voxel_size) * torch.randn_like(pc._anchor))      # other voxels, other levels
        pkg, loss = _ctx_step(pc, cams[2], pipe, bg)
    finally:
        cm._early_levels = orig
    assert seen["n"] >= 1, "the early path was not taken: the test does not exercise the fallback"
    assert pc._level_cache is not cache, "the plan was not rebuilt"
    assert math.isfinite(loss) and torch.isfinite(pkg["render"]).all()
    for name in ("_anchor", "_offset", "_mask", "_anchor_feat", "_scaling", "_hyper_latent"):
        g = getattr(pc, name).grad
        assert g is not None and torch.isfinite(g).all() and float(g.abs().sum()) > 0, name
    _ctx_step(pc, cams[3], pipe, bg)                     # and the next step is an early one again, on the new plan


def test_early_launches_change_nothing_but_the_order():
    """Same seeds, same scene: a training step with the early launches and one without give the same image, rate and gradients
    (the kernels and their operands are the same, only their place in the queue differs)."""
    from contextgs_amd import context_model as cm, ctx_ops, renderer as rd
    outs = []
    for early in (True, False):
        pc, cams, pipe, bg = _setup(N=12000, W=256, H=144, seed=9)
        old = (cm.EARLY_LEVELS, rd.EARLY_MLP3)
        cm.EARLY_LEVELS, rd.EARLY_MLP3 = early, early
        try:
            _ctx_step(pc, cams[0], pipe, bg)             # builds the plan (never early)
            import itertools
            ctx_ops._seed_counter = itertools.count(1000)        # the same stream ids for both runs
            pkg, loss = _ctx_step(pc, cams[1], pipe, bg)
        finally:
            cm.EARLY_LEVELS, rd.EARLY_MLP3 = old
        outs.append((pkg["render"].detach().clone(), float(pkg["bit_per_param"]), pc._anchor_feat.grad.clone(), pc._mask.grad.clone(),
                     [p.grad.clone() for p in pc.mlp_grid.parameters()]))
    a, b = outs
    assert torch.equal(a[0], b[0]) and a[1] == b[1]                  # forward: bit for bit
    # (gradients: the blend backward's flush adds with float atomics, whose order differs from run to run of the SAME schedule too)
    close = lambda x, y: float((x - y).abs().max()) <= 2e-5 * float(x.abs().max()) + 1e-12
    assert close(a[2], b[2]) and close(a[3], b[3])
    for x, y in zip(a[4], b[4]):
        assert close(x, y)


@pytest.mark.parametrize("knob_off", [None, "ROW_SOURCE", "LEVEL_FUSED", "RATE_FUSED", "RATE_SIDE", "FUSED_TRAINING", "EARLY_LEVELS"])
def test_early_launch_and_level_loop_agree_on_the_route(monkeypatch, knob_off):
    """The early launch (context_model._early_levels) and the level loop answer "is this the all-fused step?" from the same
    predicates: on a cached plan they can only disagree over data.  Second step of a scene, launches counted:
    * all knobs at their defaults: one early launch per non-empty level and no other launch of the level kernel — nothing is
      launched twice — and the context model runs once;
    * any one knob off: nothing is enqueued early and the context model still runs once (no _EarlyMismatch rerun), with finite,
      non-zero results and gradients."""
    from contextgs_amd import context_model as cm, ctx_ops
    for knob in ("ROW_SOURCE", "LEVEL_FUSED", "RATE_FUSED", "RATE_SIDE", "FUSED_TRAINING", "EARLY_LEVELS"):
        monkeypatch.setattr(cm, knob, knob != knob_off)
    pc, cams, pipe, bg = _setup(N=12000, W=256, H=144, seed=7)
    _ctx_step(pc, cams[0], pipe, bg)                     # builds the plan
    seen = {"early": 0, "launch": 0, "mismatch": 0}
    real_early, real_launch = ctx_ops.level_fused_launch, ctx_ops._LevelFused.launch

    def early(*a, **k):
        seen["early"] += 1
        return real_early(*a, **k)

    def launch(*a, **k):
        seen["launch"] += 1
        return real_launch(*a, **k)

    def mismatch(self, *a):
        seen["mismatch"] += 1
        Exception.__init__(self, *a)
    ctx_ops.level_fused_launch, ctx_ops._LevelFused.launch, cm._EarlyMismatch.__init__ = early, staticmethod(launch), mismatch
    try:
        pkg, loss = _ctx_step(pc, cams[1], pipe, bg)     # a step on the cached plan
    finally:
        ctx_ops.level_fused_launch, ctx_ops._LevelFused.launch = real_early, staticmethod(real_launch)
        del cm._EarlyMismatch.__init__
    levels = sum(1 for s in pc._level_cache["sizes"] if s > 0)
    print(f"[route] {knob_off}: levels {levels}, early launches {seen['early']}, level-kernel launches {seen['launch']}, "
          f"reruns {seen['mismatch']}")
    assert levels >= 2 and seen["mismatch"] == 0
    if knob_off is None:
        assert seen["early"] == levels and seen["launch"] == levels
    else:
        assert seen["early"] == 0
    assert math.isfinite(loss) and torch.isfinite(pkg["render"]).all() and float(pkg["bit_per_param"]) > 0
    for name in ("_anchor", "_offset", "_mask", "_anchor_feat", "_scaling", "_hyper_latent"):
        g = getattr(pc, name).grad
        assert g is not None and torch.isfinite(g).all() and float(g.abs().sum()) > 0, name


def test_hyper_latent_gradient_rows_written_by_the_levels_equal_the_gathered_blocks():
    """The fused levels' backward writes the hyper latents' gradient rows straight into one buffer in parameter order
    (ctx_ops.HyperDirect, cgs_ctx_level_bwd2) instead of handing one strided block per level to the hyper prior's backward, which
    gathered them through the inverse coding permutation: the same values by another route (compared up to the run-to-run noise of
    the blend backward's float atomics, which reaches the level kernels through dy), and the direct route must actually be taken;
    the kernel-level statement is bit-exact: tests/test_ctx_level_gpu.py."""
    import itertools
    from contextgs_amd import ctx_ops
    outs, taken = [], []
    for direct in (True, False):
        pc, cams, pipe, bg = _setup(N=12000, W=256, H=144, seed=11)
        old = ctx_ops.HYPER_DIRECT
        ctx_ops.HYPER_DIRECT = direct
        real = ctx_ops.HyperDirect.take
        seen = []

        def take(self, _real=real, _seen=seen):
            buf, done = _real(self)
            _seen.append((buf is not None, len(done)))
            return buf, done
        ctx_ops.HyperDirect.take = take
        try:
            _ctx_step(pc, cams[0], pipe, bg)
            ctx_ops._seed_counter = itertools.count(2000)
            pkg, loss = _ctx_step(pc, cams[1], pipe, bg)
        finally:
            ctx_ops.HYPER_DIRECT = old
            ctx_ops.HyperDirect.take = real
        taken.append(list(seen))
        outs.append((pc._hyper_latent.grad.clone(), [p.grad.clone() for p in pc.latent_codec.parameters() if p.grad is not None]))
    assert taken[0] and all(t[0] and t[1] >= 1 for t in taken[0]), f"the direct route was not taken: {taken[0]}"
    assert all(not t[0] for t in taken[1])
    assert float(outs[0][0].abs().sum()) > 0
    close = lambda x, y: float((x - y).abs().max()) <= 2e-5 * float(x.abs().max()) + 1e-12
    assert close(outs[0][0], outs[1][0])
    assert bool(((outs[0][0] != 0) == (outs[1][0] != 0)).all())              # the same rows carry a gradient
    for x, y in zip(outs[0][1], outs[1][1]):
        assert close(x, y)
