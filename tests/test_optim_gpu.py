"""contextgs_amd.optim.FusedAdam (cgs_adam_step, csrc/adam.hip) on the device.

Oracle: torch.optim.Adam on CPU float64 copies of the same float32 inputs.  Tolerance, measured in the same test: for each of
p, exp_avg and exp_avg_sq, FusedAdam's max absolute error against that oracle must be at most TWICE the max absolute error of
torch's own fp32 Adam (on the device, default path) against it, plus a floor of one fp32 ulp of the largest value in the tensor.
The factor two covers differently contracted multiply-adds and a differently rounded divide and square root, no more: on the
CPU the plain fp32 formula and torch's fp32 Adam land at the same error against float64 on these inputs (1.4e-7 absolute after
six steps on parameters that moved by 4e-2).  Every parity test prints both errors; on the MI355X the two agree to the printed
digits (40-tensor dense case: p 6.225e-07 | 6.225e-07, exp_avg 6.133e-09 | 6.133e-09, exp_avg_sq 1.274e-10 | 1.274e-10).

Inputs: gradients randn x 10^U(-8, -1) per row (with eps = 1e-15 no square falls into the fp32 denormal range, where a flush
would be the thing measured), every third row exactly zero, one row zero on the first step only; lr = 7.5e-3; six steps with
fresh gradients each."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
LR, STEPS = 7.5e-3, 6
KINDS = ("p", "exp_avg", "exp_avg_sq")


def _rows_of(p):
    return p.shape[0] if p.dim() >= 1 else 1


def _grad(p, gen, step):
    """CPU fp32 gradient for parameter p (rows = the leading dimension; a 1-D tensor has one element per row)."""
    rows = _rows_of(p)
    if p.numel() == 0:
        return torch.zeros(p.shape)
    g = torch.randn(rows, p.numel() // rows, generator=gen) * 10.0 ** (torch.rand(rows, 1, generator=gen) * 7.0 - 8.0)
    g[::3] = 0.0
    if step == 0 and rows > 1:
        g[1] = 0.0
    return g.reshape(p.shape)


def _clone_optimizer(opt, device, dtype, cls=torch.optim.Adam):
    """A `cls` over copies of opt's parameters (same values, layout, group options and state) on device / dtype.
    Returns (optimizer, [copies in opt's parameter order])."""
    groups, copies, pairs = [], [], []
    for g in opt.param_groups:
        ps = []
        for p in g["params"]:
            q = p.detach().to(device=device, dtype=dtype or p.dtype).clone(memory_format=torch.preserve_format).requires_grad_(True)
            ps.append(q); copies.append(q); pairs.append((p, q))
        ng = {k: v for k, v in g.items() if k != "params" and (k != "row_sparse" or cls is not torch.optim.Adam)}
        ng["params"] = ps
        groups.append(ng)
    new = cls(groups, lr=0.0)
    for p, q in pairs:
        st = opt.state.get(p)
        if st:
            new.state[q] = {"step": st["step"].clone(),
                            "exp_avg": st["exp_avg"].to(device=device, dtype=dtype or p.dtype).clone(memory_format=torch.preserve_format),
                            "exp_avg_sq": st["exp_avg_sq"].to(device=device, dtype=dtype or p.dtype).clone(memory_format=torch.preserve_format)}
    return new, copies


def _params(opt):
    return [p for g in opt.param_groups for p in g["params"]]


def _set_grads(opts_and_params, gen, step, skip=()):
    """The same fresh gradients for the k-th parameter of every optimizer (the first one decides the shapes)."""
    first = opts_and_params[0]
    for k, p in enumerate(first):
        if k in skip:
            continue
        g = _grad(p, gen, step)
        for ps in opts_and_params:
            ps[k].grad = g.to(device=ps[k].device, dtype=ps[k].dtype).reshape(ps[k].shape)


def _tensors(opt, p):
    st = opt.state.get(p) or {}
    return {"p": p.detach(), "exp_avg": st.get("exp_avg"), "exp_avg_sq": st.get("exp_avg_sq")}


def _check_parity(tag, fused, f_params, plain, t_params, oracle, o_params):
    """FusedAdam within 2 x torch's fp32 error + one ulp of the largest value, per parameter and kind; prints the worst of each."""
    worst = {k: [0.0, 0.0] for k in KINDS}
    bad = []
    for k, (pf, pt, po) in enumerate(zip(f_params, t_params, o_params)):
        tf, tt, to = _tensors(fused, pf), _tensors(plain, pt), _tensors(oracle, po)
        for kind in KINDS:
            if to[kind] is None:
                assert tf[kind] is None and tt[kind] is None, (tag, k, kind)
                continue
            ref = to[kind].double().cpu()
            if ref.numel() == 0:
                continue
            e_f = float((tf[kind].double().cpu() - ref).abs().max())
            e_t = float((tt[kind].double().cpu() - ref).abs().max())
            ulp = float(np.spacing(np.float32(ref.abs().max())))
            worst[kind][0], worst[kind][1] = max(worst[kind][0], e_f), max(worst[kind][1], e_t)
            if not e_f <= 2.0 * e_t + ulp:
                bad.append((k, tuple(pf.shape), kind, e_f, e_t, ulp))
    print(f"[fused_adam] {tag}: max abs error against float64, FusedAdam | torch fp32: " +
          ", ".join(f"{kind} {worst[kind][0]:.3e} | {worst[kind][1]:.3e}" for kind in KINDS))
    assert not bad, bad


SIZES = [(1,), (3,), (4,), (5,), (255,), (4095,), (4096,), (4097,), (257, 3), (257, 50)]


def _dense_groups(gen):
    P = lambda *shape: torch.nn.Parameter(torch.randn(*shape, generator=gen).cuda())
    return [
        {"params": [P(*s) for s in SIZES], "lr": LR, "eps": 1e-15, "name": "a"},
        {"params": [P(*s) for s in SIZES], "lr": 2e-3, "eps": 1e-8, "betas": (0.8, 0.99), "weight_decay": 0.01, "name": "b"},
        {"params": [P(*s) for s in SIZES[:8]] + [P(0, 3), P(17)], "lr": 0.0, "eps": 1e-10, "betas": (0.95, 0.9999), "name": "c"},
        {"params": [P(*s) for s in SIZES], "lr": 1e-2, "eps": 1e-12, "betas": (0.85, 0.995), "name": "d"},
    ]


def test_dense_parity_forty_parameters_two_launches(monkeypatch):
    from contextgs_amd import _lib
    from contextgs_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(11)
    fused = FusedAdam(_dense_groups(gen), lr=0.0)
    f_params = _params(fused)
    assert len(f_params) == 40
    NO_GRAD = 29                                            # group c's last parameter never receives a gradient
    assert f_params[NO_GRAD].shape == (17,) and f_params[28].numel() == 0
    plain, t_params = _clone_optimizer(fused, "cuda", torch.float32)
    oracle, o_params = _clone_optimizer(fused, "cpu", torch.float64)
    start = [p.detach().clone() for p in f_params]
    launches = []
    real = _lib.lib().cgs_adam_step
    monkeypatch.setattr(_lib.lib(), "cgs_adam_step", lambda nt, *a: (launches.append(nt), real(nt, *a))[1])
    for step in range(STEPS):
        _set_grads([f_params, t_params, o_params], gen, step, skip=(NO_GRAD,))
        fused.step(); plain.step(); oracle.step()
    monkeypatch.undo()
    assert launches == [32, 6] * STEPS, launches           # 39 parameters with a gradient, one of them empty: 38 descriptors
    _check_parity("dense, 40 parameters", fused, f_params, plain, t_params, oracle, o_params)
    # written through raw pointers, announced like an in-place op (the model's caches are keyed on the version counter)
    assert f_params[0]._version >= STEPS and f_params[NO_GRAD]._version == 0
    assert len(fused.state[f_params[NO_GRAD]]) == 0 and torch.equal(f_params[NO_GRAD].detach(), start[NO_GRAD])
    for k, p in enumerate(f_params):
        if k != NO_GRAD:
            assert float(fused.state[p]["step"]) == STEPS and not fused.state[p]["step"].is_cuda
    moved = 0.0
    for k in range(20, 28):                                 # lr = 0: the moments move, the parameter does not
        assert torch.equal(f_params[k].detach(), start[k])
        assert float(fused.state[f_params[k]]["exp_avg"].abs().max()) > 0 or f_params[k].numel() < 3
    for k in range(0, 10):
        moved = max(moved, float((f_params[k].detach() - start[k]).abs().max()))
    assert moved > 1e-2, moved                              # lr = 7.5e-3 over six steps


@pytest.mark.parametrize("sparse", [False, True])
def test_misaligned_views_match_aligned_copies_and_leave_the_guards(sparse):
    from contextgs_amd.optim import FusedAdam
    N, W = 1367, 3                                          # 4101 elements: a vector body, a tail, two chunks
    n, S = N * W, 12345.678
    gen = torch.Generator().manual_seed(5)
    offs = {"p": 1, "g": 1, "exp_avg": 2, "exp_avg_sq": 3}
    bufs = {k: torch.full((n + 8,), S, device="cuda") for k in offs}
    view = lambda k: bufs[k][offs[k]:offs[k] + n].view(N, W)
    assert all(view(k).data_ptr() % 16 == 4 * offs[k] and view(k).is_contiguous() for k in offs)
    view("p").copy_(torch.randn(N, W, generator=gen)); view("exp_avg").zero_(); view("exp_avg_sq").zero_()
    p = torch.nn.Parameter(view("p"))
    assert p.data_ptr() == view("p").data_ptr()
    q = torch.nn.Parameter(p.detach().clone())
    group = lambda x: [{"params": [x], "lr": LR, "eps": 1e-15, "row_sparse": True}]
    a, b = FusedAdam(group(p), lr=0.0), FusedAdam(group(q), lr=0.0)
    a.state[p] = {"step": torch.tensor(0.0), "exp_avg": view("exp_avg"), "exp_avg_sq": view("exp_avg_sq")}
    assert q.data_ptr() % 16 == 0
    for step in range(3):
        g = _grad(p, gen, step).cuda()
        view("g").copy_(g)
        p.grad, q.grad = view("g"), g.clone()
        rows = (torch.rand(N, generator=gen) < 0.4).cuda() if sparse else None
        a.step(rows=rows); b.step(rows=rows)
    assert a.state[p]["exp_avg"].data_ptr() == view("exp_avg").data_ptr()
    assert torch.equal(p.detach(), q.detach())
    assert torch.equal(a.state[p]["exp_avg"], b.state[q]["exp_avg"]) and torch.equal(a.state[p]["exp_avg_sq"], b.state[q]["exp_avg_sq"])
    assert float(b.state[q]["exp_avg_sq"].max()) > 0
    for k in offs:                                          # the sentinels on both sides, bit for bit
        guard = torch.cat([bufs[k][:offs[k]], bufs[k][offs[k] + n:]])
        assert guard.numel() == 8 and torch.equal(guard, torch.full((8,), S, device="cuda")), k


def test_batching_independence():
    from contextgs_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(7)
    shapes = [(4097,), (257, 3), (5,), (300, 10, 3), (257, 50)]
    base = [torch.randn(*s, generator=gen).cuda() for s in shapes]
    mk = lambda t, sp: {"params": [torch.nn.Parameter(t.clone())], "lr": LR, "eps": 1e-15, "row_sparse": sp}
    together = FusedAdam([mk(t, t.shape[0] == 257) for t in base], lr=0.0)
    apart = [FusedAdam([mk(t, t.shape[0] == 257)], lr=0.0) for t in base]
    for step in range(3):
        rows = (torch.rand(257, generator=gen) < 0.5).cuda()
        for k, p in enumerate(_params(together)):
            q = _params(apart[k])[0]
            p.grad = _grad(p, gen, step).cuda()
            q.grad = p.grad.clone()
        together.step(rows=rows)
        for o in apart:
            o.step(rows=rows)
    for k, p in enumerate(_params(together)):
        q = _params(apart[k])[0]
        assert torch.equal(p.detach(), q.detach()), k
        for kind in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(together.state[p][kind], apart[k].state[q][kind]), (k, kind)


def _sparse_groups(N, gen):
    P = lambda *shape: torch.nn.Parameter(torch.randn(*shape, generator=gen).cuda())
    return [{"params": [P(N, 1)], "lr": LR, "eps": 1e-15, "row_sparse": True, "name": "w1"},
            {"params": [P(N, 3)], "lr": LR, "eps": 1e-15, "row_sparse": True, "name": "w3"},
            {"params": [P(N, 6)], "lr": 2e-3, "eps": 1e-15, "row_sparse": True, "weight_decay": 0.01, "name": "w6"},
            {"params": [P(N, 10, 3)], "lr": LR, "eps": 1e-15, "row_sparse": True, "name": "w30"},
            {"params": [P(N, 50)], "lr": LR, "eps": 1e-15, "betas": (0.8, 0.99), "row_sparse": True, "name": "w50"},
            {"params": [P(N, 3)], "lr": LR, "eps": 1e-15, "name": "dense with N rows"}]


def _restore(opt, params, before, rows_dev, upto):
    """Put p, exp_avg, exp_avg_sq of the masked-out rows of params[:upto] back: the sparse oracle."""
    for p, b in zip(params[:upto], before[:upto]):
        out = ~rows_dev.to(p.device)
        p.data[out] = b["p"][out]
        for kind in ("exp_avg", "exp_avg_sq"):
            opt.state[p][kind][out] = b[kind][out] if b[kind] is not None else 0


def _snapshot(opt, params):
    return [{k: (None if v is None else v.clone()) for k, v in _tensors(opt, p).items()} for p in params]


@pytest.mark.parametrize("density", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("N", [1, 257, 1025])
def test_row_sparse_parity(N, density):
    from contextgs_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(100 + N)
    fused = FusedAdam(_sparse_groups(N, gen), lr=0.0)
    f_params = _params(fused)
    plain, t_params = _clone_optimizer(fused, "cuda", torch.float32)
    oracle, o_params = _clone_optimizer(fused, "cpu", torch.float64)
    dense, d_params = _clone_optimizer(fused, "cuda", torch.float32, cls=FusedAdam)
    start = _snapshot(fused, f_params)
    for step in range(STEPS):
        rows = torch.rand(N, generator=gen) < density if density < 1.0 else torch.ones(N, dtype=torch.bool)
        if N == 1 and density == 0.3:
            rows[0] = step % 2 == 0
        _set_grads([f_params, t_params, o_params, d_params], gen, step)
        before = [_snapshot(o, ps) for o, ps in ((fused, f_params), (plain, t_params), (oracle, o_params))]
        fused.step(rows=rows.cuda()); plain.step(); oracle.step(); dense.step(rows=None)
        _restore(plain, t_params, before[1], rows, 5)
        _restore(oracle, o_params, before[2], rows, 5)
        out = ~rows.cuda()
        for p, b in zip(f_params[:5], before[0]):          # rows outside the mask: bit-identical to before the step
            assert torch.equal(p.detach()[out], b["p"][out])
            for kind in ("exp_avg", "exp_avg_sq"):
                was = b[kind][out] if b[kind] is not None else torch.zeros_like(p.detach()[out])
                assert torch.equal(fused.state[p][kind][out], was), kind
    _check_parity(f"row-sparse N = {N}, density {density}", fused, f_params, plain, t_params, oracle, o_params)
    for p in f_params:
        assert float(fused.state[p]["step"]) == STEPS       # the step count advances whatever the mask says
    if density == 0.0:
        for p, s in zip(f_params[:5], start):
            assert torch.equal(p.detach(), s["p"])
            assert not fused.state[p]["exp_avg"].any() and not fused.state[p]["exp_avg_sq"].any()
    if density == 1.0:                                      # an all-true mask is the dense step, bit for bit
        for p, d in zip(f_params, d_params):
            assert torch.equal(p.detach(), d.detach())
            for kind in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(fused.state[p][kind], dense.state[d][kind])
    # the group without the flag has N rows too and is stepped densely all the same
    assert torch.equal(f_params[5].detach(), d_params[5].detach())
    assert torch.equal(fused.state[f_params[5]]["exp_avg_sq"], dense.state[d_params[5]]["exp_avg_sq"])


def test_row_count_mismatch_raises_before_any_launch(monkeypatch):
    from contextgs_amd import _lib
    from contextgs_amd.optim import FusedAdam
    a, b = torch.nn.Parameter(torch.ones(10, 3).cuda()), torch.nn.Parameter(torch.ones(12, 3).cuda())
    opt = FusedAdam([{"params": [a], "row_sparse": True}, {"params": [b], "row_sparse": True}], lr=1e-2)
    a.grad, b.grad = torch.ones_like(a), torch.ones_like(b)
    launches = []
    monkeypatch.setattr(_lib.lib(), "cgs_adam_step", lambda *args: launches.append(args) or 0)
    with pytest.raises(ValueError, match="rows"):
        opt.step(rows=torch.ones(10, dtype=torch.bool, device="cuda"))
    assert not launches and len(opt.state[a]) == 0 and len(opt.state[b]) == 0
    assert torch.equal(a.detach(), torch.ones_like(a)) and torch.equal(b.detach(), torch.ones_like(b))


def test_fp16_and_non_contiguous_parameters_take_the_parent_path():
    from contextgs_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(3)
    half = torch.nn.Parameter(torch.randn(33, 5, generator=gen).cuda().half())
    strided = torch.nn.Parameter(torch.randn(8, 6, generator=gen).cuda().t())
    normal = torch.nn.Parameter(torch.randn(40, generator=gen).cuda())
    assert not strided.is_contiguous()
    fused = FusedAdam([{"params": [half, strided], "lr": LR, "eps": 1e-3}, {"params": [normal], "lr": LR, "eps": 1e-15}], lr=0.0)
    plain, t_params = _clone_optimizer(fused, "cuda", None)
    f_params = _params(fused)
    assert t_params[0].dtype == torch.float16 and t_params[1].stride() == strided.stride()
    for step in range(3):
        for p, q in zip(f_params, t_params):
            # 0.5 <= |g| < 1.5: its square times 1 - beta2 = 1e-3 is a normal fp16 number, so no moment underflows to 0 / 0
            g = ((torch.rand(p.shape, generator=gen) + 0.5) * torch.sign(torch.randn(p.shape, generator=gen))).cuda().to(p.dtype)
            p.grad, q.grad = g.clone(), g.clone()
        fused.step(); plain.step()
    for k, (p, q) in enumerate(zip(f_params, t_params)):
        assert float(fused.state[p]["step"]) == 3.0
        assert bool(torch.isfinite(p.detach()).all()) and bool(torch.isfinite(fused.state[p]["exp_avg_sq"]).all()), k
        if k < 2:                                           # the parent's own kernels on the same inputs
            assert torch.equal(p.detach(), q.detach()), k
            assert torch.equal(fused.state[p]["exp_avg_sq"], plain.state[q]["exp_avg_sq"]), k
        else:
            assert torch.allclose(p.detach(), q.detach(), rtol=0, atol=1e-6)
    assert float((normal.detach() - t_params[2].detach()).abs().max()) <= 1e-6


ARGS = types.SimpleNamespace(
    percent_dense=0.01, position_lr_init=0.0, position_lr_final=0.0, position_lr_delay_mult=0.01, position_lr_max_steps=30000,
    offset_lr_init=0.01, offset_lr_final=0.0001, offset_lr_delay_mult=0.01, offset_lr_max_steps=30000,
    mask_lr_init=0.01, mask_lr_final=0.0001, mask_lr_delay_mult=0.01, mask_lr_max_steps=30000,
    feature_lr=0.0075, hyper_latent_lr=0.0075, opacity_lr=0.02, scaling_lr=0.007, rotation_lr=0.002,
    mlp_opacity_lr_init=0.002, mlp_opacity_lr_final=0.00002, mlp_opacity_lr_delay_mult=0.01, mlp_opacity_lr_max_steps=30000,
    mlp_cov_lr_init=0.004, mlp_cov_lr_final=0.004, mlp_cov_lr_delay_mult=0.01, mlp_cov_lr_max_steps=30000,
    mlp_color_lr_init=0.008, mlp_color_lr_final=0.00005, mlp_color_lr_delay_mult=0.01, mlp_color_lr_max_steps=30000,
    latent_codec_lr_init=0.005, latent_codec_lr_final=0.00001, latent_codec_lr_delay_mult=0.33, latent_codec_lr_max_steps=30000,
    mlp_grid_lr_init=0.005, mlp_grid_lr_final=0.00001, mlp_grid_lr_delay_mult=0.01, mlp_grid_lr_max_steps=30000)
PER_ANCHOR = ("_anchor", "_offset", "_mask", "_anchor_feat", "_hyper_latent", "_scaling")


def _scene(N, kind, monkeypatch):
    from contextgs_amd.optim import FusedAdam
    from contextgs_amd.synth import make_scene
    monkeypatch.delenv("CGS_OPTIMIZER", raising=False)
    pc = make_scene(N, seed=3); pc.train(); pc.spatial_lr_scale = 1.0
    args = types.SimpleNamespace(**vars(ARGS)); args.optimizer_type = kind
    pc.training_setup(args)
    assert type(pc.optimizer) is FusedAdam
    return pc


def test_surgery_then_a_further_step(monkeypatch):
    pc = _scene(400, "fused_adam", monkeypatch)
    gen = torch.Generator().manual_seed(9)
    for step in range(2):
        for attr in PER_ANCHOR:
            getattr(pc, attr).grad = _grad(getattr(pc, attr), gen, step).cuda()
        pc.optimizer.step()
    N0 = pc._anchor.shape[0]
    drop = (torch.rand(N0, generator=gen) < 0.25).cuda()
    pc.prune_anchor(drop)
    N1 = N0 - int(drop.sum())
    M = 37
    new = {"anchor": torch.randn(M, 3, generator=gen), "offset": torch.randn(M, pc.n_offsets, 3, generator=gen),
           "mask": torch.randn(M, pc.n_offsets, 1, generator=gen), "anchor_feat": torch.randn(M, 50, generator=gen),
           "hyper_latent": torch.randn(M, 12, generator=gen), "opacity": torch.zeros(M, 1),
           "scaling": torch.randn(M, 6, generator=gen), "rotation": torch.randn(M, 4, generator=gen)}
    t = pc.cat_tensors_to_optimizer({k: v.cuda() for k, v in new.items()})
    for name, attr in (("anchor", "_anchor"), ("offset", "_offset"), ("mask", "_mask"), ("anchor_feat", "_anchor_feat"),
                       ("hyper_latent", "_hyper_latent"), ("scaling", "_scaling"), ("rotation", "_rotation"), ("opacity", "_opacity")):
        setattr(pc, attr, t[name])
    for attr in PER_ANCHOR:                                 # the moments follow the parameters through both operations
        p = getattr(pc, attr)
        st = pc.optimizer.state[p]
        assert p.shape[0] == N1 + M and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape, attr
        assert float(st["step"]) == 2.0 and not st["exp_avg"][N1:].any() and st["exp_avg"][:N1].any()
    fused = pc.optimizer
    f_params = _params(fused)
    plain, t_params = _clone_optimizer(fused, "cuda", torch.float32)
    oracle, o_params = _clone_optimizer(fused, "cpu", torch.float64)
    with_grad = {id(getattr(pc, a)) for a in PER_ANCHOR}
    skip = tuple(k for k, p in enumerate(f_params) if id(p) not in with_grad)
    _set_grads([f_params, t_params, o_params], gen, 2, skip=skip)
    fused.step(); plain.step(); oracle.step()
    _check_parity("one step after prune + cat", fused, f_params, plain, t_params, oracle, o_params)
    for attr in PER_ANCHOR:
        assert float(fused.state[getattr(pc, attr)]["step"]) == 3.0


def test_sparse_adam_through_the_renderer(monkeypatch):
    from contextgs_amd.renderer import prefilter_voxel, render
    from contextgs_amd.synth import SynthPipe, look_at_camera
    pc = _scene(3000, "sparse_adam", monkeypatch)
    fused = pc.optimizer
    sparse_names = {g["name"] for g in fused.param_groups if g.get("row_sparse")}
    assert sparse_names == {"anchor", "offset", "anchor_feat", "hyper_latent", "scaling", "rotation"}
    # close to the unit-sphere scene with a narrow lens: each view sees part of the anchors only
    cams = [look_at_camera(eye, (0, 0, 0), 96, 64, fovx_deg=40.0).to_torch("cuda") for eye in ((1.6, 0.3, 0.4), (-0.3, 1.6, 0.4))]
    pipe, bg = SynthPipe(), torch.zeros(3, device="cuda")

    def iteration(cam, step):
        fused.zero_grad(set_to_none=True)
        vis = prefilter_voxel(cam, pc, pipe, bg)
        pkg = render(cam, pc, pipe, bg, visible_mask=vis, retain_grad=True, step=step)
        loss = (1.0 - pkg["render"]).abs().mean() + 0.01 * pkg["scaling"].prod(dim=1).mean()
        loss = loss + 5e-4 * torch.sigmoid(pc._mask).mean()          # train.py:209's regulariser: gradient on EVERY row of _mask
        if pkg["bit_per_param"] is not None:
            loss = loss + 0.001 * pkg["bit_per_param"]
        loss.backward()
        before = {g["name"]: _snapshot(fused, g["params"]) for g in fused.param_groups}
        had_grad = {g["name"]: [p.grad is not None for p in g["params"]] for g in fused.param_groups}
        fused.step()                                                  # rows="auto": the renderer's note
        return vis.clone(), before, had_grad

    vis, before, had_grad = iteration(cams[0], 1000)
    assert 0 < int(vis.sum()) < vis.numel(), "the view must see some anchors and miss some"
    out, stepped_sparse, stepped_dense = ~vis, 0, 0
    for g in fused.param_groups:
        for p, b, has in zip(g["params"], before[g["name"]], had_grad[g["name"]]):
            if not has:
                continue
            st = fused.state[p]
            if g["name"] in sparse_names:
                stepped_sparse += 1
                assert torch.equal(p.detach()[out], b["p"][out]), g["name"]
                assert not st["exp_avg"][out].any() and not st["exp_avg_sq"][out].any(), g["name"]
                assert not torch.equal(p.detach()[vis], b["p"][vis]) or float(g["lr"]) == 0.0, g["name"]
                assert st["exp_avg_sq"][vis].any(), g["name"]
            else:                                                     # _mask and the MLPs: dense
                if float(g["lr"]) == 0.0:
                    continue
                # first step: p moves by ~lr * sign(g) wherever g is far above eps = 1e-15
                big = p.grad.abs() > 1e-12
                stepped_dense += int(big.any())
                assert bool((p.detach() != b["p"])[big].all()), g["name"]
                if g["name"] == "mask":                               # rows the view did not see included
                    assert bool((p.detach()[out] != b["p"][out]).all()) and bool(st["exp_avg_sq"][out].ne(0).all())
    assert stepped_sparse >= 3 and stepped_dense >= 4, (stepped_sparse, stepped_dense)

    vis, before, had_grad = iteration(cams[1], 20000)                 # the context model runs over all anchors: the note is None
    assert 0 < int(vis.sum()) < vis.numel()
    checked = 0
    for g in fused.param_groups:
        if g["name"] in ("anchor_feat", "hyper_latent", "scaling", "offset") and had_grad[g["name"]][0]:
            p, b, st = g["params"][0], before[g["name"]][0], fused.state[g["params"][0]]
            N = p.shape[0]
            strong = (p.grad.abs() > 1e-12).reshape(N, -1).any(dim=1) & ~vis      # rows this view did not see, with a real gradient
            if not bool(strong.any()):
                continue
            checked += 1
            was = b["exp_avg_sq"] if b["exp_avg_sq"] is not None else torch.zeros_like(p)
            changed = (st["exp_avg_sq"] != was).reshape(N, -1).any(dim=1) & (p.detach() != b["p"]).reshape(N, -1).any(dim=1)
            assert bool(changed[strong].all()), g["name"]
    assert checked >= 2, checked
