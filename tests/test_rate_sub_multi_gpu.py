"""The rate subset of all levels in one launch per stage (csrc/rate_sub.hip: cgs_rate_sub_fwd_multi / cgs_rate_sub_bwd_multi, and
the group form the training step uses, cgs_rate_sub_group_begin / _end around the per-level calls) against one call per level on
the same operands: a workgroup belongs to one level, so every per-row output, every per-workgroup image and their block-order
sums must have the bits of the per-level launches; only the forward's three sums, closed by float atomics, are held to the fp64
statement instead.  Plus: nothing is written outside the levels' spans and the scratch, the workgroup partition
(cgs_rate_sub_partition, no kernel) keeps its promises, and one training step is the same with and without the grouping."""
import contextlib
import ctypes
import functools
import itertools

import pytest
import torch

gpu = pytest.mark.gpu
GUARD = 64                      # floats of NaN behind every output span
SCRATCH_TAIL = 4096             # bytes behind the scratch
OUT_KEYS = ("side_f", "side_s", "side_o", "side_Q", "dx_sub", "d_masks", "dW1", "db1", "dW2", "db2")


def _level_sets(C):
    """(in_dim, m) per level: the four sets; C = compute units (a workgroup pass takes 8 tiles of 16 rows)."""
    return ([(15, 1), (71, 17), (71, 129)],
            [(15, 1000), (71, 0), (71, 4099)],                        # an empty level in the middle
            [(71, 16 * 8 * C + 5)],                                   # more than one pass per wave, L = 1
            [(15, 40), (71, 16 * 8 * C + 5), (71, 33)])               # a large level between two of one workgroup each


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _operands(in_dim, m, seed):
    """One level's operands in the regime of test_rate_sub_gpu.py (likelihoods well above the 1e-6 bound, a few scale outputs far
    below the 1e-9 clamp), float32 on the device."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    R = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    n = 3 * m + 5
    o = dict(in_dim=in_dim, m=m, n=n, X=R(n, in_dim), loc=torch.sort(torch.randperm(n, generator=gen)[:m])[0],
             W1=R(100, in_dim) * 0.2, b1=R(100) * 0.1, W2=R(175, 100) * 0.02, b2=R(175) * 0.1, yf=R(n, 50), ys=R(n, 6), yo=R(n, 30),
             Q=torch.rand(n, 3, generator=gen) * 0.5 + 0.05, masks=(torch.rand(m, 10, generator=gen) < 0.6).float(),
             x_means=torch.tensor([0.1, -0.2, 0.05]), g_sums=torch.tensor([0.7, -1.3, 2.1]))
    o["b2"][50:100] += 2.5; o["b2"][106:112] += 2.5; o["b2"][142:172] += 2.5
    o["b2"][[53, 107, 150]] = -3.0
    return {k: v.cuda().contiguous() if torch.is_tensor(v) else v for k, v in o.items()}


def _widths(o):
    return dict(side_f=(o["m"], 50), side_s=(o["m"], 6), side_o=(o["m"], 30), side_Q=(o["m"], 3), dx_sub=(o["m"], o["in_dim"]),
                d_masks=(o["m"], 10), dW1=(100, o["in_dim"]), db1=(100,), dW2=(175, 100), db2=(175,))


def _guarded_outputs(ops):
    """Every output of every level in ONE NaN-filled buffer, GUARD floats between and behind the spans -> (flat, per-level views,
    mask of the floats that belong to no span)."""
    sizes = [[int(torch.Size(s).numel()) for s in _widths(o).values()] for o in ops]
    total = sum(sz + GUARD for lv in sizes for sz in lv)
    flat = torch.full((total,), float("nan"), device="cuda")
    outside = torch.ones(total, dtype=torch.bool, device="cuda")
    views, at = [], 0
    for o, lv in zip(ops, sizes):
        v = {}
        for (k, shape), sz in zip(_widths(o).items(), lv):
            v[k] = flat[at:at + sz].view(shape)
            outside[at:at + sz] = False
            at += sz + GUARD
        views.append(v)
    return flat, views, outside


def _record(o, use_mask, use_clamp, sums, out):
    from contextgs_amd import _lib
    p = _lib.ptr
    r = _lib.RateSubLevel()
    r.in_dim, r.use_clamp, r.n, r.m = o["in_dim"], use_clamp, o["n"], o["m"]
    for k in ("X", "loc", "W1", "b1", "W2", "b2", "yf", "ys", "yo", "Q", "x_means"):
        setattr(r, k, p(o[k]))
    r.masks = p(o["masks"]) if (use_mask and o["m"]) else None
    r.sums3, r.g_sums3 = p(sums), p(o["g_sums"])
    for k in OUT_KEYS:
        setattr(r, k, p(out[k]) if out[k].numel() else None)
    return r


def _single_args(o, use_mask, use_clamp):
    from contextgs_amd import _lib
    p = _lib.ptr
    return (o["in_dim"], p(o["X"]), o["n"], p(o["loc"]), o["m"], p(o["W1"]), p(o["b1"]), p(o["W2"]), p(o["b2"]), p(o["yf"]),
            p(o["ys"]), p(o["yo"]), p(o["Q"]), p(o["masks"]) if use_mask else None, p(o["x_means"]), use_clamp)


def _per_level(ops, use_mask, use_clamp, grouped):
    """cgs_rate_sub_fwd / _bwd level by level — launched one by one, or recorded between group_begin / group_end."""
    from contextgs_amd import _lib
    L, p, st = _lib.lib(), _lib.ptr, _lib.current_stream()
    sums = torch.zeros(len(ops), 3, device="cuda")
    outs = [{k: torch.full(s, float("nan"), device="cuda") for k, s in _widths(o).items()} for o in ops]
    scratch = [torch.empty(int(L.cgs_rate_sub_bwd_scratch_bytes(o["in_dim"], o["m"])), dtype=torch.uint8, device="cuda") for o in ops]

    @contextlib.contextmanager
    def group():
        if grouped:
            _lib.check(L.cgs_rate_sub_group_begin(), "group_begin")
        yield
        if grouped:
            _lib.check(L.cgs_rate_sub_group_end(1), "group_end")
    with group():
        for j, o in enumerate(ops):
            _lib.check(L.cgs_rate_sub_fwd(*_single_args(o, use_mask, use_clamp), p(sums[j]), st), "fwd")
    with group():
        for j, o in enumerate(ops):
            if o["m"]:
                _lib.check(L.cgs_rate_sub_bwd(*_single_args(o, use_mask, use_clamp), p(o["g_sums"]), *(p(outs[j][k]) for k in OUT_KEYS),
                                              p(scratch[j]), scratch[j].numel(), st), "bwd")
    torch.cuda.synchronize()
    return sums, outs


@functools.lru_cache(maxsize=None)
def _case(set_id, use_mask, use_clamp):
    """Everything the tests of one case read, computed once: the per-level launches, the group form, the array form inside guarded
    buffers, and the fp64 sums."""
    from contextgs_amd import _lib
    from test_rate_sub_gpu import _torch_rate
    L, p, st = _lib.lib(), _lib.ptr, _lib.current_stream()
    spec = _level_sets(_cus())[set_id]
    ops = [_operands(in_dim, m, 1000 * set_id + 10 * j + 1) for j, (in_dim, m) in enumerate(spec)]
    single = _per_level(ops, use_mask, use_clamp, grouped=False)
    group = _per_level(ops, use_mask, use_clamp, grouped=True)
    # the array form, every output inside one guarded buffer, the scratch with a tail
    flat, views, outside = _guarded_outputs(ops)
    sums = torch.zeros(len(ops), 3, device="cuda")
    recs = (_lib.RateSubLevel * len(ops))(*[_record(o, use_mask, use_clamp, sums[j], views[j]) for j, o in enumerate(ops)])
    _lib.check(L.cgs_rate_sub_fwd_multi(len(ops), recs, st), "fwd_multi")
    need = int(L.cgs_rate_sub_bwd_multi_scratch_bytes(len(ops), recs))
    scratch = torch.full((need + SCRATCH_TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
    _lib.check(L.cgs_rate_sub_bwd_multi(len(ops), recs, p(scratch), need, st), "bwd_multi")
    torch.cuda.synchronize()
    ref = []
    for o in ops:
        d = lambda k: o[k].double()
        masks = d("masks") if use_mask else torch.ones(o["m"], 10, dtype=torch.float64, device="cuda")
        ref.append(_torch_rate(d("X"), o["loc"], d("W1"), d("b1"), d("W2"), d("b2"), d("yf"), d("ys"), d("yo"), d("Q"), masks,
                               d("x_means"), use_clamp).float() if o["m"] else torch.zeros(3, device="cuda"))
    return dict(spec=spec, single=single, group=group, multi=(sums, views), flat=flat, outside=outside, scratch=scratch, need=need,
                ref=torch.stack(ref))


CASES = [(s, mk, cl) for s in range(4) for mk in (True, False) for cl in (0, 1)]


@gpu
@pytest.mark.parametrize("set_id,use_mask,use_clamp", CASES)
def test_grouped_launches_have_the_bits_of_one_launch_per_level(set_id, use_mask, use_clamp):
    c = _case(set_id, use_mask, use_clamp)
    sums1, outs1 = c["single"]
    for form in ("group", "multi"):
        sums, outs = c[form]
        for j, (in_dim, m) in enumerate(c["spec"]):
            for k in OUT_KEYS:
                if m == 0 or (k == "d_masks" and not use_mask):
                    continue                    # (nothing of an empty level is written; d_masks only with masks: test below)
                assert torch.equal(outs[j][k], outs1[j][k]), (form, j, in_dim, m, k)
        # the three sums per level: float atomics close them — against the fp64 statement, at the tolerance of test_rate_sub_gpu.py
        print(form, "sums", sums.tolist(), "fp64", c["ref"].tolist())
        assert torch.allclose(sums, c["ref"], rtol=3e-5, atol=1e-3), (form, sums, c["ref"])
    assert torch.allclose(sums1, c["ref"], rtol=3e-5, atol=1e-3), (sums1, c["ref"])


@gpu
@pytest.mark.parametrize("set_id,use_mask,use_clamp", CASES)
def test_nothing_is_written_outside_the_spans_and_the_scratch(set_id, use_mask, use_clamp):
    c = _case(set_id, use_mask, use_clamp)
    _sums, views = c["multi"]
    for j, (in_dim, m) in enumerate(c["spec"]):
        for k in OUT_KEYS:
            t = views[j][k]
            if m == 0 or (k == "d_masks" and not use_mask):
                assert bool(torch.isnan(t).all()), (j, k, "an empty level / an absent mask gradient must stay untouched")
            else:
                assert bool(torch.isfinite(t).all()), (j, in_dim, m, k)          # every row of every level written
    assert bool(torch.isnan(c["flat"][c["outside"]]).all())                       # the floats behind each span
    assert bool((c["scratch"][c["need"]:] == 0xA5).all())                         # the bytes behind scratch_bytes


def _partition(spec, C):
    from contextgs_amd import _lib
    L = len(spec)
    in_dim = (ctypes.c_int * L)(*[d for d, _ in spec])
    m = (ctypes.c_int64 * L)(*[m_ for _, m_ in spec])
    blocks, first = (ctypes.c_int * L)(), (ctypes.c_int * (L + 1))()
    _lib.check(_lib.lib().cgs_rate_sub_partition(L, in_dim, m, C, blocks, first), "partition")
    return list(blocks), list(first)


@pytest.mark.parametrize("C", [1, 8, 256, 304])
@pytest.mark.parametrize("set_id", range(4))
def test_the_partition_of_the_workgroups(set_id, C):
    spec = _level_sets(C)[set_id]
    blocks, first = _partition(spec, C)
    tiles = [(m + 15) // 16 for _, m in spec]
    nonempty = sum(1 for t in tiles if t)
    for b, t in zip(blocks, tiles):
        if t == 0:
            assert b == 0
        else:
            assert 1 <= b <= (t + 7) // 8, (blocks, tiles)
    assert sum(blocks) <= max(C, nonempty), (blocks, C)
    assert first == [0] + list(itertools.accumulate(blocks)), (first, blocks)
    # in proportion to tiles x matrix instructions per tile (476 / 364 for 71 / 15 inputs): a level that could use one more
    # workgroup carries no more per workgroup than another level would with one less
    load = [t * {71: 476, 15: 364}[d] for t, (d, _) in zip(tiles, spec)]
    for i, j in itertools.permutations(range(len(spec)), 2):
        if blocks[i] and blocks[i] < (tiles[i] + 7) // 8 and blocks[j] > 1:
            assert load[i] * (blocks[j] - 1) <= load[j] * blocks[i], (blocks, load)
    if sum(blocks) < C:         # workgroups left over: every level has all it can use
        assert all(b == (t + 7) // 8 for b, t in zip(blocks, tiles)), (blocks, tiles, C)


@gpu
def test_one_training_step_is_the_same_with_and_without_the_grouping(monkeypatch):
    """The 3 000-anchor scene, a rate-only loss through render(), default knobs: the step with the levels' rate launches grouped
    against the same step with one launch per level (the group replaced by nothing).  The image and what the rate kernels do not
    touch, and every gradient, bit for bit; the four rate values — sums closed by float atomics — within 4 ulp, the bound
    tests/test_ctx_level_gpu.py holds them to."""
    from contextgs_amd import ctx_ops
    from contextgs_amd.renderer import prefilter_voxel, render
    from contextgs_amd.synth import SynthPipe, make_scene, orbit_cameras
    pipe, bg = SynthPipe(), torch.zeros(3, device="cuda")
    cam = orbit_cameras(2, 96, 64)[0].to_torch("cuda")
    pc = make_scene(3000, seed=1)
    pc.train()
    rates = ("bit_per_param", "bit_per_feat_param", "bit_per_scaling_param", "bit_per_offsets_param")
    L = ctx_ops._lib.lib()
    calls = {"begin": 0, "fwd": 0, "bwd": 0}
    for key, name in (("begin", "cgs_rate_sub_group_begin"), ("fwd", "cgs_rate_sub_fwd"), ("bwd", "cgs_rate_sub_bwd")):
        def counted(*a, _fn=getattr(L, name), _key=key):
            calls[_key] += 1
            return _fn(*a)
        monkeypatch.setattr(L, name, counted, raising=False)

    def step():
        torch.manual_seed(0)
        monkeypatch.setattr(ctx_ops, "_seed_counter", itertools.count(1))
        pc.zero_grad()
        vis = prefilter_voxel(cam, pc, pipe, bg)
        pkg = render(cam, pc, pipe, bg, visible_mask=vis, step=20000)
        sum(w * pkg[k] for w, k in zip((1.0, 0.3, 0.2, 0.1), rates)).backward()
        torch.cuda.synchronize()
        return ({k: pkg[k].detach().clone() for k in ("render", "scaling", "neural_opacity")},
                torch.stack([pkg[k].detach() for k in rates]),
                {k: p.grad.clone() for k, p in pc.named_parameters() if p.grad is not None})

    new = step()
    assert calls["begin"] == 2 and calls["fwd"] == calls["bwd"] >= 2, calls           # the grouped path ran, on several levels
    monkeypatch.setattr(ctx_ops, "_rate_sub_group", contextlib.nullcontext)
    old = step()
    assert calls["begin"] == 2, calls
    for k in new[0]:
        assert torch.equal(new[0][k], old[0][k]), k
    print("rates", new[1].tolist(), old[1].tolist())
    assert bool(((new[1] - old[1]).abs() <= 4 * 2.0 ** -23 * old[1].abs()).all()), (new[1], old[1])
    assert set(new[2]) == set(old[2]) and len(new[2]) > 0
    for k in sorted(new[2]):
        print(k, float((new[2][k] - old[2][k]).abs().max()))
    for k in sorted(new[2]):
        assert torch.equal(new[2][k], old[2][k]), (k, float((new[2][k] - old[2][k]).abs().max()))
