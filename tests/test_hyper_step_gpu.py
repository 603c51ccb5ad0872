"""The hyper prior's training forms (csrc/eb.hip: cgs_hyper_noise_gather, cgs_eb_bits_fwd / _bwd, and the autograd node
_HyperStep that merges their gradients) against the integer / float64 restatement in tests/hyper_ref.py.

Inputs: C in {1, 5, 12, 16} (1 and 5 take the scalar noise kernel, 12 and 16 the float4 one), two parameter sets each, and
values in three regimes of the float64 likelihood: body (>= 1e-3), tail ([1e-8, 1e-3)) and bounded (<= 1e-10, |x| in
[400, 3000], logits below -100 in every channel); nothing in (1e-10, 1e-8), which fp32 can not classify as fp64 does.

Tolerances.  Exact (torch.equal): the noise, the gathers, subset against compacted subset, repeated calls, blocked gradients,
the dense part of the node's gradient.  Against float64:
  likelihood, body      3e-7 absolute (the project's bound for a difference of two fp32 sigmoids); measured worst 1.5e-7
  likelihood, tail      relative error <= TAIL_FACTOR times the worst relative error of the fp32 torch composition
                        (interval_likelihood in float32) on the same parameter set's tail elements, which is 1.5e-5 .. 2.5e-5
                        here; the kernel's worst error measured 1.22 times that (its exp, rcp and tanh are approximations),
                        doubled and rounded up to a power of two: TAIL_FACTOR = 4
  bit sum               the sum of the per-element tolerances through -log2 (bits_tol); the sums use at most 7 % of it, the
                        planted rows at most 34 %
  d/dv                  test_eb_gpu.py's ceiling, 2e-3 relative + 2e-5 of the largest entry, used to 14.6 % at worst (the
                        36000-row subset at C = 12), doubled: GRAD_SCALE = 0.3 of the ceiling
  parameter gradients   3e-4 of the tensor's largest entry, used to 5.9 % at worst, doubled: PARAM_SCALE = 0.12 of the ceiling
(figures of one MI355X run with the clamped sigmoid; `pytest -s` prints the worst of each kind as MEASURE lines).

The bounded regime is what sigmoidf's clamp of the exponential is for: without it every element whose logit lies below -88.7
puts NaN into g_sub and into the 58 parameter gradients of its channel, for every g_sum including 0 (119 of these cases fail).
"""
import math
import os

import numpy as np
import pytest
import torch

import hyper_ref as hr

gpu = pytest.mark.gpu
GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")
CS, SEEDS = (1, 5, 12, 16), (0, 1)
NS = (1, 63, 64, 65, 257)
N_POOL = 257                     # the cases of one (C, seed) are the first n rows of one 257-row draw
N_BIG, M_BIG = 40000, 36000      # rows / subset size of the structure tests: >= 3 trips of both row loops (see _stride)
BIG = ((12, 0), (16, 0))
NOISE_SEEDS = (0, 1, 2 ** 32 + 1, 2 ** 63 - 1)
N_NODE, NODE_SEED = 300, 2 ** 32 + 5
LN2 = math.log(2.0)

# ---- tolerances -----------------------------------------------------------------------------------------------------------------
LIK_ABS = 3e-7                   # the project's bound on a likelihood: a difference of two fp32 sigmoids
TAIL_FACTOR = 4.0                # kernel's worst relative tail error over the fp32 torch composition's
GV_RTOL, GV_ATOL = 2e-3, 2e-5    # d/dv: relative + share of the largest entry (test_eb_gpu.py's ceilings)
PARAM_TOL = 3e-4                 # share of the largest entry of each parameter tensor's gradient
GRAD_SCALE = 0.3                 # measured share of the d/dv ceiling, doubled
PARAM_SCALE = 0.12               # measured share of the parameter ceiling, doubled


_worst = {}


def _report(name, value):
    """Print a measured figure when it is the worst of its kind so far (shown by pytest -s)."""
    kind = name.split("[")[0]
    if value > _worst.get(kind, -1.0):
        _worst[kind] = value
        print(f"MEASURE {name} {value:.4g}")


def _stride(n, C, blocks_per_cu):
    """Rows one trip of the row loop covers (eb_grid: min(ceil(n / 256), 256 * blocks_per_cu / C) workgroups of 256 rows per
    channel); blocks_per_cu is 3 in cgs_eb_bits_fwd and 2 in cgs_eb_bits_bwd.  C = 12: 16384 and 10752 rows."""
    return min(-(-n // 256), max(1, 256 * blocks_per_cu // C)) * 256


def _yardstick(case):
    """Worst relative error of the fp32 torch composition on the tail elements of `case`."""
    y = hr.likelihood(case.p, case.v, torch.float32).numpy()
    return float((np.abs(y - case.lik) / case.lik)[case.tail].max())


_yard = {}


def yardstick(C, seed, n):
    if (C, seed, n) not in _yard:
        _yard[(C, seed, n)] = _yardstick(hr.case(C, seed, n))
    return _yard[(C, seed, n)]


def bits_tol(case, yard):
    """Per-element tolerance of -log2(max(lik, 1e-9)): the likelihood's tolerance through the logarithm (body: 3e-7 absolute,
    tail: TAIL_FACTOR * yardstick relative, bounded: both sides sit on the bound) + 2^-21 of the value (the hardware log2 is
    good to 1 ulp, 2^-23, and a lane's fp32 running sum of at most four elements rounds at most 4 * 2^-24 of itself)."""
    t = np.where(case.body, LIK_ABS / (case.lik * LN2), np.where(case.tail, TAIL_FACTOR * yard / LN2, 0.0))
    return t + 2.0 ** -21 * case.bits


def grad_check(name, got, ref, extra=0.0):
    """|got - ref| <= GRAD_SCALE * (2e-3 |ref| + 2e-5 max|ref|) + extra, per element."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    if ref.size == 0:
        return
    assert np.isfinite(got).all(), f"{name}: {int((~np.isfinite(got)).sum())} non-finite entries"
    big = float(np.abs(ref).max())
    ceil = GV_RTOL * np.abs(ref) + GV_ATOL * big
    err = np.maximum(np.abs(got - ref) - extra, 0.0)
    if big > 0:
        _report(f"grad_share[{name}]", float((err / ceil).max()))
    assert (err <= GRAD_SCALE * ceil).all(), (name, float(err.max()), big)


def _spans():
    spans, a = {}, 0
    for n in hr.NAMES:
        w = 1 if n == "biases.4" else 9 if n.startswith("matrices") and n[-1] in "123" else 3
        spans[n] = (a, a + w)
        a += w
    assert a == 58
    return spans


def image64(g, C):
    """{name: gradient or None} -> the [C, 58] float64 image csrc/eb.hip reads and writes (the packing order of hr.NAMES)."""
    spans = _spans()
    cols = [hr._as64(g[n]).reshape(C, -1) if g[n] is not None else torch.zeros(C, spans[n][1] - spans[n][0]).double()
            for n in hr.NAMES]
    return torch.cat(cols, 1).numpy()


def param_check(name, got, ref, extra=0.0):
    """got, ref: [C, 58] images.  Per parameter tensor: |got - ref| <= PARAM_SCALE * 3e-4 * max|ref| + extra."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), f"{name}: non-finite parameter gradient"
    for n, (a, b) in _spans().items():
        big = float(np.abs(ref[:, a:b]).max())
        err = max(float(np.abs(got[:, a:b] - ref[:, a:b]).max()) - extra, 0.0)
        if big > 0:
            _report(f"param_share[{name}:{n}]", err / (PARAM_TOL * big))
        assert err <= PARAM_SCALE * PARAM_TOL * big, (name, n, err, big)


# ---- CPU: the reference itself ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [2, 7])
def test_ref_reproduces_the_reference_goldens(seed):
    """bits_and_grads in float64 against the REFERENCE's fp32 outputs (entropy_api.npz), at test_entropy_api_gpu.py's bounds.
    The goldens differentiate sum(lik * gw); the same gradient is sum(g * bits) with g = -gw * lik * ln 2 held constant."""
    import golden_inputs as gi
    g = np.load(os.path.join(GOLD_DIR, "entropy_api.npz"))
    W = gi.mlp_weights(seed)
    p = {n: torch.from_numpy(W["latent_codec." + n]).double() for n in hr.NAMES}
    v = gi.factorized_inputs(seed)
    lik = hr.likelihood(p, v).numpy()
    assert np.abs(lik - g[f"fz{seed}_lik"]).max() <= 3e-7
    assert np.abs(-np.log2(np.maximum(lik, hr.BOUND)) - g[f"fz{seed}_bits"]).max() <= 1e-4
    total, lik2, gv, gp = hr.bits_and_grads(p, v, None, -g[f"fz{seed}_gw"].astype(np.float64) * lik * LN2)
    assert np.array_equal(lik2.numpy(), lik)
    assert abs(total - float((-g[f"fz{seed}_gw"].astype(np.float64) * lik * LN2 * -np.log2(lik)).sum())) <= 1e-9 * abs(total)
    ref = g[f"fz{seed}_gv"]
    assert np.abs(gv.numpy() - ref).max() <= 2e-4 * np.abs(ref).max()
    for n in hr.NAMES:
        r = g[f"fz{seed}_g_{n}"]
        assert np.abs(gp[n].numpy() - r).max() <= 3e-4 * max(1e-6, np.abs(r).max()), n


def test_ref_noise_is_uniform_and_keyed_by_the_whole_seed():
    e = np.arange(100000)
    u = hr.noise(0, e)
    assert u.dtype == np.float32 and u.min() >= -0.5 and u.max() < 0.5
    assert np.array_equal(u.astype(np.float64) * 2 ** 24, np.round(u.astype(np.float64) * 2 ** 24))
    # mean of 1e5 uniforms: sigma = sqrt(1/12 / 1e5) = 9.1e-4; their variance: sigma = sqrt((1/80 - 1/144) / 1e5) = 2.4e-4
    assert abs(u.astype(np.float64).mean()) < 4 * 9.13e-4 and abs(u.astype(np.float64).var() - 1 / 12) < 4 * 2.36e-4
    streams = [hr.noise(s, e) for s in (0, 1, 2, 2 ** 32, 2 ** 32 + 1, 2 ** 33 + 1, 2 ** 63 - 1)]
    for i in range(len(streams)):
        for j in range(i):
            assert (streams[i] == streams[j]).mean() < 1e-3           # 24-bit values: chance equality is 6e-8 per element
    # elements past 2^32 (the high word of e enters the hash): same properties, another stream than the low word alone
    hi = hr.noise(0, e.astype(np.uint64) + np.uint64(2 ** 32))
    assert hi.min() >= -0.5 and hi.max() < 0.5 and (hi == u).mean() < 1e-3
    assert np.array_equal(hr.noise_rows(5, [3, 0], 4), hr.noise(5, [[12, 13, 14, 15], [0, 1, 2, 3]]))


def _regimes_ok(c, per_channel):
    assert int(hr.in_band(c.lik).sum()) == 0
    assert (c.body | c.tail | c.bounded).all()
    if per_channel:
        lo, up = hr.tail_logits(c.p, c.v)
        deep = ((lo < -100) & (up < -100)).numpy()
        assert (deep & c.bounded).sum(0).min() >= 1 and c.body.sum(0).min() >= 1 and c.tail.sum() >= 1
        assert c.lik[np.abs(c.v) >= 400].max() <= hr.BAND[0]


def test_inputs_leave_the_excluded_band_empty():
    """Zero elements with a float64 likelihood in (1e-10, 1e-8), for every (C, seed) the GPU tests use, and every regime
    present: bounded elements with both logits below -100 in every channel."""
    for C in CS:
        for seed in SEEDS:
            pool = hr.case(C, seed, N_POOL)
            _regimes_ok(pool, True)
            for n in NS:
                _regimes_ok(pool.head(n), n >= 63)
            planted = hr.likelihood(pool.p, np.full((1, C), 3000.0, dtype=np.float32)).numpy()
            assert planted.max() <= hr.BAND[0]                       # a planted row of 3000 sits on the bound in every channel
    for C, seed in BIG:
        _regimes_ok(hr.case(C, seed, N_BIG), True)
    for C in (5, 12):
        for permuted in (False, True):
            _regimes_ok(hr.node_case(C, 0, N_NODE, permuted, NODE_SEED)[2], True)


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------------
def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _L():
    from contextgs_amd import _lib
    return _lib, _lib.lib()


_packed_cache = {}


def packed_of(C, seed):
    if (C, seed) not in _packed_cache:
        _packed_cache[(C, seed)] = hr.make_bottleneck(C, seed).cuda()._packed_params().detach().contiguous()
    return _packed_cache[(C, seed)]


def scratch():
    _lib, L = _L()
    return torch.zeros(int(L.cgs_eb_bits_scratch_bytes()), dtype=torch.uint8, device="cuda")


def bits_fwd(v, rows, packed, ws=None):
    _lib, L = _L()
    ws = scratch() if ws is None else ws
    out = torch.full((1,), float("nan"), device="cuda")
    n = int(v.shape[0]) if rows is None else int(rows.shape[0])
    _lib.check(L.cgs_eb_bits_fwd(_lib.ptr(v), _lib.ptr(rows), _lib.ptr(packed), n, int(v.shape[1]), _lib.ptr(ws), ws.numel(),
                                 _lib.ptr(out), _lib.current_stream()), "cgs_eb_bits_fwd")
    return out


def raw_pattern(C):
    return ((torch.arange(C * 58, device="cuda") % 7).float() + 1.0).reshape(C, 58) * 0.125       # 0.125 .. 0.875, never 0


def bits_bwd(v, rows, packed, g_sum):
    """-> (g_sub [n, C] prefilled with NaN, g_raw - pattern in float64 [C, 58])."""
    _lib, L = _L()
    n, C = (int(v.shape[0]) if rows is None else int(rows.shape[0])), int(v.shape[1])
    g_sub = torch.full((n, C), float("nan"), device="cuda")
    g_raw = raw_pattern(C)
    gs = torch.tensor([g_sum], dtype=torch.float32, device="cuda")
    _lib.check(L.cgs_eb_bits_bwd(_lib.ptr(v), _lib.ptr(rows), _lib.ptr(packed), _lib.ptr(gs), n, C, _lib.ptr(g_sub),
                                 _lib.ptr(g_raw), _lib.current_stream()), "cgs_eb_bits_bwd")
    return g_sub.cpu().numpy(), (g_raw.double() - raw_pattern(C).double()).cpu().numpy()


def noise_gather(x, perm, seed, out=None):
    _lib, L = _L()
    out = torch.full_like(x, float("nan")) if out is None else out
    _lib.check(L.cgs_hyper_noise_gather(_lib.ptr(x), _lib.ptr(perm), int(x.shape[0]), int(x.shape[1]), int(seed), _lib.ptr(out),
                                        _lib.current_stream()), "cgs_hyper_noise_gather")
    return out


def subset_of(n, rng):
    """A random distinct subset of range(n), unsorted, about 40 % of the rows (at least one)."""
    return rng.permutation(n)[:max(1, (2 * n) // 5)].astype(np.int64)


# ---- GPU: noise gather ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("n", [1, 63, 257, 4099])
def test_noise_gather_is_the_integer_generator_bit_for_bit(C, n):
    """out == x[perm] + u(seed, perm[r] * C + c) as float32; n = 4099 runs the float4 kernel's grid-stride loop four times
    at C = 12 (4099 * 3 float4 over 4 workgroups of 256)."""
    rng = np.random.default_rng(n * 100 + C)
    x = (rng.normal(size=(n, C)) * 4).astype(np.float32)
    perm = rng.permutation(n).astype(np.int64)
    xd, pd = T(x), T(perm)
    for seed in NOISE_SEEDS:
        ident = noise_gather(xd, None, seed)
        assert torch.equal(ident.cpu(), torch.from_numpy(x + hr.noise_rows(seed, np.arange(n), C))), (seed, "identity")
        out = noise_gather(xd, pd, seed)
        assert torch.equal(out.cpu(), torch.from_numpy(x[perm] + hr.noise_rows(seed, perm, C))), (seed, "perm")
        assert torch.equal(out, ident[pd])


@gpu
@pytest.mark.parametrize("n", [63, 4099])
def test_noise_gather_misaligned_base_equals_aligned(n):
    """C = 12 from a base one float past a 16-byte boundary (input, output, both): the scalar kernel, same bits."""
    C, seed = 12, 2 ** 32 + 1
    rng = np.random.default_rng(n)
    x = (rng.normal(size=(n, C)) * 4).astype(np.float32)
    perm = T(rng.permutation(n).astype(np.int64))
    want = noise_gather(T(x), perm, seed)
    assert torch.equal(want.cpu(), torch.from_numpy(x[perm.cpu().numpy()] + hr.noise_rows(seed, perm.cpu().numpy(), C)))
    shifted = torch.zeros(n * C + 1, device="cuda")
    shifted[1:] = T(x).reshape(-1)
    xs = shifted[1:].view(n, C)
    assert xs.data_ptr() % 16 == 4 and xs.is_contiguous()
    assert torch.equal(noise_gather(xs, perm, seed), want)
    outbuf = torch.full((n * C + 1,), float("nan"), device="cuda")
    assert torch.equal(noise_gather(T(x), perm, seed, out=outbuf[1:].view(n, C)), want)
    outbuf.fill_(float("nan"))
    assert torch.equal(noise_gather(xs, perm, seed, out=outbuf[1:].view(n, C)), want) and bool(torch.isnan(outbuf[0]))


@gpu
@pytest.mark.parametrize("permuted", [False, True])
def test_noisy_latents_launched_ahead_are_the_nodes_own(permuted):
    C, seed = 12, 2 ** 63 - 1
    eb = hr.make_bottleneck(C, 0).cuda()
    x, perm, _ = hr.node_case(C, 0, N_NODE, permuted, NODE_SEED)
    xd = T(x)
    pd = None if perm is None else T(perm)
    inv = None if perm is None else T(np.argsort(perm).astype(np.int64))
    rows = T(subset_of(N_NODE, np.random.default_rng(3)))
    with torch.no_grad():
        _, noisy, s = eb.noisy_latents_launch(xd, pd, seed)
        v1, b1 = eb.training_step_forms(xd, pd, inv, rows, s, noisy=noisy)
        v2, b2 = eb.training_step_forms(xd, pd, inv, rows, seed)
    order = np.arange(N_NODE) if perm is None else perm
    assert torch.equal(v1, noisy) and torch.equal(v1, v2) and torch.equal(b1.total, b2.total) and b1.numel == b2.numel == rows.numel() * C
    assert torch.equal(v2.cpu(), torch.from_numpy(x[order] + hr.noise_rows(seed, order, C)))


# ---- GPU: likelihood and bit sum, values ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("seed", SEEDS)
def test_likelihood_per_element_in_every_regime(C, seed):
    """cgs_eb_likelihood_fwd (the arithmetic the bit sum shares) per element: body 3e-7 absolute, tail relative to float64 within
    TAIL_FACTOR times the fp32 torch composition's worst error, bounded exactly on the bound."""
    from contextgs_amd.entropy_bottleneck import fused_likelihood
    c = hr.case(C, seed, N_POOL)
    lik = fused_likelihood(T(c.v), packed_of(C, seed)).cpu().numpy().astype(np.float64)
    assert np.isfinite(lik).all()
    yard = yardstick(C, seed, N_POOL)
    rel = (np.abs(lik - c.lik) / c.lik)[c.tail].max()
    _report(f"body_abs[{C},{seed}]", np.abs(lik - c.lik)[c.body].max())
    _report(f"tail_yardstick[{C},{seed}]", yard)
    _report(f"tail_ratio[{C},{seed}]", rel / yard)
    assert np.abs(lik - c.lik)[c.body].max() <= LIK_ABS
    assert rel <= TAIL_FACTOR * yard
    assert (lik[c.bounded] == np.float64(np.float32(1e-9))).all()


@gpu
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("seed", SEEDS)
def test_bits_fwd_value_against_fp64(C, seed):
    pool, yard, packed = hr.case(C, seed, N_POOL), yardstick(C, seed, N_POOL), packed_of(C, seed)
    rng = np.random.default_rng(C * 10 + seed)
    worst = 0.0
    for n in NS:
        c = pool.head(n)
        vd = T(c.v)
        for rows in (None, subset_of(n, rng)):
            s = c if rows is None else c.take(rows)
            got = float(bits_fwd(vd, None if rows is None else T(rows), packed))
            want = float(s.bits.sum())
            tol = float(bits_tol(s, yard).sum()) + 2.0 ** -23 * want            # + the result's rounding to float
            worst = max(worst, abs(got - want) / tol)
            assert abs(got - want) <= tol, (n, rows is None, got, want, tol)
    _report(f"bits_sum_share[{C},{seed}]", worst)
    out = bits_fwd(torch.empty(0, C, device="cuda"), None, packed)
    assert float(out) == 0.0 and not math.copysign(1.0, float(out)) < 0


# ---- GPU: bit sum, structure ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C,seed", BIG)
def test_bits_fwd_rows_prefetch_repeat_and_ticket(C, seed):
    """At 40000 rows (36000 in the subset) the forward's row loop makes three trips or more: one trip covers
    min(ceil(n / 256), 768 / C) * 256 rows (eb_grid with 3 workgroups per CU): 16384 at C = 12, 12288 at C = 16."""
    stride = _stride(N_BIG, C, 3)
    assert stride == {12: 16384, 16: 12288}[C] and M_BIG > 2 * _stride(M_BIG, C, 3) and _stride(M_BIG, C, 3) == stride
    c, packed = hr.case(C, seed, N_BIG), packed_of(C, seed)
    vd = T(c.v)
    rows = np.random.default_rng(C).permutation(N_BIG)[:M_BIG].astype(np.int64)
    rd = T(rows)
    # the subset through the index == the compacted subset without one: same grid, same lanes, only the gather differs
    through = bits_fwd(vd, rd, packed)
    compact = bits_fwd(vd[rd].contiguous(), None, packed)
    assert torch.equal(through, compact), (float(through), float(compact))
    assert torch.equal(bits_fwd(vd, rd, packed), through)
    # one scratch buffer across calls of different grids: the arrival ticket is left at zero
    ws = scratch()
    small1, small63 = T(c.v[:1]), T(c.v[:63])
    for arg in (small1, vd, small63, vd):
        assert torch.equal(bits_fwd(arg, None, packed, ws), bits_fwd(arg, None, packed)), int(arg.shape[0])
    assert torch.equal(bits_fwd(vd, rd, packed, ws), through)


@gpu
@pytest.mark.parametrize("C,seed", BIG)
def test_bits_fwd_planted_row_is_counted_once(C, seed):
    """Row k replaced by 3000 in every channel (on the bound everywhere): the sum rises by C log2(1e9) - bits64(row k), for k at
    both ends of the rows, either side of the first trip's end, and the first and last entry of a subset."""
    c, packed, yard = hr.case(C, seed, N_BIG), packed_of(C, seed), yardstick(C, seed, N_BIG)
    tol_el = bits_tol(c, yard)
    stride = _stride(N_BIG, C, 3)
    rows = np.random.default_rng(C).permutation(N_BIG)[:M_BIG].astype(np.int64)
    vd, rd = T(c.v), T(rows)
    top = math.log2(1e9)
    for which, index, ks in (("all", None, (0, stride - 1, stride, N_BIG - 1)), ("subset", rd, (int(rows[0]), int(rows[-1])))):
        base = float(bits_fwd(vd, index, packed))
        for k in ks:
            v2 = vd.clone()
            v2[k, :] = 3000.0
            got = float(bits_fwd(v2, index, packed)) - base
            want = C * top - float(c.bits[k].sum())
            tol = float(tol_el[k].sum()) + C * 2.0 ** -21 * top + 2.0 ** -22 * base
            _report(f"planted_share[{C},{which},{k}]", abs(got - want) / tol)
            assert abs(got - want) <= tol, (which, k, got, want, tol)


# ---- GPU: backward ----------------------------------------------------------------------------------------------------------------
def _check_bits_bwd(tag, c, rows, packed, g_sum, C):
    s = c if rows is None else c.take(rows)
    g_sub, g_raw = bits_bwd(T(c.v), None if rows is None else T(rows), packed, g_sum)
    assert not np.isnan(g_sub).any(), f"{tag}: g_sub keeps {int(np.isnan(g_sub).sum())} NaN (unwritten or computed)"
    assert np.isfinite(g_sub).all() and np.isfinite(g_raw).all(), tag
    _, _, gv, gp = hr.bits_and_grads(c.p, c.v, rows, g_sum)
    if g_sum <= 0:
        assert (g_sub[s.bounded] == 0).all(), tag             # blocked, as _LowerBound blocks them
    if g_sum == 0:
        assert (g_sub == 0).all() and (g_raw == 0).all(), tag
        return
    grad_check(tag, g_sub, gv.numpy())                        # row r of g_sub belongs to rows[r]
    n = s.v.shape[0]
    blocks = min(-(-n // 256), max(1, 512 // C))              # atomics per entry of g_raw; each rounds pattern + partial sum
    param_check(tag, g_raw, image64(gp, C), extra=blocks * 2.0 ** -24 * 0.875)


@gpu
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("g_sum", [1.5, -1.5, 0.0])
def test_bits_bwd_against_fp64(C, seed, g_sum):
    pool, packed = hr.case(C, seed, N_POOL), packed_of(C, seed)
    rng = np.random.default_rng(C * 10 + seed)
    for n in NS:
        c = pool.head(n)
        for rows in (None, subset_of(n, rng)):
            _check_bits_bwd(f"bits_bwd[{C},{seed},{g_sum},{n},{'all' if rows is None else 'subset'}]", c, rows, packed, g_sum, C)


@gpu
@pytest.mark.parametrize("C,seed", BIG)
def test_bits_bwd_many_trips_against_fp64(C, seed):
    """36000 of 40000 rows: four trips of the backward's row loop at C = 12 (10752 rows a trip), five at C = 16 (8192)."""
    assert M_BIG > 3 * _stride(M_BIG, C, 2) and _stride(M_BIG, C, 2) == {12: 10752, 16: 8192}[C]
    rows = np.random.default_rng(C).permutation(N_BIG)[:M_BIG].astype(np.int64)
    _check_bits_bwd(f"bits_bwd_big[{C}]", hr.case(C, seed, N_BIG), rows, packed_of(C, seed), 1.5, C)


@gpu
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("seed", SEEDS)
def test_likelihood_bwd_bounded_and_extreme_inputs(C, seed):
    """cgs_eb_likelihood_bwd on the same three regimes with upstream gradients of both signs: finite everywhere, bounded
    elements blocked exactly where the gradient would push the likelihood further down, float64 elsewhere."""
    from contextgs_amd.entropy_bottleneck import fused_likelihood
    c = hr.case(C, seed, N_POOL)
    g = np.random.default_rng(seed).normal(size=c.v.shape).astype(np.float32)
    v = T(c.v).requires_grad_(True)
    packed = packed_of(C, seed).clone().requires_grad_(True)
    (fused_likelihood(v, packed) * T(g)).sum().backward()
    gv, gp = hr.likelihood_grads(c.p, c.v, g)
    got = v.grad.cpu().numpy()
    assert np.isfinite(got).all() and bool(torch.isfinite(packed.grad).all())
    assert (got[c.bounded & (g > 0)] == 0).all()
    grad_check(f"lik_bwd[{C},{seed}]", got, gv.numpy())
    param_check(f"lik_bwd[{C},{seed}]", packed.grad.cpu().numpy(), image64(gp, C))


# ---- GPU: the node ----------------------------------------------------------------------------------------------------------------
class Node:
    """One forward of training_step_forms on node_case's latents, with everything the checks need."""

    def __init__(self, C, permuted, rows_mode, sizes=None, with_rows_orig=True):
        self.C, self.sizes = C, sizes
        self.x_np, self.perm, self.case = hr.node_case(C, 0, N_NODE, permuted, NODE_SEED)
        self.order = np.arange(N_NODE) if self.perm is None else self.perm
        self.rows = {"subset": subset_of(N_NODE, np.random.default_rng(11)), "none": None,
                     "empty": np.zeros(0, dtype=np.int64)}[rows_mode]
        self.eb = hr.make_bottleneck(C, 0).cuda()
        self.p = hr.params(C, 0)
        self.x = T(self.x_np).requires_grad_(True)
        pd = None if self.perm is None else T(self.perm)
        inv = None if self.perm is None else T(np.argsort(self.perm).astype(np.int64))
        rd = None if self.rows is None else T(self.rows)
        ro = None if (self.rows is None or self.perm is None or not with_rows_orig) else T(self.perm[self.rows])
        self.out, self.bits = self.eb.training_step_forms(self.x, pd, inv, rd, NODE_SEED, sizes=sizes, rows_orig=ro)
        rng = np.random.default_rng(5)
        self.w = rng.normal(size=(N_NODE, C)).astype(np.float32)           # the dense gradient, in coding order

    def check_forward(self):
        v = torch.cat(list(self.out)) if isinstance(self.out, tuple) else self.out
        assert torch.equal(v.detach().cpu(), torch.from_numpy(self.case.v))
        s = self.case if self.rows is None else self.case.take(self.rows)
        yard = _yardstick(self.case)
        want = float(s.bits.sum())
        assert abs(float(self.bits.total.detach()) - want) <= float(bits_tol(s, yard).sum()) + 2.0 ** -23 * want
        assert self.bits.numel == s.v.shape[0] * self.C

    def check_grads(self, tag, dense_rows, a):
        """dense_rows: bool [N] in coding order, the rows whose gradient w reached the node; a: weight of the bits or None."""
        N, C = N_NODE, self.C
        weights = [np.where(dense_rows[:, None], self.w, 0).astype(np.float32)]
        _, _, gx, gp = hr.step_ref(self.p, self.x_np, self.perm, NODE_SEED, None, weights, self.rows, a)
        got = self.x.grad.cpu().numpy()
        assert np.isfinite(got).all(), tag
        dense = np.zeros((N, C), dtype=np.float32)
        dense[self.order] = weights[0]                                     # the torch gather of the incoming gradients
        in_sub = np.zeros(N, dtype=bool)
        if a is not None:
            in_sub[self.order if self.rows is None else self.order[self.rows]] = True
        assert np.array_equal(got[~in_sub], dense[~in_sub]), tag           # bit-equal off the subset
        if in_sub.any():
            ref_sub = gx.numpy()[in_sub] - dense[in_sub]
            grad_check(tag, got[in_sub].astype(np.float64) - dense[in_sub], ref_sub,
                       extra=2.0 ** -23 * np.abs(gx.numpy()[in_sub]))     # the fp32 sum dense + g_sub rounds once
        grads = {k: q.grad for k, q in self.eb.named_parameters() if k in hr.NAMES}
        if a is None or (self.rows is not None and len(self.rows) == 0):
            assert all(g is None or not bool(g.any()) for g in grads.values()), tag
        else:
            param_check(tag, image64(grads, C), image64(gp, C))


@gpu
@pytest.mark.parametrize("C", [5, 12])
@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("rows_mode", ["subset", "none", "empty"])
@pytest.mark.parametrize("parts", ["dense+bits", "dense", "bits"])
@pytest.mark.parametrize("sizes", [None, (60, 60, 60, 60, 60)])
def test_node_plain_route(C, permuted, rows_mode, parts, sizes):
    """sizes None, and five blocks (more than the block route takes: the node falls back to one tensor)."""
    nd = Node(C, permuted, rows_mode, sizes)
    assert torch.is_tensor(nd.out)
    nd.check_forward()
    seen = []
    if "dense" in parts:
        nd.out.register_hook(lambda g: seen.append(g))
    obj = 0.0
    if "dense" in parts:
        obj = obj + (nd.out * T(nd.w)).sum()
    a = 1.5 if "bits" in parts else None
    if a is not None:
        obj = obj + a * nd.bits.total.sum()
    obj.backward(retain_graph=True)
    tag = f"plain[{C},{permuted},{rows_mode},{parts},{sizes is not None}]"
    dense_rows = np.full(N_NODE, "dense" in parts)
    nd.check_grads(tag, dense_rows, a)
    first = nd.x.grad.clone()
    incoming = [g.clone() for g in seen]
    nd.x.grad = None
    nd.eb.zero_grad()
    obj.backward()                                                       # a second pass over the retained graph
    assert torch.equal(nd.x.grad, first), tag
    if "dense" in parts:
        assert torch.equal(incoming[0], T(nd.w)) and torch.equal(seen[0], T(nd.w)), tag       # the incoming buffer is not summed into


@gpu
def test_node_unused_leaves_no_gradient():
    nd = Node(12, True, "subset")
    other = torch.ones(3, device="cuda", requires_grad=True)
    (other * 2).sum().backward()
    assert nd.x.grad is None and all(q.grad is None for q in nd.eb.parameters())


def _blocks_objective(nd, used, cat_block, a, rng):
    """Objective over the blocks `used` (block cat_block through a cat with another tensor, so that its gradient arrives as a
    strided column slice) -> (objective, dense_rows)."""
    begin = np.concatenate([[0], np.cumsum(nd.sizes)])
    dense_rows = np.zeros(N_NODE, dtype=bool)
    obj = 0.0
    for j in used:
        blk, w = nd.out[j], T(nd.w[begin[j]:begin[j + 1]])
        if j == cat_block:
            other = T(rng.normal(size=(nd.sizes[j], 3)).astype(np.float32))
            both = torch.cat([blk, other], 1) * torch.cat([w, other], 1)
            obj = obj + both.sum()
        else:
            obj = obj + (blk * w).sum()
        dense_rows[begin[j]:begin[j + 1]] = True
    if a is not None:
        obj = obj + a * nd.bits.total.sum()
    return obj, dense_rows


@gpu
@pytest.mark.parametrize("C", [5, 12])
@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("sizes,used,cat_block,a", [
    ((100, 0, 120, 80), (0, 2), 2, 1.5),          # block 3 unused (None), block 2 as a column slice
    ((100, 0, 120, 80), (0, 2, 3), 0, None),      # bits unused
    ((150, 0, 150), (), None, 1.5),               # no block used: the subset's rows alone
    ((150, 0, 150), (2,), 2, -1.5),
])
def test_node_block_route(C, permuted, sizes, used, cat_block, a):
    nd = Node(C, permuted, "subset", sizes)
    assert isinstance(nd.out, tuple) and [int(b.shape[0]) for b in nd.out] == list(sizes)
    nd.check_forward()
    obj, dense_rows = _blocks_objective(nd, used, cat_block, a, np.random.default_rng(1))
    obj.backward()
    nd.check_grads(f"blocks[{C},{permuted},{sizes},{used},{a}]", dense_rows, a)


@gpu
def test_node_block_route_without_rows_orig_and_identity_order():
    """perm None needs no rows_orig (the subset's positions are its rows)."""
    nd = Node(12, False, "subset", (100, 0, 120, 80), with_rows_orig=False)
    assert isinstance(nd.out, tuple)
    obj, dense_rows = _blocks_objective(nd, (0, 3), None, 1.5, np.random.default_rng(1))
    obj.backward()
    nd.check_grads("blocks[no rows_orig]", dense_rows, 1.5)


@gpu
@pytest.mark.parametrize("C", [5, 12])
@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("done,used,cat_block", [
    ((0, 2, 3), (), None),          # every non-empty block written by its level
    ((0, 3), (2,), 2),              # a mix: block 2 comes back through autograd
    ((2,), (0,), None),             # block 3 neither done nor used
    ((), (0, 2, 3), 0),             # a buffer was created, nothing marked done: ignored
])
def test_node_direct_route(C, permuted, done, used, cat_block):
    """A fused level stands in for autograd: it writes its rows of the latents' gradient into the holder's buffer, in the
    latents' own row order, and marks its block done; the block is then left out of the objective."""
    sizes = (100, 0, 120, 80)
    nd = Node(C, permuted, "subset", sizes)
    begin = np.concatenate([[0], np.cumsum(sizes)])
    holder = None
    for j, blk in enumerate(nd.out):
        h, jj = blk._cgs_hyp_direct
        assert jj == j and (holder is None or h is holder)
        holder = h
    buf = holder.buffer(nd.x.device)
    buf.fill_(float("nan"))                                           # rows nobody writes must not be read
    obj, dense_rows = _blocks_objective(nd, used, cat_block, 1.5, np.random.default_rng(1))
    for j in done:
        buf[T(nd.order[begin[j]:begin[j + 1]])] = T(nd.w[begin[j]:begin[j + 1]])
        holder.done.add(j)
        dense_rows[begin[j]:begin[j + 1]] = True
    obj.backward()
    nd.check_grads(f"direct[{C},{permuted},{done},{used}]", dense_rows, 1.5)
