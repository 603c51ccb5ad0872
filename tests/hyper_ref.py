"""fp64 / integer restatement of the hyper prior's training forms (a helper, not a test).

Written from the definitions, not from the kernels:
  1. noise: a counter-based generator.  mix(x) is the 32-bit xor-shift-multiply permutation
         x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16        (mod 2^32)
     key(seed, t) = mix(low32(seed) ^ 0x9E3779B9 (t + 1)) ^ high32(seed), the hyper latents are tensor t = 3, and element
     e = original_row * C + c draws h = mix(low32(e) + key + high32(e) * 0x632BE5AB) and u = (h >> 8) 2^-24 - 1/2: 24 uniform
     bits, a multiple of 2^-24 in [-1/2, 1/2).  Integer arithmetic throughout, so the values are exact.
  2. bits: sum over the rows `rows` of v and all channels of -log2(max(likelihood, 1e-9)), the likelihood being the package's
     own torch statement of the factorised density (interval_likelihood, pinned to the reference by
     tests/golden/entropy_api.npz) evaluated in float64, the bound being _LowerBound (gradient blocked below the bound unless it
     pushes the likelihood up).
  3. step: v = x[perm] + u keyed by the original row, blocks = split(v, sizes), objective sum_j <w_j, block_j> + a * bits.
and the inputs of the GPU tests: three regimes of the likelihood (body, tail, bounded), none in the band (1e-10, 1e-8) that fp32
and fp64 can not classify alike.
"""
import functools

import numpy as np
import torch

BOUND = 1e-9
BAND = (1e-10, 1e-8)          # likelihoods the inputs avoid
_M32 = np.uint64(0xFFFFFFFF)


def _mix(x):
    x = x & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def noise_key(seed, tensor=3):
    seed = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    golden = np.uint64((0x9E3779B9 * (int(tensor) + 1)) & 0xFFFFFFFF)
    return _mix((seed & _M32) ^ golden) ^ (seed >> np.uint64(32))


def noise(seed, e):
    """u(seed, e) as float32 for every element index e (any integer array < 2^64)."""
    e = np.asarray(e).astype(np.uint64)
    h = _mix((e & _M32) + noise_key(seed) + (((e >> np.uint64(32)) * np.uint64(0x632BE5AB)) & _M32))
    return ((h >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24) - np.float32(0.5)).astype(np.float32)


def noise_rows(seed, rows, C):
    """u [len(rows), C] of the latents' rows `rows` (ORIGINAL row numbers)."""
    rows = np.asarray(rows).astype(np.uint64)
    return noise(seed, rows[:, None] * np.uint64(C) + np.arange(C, dtype=np.uint64)[None, :])


# ---- density ------------------------------------------------------------------------------------------------------------------
NAMES = tuple(n for i in range(5) for n in ((f"matrices.{i}", f"biases.{i}") + ((f"factors.{i}",) if i < 4 else ())))


def params64(eb):
    """The 14 parameter tensors of an EntropyBottleneck as float64 CPU copies: {name: tensor} in packing order."""
    src = dict(eb.named_parameters())
    return {n: src[n].detach().double().cpu().clone() for n in NAMES}


def _groups(p):
    return ([p[f"matrices.{i}"] for i in range(5)], [p[f"biases.{i}"] for i in range(5)], [p[f"factors.{i}"] for i in range(4)])


def _as64(a):
    return (a.detach().cpu() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).double()


def _density(p, v, dtype=torch.float64):
    """(likelihood, lower logit, upper logit), each [n, C], of v [n, C] in `dtype` (no bound)."""
    from contextgs_amd.entropy_bottleneck import cumulative_logits, interval_likelihood
    n, C = v.shape
    m, b, f = _groups({k: t.to(dtype) for k, t in p.items()})
    x = v.to(dtype).t().reshape(C, 1, n)
    back = lambda t: t.reshape(C, n).t()
    return (back(interval_likelihood(m, b, f, x, 0.5)), back(cumulative_logits(m, b, f, x - 0.5)),
            back(cumulative_logits(m, b, f, x + 0.5)))


def likelihood(p, v, dtype=torch.float64):
    """Unbounded likelihood [n, C] of v in `dtype` (float32: the yardstick of the tail tolerance), returned as float64."""
    with torch.no_grad():
        return _density(p, _as64(v), dtype)[0].double()


def tail_logits(p, v):
    """The two logits the sigmoids see, s * lower and s * upper with s = -sign(lower + upper), in float64."""
    with torch.no_grad():
        _, lo, up = _density(p, _as64(v))
        s = -torch.sign(lo + up)
        return s * lo, s * up


def bits_and_grads(p, v, rows, g_sum):
    """(sum over v[rows] of g_sum * -log2(max(lik, 1e-9)), lik [n, C] unbounded, d/dv[rows] [n, C], {name: gradient}) in
    float64.  g_sum: a number, or per-element weights [n, C]."""
    from contextgs_amd.entropy_bottleneck import _LowerBound
    q = {k: t.clone().requires_grad_(True) for k, t in p.items()}
    v = _as64(v)
    sub = (v if rows is None else v[torch.as_tensor(np.asarray(rows), dtype=torch.int64)]).clone().requires_grad_(True)
    lik = _density(q, sub)[0]
    bits = -torch.log2(_LowerBound.apply(lik, BOUND))
    total = (bits * (g_sum if not isinstance(g_sum, np.ndarray) else torch.from_numpy(g_sum).double())).sum()
    if sub.numel():
        total.backward()
    g = {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in q.items()}
    return float(total.detach()), lik.detach(), (sub.grad if sub.grad is not None else torch.zeros_like(sub)), g


def likelihood_grads(p, v, g_lik):
    """Gradients of sum(g_lik * max(lik, 1e-9)) (the fused likelihood's backward): (d/dv [n, C], {name: gradient})."""
    from contextgs_amd.entropy_bottleneck import _LowerBound
    q = {k: t.clone().requires_grad_(True) for k, t in p.items()}
    x = _as64(v).clone().requires_grad_(True)
    (_LowerBound.apply(_density(q, x)[0], BOUND) * _as64(g_lik)).sum().backward()
    return x.grad, {k: t.grad for k, t in q.items()}


def step_ref(p, x, perm, seed, sizes, weights, rows_pos, a):
    """The whole node in float64 autograd.  x [N, C] float32 latents; perm: coding order (None: identity); weights: one
    [size_j, C] array (or None) per block of split(v, sizes) (sizes None: one block); rows_pos: positions of the rate subset
    in coding order (None: all rows); a: weight of the bit sum (None: the bits are not used).
    The noisy latents are the float32 sum x[perm] + u (what the node hands on), carried in float64.
    -> (v float32 [N, C], bits, d objective / dx [N, C], {name: gradient})."""
    from contextgs_amd.entropy_bottleneck import _LowerBound
    x32 = np.ascontiguousarray(x, dtype=np.float32)
    N, C = x32.shape
    order = np.arange(N) if perm is None else np.asarray(perm)
    v32 = (x32[order] + noise_rows(seed, order, C)).astype(np.float32)
    q = {k: t.clone().requires_grad_(True) for k, t in p.items()}
    xd = torch.from_numpy(x32).double().requires_grad_(True)
    xp = xd[torch.from_numpy(order)]
    v = xp + (torch.from_numpy(v32).double() - xp.detach())           # == v32 exactly, d v / d x = the gather
    obj = v.sum() * 0.0
    for w, blk in zip(weights, torch.split(v, list(sizes) if sizes is not None else [N])):
        if w is not None:
            obj = obj + (blk * _as64(w)).sum()
    sub = v if rows_pos is None else v[torch.as_tensor(np.asarray(rows_pos), dtype=torch.int64)]
    bits = -torch.log2(_LowerBound.apply(_density(q, sub)[0], BOUND)).sum() if sub.numel() else v.sum() * 0.0
    if a is not None:
        obj = obj + a * bits
    obj.backward()
    return v32, float(bits.detach()), xd.grad, {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in q.items()}


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def make_bottleneck(C, seed):
    """The parameter sets of the tests: a default EntropyBottleneck(C) with matrices and factors perturbed by 0.3 randn."""
    from contextgs_amd.entropy_bottleneck import EntropyBottleneck
    torch.manual_seed(100 * C + seed)
    eb = EntropyBottleneck(C)
    with torch.no_grad():
        for q in list(eb.matrices) + list(eb.factors):
            q.add_(0.3 * torch.randn_like(q))
    return eb


def _draw(rng, n, C):
    """Element (r, c) is drawn for the regime (7 r + c) mod 4: 0, 1 body |x| <= 12, 2 tail 30 <= |x| <= 90, 3 bounded
    400 <= |x| <= 3000 (exactly 3000 in rows r with (r // 4) even: every channel owns one among its first four rows)."""
    r, c = np.arange(n)[:, None], np.arange(C)[None, :]
    regime = (7 * r + c) % 4
    sign = np.where(rng.random((n, C)) < 0.5, -1.0, 1.0)
    body, body2 = rng.uniform(-12, 12, (n, C)), rng.uniform(-12, 12, (n, C))
    tail = sign * rng.uniform(30, 90, (n, C))
    far = sign * np.where((r // 4) % 2 == 0, 3000.0, np.exp(rng.uniform(np.log(400.0), np.log(3000.0), (n, C))))
    return np.where(regime < 2, body, np.where(regime == 2, tail, far)).astype(np.float32), body2.astype(np.float32)


def in_band(lik):
    return (lik > BAND[0]) & (lik < BAND[1])


class Case:
    """v [n, C] float32 with its float64 likelihood and the regime of every element."""

    def __init__(self, p, v):
        self.p, self.v = p, v
        self.lik = likelihood(p, v).numpy()
        self.body, self.tail, self.bounded = self.lik >= 1e-3, (self.lik >= BAND[1]) & (self.lik < 1e-3), self.lik <= BAND[0]
        self.bits = -np.log2(np.maximum(self.lik, BOUND))

    def take(self, rows):
        """The case of the rows `rows` (an index array or a slice)."""
        c = Case.__new__(Case)
        c.p = self.p
        for k in ("v", "lik", "body", "tail", "bounded", "bits"):
            setattr(c, k, getattr(self, k)[rows])
        return c

    def head(self, n):
        return self.take(slice(0, n))


@functools.lru_cache(maxsize=None)
def params(C, seed):
    return params64(make_bottleneck(C, seed))


@functools.lru_cache(maxsize=None)
def case(C, seed, n):
    """The values the kernels are called on directly: n rows in the three regimes, band elements redrawn as body values."""
    p = params(C, seed)
    v, body2 = _draw(np.random.default_rng(1000 * C + 10 * seed + 1), n, C)
    band = in_band(likelihood(p, v).numpy())
    v[band] = body2[band]
    return Case(p, v)


@functools.lru_cache(maxsize=None)
def node_case(C, seed, N, permuted, noise_seed):
    """Latents x [N, C] for the node: the noisy latents v = x[perm] + u are what the regimes and the band refer to.
    -> (x float32, perm int64 or None, Case of v)."""
    p = params(C, seed)
    rng = np.random.default_rng(1000 * C + 10 * seed + 2)
    x, body2 = _draw(rng, N, C)
    perm = rng.permutation(N).astype(np.int64) if permuted else None
    order = np.arange(N) if perm is None else perm
    u = noise_rows(noise_seed, order, C)
    band = in_band(likelihood(p, x[order] + u).numpy())
    x[order[np.nonzero(band)[0]], np.nonzero(band)[1]] = body2[band]
    return x, perm, Case(p, (x[order] + u).astype(np.float32))
