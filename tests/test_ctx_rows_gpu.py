"""The row movers, row accumulators and element-wise noise kernels of csrc/ctx.hip on every dispatch path, through the C ABI, against
tests/ctx_rows_ref.py (numpy; float64 wherever anything is summed): rowcat forward and backward, the unique-row gather and its sorted
scatter, add_rows, the mark / zero-unmarked pair, the segmented gather, the CSR parent sums and noise_quant with its mean accumulators.

Conventions.  Every output is carved from a NaN-filled allocation with 8 guard rows in front and behind (`Out`), which must still be
NaN afterwards; rows a call must not touch hold a sentinel and must keep it.  An unaligned base is a slice of a flat tensor that
starts 1 float (4-byte aligned) or 2 floats (8-byte, not 16-byte aligned) in; its result equals the aligned one bit for bit (both equal
the one numpy reference).  Index lists hit row 0 and the last row of their source and hold repeats where those are legal.  Every input
is inside its entry point's contract.  One case per kernel sits just above the count at which its launcher's grid reaches the
4096-workgroup cap (ctx_rows_ref.SECOND_TRIP), every other case is small.

Dispatch (ctx.hip; `_rowcat_path`, `_rows_form`, ctx_rows_ref.nq_vec2 / nq_bwd_fast restate it, and every case asserts the path it is
listed under):
  cgs_rowcat_fwd[_masked]  :248  one source with idx, no mask, W % 4 == 0, ld % 4 == 0, src and out 16-byte aligned -> rowgather4_kernel
                           :256  2..4 sources, 16 <= W <= 256, n >= 128, out 16-byte aligned -> rowcat_fwd_lds_kernel; :259 bit s of
                                 pair_mask: width and ld even, base 8-byte aligned (float2 loads), else scalar loads
                           :264  everything else -> rowcat_fwd_kernel (one element per lane, four per trip)
  cgs_rowcat_bwd[_masked]  :286  rowcat_bwd_kernel; per source mode 0 skip, 1 store, 2 atomicAdd
  cgs_gather_rows          :443  w == 3 / 1 -> gather_rows_row_kernel<W>; :447 w % 4 == 0 and x, out 16-byte aligned -> <float4>;
                           :450  w % 2 == 0 and 8-byte aligned -> <float2>; :454 else <float>
  cgs_scatter_rows_sorted  :385  n == 0 -> hipMemsetAsync; :392-405 the same four forms as the gather
  cgs_noise_quant_fwd      :716  nq_vec2_ok (D, S, O even, D <= 64, S, O <= 32, the six bases 8-byte aligned) -> noise_quant_fwd2_kernel,
                                 else noise_quant_fwd_kernel
  cgs_noise_quant_bwd      :738  D <= 64, S <= 16, O <= 32 -> noise_quant_bwd_kernel<true>, else <false>
  cgs_ctx_gather_bwd[_acc] :1047 (wa, DF, DS) == (3, 50, 6) and ldo >= 64 -> ctx_gather_bwd4_kernel, else :1053 ctx_gather_bwd_kernel
  cgs_add_rows, cgs_mark_rows, cgs_zero_unmarked_rows, cgs_gather_rows_segmented, cgs_means_finalize: one kernel each

Bounds (none is taken from a kernel's result; `pytest -s` prints the maxima as [rows-bounds] lines):
  data movement, one product, one add       equality, bit for bit (the sign of zero counts)
  rowcat mode 2, exactly summable terms     equality with the fp64 sum (integers in +-2^10 times 2^-8: every partial sum is exact)
  rowcat mode 2, normal terms               (k - 1) u sum |terms| around the fp64 sum, k the row's number of terms
  CSR sums                                  equality with the sequential float32 sum in child order, and (k - 1) u sum |terms| (+ u |result|
                                            where the accumulate bit adds what the buffer held) around the fp64 sum
  Q, d qadj                                 13.2 units of ctx_level_ref.Head / Backward's units (UNITS_KERNEL_LEVEL, the limit of
                                            test_ctx_level_fp64_gpu.py) with U(qadj) = 0; rows of Head.ambiguous_clamp are left out (their
                                            share stays below ctx_rows_ref.AMBIGUOUS_CAP = 2 %); exactly 0 where Head.flat
  y                                         u (|x + n Q| + |n Q|) around x + n Q in fp64, n the integer generator's noise, Q the kernel's own
  means                                     t u sum |v| / count, t the float32 terms of one lane

Measured maxima as a fraction of the bound (MI355X, 256 CUs, 258 tests, 7.6 s for the whole file, the slowest test 1.5 s):
  rowcat_bwd mode 2, normal terms   0.9989
  CSR sums against fp64             1.0000 (rounded: no element is outside) for both kernels, the same figure since both give the
                                    same bits; every element equals the sequential float32 sum
  noise_quant Q                     0.0792 of 13.2 units = 1.05 units
  noise_quant d qadj                0.0878 of 13.2 units = 1.16 units
  noise_quant y                     0.9998
  means                             0.0600; a second round differs from the first by 0.0000
Every equality held on the first run: no kernel had to change.  (One mistake of this file's own showed at 262 149 rows: the checks
"Q is the clamp" and "d qadj is exactly 0" took in the rows of Head.ambiguous_clamp, where float32 may open the gate that fp64 closes;
they now leave those rows out as the unit checks do.)

That the tests bite (each alteration built once into a copy of the library outside the source tree, this file run once on it; arithmetic
only, no index, bound or address changed; the product library passes all 258):
  1. noise_quant_bwd_kernel, `1.f - t * t` -> `1.f - t`: 36 fail, every test that runs the backward (test_noise_quant_bwd_both_kernels
     12 / 12, _each_cotangent_null 16 / 16, _row_counts 6 / 6, test_noise_quant_second_trip[2], the wrapper test), on d qadj.
  2. ctx_gather_bwd4_kernel, the clamped duplicate of the last child added again: 35 fail, every test that reaches the four-parent
     kernel (test_csr_sums_four_parent_kernel 21 / 21, _accumulate_bits 8 / 8 at ldo 64, _each_output_null 3 / 3 at ldo 71,
     _both_kernels_agree_bit_for_bit, _second_trip[ctx_gather_bwd4-64], test_ctx_assemble_backward_is_the_sequential_sum), none that
     reaches the generic one; the parents whose child count is a multiple of 4 still agree.  The select sits in two places: dropping
     `if (k + u < e)` on the add alone changes nothing, because the loaded row is zeroed by the same condition one statement earlier
     (`ok`), so the alteration drops it there too.
  3. noise_quant_fwd2_kernel, `ef + 32` -> `ef + 31`: 18 fail (test_noise_quant_fwd_both_kernels 15 / 30: the three shapes that take the
     float2 kernel at all five row counts, on y and on the equality with the scalar kernel; test_noise_quant_seeds,
     test_noise_quant_second_trip[2], the wrapper test); the scalar kernel's cases pass.
  4. rowcat_bwd_kernel, `atomicAdd(p, gv)` -> `*p = gv` in mode 2: 4 fail (test_rowcat_bwd_atomics_sum_exactly_summable_terms_exactly,
     test_rowcat_bwd_atomics_within_the_summation_bound, test_rowcat_bwd_second_trip, test_rowcat_autograd_node_chooses_modes_and_fills).
No alteration went uncaught.
"""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import ctx_rows_ref as rr
from ctx_rows_ref import Q0, SEED, U

pytestmark = pytest.mark.gpu
GUARD = 8
NAN = float("nan")
SENTINEL = -7.25                       # (a multiple of 2^-8: the exactly summable sums stay exact on top of it)
MAXIMA = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(MAXIMA.items()):
        print(f"[rows-bounds] {k:34s} {v:.4f} of its bound")


def _note(name, frac, limit=1.0):
    worst = float(np.max(frac, initial=0.0))
    MAXIMA[name] = max(MAXIMA.get(name, 0.0), worst / limit)
    return worst


def _api():
    from contextgs_amd import _lib
    return _lib, _lib.lib(), _lib.current_stream()


def _ok(rc, what):
    from contextgs_amd import _lib
    _lib.check(rc, what)


def _rng(*key):
    return np.random.default_rng([zlib.crc32(k.encode()) if isinstance(k, str) else int(k) for k in key])


def dev(a, off=0):
    """A numpy array on the device, its base `off` elements into a fresh allocation."""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a if a.flags.writeable else a.copy())
    if not off:
        return t.cuda()
    flat = torch.zeros(t.numel() + off + 4, dtype=t.dtype, device="cuda")
    v = flat[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * off) % 16 and v.is_contiguous()
    return v


class Out:
    """[rows, width] float32 inside a NaN-filled allocation: GUARD rows in front and behind, the body `off` floats past a 16-byte
    boundary, filled with `fill` (NaN: every element must be written; a number: the value an untouched element keeps)."""

    def __init__(self, rows, width, fill=NAN, off=0):
        self.lo = off + GUARD * width
        self.hi = self.lo + rows * width
        self.flat = torch.full((self.hi + GUARD * width + 4,), NAN, dtype=torch.float32, device="cuda")
        self.t = self.flat[self.lo:self.hi].view(rows, width)
        assert self.t.data_ptr() % 16 == (4 * off) % 16
        if isinstance(fill, np.ndarray):
            self.t.copy_(torch.from_numpy(fill))
        elif fill == fill:
            self.t.fill_(fill)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self, what=""):
        assert bool(torch.isnan(self.flat[:self.lo]).all()), (what, "a guard row in front of the buffer was written")
        assert bool(torch.isnan(self.flat[self.hi:]).all()), (what, "a guard row behind the buffer was written")
        return self.t.cpu().numpy()


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError((what, "differs in", int(bad.sum()), "elements; first at", at, float(got[at]), float(want[at])))


def _vp(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def _ci(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def _p(t):
    return None if t is None else t.data_ptr()


# ==== a. cgs_rowcat_fwd / _fwd_masked ================================================================================================
class Src:
    """A source of `rows` rows: columns [col, col + width) of a [rows, ld] array whose base lies `off` floats past a 16-byte boundary."""

    def __init__(self, rng, n, width, rows=40, ld=None, col=0, off=0, idx="rep", mask=False):
        self.rows = rows = n if idx is None else rows
        self.width, self.ld, self.col = width, ld or width, col
        assert col + width <= self.ld
        wide = rng.normal(size=(rows, self.ld)).astype(np.float32)
        self.wide = dev(wide, off)
        self.x = wide[:, col:col + width]
        self.ptr = self.wide.data_ptr() + 4 * col
        self.idx = None if idx is None else rr.draw_idx(rng, n, rows, repeats=(idx == "rep"))
        self.idx_t = None if idx is None else dev(self.idx)
        self.mask = None
        if mask:
            self.mask = (rng.random(rows) < 0.7).astype(np.uint8)
            self.mask[[0, rows - 1]] = (0, 1)
        self.mask_t = None if self.mask is None else dev(self.mask)

    @property
    def part(self):
        return (self.x, self.idx, self.mask)


def S(width, **kw):
    return (width, kw)


def _rowcat_path(srcs, n, out_ptr):
    W = sum(s.width for s in srcs)
    s0 = srcs[0]
    if len(srcs) == 1 and s0.idx is not None and s0.mask is None and W % 4 == 0 and s0.ld % 4 == 0 and (s0.ptr | out_ptr) % 16 == 0:
        return "rowgather4"
    if len(srcs) >= 2 and 16 <= W <= 256 and n >= 4 * rr.RC_ROWS and out_ptr % 16 == 0:
        pm = sum(1 << k for k, s in enumerate(srcs) if s.width % 2 == 0 and s.ld % 2 == 0 and s.ptr % 8 == 0)
        return f"lds:{pm:04b}"
    return "element"


def _rowcat_fwd(srcs, n, out_off=0, masked=None):
    _lib, L, st = _api()
    W = sum(s.width for s in srcs)
    out = Out(n, W, off=out_off)
    masked = any(s.mask is not None for s in srcs) if masked is None else masked
    head = (len(srcs), _vp([s.ptr for s in srcs]), _vp([_p(s.idx_t) for s in srcs]))
    tail = (_ci([s.width for s in srcs]), _ci([s.ld for s in srcs]), n, out.ptr, st)
    if masked:
        _ok(L.cgs_rowcat_fwd_masked(*head, _vp([_p(s.mask_t) for s in srcs]), *tail), "cgs_rowcat_fwd_masked")
    else:
        _ok(L.cgs_rowcat_fwd(*head, *tail), "cgs_rowcat_fwd")
    return out, _rowcat_path(srcs, n, out.ptr)


def _rowcat_case(name, n, specs, out_off=0):
    rng = _rng("rowcat", name, n)
    srcs = [Src(rng, n, w, **kw) for w, kw in specs]
    out, path = _rowcat_fwd(srcs, n, out_off)
    same_bits(out.get(name), rr.rowcat([s.part for s in srcs], n), name)
    return path


CTX71 = [S(3), S(50), S(6), S(12, idx=None)]
ROWCAT_CASES = {
    # ---- the element kernel
    "elem n=127 of the level's row":   (127, CTX71, 0, "element"),
    "elem 2 sources W=9":              (300, [S(4), S(5)], 0, "element"),
    "elem W=15 masked":                (200, [S(3, mask=True), S(12, idx=None)], 0, "element"),
    "elem W=257":                      (130, [S(129), S(128, idx=None)], 0, "element"),
    "elem strided":                    (200, [S(3, ld=7, col=2), S(6, ld=9, col=1, idx=None)], 0, "element"),
    "elem 1 source W=5":               (300, [S(5)], 0, "element"),
    "elem 1 source no idx W=8":        (300, [S(8, idx=None)], 0, "element"),
    "elem 3 sources":                  (64, [S(1), S(2, mask=True), S(7, idx=None)], 0, "element"),
    "elem out on a 4-byte base":       (160, CTX71, 1, "element"),
    "elem out on an 8-byte base":      (160, CTX71, 2, "element"),
    # ---- the LDS kernel
    "lds W=71 n=128":                  (128, CTX71, 0, "lds:1110"),
    "lds W=71 n=129 (R W % 4 = 3)":    (129, CTX71, 0, "lds:1110"),
    "lds W=71 n=160":                  (160, CTX71, 0, "lds:1110"),
    "lds W=71 n=32 k + 17":            (177, CTX71, 0, "lds:1110"),
    "lds W=16 every source paired":    (129, [S(2), S(4), S(10, idx=None)], 0, "lds:0111"),
    "lds W=256 no source paired":      (160, [S(127), S(129, idx=None)], 0, "lds:0000"),
    "lds W=256 paired":                (161, [S(128), S(64), S(62), S(2, idx=None)], 0, "lds:1111"),
    "lds mixed pair_mask":             (177, [S(6), S(5), S(8, off=1), S(4, ld=7, idx=None)], 0, "lds:0001"),
    "lds 8-byte base stays paired":    (177, [S(6, off=2), S(11), S(8, idx=None, off=2)], 0, "lds:0101"),
    "lds strided":                     (160, [S(3, ld=5, col=1), S(50, ld=60, col=4), S(6, ld=8, col=2), S(12, idx=None)], 0, "lds:1110"),
    "lds strided odd column":          (160, [S(50, ld=60, col=3), S(12, ld=16, col=4, idx=None)], 0, "lds:0010"),
    "lds masked":                      (177, [S(4, mask=True), S(51, mask=True), S(12, idx=None)], 0, "lds:0101"),
    "lds 2 sources no idx":            (130, [S(9, idx=None), S(8, idx=None)], 0, "lds:0010"),
    # ---- rowgather4 and its fall-backs
    "rg4 W=4":                         (300, [S(4, rows=200)], 0, "rowgather4"),
    "rg4 W=12":                        (300, [S(12, rows=200)], 0, "rowgather4"),
    "rg4 W=64":                        (300, [S(64, rows=200)], 0, "rowgather4"),
    "rg4 strided ld=8":                (300, [S(4, rows=200, ld=8, col=4)], 0, "rowgather4"),
    "rg4 W=12 ld=13 falls back":       (300, [S(12, rows=200, ld=13)], 0, "element"),
    "rg4 W=4 source 4-byte base":      (300, [S(4, rows=200, off=1)], 0, "element"),
    "rg4 W=12 source 8-byte base":     (300, [S(12, rows=200, off=2)], 0, "element"),
    "rg4 W=64 out 8-byte base":        (300, [S(64, rows=200)], 2, "element"),
    "rg4 W=12 odd column":             (300, [S(12, rows=200, ld=16, col=3)], 0, "element"),
    "rg4 masked falls back":           (300, [S(12, rows=200, mask=True)], 0, "element"),
}


@pytest.mark.parametrize("name", list(ROWCAT_CASES))
def test_rowcat_fwd_every_path(name):
    n, specs, out_off, path = ROWCAT_CASES[name]
    assert _rowcat_case(name, n, specs, out_off) == path


@pytest.mark.parametrize("kernel", ["rowcat_fwd", "rowcat_fwd_lds", "rowgather4"])
def test_rowcat_fwd_second_trip(kernel):
    if kernel == "rowcat_fwd":
        n, specs, path = rr.rows_for(kernel, 9), [S(4, rows=1000), S(5, rows=999, mask=True)], "element"
    elif kernel == "rowcat_fwd_lds":
        n, specs, path = rr.second_trip(kernel), [S(3, rows=1000), S(50, rows=777), S(6, rows=777), S(12, idx=None)], "lds:1110"
    else:
        n, specs, path = rr.rows_for(kernel, 4), [S(4, rows=1000)], "rowgather4"
    assert _rowcat_case(kernel, n, specs) == path


def test_rowcat_fwd_empty_call_and_unmasked_entry():
    rng = _rng("rowcat empty")
    srcs = [Src(rng, 5, 3), Src(rng, 5, 12, idx=None)]
    _lib, L, st = _api()
    out = Out(4, 15)
    for entry in ("masked", "plain"):
        head = (2, _vp([s.ptr for s in srcs]), _vp([_p(s.idx_t) for s in srcs]))
        tail = (_ci([3, 12]), _ci([3, 12]), 0, out.ptr, st)
        rc = L.cgs_rowcat_fwd_masked(*head, None, *tail) if entry == "masked" else L.cgs_rowcat_fwd(*head, *tail)
        _ok(rc, "an empty rowcat")
    assert np.isnan(out.get("empty")).all()
    # the masked entry with a NULL mask list, and with a list of NULL masks, is the plain one
    for masks in (None, _vp([None, None])):
        o = Out(5, 15)
        _ok(L.cgs_rowcat_fwd_masked(2, _vp([s.ptr for s in srcs]), _vp([_p(s.idx_t) for s in srcs]), masks, _ci([3, 12]), _ci([3, 12]), 5,
                                    o.ptr, st), "cgs_rowcat_fwd_masked")
        same_bits(o.get(), rr.rowcat([s.part for s in srcs], 5), "NULL masks")


def test_rowcat_wrappers_choose_the_same_rows():
    from contextgs_amd import ctx_ops
    rng = _rng("rowcat wrappers")
    n = 177
    srcs = [Src(rng, n, 3, mask=True), Src(rng, n, 50), Src(rng, n, 6), Src(rng, n, 12, idx=None)]
    out = ctx_ops.rowcat([(s.wide, s.idx_t, False) + ((s.mask_t,) if s.mask is not None else ()) for s in srcs])
    same_bits(out.cpu().numpy(), rr.rowcat([s.part for s in srcs], n), "ctx_ops.rowcat")
    for w in (12, 10, 3):
        s = Src(rng, 300, w, rows=200)
        same_bits(ctx_ops.gather_rows_nograd(s.wide, s.idx_t).cpu().numpy(), rr.gather_rows(s.x, s.idx), ("gather_rows_nograd", w))


# ==== b. cgs_rowcat_bwd / _bwd_masked ===============================================================================================
def _rowcat_bwd(n, parts, dout, fill, masked=None):
    """parts: (rows, width, ld, col, idx, mask, mode) -> per source the [rows, ld] array afterwards (its other columns checked)."""
    _lib, L, st = _api()
    bufs = [Out(rows, ld, fill=fill) for rows, w, ld, col, idx, mask, mode in parts]
    keep = [dev(dout)] + [None if p[4] is None else dev(p[4]) for p in parts] + [None if p[5] is None else dev(p[5]) for p in parts]
    k = len(parts)
    masked = any(p[5] is not None for p in parts) if masked is None else masked
    head = (k, _vp([b.ptr + 4 * p[3] for b, p in zip(bufs, parts)]), _vp([_p(t) for t in keep[1:1 + k]]))
    tail = (_ci([p[1] for p in parts]), _ci([p[2] for p in parts]), _ci([p[6] for p in parts]), n, keep[0].data_ptr(), st)
    if masked:
        _ok(L.cgs_rowcat_bwd_masked(*head, _vp([_p(t) for t in keep[1 + k:]]), *tail), "cgs_rowcat_bwd_masked")
    else:
        _ok(L.cgs_rowcat_bwd(*head, *tail), "cgs_rowcat_bwd")
    got = []
    for b, (rows, w, ld, col, idx, mask, mode) in zip(bufs, parts):
        a = b.get("rowcat_bwd")
        rest = np.ones(ld, bool)
        rest[col:col + w] = False
        same_bits(a[:, rest], np.full((rows, int(rest.sum())), fill, np.float32), "a column outside the source's slice changed")
        got.append(a[:, col:col + w])
    return got


def _ref_parts(parts):
    return [(rows, w, idx, mask, mode) for rows, w, ld, col, idx, mask, mode in parts]


def test_rowcat_bwd_store_skip_and_strides():
    rng = _rng("rowcat bwd store")
    n = 200
    mask = (rng.random(300) < 0.6).astype(np.uint8)
    parts = [(300, 3, 5, 1, rr.draw_idx(rng, n, 300, repeats=False), mask, 1), (40, 50, 50, 0, rr.draw_idx(rng, n, 40), None, 0),
             (n, 6, 9, 2, None, None, 1), (n, 12, 12, 0, None, None, 1)]
    dout = rng.normal(size=(n, 71)).astype(np.float32)
    got = _rowcat_bwd(n, parts, dout, SENTINEL)
    want = rr.rowcat_bwd(dout, _ref_parts(parts), n, SENTINEL)
    for k, (g, w) in enumerate(zip(got, want)):
        same_bits(g, np.full_like(g, SENTINEL) if w is None else w, ("source", k))          # mode 0: untouched
    # the unmasked entry point
    plain = [p[:5] + (None,) + p[6:] for p in parts]
    for k, (g, w) in enumerate(zip(_rowcat_bwd(n, plain, dout, SENTINEL, masked=False), rr.rowcat_bwd(dout, _ref_parts(plain), n, SENTINEL))):
        same_bits(g, np.full_like(g, SENTINEL) if w is None else w, ("plain source", k))


def _mode2_parts(rng, rows):
    idx = rr.draw_occurrences(rng, rows)
    n = len(idx)
    mask = (rng.random(rows) < 0.7).astype(np.uint8)
    mask[[0, rows - 1]] = 1
    parts = [(rows, 3, 3, 0, idx, mask, 2), (rows, 50, 53, 2, idx, None, 2), (rows, 6, 6, 0, idx[rng.permutation(n)], None, 2),
             (n, 12, 12, 0, None, None, 1)]
    return n, parts


def test_rowcat_bwd_atomics_sum_exactly_summable_terms_exactly():
    rng = _rng("rowcat bwd exact")
    n, parts = _mode2_parts(rng, 400)
    dout = rr.draw_summable(rng, (n, 71))
    for p in parts[:3]:
        assert rr.exactly_summable(dout[:, :p[1]], p[4], p[0])
    got = _rowcat_bwd(n, parts, dout, SENTINEL)
    want = rr.rowcat_bwd(dout, _ref_parts(parts), n, SENTINEL)
    for k in range(3):
        s, a, cnt = want[k]
        assert set(rr.OCCURRENCES) <= set(cnt.tolist())
        same_bits(got[k], (SENTINEL + s).astype(np.float32), ("mode 2, exactly summable, source", k))
        same_bits(got[k][cnt == 0], np.full((int((cnt == 0).sum()), parts[k][1]), SENTINEL, np.float32), "an unlisted row changed")
    same_bits(got[3], want[3], "mode 1 next to mode 2")


def test_rowcat_bwd_atomics_within_the_summation_bound():
    rng = _rng("rowcat bwd normal")
    n, parts = _mode2_parts(rng, 400)
    dout = rng.normal(size=(n, 71)).astype(np.float32)
    got = _rowcat_bwd(n, parts, dout, 0.0)
    want = rr.rowcat_bwd(dout, _ref_parts(parts), n, 0.0)
    for k in range(3):
        s, a, cnt = want[k]
        frac = rr.fraction(np.abs(got[k] - s), rr.sum_bound(a, cnt), ("mode 2 source", k))        # bound 0 at k <= 1: exact
        assert _note("rowcat_bwd mode 2", frac) <= 1.0
        assert not np.signbit(got[k][cnt == 0]).any() and (got[k][cnt == 0] == 0).all()


def test_rowcat_bwd_second_trip():
    rng = _rng("rowcat bwd big")
    n = rr.rows_for("rowcat_bwd", 12)
    rows = 100_000
    idx = rr.draw_idx(rng, n, rows)
    mask = (rng.random(rows) < 0.7).astype(np.uint8)
    parts = [(rows, 3, 3, 0, idx, mask, 2), (n, 9, 9, 0, None, None, 1)]
    dout = rr.draw_summable(rng, (n, 12))
    assert rr.exactly_summable(dout[:, :3], idx, rows)
    got = _rowcat_bwd(n, parts, dout, SENTINEL)
    want = rr.rowcat_bwd(dout, _ref_parts(parts), n, SENTINEL)
    same_bits(got[0], (SENTINEL + want[0][0]).astype(np.float32), "mode 2 above the grid cap")
    same_bits(got[1], want[1], "mode 1 above the grid cap")


def test_rowcat_autograd_node_chooses_modes_and_fills():
    from contextgs_amd import ctx_ops
    rng = _rng("rowcat node")
    rows = 400
    idx = rr.draw_occurrences(rng, rows)
    n = len(idx)
    a, f = (torch.from_numpy(rng.normal(size=(rows, w)).astype(np.float32)).cuda().requires_grad_() for w in (3, 50))
    own = torch.from_numpy(rng.normal(size=(n, 12)).astype(np.float32)).cuda().requires_grad_()
    d = torch.from_numpy(rng.normal(size=(n + 50, 6)).astype(np.float32)).cuda().requires_grad_()
    didx = rr.draw_idx(rng, n, n + 50, repeats=False)
    out = ctx_ops.rowcat([(a, dev(idx), False), (f, dev(idx), False), (own, None, True), (d, dev(didx), True)])
    dout = rr.draw_summable(rng, tuple(out.shape))
    out.backward(dev(dout))
    ref = rr.rowcat_bwd(dout, [(rows, 3, idx, None, 2), (rows, 50, idx, None, 2), (n, 12, None, None, 1), (n + 50, 6, didx, None, 1)], n, 0.0)
    same_bits(a.grad.cpu().numpy(), ref[0][0].astype(np.float32), "rowcat node, repeated rows")
    same_bits(f.grad.cpu().numpy(), ref[1][0].astype(np.float32), "rowcat node, repeated rows")
    same_bits(own.grad.cpu().numpy(), ref[2], "rowcat node, identity rows")
    same_bits(d.grad.cpu().numpy(), ref[3], "rowcat node, distinct rows: zeros elsewhere")


# ==== c. cgs_gather_rows / cgs_scatter_rows_sorted ===================================================================================
ROW_W, VEC4_W, VEC2_W, GEN_W = (1, 3), (4, 12, 64, 256), (2, 10, 30, 254), (5, 7, 129, 255)


def _rows_form(w, *ptrs):
    al = 0
    for p in ptrs:
        al |= p
    if w in (1, 3):
        return "row"
    if w % 4 == 0 and al % 16 == 0:
        return "float4"
    if w % 2 == 0 and al % 8 == 0:
        return "float2"
    return "generic"


def _gather(x, idx, w, x_off=0, out_off=0):
    _lib, L, st = _api()
    xt, it = dev(x, x_off), dev(idx)
    out = Out(len(idx), w, off=out_off)
    _ok(L.cgs_gather_rows(xt.data_ptr(), it.data_ptr(), len(idx), w, out.ptr, st), "cgs_gather_rows")
    return out.get(("gather", w)), _rows_form(w, xt.data_ptr(), out.ptr)


def _scatter(g, idx, N, w, g_off=0, out_off=0):
    _lib, L, st = _api()
    gt, it = dev(g, g_off), dev(idx)
    out = Out(N, w, off=out_off)
    _ok(L.cgs_scatter_rows_sorted(_p(gt) if len(idx) else None, _p(it) if len(idx) else None, len(idx), N, w, out.ptr, st),
        "cgs_scatter_rows_sorted")
    return out.get(("scatter", w)), _rows_form(w, gt.data_ptr(), out.ptr)


@pytest.mark.parametrize("w,form", [(w, f) for ws, f in ((ROW_W, "row"), (VEC4_W, "float4"), (VEC2_W, "float2"), (GEN_W, "generic")) for w in ws])
def test_gather_and_scatter_every_width(w, form):
    rng = _rng("rows", w)
    N = 500
    x = rng.normal(size=(N, w)).astype(np.float32)
    for idx in (rr.draw_sorted(rng, N, "dense"), rr.draw_idx(rng, 333, N, repeats=False), rr.draw_idx(rng, 1, N)):
        got, path = _gather(x, idx, w)
        assert path == form
        same_bits(got, rr.gather_rows(x, idx), ("gather", w))
    idx = rr.draw_sorted(rng, N, "dense")
    g = rng.normal(size=(len(idx), w)).astype(np.float32)
    got, path = _scatter(g, idx, N, w)
    assert path == form
    same_bits(got, rr.scatter_sorted(g, idx, N), ("scatter", w))


@pytest.mark.parametrize("w", [12, 10])
@pytest.mark.parametrize("side", ["in", "out", "both"])
@pytest.mark.parametrize("off", [1, 2])
def test_gather_and_scatter_fall_back_on_unaligned_bases(off, side, w):
    """float4 -> float2 -> scalar as the base loses alignment: the same bits as on an aligned base."""
    rng = _rng("rows unaligned", w)
    N = 500
    x = rng.normal(size=(N, w)).astype(np.float32)
    idx = rr.draw_sorted(rng, N, "dense")
    io, oo = (off if side in ("in", "both") else 0), (off if side in ("out", "both") else 0)
    form = "generic" if off == 1 else "float2"
    aligned, base_form = _gather(x, idx, w)
    got, path = _gather(x, idx, w, io, oo)
    assert path == form and base_form == ("float4" if w == 12 else "float2")
    same_bits(got, aligned, ("gather", w, off, side))
    same_bits(got, rr.gather_rows(x, idx), ("gather", w, off, side))
    g = rng.normal(size=(len(idx), w)).astype(np.float32)
    aligned, _ = _scatter(g, idx, N, w)
    got, path = _scatter(g, idx, N, w, io, oo)
    assert path == form
    same_bits(got, aligned, ("scatter", w, off, side))
    same_bits(got, rr.scatter_sorted(g, idx, N), ("scatter", w, off, side))


@pytest.mark.parametrize("w", [3, 12, 10, 7])
@pytest.mark.parametrize("kind", ["dense", "eighth", "first", "last", "all", "gap", "none"])
def test_scatter_sorted_lists(kind, w):
    rng = _rng("scatter lists", w)
    N = 100_777 if kind == "gap" else 1000
    idx = rr.draw_sorted(rng, N, kind)
    assert (kind != "all" or len(idx) == N) and (kind != "none" or len(idx) == 0)
    g = rng.normal(size=(len(idx), w)).astype(np.float32)
    got, _ = _scatter(g, idx, N, w)
    same_bits(got, rr.scatter_sorted(g, idx, N), (kind, w))


@pytest.mark.parametrize("name,w,form", [("row", 3, "row"), ("vec4_w12", 12, "float4"), ("generic_w7", 7, "generic")])
def test_gather_and_scatter_second_trip(name, w, form):
    rng = _rng("rows big", w)
    n = rr.second_trip("gather_" + name)
    N = n + 1000
    keep = np.ones(N, bool)
    keep[rng.integers(1, N - 1, 900)] = False                                    # (at least n + 100 rows stay listed)
    idx = np.nonzero(keep)[0][:n].astype(np.int64)
    idx[-1] = N - 1
    assert len(idx) == n == rr.second_trip("scatter_" + name) and (np.diff(idx) > 0).all()
    x = rng.normal(size=(N, w)).astype(np.float32)
    got, path = _gather(x, idx, w)
    assert path == form
    same_bits(got, x[idx], ("gather above the grid cap", w))
    got2, path = _scatter(got, idx, N, w)
    assert path == form
    same_bits(got2, rr.scatter_sorted(x[idx], idx, N), ("scatter above the grid cap", w))


# ==== d. cgs_add_rows, cgs_mark_rows / cgs_zero_unmarked_rows, cgs_gather_rows_segmented =============================================
def _add_rows(out0, idx, g):
    _lib, L, st = _api()
    out = Out(out0.shape[0], out0.shape[1], fill=out0)
    gt, it = dev(g), dev(idx)
    _ok(L.cgs_add_rows(gt.data_ptr(), it.data_ptr(), len(idx), out0.shape[0], out0.shape[1], out.ptr, st), "cgs_add_rows")
    return out.get("add_rows")


@pytest.mark.parametrize("w", [1, 3, 12, 256])
def test_add_rows_is_one_add_per_element(w):
    rng = _rng("add rows", w)
    N = 500
    out0 = rng.normal(size=(N, w)).astype(np.float32)
    for n in (300, 1, N):
        idx = rr.draw_idx(rng, n, N, repeats=False)
        g = rng.normal(size=(n, w)).astype(np.float32)
        same_bits(_add_rows(out0, idx, g), rr.add_rows(out0, idx, g), ("add_rows", w, n))


def test_add_rows_second_trip_and_wrapper():
    from contextgs_amd import ctx_ops
    rng = _rng("add rows big")
    n = rr.rows_for("add_rows", 3)
    N = n + 100
    out0 = rng.normal(size=(N, 3)).astype(np.float32)
    idx = rr.draw_idx(rng, n, N, repeats=False)
    g = rng.normal(size=(n, 3)).astype(np.float32)
    want = rr.add_rows(out0, idx, g)
    same_bits(_add_rows(out0, idx, g), want, "add_rows above the grid cap")
    t = dev(out0[:1000].reshape(1000, 1, 3))
    sub = rr.draw_idx(rng, 400, 1000, repeats=False)
    assert ctx_ops.add_rows_(t, dev(sub), dev(g[:400].reshape(400, 1, 3))) is t
    same_bits(t.cpu().numpy().reshape(1000, 3), rr.add_rows(out0[:1000], sub, g[:400]), "ctx_ops.add_rows_")


def _stamps(n_full):
    """A zeroed uint32 stamp array between two guards of 8 entries."""
    flat = torch.full((n_full + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    flat[8:8 + n_full] = 0
    return flat, flat[8:8 + n_full]


def _stamp_values(flat, n_full, what):
    a = flat.cpu().numpy().view(np.uint32)
    assert (a[:8] == 0x5A5A5A5A).all() and (a[8 + n_full:] == 0x5A5A5A5A).all(), (what, "a stamp outside the array was written")
    return a[8:8 + n_full]


def _mark_and_zero(flat, stamp, idx, gen, n_full, arrays0):
    _lib, L, st = _api()
    it = dev(idx)
    _ok(L.cgs_mark_rows(it.data_ptr(), len(idx), n_full, gen, stamp.data_ptr(), st), "cgs_mark_rows")
    outs = [Out(n_full, a.shape[1], fill=a) for a in arrays0]
    _ok(L.cgs_zero_unmarked_rows(stamp.data_ptr(), gen, n_full, len(outs), _vp([o.ptr for o in outs]), _ci([a.shape[1] for a in arrays0]), st),
        "cgs_zero_unmarked_rows")
    return _stamp_values(flat, n_full, gen), [o.get(("zero_unmarked", gen)) for o in outs]


@pytest.mark.parametrize("narr", [1, 2, 3, 4])
def test_mark_and_zero_unmarked_rows(narr):
    rng = _rng("mark", narr)
    n_full = 1000
    arrays0 = [rng.normal(size=(n_full, w)).astype(np.float32) + 3 for w in (6, 30, 1, 3)[:narr]]
    flat, stamp = _stamps(n_full)
    want_stamp = np.zeros(n_full, np.uint32)
    for gen, n in ((1, 700), (2, 40), (2 ** 32 - 1, 990)):
        idx = np.concatenate([rr.draw_idx(rng, n, n_full, repeats=False), [-1, n_full, n_full + 7, -(2 ** 40), 2 ** 40]]).astype(np.int64)
        idx = idx[rng.permutation(len(idx))]
        got_stamp, got = _mark_and_zero(flat, stamp, idx, gen, n_full, arrays0)
        want_stamp = rr.mark(want_stamp, idx, gen)                               # (stamps of earlier generations stay: stale)
        assert np.array_equal(got_stamp, want_stamp), ("stamps", gen)
        assert (want_stamp != gen).sum() == n_full - n
        for a, b in zip(got, rr.zero_unmarked(want_stamp, gen, arrays0)):
            same_bits(a, b, ("zero_unmarked", gen, narr))
    # an empty list marks nothing: every row is zeroed
    got_stamp, got = _mark_and_zero(flat, stamp, np.zeros(0, np.int64), 7, n_full, arrays0)
    assert np.array_equal(got_stamp, want_stamp) and all(not a.any() and not np.signbit(a).any() for a in got)


def test_mark_and_zero_unmarked_rows_second_trip_and_wrapper():
    from contextgs_amd import ctx_ops
    rng = _rng("mark big")
    n_full = rr.second_trip("zero_unmarked_rows")
    assert n_full == rr.second_trip("mark_rows")
    idx = rng.permutation(n_full).astype(np.int64)
    out_of_range = rng.random(n_full) < 0.1
    out_of_range[[0, n_full - 1]] = True                                         # (the ends of the LIST: the row loop's first and last entry)
    idx[out_of_range] += n_full
    a0 = (rng.random((n_full, 1)) + 1).astype(np.float32)
    flat, stamp = _stamps(n_full)
    got_stamp, (got,) = _mark_and_zero(flat, stamp, idx, 3, n_full, [a0])
    want_stamp = rr.mark(np.zeros(n_full, np.uint32), idx, 3)
    assert np.array_equal(got_stamp, want_stamp) and 0.05 < (want_stamp == 0).mean() < 0.15
    same_bits(got, rr.zero_unmarked(want_stamp, 3, [a0])[0], "zero_unmarked above the grid cap")
    # the wrapper: five arrays are two launches; the listed rows keep what they held
    n5 = 3000
    listed = rr.draw_idx(rng, 2000, n5, repeats=False)
    arrays0 = [rng.normal(size=(n5,) + s).astype(np.float32) + 3 for s in ((6,), (10, 3), (50,), (1,), (3,))]
    ts = [dev(a) for a in arrays0]
    ctx_ops.zero_unlisted_rows(dev(listed), n5, ts)
    st = rr.mark(np.zeros(n5, np.uint32), listed, 1)
    for t, a in zip(ts, arrays0):
        same_bits(t.cpu().numpy().reshape(n5, -1), rr.zero_unmarked(st, 1, [a.reshape(n5, -1)])[0], "ctx_ops.zero_unlisted_rows")


SEG_CASES = {
    "1 block":              ([("dense", 37)], True),
    "2 blocks no idx":      ([("dense", 37), ("strided", 100)], False),
    "NULL first":           ([("null", 50), ("dense", 37), ("strided", 100)], True),
    "NULL in the middle":   ([("dense", 37), ("null", 50), ("strided", 100), ("dense", 1)], True),
    "NULL last":            ([("strided", 100), ("dense", 37), ("null", 50)], True),
    "an empty block":       ([("dense", 37), ("empty", 0), ("strided", 100), ("null", 3)], True),
    "empty first and last": ([("empty", 0), ("dense", 5), ("dense", 9), ("empty", 0)], True),
    "4 blocks no idx":      ([("dense", 1), ("null", 2), ("strided", 3), ("dense", 4)], False),
}


def _segmented(name, blocks, with_idx, w=12, big=False):
    _lib, L, st = _api()
    rng = _rng("segmented", name)
    np_blocks, ptrs, lds, keep, begin = [], [], [], [], [0]
    for kind, size in blocks:
        begin.append(begin[-1] + size)
        if kind in ("null", "empty"):
            np_blocks.append(None if kind == "null" else np.zeros((0, w), np.float32))
            ptrs.append(None)
            lds.append(w)
            continue
        ld, col = (71, 59) if kind == "strided" else (w, 0)
        wide = rng.normal(size=(size, ld)).astype(np.float32)
        t = dev(wide)
        keep.append(t)
        np_blocks.append(wide[:, col:col + w])
        ptrs.append(t.data_ptr() + 4 * col)
        lds.append(ld)
    N = begin[-1]
    idx = None
    if with_idx:
        n = rr.rows_for("gather_segmented", w) if big else N + 40
        idx = rng.integers(0, N, n).astype(np.int64)
        ends = [b for k, (kind, size) in enumerate(blocks) if size for b in (begin[k], begin[k + 1] - 1)]       # first and last row of every block
        idx[rng.permutation(n)[:len(ends)]] = ends
    n = N if idx is None else len(idx)
    out = Out(n, w)
    k = len(blocks)
    it = None if idx is None else dev(idx)
    _ok(L.cgs_gather_rows_segmented(k, _vp(ptrs), (C.c_int64 * k)(*lds), (C.c_int64 * (k + 1))(*begin), _p(it), n, w, out.ptr, st),
        "cgs_gather_rows_segmented")
    same_bits(out.get(name), rr.gather_segmented(np_blocks, [s for _, s in blocks], idx, w), name)


@pytest.mark.parametrize("name", list(SEG_CASES))
def test_gather_rows_segmented(name):
    _segmented(name, *SEG_CASES[name])


def test_gather_rows_segmented_second_trip():
    _segmented("big", [("dense", 5000), ("null", 300), ("strided", 7000), ("dense", 11)], True, big=True)


# ==== e. cgs_ctx_gather_bwd / _acc ===================================================================================================
REF_SHAPE = (3, 50, 6)
_CSR_DOUT = {}


def _csr_dout(c, W, seed=0):
    key = (c.n_par, c.n_child, W, seed)
    if key in _CSR_DOUT:
        return _CSR_DOUT[key]
    a = np.random.default_rng([c.n_par, W, seed, 5]).normal(size=(c.n_child, W)).astype(np.float32)
    a.setflags(write=False)
    ref = (a, rr.csr_seq32(a, c.offs, c.order), rr.csr_f64(a, c.offs, c.order))
    if c.n_par <= 1000:                # (shared among the small cases; a second-trip case is used once)
        _CSR_DOUT[key] = ref
    return ref


def _csr_kernel(shape, ldo):
    return "bwd4" if tuple(shape) == REF_SHAPE and ldo >= 64 else "generic"


def _csr_run(c, shape, ldo, bits=0, null=(False, False, False), entry="acc", seed=0):
    """One call on buffers that hold random values -> the three blocks afterwards (None where NULL or of width 0), each judged."""
    _lib, L, st = _api()
    wa, DF, DS = shape
    W = wa + DF + DS
    dout, seq, (s64, a64) = _csr_dout(c, W, seed)
    wide = np.full((c.n_child, ldo), 123.0, np.float32)
    wide[:, :W] = dout
    dt = torch.from_numpy(wide).cuda()                                           # (exactly n_child ldo floats: at ldo 64 the buffer ends with the last row)
    rng = np.random.default_rng([c.n_par, ldo, bits, 9])
    prev = [rng.normal(size=(rows, w)).astype(np.float32) for rows, w in ((c.n_anchor, wa), (c.n_par, DF), (c.n_par, DS))]
    outs = [None if (w == 0 or off) else Out(p.shape[0], w, fill=p) for p, w, off in zip(prev, shape, null)]
    idx = [dev(c.offs), dev(c.order), dev(c.parent_row)]
    args = (dt.data_ptr(), ldo, c.n_par, idx[0].data_ptr(), idx[1].data_ptr(), idx[2].data_ptr(), *[None if o is None else o.ptr for o in outs],
            wa, DF, DS)
    if entry == "acc":
        _ok(L.cgs_ctx_gather_bwd_acc(*args, bits, st), "cgs_ctx_gather_bwd_acc")
    else:
        assert bits == 0
        _ok(L.cgs_ctx_gather_bwd(*args, st), "cgs_ctx_gather_bwd")
    what = (_csr_kernel(shape, ldo), c.n_par, shape, ldo, bits, null)
    got = [None if o is None else o.get(what) for o in outs]
    has = c.counts > 0
    col = 0
    for k, (g, w) in enumerate(zip(got, shape)):
        sl = slice(col, col + w)
        col += w
        if g is None:
            continue
        bit = bits >> k & 1
        want = np.array(prev[k])
        if k == 0:           # the anchors: rows of parents with children only, at parent_row
            at = c.parent_row[has]
            want[at] = rr.csr_store(prev[0][at], seq[has, sl], bit)
            part, ssum, asum, cnt = g[at], s64[has, sl], a64[has, sl], c.counts[has]
            before = prev[0][at]
        else:                # d_f, d_s: every parent; a parent without children gets exact zeros (or keeps its row under the bit)
            want = rr.csr_store(prev[k], seq[:, sl], bit)
            part, ssum, asum, cnt, before = g, s64[:, sl], a64[:, sl], c.counts, prev[k]
        same_bits(g, want, what + ("block", k, "the sequential float32 sums in child order"))
        # the second, independent statement: the fp64 sum
        target = ssum + (before.astype(np.float64) if bit else 0.0)
        bound = rr.sum_bound(asum, cnt) + (U * np.abs(target) if bit else 0.0)
        assert _note("ctx_gather_bwd " + what[0], rr.fraction(np.abs(part - target), bound, what)) <= 1.0
    return got


@pytest.mark.parametrize("ldo", [64, 71, 128])
@pytest.mark.parametrize("n_par", rr.PARENT_COUNTS)
def test_csr_sums_four_parent_kernel(n_par, ldo):
    assert _csr_kernel(REF_SHAPE, ldo) == "bwd4"
    _csr_run(rr.draw_csr(n_par), REF_SHAPE, ldo, entry="plain" if ldo == 71 else "acc")


@pytest.mark.parametrize("ldo", [59, 63])
@pytest.mark.parametrize("n_par", rr.PARENT_COUNTS)
def test_csr_sums_generic_kernel_reference_shape(n_par, ldo):
    assert _csr_kernel(REF_SHAPE, ldo) == "generic"
    _csr_run(rr.draw_csr(n_par), REF_SHAPE, ldo, entry="plain" if ldo == 59 else "acc")


@pytest.mark.parametrize("shape", [(0, 50, 6), (3, 0, 6), (3, 50, 0), (1, 1, 1), (3, 100, 25), (2, 61, 1)])
def test_csr_sums_generic_kernel_other_shapes(shape):
    W = sum(shape)
    for ldo in (W, W + 5):
        assert _csr_kernel(shape, ldo) == "generic"
        _csr_run(rr.draw_csr(17), shape, ldo)


def test_csr_sums_both_kernels_agree_bit_for_bit():
    c = rr.draw_csr(40)
    a, b = _csr_run(c, REF_SHAPE, 63), _csr_run(c, REF_SHAPE, 64)
    # (the buffers start from different random values: compare what the call wrote)
    has = c.counts > 0
    same_bits(a[0][c.parent_row[has]], b[0][c.parent_row[has]], "d_anchor of the two kernels")
    same_bits(a[1], b[1], "d_f of the two kernels")
    same_bits(a[2], b[2], "d_s of the two kernels")


@pytest.mark.parametrize("ldo", [63, 71])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_csr_sums_each_output_null(which, ldo):
    _csr_run(rr.draw_csr(17), REF_SHAPE, ldo, null=tuple(k == which for k in range(3)))


@pytest.mark.parametrize("ldo", [63, 64])
@pytest.mark.parametrize("bits", range(8))
def test_csr_sums_accumulate_bits(bits, ldo):
    _csr_run(rr.draw_csr(17), REF_SHAPE, ldo, bits=bits)


@pytest.mark.parametrize("kernel,ldo", [("ctx_gather_bwd4", 64), ("ctx_gather_bwd", 59)])
def test_csr_sums_second_trip(kernel, ldo):
    c = rr.draw_csr(rr.second_trip(kernel), mean=1)
    assert _csr_kernel(REF_SHAPE, ldo) == ("bwd4" if kernel.endswith("4") else "generic") and set(rr.CHILD_COUNTS) <= set(c.counts.tolist())
    _csr_run(c, REF_SHAPE, ldo, bits=5)


def test_ctx_assemble_backward_is_the_sequential_sum():
    from contextgs_amd import ctx_ops
    c = rr.draw_csr(30_011, mean=2)
    rng = _rng("assemble")
    pos = np.zeros(c.n_child, np.int64)
    pos[c.order] = np.repeat(np.arange(c.n_par), c.counts)
    idx = c.parent_row[pos]
    T = lambda *s: torch.from_numpy(rng.normal(size=s).astype(np.float32)).cuda().requires_grad_()
    anchor, base_f, base_s, own = T(c.n_anchor, 3), T(c.n_par, 50), T(c.n_par, 6), T(c.n_child, 12)
    out = ctx_ops.ctx_assemble(anchor, base_f, base_s, own, dev(idx), dev(pos), (dev(c.offs), dev(c.order), dev(c.parent_row)))
    parts = [(anchor, idx), (base_f, pos), (base_s, pos), (own, None)]
    same_bits(out.detach().cpu().numpy(), rr.rowcat([(t.detach().cpu().numpy(), i, None) for t, i in parts], c.n_child), "ctx_assemble")
    dout = rng.normal(size=(c.n_child, 71)).astype(np.float32)
    out.backward(dev(dout))
    seq = rr.csr_seq32(dout[:, :59], c.offs, c.order)
    want_a = np.zeros((c.n_anchor, 3), np.float32)
    has = c.counts > 0
    want_a[c.parent_row[has]] = seq[has, :3]
    same_bits(anchor.grad.cpu().numpy(), want_a, "d_anchor")
    same_bits(base_f.grad.cpu().numpy(), seq[:, 3:53], "d_base_f")
    same_bits(base_s.grad.cpu().numpy(), seq[:, 53:59], "d_base_s")
    same_bits(own.grad.cpu().numpy(), dout[:, 59:], "d_own")


# ==== f. cgs_noise_quant_fwd / _bwd, cgs_means_finalize ==============================================================================
NQ_SHAPES = ((50, 6, 30), (64, 16, 32), (66, 6, 30), (50, 18, 30), (50, 6, 34), (51, 7, 31))
NQ_ROWS = (1, 15, 16, 17, 257)
HI = 0x7 << 32


def _nq_fwd(c, seed, off=2, rows=True, sums=None):
    """The forward on bases `off` floats past a 16-byte boundary (2: 8-byte aligned, 1: 4-byte) -> (yf, ys, yo, Q), the path."""
    _lib, L, st = _api()
    n = c.n
    xs = [dev(x if rows else x[:n], off) for x in c.x]
    ys = [Out(n, w, off=off) for w in c.widths]
    Q = Out(n, 3)
    qt, rt = dev(c.qadj), (dev(c.rows) if rows else None)
    _ok(L.cgs_noise_quant_fwd(*[t.data_ptr() for t in xs], qt.data_ptr(), _p(rt), n, *c.widths, seed, *Q0, *[o.ptr for o in ys], Q.ptr,
                              _p(sums), st), "cgs_noise_quant_fwd")
    aligned8 = all(t.data_ptr() % 8 == 0 for t in xs) and all(o.ptr % 8 == 0 for o in ys)
    return [o.get(("noise_quant_fwd", k)) for k, o in enumerate(ys)] + [Q.get("Q")], ("fwd2" if rr.nq_vec2(c.widths, aligned8) else "fwd")


def _judge_fwd(c, seed, out, rows, what):
    yf, ys, yo, Qk = out
    err, amb = rr.q_units(c.qadj, Qk, what)
    assert _note("noise_quant Q", err, rr.UNITS) <= rr.UNITS, what
    assert amb.any(1).mean() <= rr.AMBIGUOUS_CAP
    hd = rr.head_of(c.qadj)
    closed = hd.flat & (hd.qadj < 0) & ~amb
    assert (Qk[closed] == np.float32(1e-9)).all(), (what, "Q inside the clamp is not the clamp")
    for k, (w, y) in enumerate(zip(c.widths, (yf, ys, yo))):
        x = c.x[k][c.rows] if rows else c.x[k][:c.n]
        assert _note("noise_quant y", rr.y_fraction(x, rr.noise(seed, k, c.n, w), Qk[:, k], y, what + (k,))) <= 1.0, what


@pytest.mark.parametrize("n", NQ_ROWS)
@pytest.mark.parametrize("widths", NQ_SHAPES)
def test_noise_quant_fwd_both_kernels(widths, n):
    c = rr.draw_nq(n, widths)
    a, path_a = _nq_fwd(c, SEED, off=2)
    b, path_b = _nq_fwd(c, SEED, off=1)
    assert path_a == ("fwd2" if rr.nq_vec2(widths) else "fwd") and path_b == "fwd"
    _judge_fwd(c, SEED, a, True, ("fwd", widths, n, path_a))
    for x, y in zip(a, b):
        same_bits(x, y, ("an 8-byte and a 4-byte base give different bits", widths, n))
    if n == 17:          # without the row list
        d, path_d = _nq_fwd(c, SEED, off=2, rows=False)
        assert path_d == path_a
        _judge_fwd(c, SEED, d, False, ("fwd, no rows", widths, n))
        same_bits(d[3], a[3], "Q does not depend on the rows")


def test_noise_quant_seeds():
    c = rr.draw_nq(257, (50, 6, 30))
    assert SEED >> 32 and (SEED & 0xFFFFFFFF)
    outs = {}
    for seed in (SEED, SEED & 0xFFFFFFFF, (SEED & 0xFFFFFFFF) | HI, 2 ** 64 - 1):
        for off in (2, 1):
            out, _ = _nq_fwd(c, seed, off=off)
            _judge_fwd(c, seed, out, True, ("seed", hex(seed), off))
            if seed in outs:
                same_bits(out[0], outs[seed][0], "one seed, two kernels")
            outs[seed] = out
    ys = [outs[s][0] for s in outs]
    for i in range(len(ys)):
        for j in range(i):
            assert (ys[i] != ys[j]).mean() > 0.9                                 # seeds that differ in the high word only differ


def _nq_bwd(c, seed, dy=(True, True, True), dqe=True, rows=True, side=True):
    _lib, L, st = _api()
    n = c.n
    side = side and rows
    keep = [dev(a) if g else None for a, g in zip(c.dy, dy)] + [dev(c.dQe) if dqe else None, dev(c.qadj), dev(c.rows) if rows else None,
                                                                 dev(c.side_map) if side else None] + [dev(a) if side else None for a in c.side + [c.side_Q]]
    dq = Out(n, 3)
    dx = [Out(c.N, w, fill=SENTINEL) if rows else None for w in c.widths]
    _ok(L.cgs_noise_quant_bwd(*[_p(t) for t in keep[:5]], n, *c.widths, seed, *Q0, dq.ptr, _p(keep[5]), *[None if o is None else o.ptr for o in dx],
                              *[_p(t) for t in keep[6:]], st), "cgs_noise_quant_bwd")
    return dq.get("d qadj"), [None if o is None else o.get("dx") for o in dx]


def _judge_bwd(c, seed, got, dy, dqe, rows, side, what):
    dq, dx = got
    side = side and rows
    want_dx, sQ = rr.dx_of(c, dy, side)
    if rows:
        named = np.zeros(c.N, bool)
        named[c.rows] = True
        for k in range(3):
            same_bits(dx[k][c.rows], want_dx[k], what + ("dx", k, "is not dy + side: one fp32 add"))
            same_bits(dx[k][~named], np.full((int((~named).sum()), c.widths[k]), SENTINEL, np.float32), what + ("dx", k, "an unlisted row changed"))
    u = [rr.noise(seed, k, c.n, w) for k, w in enumerate(c.widths)]
    terms = want_dx if rows else [c.dy[k] if dy[k] else None for k in range(3)]
    ref, unit, hd = rr.dqadj_ref(c.qadj, terms, u, c.dQe if dqe else None, sQ if side else None)
    amb = hd.ambiguous_clamp()
    assert amb.any(1).mean() <= rr.AMBIGUOUS_CAP
    assert (dq[hd.flat & ~amb] == 0).all(), (what, "d qadj inside the clamp is not exactly 0")
    err = rr.mr.units_error(np.where(amb, ref, dq), ref, unit, what)
    assert _note("noise_quant d qadj", err, rr.UNITS) <= rr.UNITS, (what, float(err.max()), np.unravel_index(int(err.argmax()), err.shape))


@pytest.mark.parametrize("n", [17, 257])
@pytest.mark.parametrize("widths", NQ_SHAPES)
def test_noise_quant_bwd_both_kernels(widths, n):
    c = rr.draw_nq(n, widths)
    for rows, side in ((True, True), (True, False), (False, False)):
        what = ("bwd<%s>" % ("true" if rr.nq_bwd_fast(widths) else "false"), widths, n, rows, side)
        _judge_bwd(c, SEED, _nq_bwd(c, SEED, rows=rows, side=side), (True,) * 3, True, rows, side, what)


@pytest.mark.parametrize("n", [1, 15, 16])
@pytest.mark.parametrize("widths", [(50, 6, 30), (51, 7, 31)])
def test_noise_quant_bwd_row_counts(widths, n):
    c = rr.draw_nq(n, widths)
    _judge_bwd(c, SEED | HI, _nq_bwd(c, SEED | HI), (True,) * 3, True, True, True, ("bwd rows", widths, n))


NQ_NULLS = {"dyf": dict(dy=(False, True, True)), "dys": dict(dy=(True, False, True)), "dyo": dict(dy=(True, True, False)), "dQ_ext": dict(dqe=False)}


@pytest.mark.parametrize("rows", [True, False])
@pytest.mark.parametrize("widths", [(50, 6, 30), (66, 6, 30)])
@pytest.mark.parametrize("null", list(NQ_NULLS))
def test_noise_quant_bwd_each_cotangent_null(null, widths, rows):
    c = rr.draw_nq(65, widths)
    opt = dict(dict(dy=(True,) * 3, dqe=True), **NQ_NULLS[null])
    _judge_bwd(c, SEED, _nq_bwd(c, SEED, rows=rows, side=rows, **opt), opt["dy"], opt["dqe"], rows, rows, ("bwd NULL", null, widths, rows))


def _accumulator():
    """cgs_means_accum_doubles() zeroed doubles between two NaN guards of 16."""
    _lib, L, st = _api()
    nd = int(L.cgs_means_accum_doubles())
    flat = torch.full((nd + 32,), NAN, dtype=torch.float64, device="cuda")
    acc = flat[16:16 + nd]
    acc.zero_()
    return acc


def _finalize(acc, counts):
    _lib, L, st = _api()
    out = Out(1, 3)
    _ok(L.cgs_means_finalize(acc.data_ptr(), *counts, out.ptr, st), "cgs_means_finalize")
    got = out.get("means")[0]
    assert not bool(acc.any()), "the accumulator is not zero after cgs_means_finalize"
    flat = acc._base
    assert bool(torch.isnan(flat[:16]).all()) and bool(torch.isnan(flat[16 + acc.numel():]).all()), "a double outside the accumulator was written"
    return got


def _means_bounds(levels, off):
    """(fp64 mean, bound) of the three tensors over the rows the levels read."""
    want, bound = [], []
    for k in range(3):
        terms, total, count = [], 0.0, 0
        for c in levels:
            v = c.x[k][c.rows].astype(np.float64)
            terms.append((rr.means_terms(c.n, c.widths[k], k, rr.nq_vec2(c.widths, off % 2 == 0)), np.abs(v).sum()))
            total += v.sum()
            count += v.size
        want.append(total / count)
        bound.append(rr.means_bound(terms, count))
    return np.array(want), np.array(bound)


@pytest.mark.parametrize("off", [2, 1])
@pytest.mark.parametrize("widths", [(50, 6, 30), (51, 7, 31)])
def test_means_accumulators(widths, off):
    levels = [rr.draw_nq(n, widths) for n in (257, 17, 4001)]
    acc = _accumulator()
    rounds = []
    for _ in range(2):
        for j, c in enumerate(levels):
            _nq_fwd(c, SEED + j, off=off, sums=acc)
        slots = acc.view(-1, 16).cpu().numpy()
        assert not slots[:, 3:].any() and slots[:, :3].any()
        rounds.append(_finalize(acc, [sum(c.n for c in levels) * w for w in widths]))
    want, bound = _means_bounds(levels, off)
    assert (np.abs(want - 0.3) < 0.05).all() and (bound < 1e-5).all()           # (a lost workgroup is thousands of bounds away)
    assert _note("means", rr.fraction(np.abs(rounds[0] - want), bound)) <= 1.0
    assert _note("means, second round", rr.fraction(np.abs(rounds[1].astype(np.float64) - rounds[0]), bound)) <= 1.0
    # a zero count gives 0, whatever the slots hold
    _nq_fwd(levels[1], SEED, off=off, sums=acc)
    got = _finalize(acc, [0, 17 * widths[1], 0])
    assert got[0] == 0 and got[2] == 0 and got[1] != 0


@pytest.mark.parametrize("off", [2, 1])
def test_noise_quant_second_trip(off):
    n = rr.second_trip("noise_quant")
    widths = (50, 6, 30)
    c = rr.draw_nq(n, widths)
    acc = _accumulator()
    out, path = _nq_fwd(c, SEED, off=off, sums=acc)
    assert path == ("fwd2" if off == 2 else "fwd")
    _judge_fwd(c, SEED, out, True, ("fwd above the grid cap", path))
    got = _finalize(acc, [n * w for w in widths])
    want, bound = _means_bounds([c], off)
    assert _note("means", rr.fraction(np.abs(got - want), bound)) <= 1.0
    if off == 2:
        _judge_bwd(c, SEED, _nq_bwd(c, SEED), (True,) * 3, True, True, True, ("bwd above the grid cap",))


def test_noise_quant_wrapper_plain_and_row_source():
    from contextgs_amd import ctx_ops
    c = rr.draw_nq(300, (50, 6, 30), N=300)
    seed = SEED & (2 ** 63 - 1)
    G = lambda a: dev(a).requires_grad_()
    # plain: x in level order
    x = [G(a[c.rows]) for a in c.x]
    q = G(c.qadj)
    yf, ys, yo, Q = ctx_ops.noise_quant(*x, q, Q0, seed=seed)
    plain = [t.detach().cpu().numpy() for t in (yf, ys, yo, Q)]
    _judge_fwd(c, seed, plain, True, ("ctx_ops.noise_quant",))
    torch.autograd.backward([yf, ys, yo, Q], [dev(a) for a in c.dy] + [dev(c.dQe)])
    for k in range(3):
        same_bits(x[k].grad.cpu().numpy(), c.dy[k], "d x = d y")
    u = [rr.noise(seed, k, c.n, w) for k, w in enumerate(c.widths)]
    ref, unit, hd = rr.dqadj_ref(c.qadj, c.dy, u, c.dQe)
    dq = q.grad.cpu().numpy()
    err = rr.mr.units_error(np.where(hd.ambiguous_clamp(), ref, dq), ref, unit)
    assert _note("noise_quant d qadj", err, rr.UNITS) <= rr.UNITS and (dq[hd.flat & ~hd.ambiguous_clamp()] == 0).all()
    # a RowSource: the rows are read in place, the gradients scattered, the means accumulated
    feat, scal, off3 = G(c.x[0]), G(c.x[1]), G(c.x[2].reshape(c.N, 10, 3))
    src = ctx_ops.RowSource(feat, scal, off3, True)
    q2 = G(c.qadj)
    outs = ctx_ops.noise_quant(None, None, None, q2, Q0, seed=seed, src=src, rows=dev(c.rows))
    for a, b in zip(outs, plain):
        same_bits(a.detach().cpu().numpy(), b, "RowSource forward")
    means = src.means().cpu().numpy()
    want, bound = _means_bounds([c], 0)
    assert _note("means", rr.fraction(np.abs(means - want), bound)) <= 1.0
    torch.autograd.backward(list(outs), [dev(a) for a in c.dy] + [dev(c.dQe)])
    for t, k in ((feat, 0), (scal, 1), (off3, 2)):
        want_g = np.zeros_like(c.x[k])
        want_g[c.rows] = c.dy[k]
        same_bits(t.grad.cpu().numpy().reshape(c.N, -1), want_g, "RowSource gradient")
    same_bits(q2.grad.cpu().numpy(), dq, "RowSource d qadj")
