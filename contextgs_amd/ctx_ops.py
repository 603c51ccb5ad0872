"""Fused element-wise stages of the per-level context model (training path), include/cgs.h
`cgs_rowcat_*`, `cgs_noise_quant_*`, `cgs_level_rate_*` (csrc/ctx.hip).

Reference: scene/gaussian_model.py:1556-1707 (multi_scale_generating).  Each op is an
autograd.Function whose forward and backward are ONE HIP launch each; the torch composition
they replace stays in context_model.py as the eval / unsupported-shape path and as the
parity reference of tests/test_ctx_ops_gpu.py.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import itertools
import threading
import weakref

import collections
import os

import torch

from . import _lib

_f32 = torch.float32


def _c(t):
    t = t if t.dtype == _f32 else t.float()
    return t if t.is_contiguous() else t.contiguous()


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _ints(v):
    return (C.c_int * len(v))(*v)


def _u8(t):
    """A bool / uint8 row mask as the contiguous uint8 tensor the kernels read (None stays None)."""
    return None if t is None else (t if t.dtype == torch.uint8 else t.view(torch.uint8)).contiguous()


class _RowCat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec, *srcs):
        # spec[s] = (idx LongTensor | None, distinct: bool, rowmask uint8/bool [rows] | None)
        srcs = [_c(s) for s in srcs]
        _lib.require_device(*srcs)
        idxs = [sp[0] for sp in spec]
        masks = ctx.masks = [_u8(sp[2]) for sp in spec]
        n = next((i.shape[0] for i in idxs if i is not None), srcs[0].shape[0])
        for s, i in zip(srcs, idxs):
            if i is None and s.shape[0] != n:
                raise ValueError("rowcat: an un-indexed source must have one row per output row")
        widths = [int(s.shape[1]) for s in srcs]
        out = torch.empty(n, sum(widths), dtype=_f32, device=srcs[0].device)
        if n > 0:
            _lib.check(_lib.lib().cgs_rowcat_fwd_masked(len(srcs), _ptrs(srcs), _ptrs(idxs), _ptrs(masks), _ints(widths),
                                                        _ints(widths), n, _lib.ptr(out), _lib.current_stream()),
                       "cgs_rowcat_fwd")
        ctx.spec, ctx.widths, ctx.n = spec, widths, n
        ctx.rows = [int(s.shape[0]) for s in srcs]
        return out

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        grads, modes = [], []
        for k, ((idx, distinct, _m), w, rows) in enumerate(zip(ctx.spec, ctx.widths, ctx.rows)):
            if not ctx.needs_input_grad[1 + k]:
                grads.append(None)
                modes.append(0)
            elif idx is None:
                grads.append(torch.empty(rows, w, dtype=_f32, device=g.device))      # every row written
                modes.append(1)
            else:
                # distinct rows that number as many as the source has: every row is written, no zero fill
                full = distinct and ctx.n == rows
                grads.append((torch.empty if full else torch.zeros)(rows, w, dtype=_f32, device=g.device))
                modes.append(1 if distinct else 2)
        if any(modes) and ctx.n > 0:
            _lib.check(_lib.lib().cgs_rowcat_bwd_masked(len(grads), _ptrs(grads), _ptrs([sp[0] for sp in ctx.spec]),
                                                        _ptrs(ctx.masks), _ints(ctx.widths), _ints(ctx.widths), _ints(modes),
                                                        ctx.n, _lib.ptr(g), _lib.current_stream()), "cgs_rowcat_bwd")
        return (None, *grads)


def rowcat(parts):
    """cat([src[idx] for (src, idx, distinct[, rowmask]) in parts], dim=1) in one launch; idx None = all rows in order;
    distinct says the rows of idx do not repeat (plain scatter backward instead of atomics); rowmask (bool / uint8 per
    SOURCE row): the source counts as src * rowmask[:, None]."""
    spec = tuple((p[1], bool(p[2]), p[3] if len(p) > 3 else None) for p in parts)
    return _RowCat.apply(spec, *[p[0] for p in parts])


def gather_rows_nograd(x, idx):
    """x[idx] (rows) through the rowcat kernel, no autograd: for use inside backward passes."""
    x = _c(x)
    n, w = int(idx.shape[0]), int(x[0].numel())
    out = torch.empty((n,) + tuple(x.shape[1:]), dtype=_f32, device=x.device)
    if n > 0:
        _lib.check(_lib.lib().cgs_rowcat_fwd(1, _ptrs([x]), _ptrs([idx]), _ints([w]), _ints([w]), n, _lib.ptr(out),
                                             _lib.current_stream()), "cgs_rowcat_fwd")
    return out


_ROW_STAMPS = {}      # (device, n_full) -> [uint32 stamp tensor, generation]
_ROW_STAMPS_LOCK = threading.Lock()     # autograd runs backward nodes on its own threads


def add_rows_(out, idx, g):
    """out[idx] += g for DISTINCT rows idx (out [N, ...], g [n, ...] fp32): cgs_add_rows on the device, index_add_ elsewhere."""
    n = int(idx.shape[0])
    if n == 0:
        return out
    w = int(out[0].numel())
    if (out.is_cuda and out.dtype == _f32 and g.dtype == _f32 and out.is_contiguous() and idx.dtype == torch.int64
            and idx.is_contiguous() and 1 <= w <= 256 and int(g.numel()) == n * w):
        g = g.contiguous()
        _lib.check(_lib.lib().cgs_add_rows(_lib.ptr(g), _lib.ptr(idx), n, int(out.shape[0]), w, _lib.ptr(out), _lib.current_stream()),
                   "cgs_add_rows")
        return out
    out.view(out.shape[0], -1).index_add_(0, idx, g.reshape(n, -1).to(out.dtype))
    return out


def zero_unlisted_rows(idx, n_full, arrays):
    """Zeros in every row of `arrays` ([n_full, ...] float32, same device) that `idx` (int64, distinct rows < n_full) does not
    name — what torch.zeros gave the gradient buffers of a view's backward before the kernel overwrote the listed rows, without
    filling the 99 % that are overwritten anyway (cgs_mark_rows / cgs_zero_unmarked_rows).  The listed rows stay as they
    are (uninitialised: the caller's kernel writes them).  Every call marks afresh (an index buffer refilled through
    a raw pointer keeps its Python identity and version, so marks can not be reused on that evidence); an index >= n_full is
    ignored by the kernel."""
    if int(n_full) == 0 or not arrays:
        return
    dev = arrays[0].device
    L = _lib.lib()
    key = (str(dev), int(n_full))
    stream = _lib.current_stream()
    with _ROW_STAMPS_LOCK:
        st = _ROW_STAMPS.get(key)
        if st is None or st[1] >= 0xFFFFFFF0:
            if st is None and len(_ROW_STAMPS) >= 8:       # anchor counts change with densification: keep the newest few arrays
                _ROW_STAMPS.pop(next(iter(_ROW_STAMPS)))
            st = _ROW_STAMPS[key] = [torch.zeros(max(int(n_full), 1), dtype=torch.int32, device=dev), 0]
        st[1] += 1
        gen, stamp = st[1], st[0]
        # (enqueued under the lock: two backward threads on one stream must not interleave mark / zero pairs of one stamp array)
        _lib.check(L.cgs_mark_rows(_lib.ptr(idx), int(idx.shape[0]), int(n_full), gen, _lib.ptr(stamp), stream), "cgs_mark_rows")
        for a0 in range(0, len(arrays), 4):
            part = arrays[a0:a0 + 4]
            _lib.check(L.cgs_zero_unmarked_rows(_lib.ptr(stamp), gen, int(n_full), len(part), _ptrs(part),
                                                _ints([int(a[0].numel()) for a in part]), stream), "cgs_zero_unmarked_rows")


_seed_counter = itertools.count(1)


def next_seed() -> int:
    """A fresh 63-bit stream id per call, derived from torch's seed without a device sync (63 bits: the value
    travels through autograd.Function.apply, whose argument recorder (torch.profiler record_shapes) only takes int64)."""
    return (torch.initial_seed() * 0x9E3779B97F4A7C15 + next(_seed_counter) * 0xD1B54A32D192ED03) & (2 ** 63 - 1)


class HyperDirect:
    """Where the fused levels' backward kernels leave the gradient of the noisy hyper latents: ONE [N, C] buffer in the latents' own
    row order, row rows[r] written by the level that owns anchor rows[r] (cgs_ctx_level_bwd2) — instead of one strided column slice
    of dX per level that the hyper prior's backward gathers through the inverse coding permutation (a 49 us pass at 1 M anchors).
    Created by EntropyBottleneck.training_step_forms(sizes=...), reachable from every level block as `block._cgs_hyp_direct =
    (holder, block index)`; the hyper prior's backward takes the buffer when every non-empty block was written this way and
    repairs the others' rows otherwise."""

    def __init__(self, n_rows: int, channels: int, sizes):
        self.n, self.c, self.sizes = int(n_rows), int(channels), tuple(int(t) for t in sizes)
        self.buf, self.done = None, set()

    def buffer(self, device):
        if self.buf is None:
            self.buf = torch.empty(self.n, self.c, dtype=_f32, device=device)
        return self.buf

    def take(self):
        buf, done = self.buf, self.done
        self.buf, self.done = None, set()
        return buf, done


# ---- gradients handed between nodes outside autograd: one ledger per step ("Hand-overs between nodes") ----------------
# A backward that adds into a tensor another node owns returns None for it.  Every such route has ONE predicate that answers "may
# this level add in place?" (the A/B knob and the preconditions) and one fallback that returns a gradient tensor for autograd to sum:
#   parameter rows    RowSource.grad_buffers()                      always in place (the RowSource path has no other form)
#   shared anchor     _anchor_shared() -> RowSource.anchor_*        else a zero-filled [N, 3] per level
#   coded prefix      _prefix_inplace() -> JoinedGrads.prefix()     else a [prefix, w] tensor per level
#   rate gradients    RateSide.give() / take()                      else N-row tensors through autograd (no RateSide)
#   hyper rows        _hyper_rows_direct() -> HyperDirect.buffer()  else the hyper columns of dX, a strided slice
ANCHOR_SHARED = os.environ.get("CGS_ANCHOR_SHARED", "1") != "0"      # A/B knob: 0 = one zero-filled [N,3] anchor gradient per level (rounds 5)
HYPER_DIRECT = os.environ.get("CGS_HYPER_DIRECT", "1") != "0"        # A/B knob: 0 = the hyper latents' gradient leaves the levels as column slices of dX (gather_rows_segmented)
PREFIX_INPLACE = os.environ.get("CGS_PREFIX_INPLACE", "1") != "0"    # A/B knob: 0 = the coded prefix's gradient as its own tensors, summed by autograd


class JoinedGrads:
    """The gradients context_model._JoinRows' backward split into per-level row slices during ONE step's backward (needs no device).

    The coded prefix a context level reads IS the earlier levels' outputs, and their gradient from the joined tensor lies in the
    same buffer right in front of this level's rows: the level's backward adds the parents' sums THERE (cgs_ctx_gather_bwd_acc
    bits 1 / 2) and returns no gradient for the prefix.  Autograd still runs the earlier levels' nodes after this one (the edges
    exist), they find the sums in their own slice.  Before: a [prefix, 50] + [prefix, 6] tensor per context level and six add
    launches by the engine per step (profiles/r06_launch_attribution.txt).

    The record holds the noted tensors themselves until the step's token node clears it, and a lookup matches a part against a
    tensor it still holds by storage and offset — never an address alone, which the allocator may have handed to another step's
    gradient since.  It heals itself: a later level that could not add in place returns a real prefix gradient, the engine then
    SUMS two gradients for the earlier level's output into a fresh tensor, that tensor is in no record, and the earlier level
    falls back too."""

    def __init__(self):
        self.noted = []

    def note(self, g):
        if g.dim() == 2 and g.dtype == _f32 and g.is_contiguous():
            self.noted.append(g)

    def clear(self):
        self.noted = []

    def prefix(self, part, n_prefix, w):
        """`part` = rows [n_prefix, n_prefix + n) of a noted [rows, w] gradient -> that gradient's first n_prefix rows as a view,
        else None."""
        if (part is None or n_prefix <= 0 or part.dim() != 2 or part.shape[1] != w or part.dtype != _f32 or not part.is_contiguous()
                or part.requires_grad):
            return None
        first, addr = part.storage_offset() - w * n_prefix, part.data_ptr() - 4 * w * n_prefix
        for g in self.noted:
            # (the address only narrows the search: what decides is the storage and offset of a tensor this record keeps alive)
            if (g.data_ptr() == addr and g.shape[1] == w and g.storage_offset() == first and g.shape[0] >= n_prefix + part.shape[0]
                    and g.untyped_storage().data_ptr() == part.untyped_storage().data_ptr()):
                return torch.as_strided(part, (n_prefix, w), (w, 1), first)
        return None


class _AnchorLedger:
    """ONE anchor-gradient buffer for the levels of a backward (round 6): every fused level gathers anchor rows (its own, or its
    parents'), and as separate [N,3] outputs that was a zero fill per level + autograd's adds (3 fills + 2 adds of 12 MB at 1 M
    anchors).  The levels that asked for the anchor gradient register in the forward; in the backward the first one to run creates
    the zeroed buffer, each ADDS its rows, and the last one to release hands the buffer to autograd.  (Needs no device: the
    counting half of RowSource.)"""

    def __init__(self):
        self.anchor_users = 0
        self.anchor_acc = None

    def anchor_register(self):
        self.anchor_users += 1

    def anchor_target(self, shape, device):
        if self.anchor_acc is None:
            self.anchor_acc = torch.zeros(shape, dtype=_f32, device=device)
        return self.anchor_acc

    def anchor_release(self):
        """-> the shared buffer for the last registered level of this backward, None for the others."""
        self.anchor_users -= 1
        if self.anchor_users > 0:
            return None
        acc, self.anchor_acc = self.anchor_acc, None
        return acc

    def anchor_finish(self):
        if self.anchor_users != 0 or self.anchor_acc is not None:
            raise RuntimeError("RowSource: a level that registered for the shared anchor gradient did not release it "
                               f"({self.anchor_users} registrations open, buffer {'left over' if self.anchor_acc is not None else 'handed on'})")


def _anchor_shared(need_anchor_grad) -> bool:
    """May this level add its anchor rows into the step's shared buffer?  (asked in the forward: the level registers)"""
    return bool(ANCHOR_SHARED and need_anchor_grad)


def _prefix_inplace(src, part, shape, need):
    """May this level add the gradient of its coded prefix (`shape` = [prefix rows, w]) into the rows in front of its own gradient
    `part`?  -> those rows as a view, or None: the caller then returns a [prefix, w] tensor of its own."""
    return src.joined.prefix(part, int(shape[0]), int(shape[1])) if (PREFIX_INPLACE and need) else None


def _hyper_rows_direct(hd, need, n, n_full, device):
    """May this level write its hyper latents' gradient rows straight into the hyper prior's buffer?  Yes when its block of latents
    came from training_step_forms(sizes=) (hd = block._cgs_hyp_direct) and the latents are indexed like the per-anchor tensors (rows
    = coding permutation).  -> the [N, 12] buffer, or None: the gradient then leaves as the hyper columns of dX."""
    if HYPER_DIRECT and hd is not None and need and hd[0].n == n_full and hd[0].c == 12 and hd[0].sizes[hd[1]] == n:
        return hd[0].buffer(device)
    return None


class RowSource(_AnchorLedger):
    """The three per-anchor parameter tensors (features [N,D], scaling [N,S], offsets [N,K,3]) read THROUGH a row
    index by the level kernels, instead of being gathered into coding order first.

    Forward: `noise_quant(..., src=self, rows=perm[lo:hi])` reads rows perm[lo:hi] in place.  Backward: every
    level scatters the gradients of its (distinct) rows straight into one full-size buffer per tensor, and the
    node behind `self.token` — which autograd runs after all the levels, because each of them consumed the token —
    hands the three buffers to the parameters.  Compared with gather -> split -> ... -> cat -> index_copy this
    drops a full read+write pass over the tensors in each direction and the per-level gradient concatenation."""

    def __init__(self, feat, scal, off, complete: bool):
        super().__init__()
        self.joined = JoinedGrads()
        self.shapes = (feat.shape, scal.shape, off.shape)
        self.f, self.s = _c(feat.detach()), _c(scal.detach())
        self.s_orig = scal                      # the tensor the caller passed (rate_model checks WHOSE scaling it is)
        self.o = _c(off.detach()).reshape(off.shape[0], -1)
        _lib.require_device(self.f, self.s, self.o)
        self.complete = bool(complete)          # the levels' rows cover every row: no zero fill needed
        self.rows_read = self.rows_written = 0
        self.grads = None
        self.sums = None           # device double [3]: sums of the values the levels read (RowSource.means())
        self.token = _RowSourceFn.apply(self, feat, scal, off)

    def sums_buffer(self):
        """The accumulator the level kernels add the sums of their source rows to: private to this RowSource (two sources
        alive at once — interleaved forwards, a second stream — never share partial sums), zeroed at creation."""
        if self.sums is None:
            # (+ 16 doubles behind the accumulator: the step's [levels, 3] table of rate sums is carved from the same zero fill,
            #  rate_sum_table)
            nd = int(_lib.lib().cgs_means_accum_doubles())
            self._sums_all = torch.zeros(nd + 16, dtype=torch.float64, device=self.f.device)
            self.sums = self._sums_all[:nd]
            self._table_taken = False
        return self.sums

    def rate_sum_table(self, levels: int):
        """A zeroed float32 [levels, 3] table for the rate node of THIS step (cgs_rate_sub_fwd / cgs_level_rate_fwd add their three
        sums into a row): the tail of the accumulator's allocation, zeroed by the same fill — once per RowSource; None otherwise."""
        if self.sums is None or self._table_taken or 3 * levels > 32:
            return None
        self._table_taken = True
        return self._sums_all[self.sums.shape[0]:].view(_f32)[:3 * levels].view(levels, 3)

    def means(self):
        """float32 [3] = (features.mean(), scaling.mean(), offsets.mean()) once every row has been read by a level:
        the three clamp centres of the rate model (scene/gaussian_model.py:1664-1668) without a pass of their own."""
        n = self.f.shape[0]
        if self.sums is None or self.rows_read != n:
            raise RuntimeError("RowSource.means(): the levels have not read every row")
        out = torch.empty(3, dtype=_f32, device=self.f.device)
        _lib.check(_lib.lib().cgs_means_finalize(_lib.ptr(self.sums), self.f.numel(), self.s.numel(), self.o.numel(),
                                                 _lib.ptr(out), _lib.current_stream()), "cgs_means_finalize")
        return out

    def grad_buffers(self):
        if self.grads is None:
            n, (D, S, O) = self.f.shape[0], (self.f.shape[1], self.s.shape[1], self.o.shape[1])
            flat = (torch.empty if self.complete else torch.zeros)(n * (D + S + O), dtype=_f32, device=self.f.device)
            gf, gs, go = torch.split(flat, [n * D, n * S, n * O])
            self.grads = (gf.view(n, D), gs.view(n, S), go.view(n, O))
        return self.grads


class _RowSourceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, feat, scal, off):
        # (a WEAK reference: `src` keeps this node's output — its token — so a strong one would be a cycle through the C++
        #  node, invisible to Python's collector; the level nodes that consumed the token hold `src` until the graph is freed)
        ctx.src_ref = weakref.ref(src)
        ctx.joined = src.joined              # (holds gradient tensors only: no way back to this node)
        ctx.set_materialize_grads(False)     # the token's gradient carries nothing: no zeros(1) for it
        return feat.new_empty(1)             # (its VALUE is never read either: no fill launch)

    @staticmethod
    def backward(ctx, _g):
        # the step's backward ends here (every level consumed the token): its hand-overs must be settled, its records go
        ctx.joined.clear()
        src = ctx.src_ref()
        if src is None:                      # no level ever took the token: nothing was read, nothing to hand on
            return None, None, None, None
        if src.rows_written != src.rows_read:
            raise RuntimeError("RowSource: a level that read rows in the forward did not run its backward "
                               f"({src.rows_written} of {src.rows_read} rows have gradients)")
        src.anchor_finish()
        gf, gs, go = src.grad_buffers()
        src.grads = None
        need = ctx.needs_input_grad
        return (None, gf.view(src.shapes[0]) if need[1] else None, gs.view(src.shapes[1]) if need[2] else None,
                go.view(src.shapes[2]) if need[3] else None)


class RateSide:
    """Hand-over of one level's rate gradients from _LevelRate.backward to _NoiseQuant.backward.

    The level outputs have two consumers: everything downstream (dense gradients) and the rate of the ~15 % chosen
    rows.  Instead of scattering the rate gradients into N-row zero buffers that autograd then adds to the dense
    ones (a fill and three full-size adds per level), _LevelRate leaves them COMPACT here and returns no gradient;
    the noise_quant backward — which autograd runs after every consumer of its outputs, so after _LevelRate — adds
    row map[r] of them on the fly.  Needs the RowSource path (the kernel that scatters is the one that adds).

    Each transfer has one producer and one consumer:
      lend()         level forward -> rate node, `rate_lazy` levels only (cgs_rate_sub_*): the level's input rows X and mlp_grid's
                     weights; the rate node reads them with loan() in both directions
      give()         rate node's backward -> (map, f, s, o, q); on lazy levels also the input-row gradient of the mean / scale
                     branch dx [m, in] and its weight gradients dW = (dW1, db1, dW2, db2: the level kernel accumulates its own
                     into them)
      take()         the level's / noise_quant's backward <- (map, f, s, o, q)
      take_branch()  the level's backward <- (dx, dW); ends the loan
    Taking clears the record, so nothing of one backward is left for the next."""

    _ABSENT = (None,) * 5

    def __init__(self):
        self._loan = self._rate = self._branch = None

    def lend(self, X, weights):
        assert self._loan is None, "RateSide: this level's input rows were lent twice"
        self._loan = (X, weights)

    @property
    def lazy(self) -> bool:
        return self._loan is not None

    def loan(self):
        assert self._loan is not None, "RateSide: the level lent nothing (or its backward already took the loan back)"
        return self._loan

    def give(self, smap, f, s, o, q, dx=None, dW=None):
        assert self._rate is None and self._branch is None, "RateSide: rate gradients given twice before the level took them"
        self._rate = (smap, f, s, o, q)
        if dW is not None:
            self._branch = (dx, dW)

    def take(self):
        """(map, f, s, o, q), or five None when nothing was given or the arrays are empty: a level without a single chosen row has
        an all -1 map and zero-row arrays — nothing to add, and empty tensors would reach the C entry point as NULL pointers."""
        rate, self._rate = self._rate, None
        return rate if (rate is not None and rate[1].numel() > 0) else self._ABSENT

    def take_branch(self):
        """(dx, dW) of a lazy level whose rate node's backward ran, else (None, None): the level then zero-fills its weight
        gradients (no chosen row on the level, or a loss without the rate)."""
        branch, self._branch, self._loan = self._branch, None, None
        return branch if branch is not None else (None, None)


class _NoiseQuant(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xf, xs, xo, qadj, seed, q0, outs, src, rows, token, side):
        qadj = _c(qadj)
        if src is not None:
            xf, xs, xo = src.f, src.s, src.o
            n = int(rows.shape[0])
            assert rows.dtype == torch.int64 and rows.is_contiguous()
            src.rows_read += n
        else:
            xf, xs, xo = _c(xf), _c(xs), _c(xo)
            n = xf.shape[0]
        _lib.require_device(xf, xs, xo, qadj)
        ctx.set_materialize_grads(False)     # an output nobody differentiates (Q outside the rate subset) arrives as None, not zeros
        D, S, O = xf.shape[1], xs.shape[1], xo.shape[1]
        if outs is None:
            mk = lambda w: torch.empty(n, w, dtype=_f32, device=qadj.device)
            yf, ys, yo = mk(D), mk(S), mk(O)
        else:           # row slices of caller-owned buffers (the level outputs land side by side: no cat afterwards)
            yf, ys, yo = outs
            assert yf.shape == (n, D) and ys.shape == (n, S) and yo.shape == (n, O)
            assert yf.is_contiguous() and ys.is_contiguous() and yo.is_contiguous()
        Q = torch.empty(n, 3, dtype=_f32, device=qadj.device)
        _lib.check(_lib.lib().cgs_noise_quant_fwd(
            _lib.ptr(xf), _lib.ptr(xs), _lib.ptr(xo), _lib.ptr(qadj), _lib.ptr(rows), n, D, S, O, seed,
            q0[0], q0[1], q0[2], _lib.ptr(yf), _lib.ptr(ys), _lib.ptr(yo), _lib.ptr(Q),
            _lib.ptr(src.sums_buffer()) if src is not None else None, _lib.current_stream()), "cgs_noise_quant_fwd")
        ctx.save_for_backward(qadj, rows)
        ctx.dims, ctx.seed, ctx.q0, ctx.src, ctx.side = (n, D, S, O), seed, q0, src, side
        return yf, ys, yo, Q

    @staticmethod
    def backward(ctx, gf, gs, go, gQ):
        qadj, rows = ctx.saved_tensors
        n, D, S, O = ctx.dims
        src = ctx.src
        gf, gs, go, gQ = (None if t is None else _c(t) for t in (gf, gs, go, gQ))
        dq = torch.empty(n, 3, dtype=_f32, device=qadj.device) if (ctx.needs_input_grad[3] or src is not None) else None
        dx = src.grad_buffers() if src is not None else (None, None, None)
        sd = ctx.side.take() if ctx.side is not None else (None,) * 5       # (a side needs src: noise_quant())
        if dq is not None:
            _lib.check(_lib.lib().cgs_noise_quant_bwd(
                _lib.ptr(gf), _lib.ptr(gs), _lib.ptr(go), _lib.ptr(gQ), _lib.ptr(qadj), n, D, S, O, ctx.seed, ctx.q0[0],
                ctx.q0[1], ctx.q0[2], _lib.ptr(dq), _lib.ptr(rows) if src is not None else None, _lib.ptr(dx[0]),
                _lib.ptr(dx[1]), _lib.ptr(dx[2]), *[_lib.ptr(t) for t in sd], _lib.current_stream()), "cgs_noise_quant_bwd")
        if src is not None:
            src.rows_written += n
            gf = gs = go = None         # (the kernel scattered them into the RowSource's buffers)
        # (no gradient VALUE for the token: it only ties _RowSourceFn into the graph, whose backward hands out the
        #  buffers this kernel filled — a zeros(1) per level cost a fill and an add launch each)
        return gf, gs, go, dq, None, None, None, None, None, None, None


def noise_quant(xf, xs, xo, qadj, q0, seed=None, outs=None, src=None, rows=None, side=None):
    """(xf + u Qf, xs + u Qs, xo + u Qo, Q[n,3]) with Q = clamp(q0 (1 + tanh(qadj)), 1e-9), u ~ U[-0.5, 0.5).
    outs = (yf, ys, yo) optionally names the (contiguous) tensors to write the three results into.
    src / rows: read x from rows `rows` of a RowSource instead of xf/xs/xo (which are then ignored).
    side: a RateSide that level_rate(..., side=side) of the same level fills in its backward (needs src)."""
    assert side is None or src is not None
    return _NoiseQuant.apply(xf, xs, xo, qadj, next_seed() if seed is None else int(seed),
                             tuple(float(v) for v in q0), outs, src, rows, None if src is None else src.token, side)


# ---- the launches the rate nodes share (one node per level: _LevelRate + _RateFinish; one node for the step: _RateAll) -----------
def _carve(n, widths, device, zero=False):
    """[n, w] tensors for w in widths, side by side in ONE allocation (one fill when zero)."""
    flat = (torch.zeros if zero else torch.empty)(n * sum(widths), dtype=_f32, device=device)
    return [t.view(n, w) for t, w in zip(torch.split(flat, [n * w for w in widths]), widths)]


def _sub_map(loc, n_level):
    """int32 [n_level]: a level row's index in the chosen list `loc`, -1 elsewhere — where the step's bookkeeping kernel
    (ctx_plan.hip, choose_rows' sub_map) did not leave one."""
    m = torch.full((n_level,), -1, dtype=torch.int32, device=loc.device)
    m[loc] = torch.arange(int(loc.shape[0]), dtype=torch.int32, device=loc.device)
    return m


def _level_rate_fwd(lv, masks_p, grows, x_means, use_clamp, K, sums_p, stream):
    """masks_p / sums_p: device addresses of the level's mask-weight rows (or None) and of its float [3] sums."""
    yf, ys, yo, Q, pred, loc = lv
    _lib.check(_lib.lib().cgs_level_rate_fwd(
        _lib.ptr(yf), _lib.ptr(ys), _lib.ptr(yo), _lib.ptr(Q), _lib.ptr(loc), _lib.ptr(pred), masks_p, _lib.ptr(grows),
        _lib.ptr(x_means), use_clamp, int(pred.shape[0]), int(yf.shape[1]), K, int(pred.shape[1]), sums_p, stream), "cgs_level_rate_fwd")


def _level_rate_bwd(lv, masks_p, grows, x_means, use_clamp, K, g_p, d_masks_p, compact, stream):
    """-> ([d_yf, d_ys, d_yo, dQ], d_pred).  Row-scattered gradients: one zero fill for the four N-row buffers — or, compact (with a
    RateSide), [n_sub, .] arrays (every row written, no fill) that the level's backward adds in."""
    yf, ys, yo, Q, pred, loc = lv
    n_sub, D = int(pred.shape[0]), int(yf.shape[1])
    d = _carve(n_sub if compact else int(yf.shape[0]), (D, 6, 3 * K, 3), yf.device, zero=not compact)
    d_pred = torch.empty_like(pred)
    _lib.check(_lib.lib().cgs_level_rate_bwd(
        _lib.ptr(yf), _lib.ptr(ys), _lib.ptr(yo), _lib.ptr(Q), _lib.ptr(loc), _lib.ptr(pred), masks_p, _lib.ptr(grows),
        _lib.ptr(x_means), use_clamp, n_sub, D, K, int(pred.shape[1]), g_p, _lib.ptr(d_pred), *[_lib.ptr(t) for t in d], d_masks_p,
        int(compact), stream), "cgs_level_rate_bwd")
    return d, d_pred


def _rate_sub_fwd(side, lv, masks_p, x_means, use_clamp, sums_p, stream):
    """A rate_lazy level: the MLP's mean / scale branch + the rate terms of the chosen rows in one launch, from the loan."""
    yf, ys, yo, Q, _pred, loc = lv
    X, (W1, b1, W2, b2) = side.loan()
    _lib.check(_lib.lib().cgs_rate_sub_fwd(
        int(X.shape[1]), _lib.ptr(X), int(X.shape[0]), _lib.ptr(loc), int(loc.shape[0]), _lib.ptr(W1), _lib.ptr(b1), _lib.ptr(W2),
        _lib.ptr(b2), _lib.ptr(yf), _lib.ptr(ys), _lib.ptr(yo), _lib.ptr(Q), masks_p, _lib.ptr(x_means), use_clamp, sums_p, stream),
        "cgs_rate_sub_fwd")


def _rate_sub_bwd_buffers(levels, K):
    """The outputs and the scratch of cgs_rate_sub_bwd for several levels [(side, lv)] from three allocations (every row and every
    weight gradient is written: no fill) -> per level ([d_yf, d_ys, d_yo, dQ], dx [n_sub, in], (dW1, db1, dW2, db2), scratch)."""
    Lc, dev = _lib.lib(), levels[0][1][0].device
    shapes = []
    for side, lv in levels:
        X, W = side.loan()
        n_sub, in_f = int(lv[5].shape[0]), int(X.shape[1])
        ws = int(Lc.cgs_rate_sub_bwd_scratch_bytes(in_f, n_sub))
        shapes.append((n_sub, (int(lv[0].shape[1]), 6, 3 * K, 3, in_f), W, (ws + 255) // 256 * 256))
    rows = torch.split(torch.empty(sum(n * sum(ws_) for n, ws_, _, _ in shapes), dtype=_f32, device=dev),
                       [n * w for n, ws_, _, _ in shapes for w in ws_])
    wg = torch.split(torch.empty(sum(w.numel() for _, _, W, _ in shapes for w in W), dtype=_f32, device=dev),
                     [w.numel() for _, _, W, _ in shapes for w in W])
    scr = torch.split(torch.empty(sum(b for *_, b in shapes), dtype=torch.uint8, device=dev), [b for *_, b in shapes])
    out = []
    for j, (n, widths, W, _) in enumerate(shapes):
        *d, dx = [t.view(n, w) for t, w in zip(rows[5 * j:5 * j + 5], widths)]
        out.append((d, dx, tuple(t.view(w.shape) for t, w in zip(wg[4 * j:4 * j + 4], W)), scr[j]))
    return out


def _rate_sub_bwd(side, lv, masks_p, x_means, use_clamp, g_p, d_masks_p, bufs, stream):
    """Fills bufs (one entry of _rate_sub_bwd_buffers) -> ([d_yf, d_ys, d_yo, dQ], dx [n_sub, in], (dW1, db1, dW2, db2)), all
    compact and fully written."""
    yf, ys, yo, Q, _pred, loc = lv
    X, W = side.loan()
    d, dx, dW, ws = bufs
    _lib.check(_lib.lib().cgs_rate_sub_bwd(
        int(X.shape[1]), _lib.ptr(X), int(X.shape[0]), _lib.ptr(loc), int(loc.shape[0]), *[_lib.ptr(w) for w in W], _lib.ptr(yf),
        _lib.ptr(ys), _lib.ptr(yo), _lib.ptr(Q), masks_p, _lib.ptr(x_means), use_clamp, g_p, *[_lib.ptr(t) for t in d], _lib.ptr(dx),
        d_masks_p, *[_lib.ptr(t) for t in dW], _lib.ptr(ws), ws.numel(), stream), "cgs_rate_sub_bwd")
    return d, dx, dW


@contextlib.contextmanager
def _rate_sub_group():
    """The cgs_rate_sub_fwd / cgs_rate_sub_bwd calls inside are recorded and leave as ONE grouped call at the end (include/cgs.h):
    no level's rate kernels depend on another level's, and a launch per level leaves most of the device idle on the small ones."""
    Lc = _lib.lib()
    _lib.check(Lc.cgs_rate_sub_group_begin(), "cgs_rate_sub_group_begin")
    done = False
    try:
        yield
        done = True
    finally:
        rc = Lc.cgs_rate_sub_group_end(int(done))
    _lib.check(rc, "cgs_rate_sub_group_end")


def _rate_finish_fwd(table_p, levels, hsum, finish, device, stream):
    """scene/gaussian_model.py:1687-1705 over a [levels, 3] table of bit sums -> (out [4], raw [2 + levels])."""
    out = torch.empty(4, dtype=_f32, device=device)
    raw = torch.empty(2 + levels, dtype=_f32, device=device)
    _lib.check(_lib.lib().cgs_rate_finish_fwd(table_p, levels, _lib.ptr(_c(hsum)), *[float(v) for v in finish], _lib.ptr(out),
                                              _lib.ptr(raw), stream), "cgs_rate_finish_fwd")
    return out, raw


def _rate_finish_bwd(gs, levels, finish, device, stream):
    """gs: the gradient of out [4], or of its four entries (None = unread) -> (dS [levels, 3], dh [1])."""
    dS = torch.empty(levels, 3, dtype=_f32, device=device)
    dh = torch.empty(1, dtype=_f32, device=device)
    entry = _lib.lib().cgs_rate_finish_bwd if len(gs) == 1 else _lib.lib().cgs_rate_finish_bwd4
    _lib.check(entry(*[_lib.ptr(None if g is None else _c(g)) for g in gs], levels, *[float(v) for v in finish[:4]], _lib.ptr(dS),
                     _lib.ptr(dh), stream), "cgs_rate_finish_bwd")
    return dS, dh


class _LevelRate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, yf, ys, yo, Q, pred, loc, masks, grows, x_means, use_clamp, K, side, out):
        lv = (_c(yf), _c(ys), _c(yo), _c(Q), _c(pred), loc)
        _lib.require_device(lv[0], lv[4])
        # out: a ZEROED float [3] the caller owns (a row of the step's [levels, 3] table: one fill for all levels)
        if out is not None:     # an independent tensor object on the caller's storage (not an autograd view of it)
            sums = torch.empty(0, dtype=_f32, device=yf.device).set_(out.untyped_storage(), out.storage_offset(), (3,), (1,))
        else:
            sums = torch.zeros(3, dtype=_f32, device=yf.device)
        masks = None if masks is None else _c(masks)
        x_means = None if x_means is None else _c(x_means)
        _level_rate_fwd(lv, _lib.ptr(masks), grows, x_means, int(use_clamp), K, _lib.ptr(sums), _lib.current_stream())
        ctx.save_for_backward(*lv, masks, grows, x_means)
        ctx.cfg = (int(use_clamp), K)
        ctx.side = side
        return sums

    @staticmethod
    def backward(ctx, g):
        *lv, masks, grows, x_means = ctx.saved_tensors
        use_clamp, K = ctx.cfg
        loc = lv[5]
        side = ctx.side if loc is not None else None
        d_masks = torch.zeros_like(masks) if (masks is not None and ctx.needs_input_grad[6]) else None
        d, d_pred = _level_rate_bwd(lv, _lib.ptr(masks), grows, x_means, use_clamp, K, _lib.ptr(_c(g)), _lib.ptr(d_masks),
                                    side is not None, _lib.current_stream())
        if side is not None:
            side.give(_sub_map(loc, int(lv[0].shape[0])), *d)
            d = (None,) * 4
        return (*d, d_pred, None, d_masks, None, None, None, None, None, None)


def level_rate(yf, ys, yo, Q, pred, loc, masks, grows, x_means, use_clamp, K, side=None, out=None):
    """[bits_feat, bits_scaling, bits_offsets (mask-weighted)] summed over the chosen rows `loc` of a level.
    side: the RateSide given to the noise_quant call that produced yf/ys/yo/Q (their rate gradients then travel
    through it instead of through autograd)."""
    return _LevelRate.apply(yf, ys, yo, Q, pred, loc, masks, grows, x_means, bool(use_clamp), int(K), side, out)


class _RateFinish(torch.autograd.Function):
    """(bit_per_param, bit_per_feat_param, bit_per_scaling_param, bit_per_offsets_param) [4] + the raw numbers of the
    per-level report, from the per-level bit sums and the hyper bit sum: scene/gaussian_model.py:1687-1705 in ONE
    launch each way (cgs_rate_finish_*).  The level rows must be consecutive rows of one [L,3] table."""

    @staticmethod
    def forward(ctx, hsum, cfg, *rows):
        base = rows[0]
        for j, r in enumerate(rows):
            if r.data_ptr() != base.data_ptr() + 12 * j:
                raise ValueError("rate_finish: level sums must be consecutive rows of one table")
        out, raw = _rate_finish_fwd(_lib.ptr(base), len(rows), hsum, cfg, base.device, _lib.current_stream())
        ctx.cfg, ctx.L = cfg, len(rows)
        ctx.mark_non_differentiable(raw)
        return out, raw

    @staticmethod
    def backward(ctx, g, _g_raw):
        dS, dh = _rate_finish_bwd((g,), ctx.L, ctx.cfg, g.device, _lib.current_stream())
        return (dh, None, *dS.unbind(0))


def rate_finish(level_sums, hsum, rate, n_feat, n_scaling, n_offsets, dead_frac):
    """level_sums: list of [3] tensors (consecutive rows of one table, see level_rate(out=)); hsum: [1] hyper bit sum.
    Returns (out [4], raw [2+L])."""
    return _RateFinish.apply(hsum, (float(rate), float(n_feat), float(n_scaling), float(n_offsets), float(dead_frac)), *level_sums)


class _RateAll(torch.autograd.Function):
    """The rate of ALL levels plus the scalar tail as one autograd node (scene/gaussian_model.py:1658-1705 on the
    fused path): per level one cgs_level_rate_* launch — the rate_lazy levels' cgs_rate_sub_* calls as one group, a launch
    per stage for all of them — then cgs_rate_finish_*.  Compared with one node per level +
    one for the tail: one zero fill for the [levels,3] sum table (forward) and one for the mask-weight gradient of all
    chosen rows (backward), no per-level slice nodes, and the level-row -> chosen-index maps come from the step's
    bookkeeping kernel (ctx_plan.hip) instead of a fill + arange + scatter per level.

    meta: dict(use_clamp, K, finish=(rate, n_f, n_s, n_o, dead), spans=[(lo, hi) rows of `masks` per level],
               sides=[RateSide | None per level], maps=[int32 [n_level] | None per level]);
    masks [T, K]: the mask weights of the chosen rows of all levels, level after level; lv: per level
    (yf, ys, yo, Q, pred, loc).  Returns (out [4], raw [2 + L])."""

    @staticmethod
    def forward(ctx, hsum, masks, x_means, meta, *lv):
        nl = len(lv) // 6
        K, use_clamp = int(meta["K"]), int(bool(meta["use_clamp"]))
        masks, x_means, hsum = _c(masks), _c(x_means), _c(hsum)
        lv = [t.contiguous() if k % 6 == 5 else _c(t) for k, t in enumerate(lv)]     # every 6th is loc (int64)
        _lib.require_device(masks, x_means, lv[0], lv[4])
        S = meta.get("sum_table")           # (zeroed with the row source's accumulator: RowSource.rate_sum_table)
        if S is None or tuple(S.shape) != (nl, 3):
            S = torch.zeros(nl, 3, dtype=_f32, device=masks.device)
        stream = _lib.current_stream()
        # a rate_lazy level (its node lent X and the weights): MLP branch + rate terms in one launch
        ctx.lazy = tuple(sd is not None and sd.lazy for sd in meta["sides"])
        with _rate_sub_group():              # the lazy levels' launches leave together
            for j in range(nl):
                lvj, (lo, hi) = lv[6 * j:6 * j + 6], meta["spans"][j]
                n_sub = int(lvj[5].shape[0])
                assert hi - lo == n_sub and (ctx.lazy[j] or int(lvj[4].shape[0]) == n_sub)
                masks_p, sums_p = masks.data_ptr() + 4 * K * lo, S.data_ptr() + 12 * j
                if not ctx.lazy[j]:
                    _level_rate_fwd(lvj, masks_p, None, x_means, use_clamp, K, sums_p, stream)
                elif n_sub > 0:
                    _rate_sub_fwd(meta["sides"][j], lvj, masks_p, x_means, use_clamp, sums_p, stream)
        out, raw = _rate_finish_fwd(_lib.ptr(S), nl, hsum, meta["finish"], masks.device, stream)
        ctx.save_for_backward(masks, x_means, *lv)
        ctx.meta = meta
        ctx.mark_non_differentiable(raw)
        # the four entries leave as four outputs: the training loss reads the first only (train.py:207), and selecting it from a [4]
        # output cost a zero fill + a copy in the backward (SelectBackward0); an unread entry now simply has no gradient
        ctx.set_materialize_grads(False)
        return out[0], out[1], out[2], out[3], raw

    @staticmethod
    def backward(ctx, g0, g1, g2, g3, _g_raw):
        masks, x_means, *lv = ctx.saved_tensors
        meta, nl = ctx.meta, len(lv) // 6
        K, use_clamp = int(meta["K"]), int(bool(meta["use_clamp"]))
        stream = _lib.current_stream()
        dS, dh = _rate_finish_bwd((g0, g1, g2, g3), nl, meta["finish"], masks.device, stream)
        # (the level-rate kernels add into it; the fused rate-subset kernels write every row of their span)
        d_masks = (torch.empty_like if all(ctx.lazy) else torch.zeros_like)(masks) if ctx.needs_input_grad[1] else None
        grads = []
        # (nothing chosen on a lazy level: nothing is given, the level node zero-fills its weight gradients)
        sub = [j for j in range(nl) if ctx.lazy[j] and int(lv[6 * j + 5].shape[0]) > 0]
        bufs = dict(zip(sub, _rate_sub_bwd_buffers([(meta["sides"][j], lv[6 * j:6 * j + 6]) for j in sub], K))) if sub else {}
        with _rate_sub_group():
            for j in range(nl):
                lvj, (lo, _hi), side, mp = lv[6 * j:6 * j + 6], meta["spans"][j], meta["sides"][j], meta["maps"][j]
                loc, n_l = lvj[5], int(lvj[0].shape[0])
                masks_p, g_p = masks.data_ptr() + 4 * K * lo, dS.data_ptr() + 12 * j
                d_masks_p = None if d_masks is None else d_masks.data_ptr() + 4 * K * lo
                if ctx.lazy[j]:
                    if j in bufs:
                        d, dx, dW = _rate_sub_bwd(side, lvj, masks_p, x_means, use_clamp, g_p, d_masks_p, bufs[j], stream)
                        side.give(mp if mp is not None else _sub_map(loc, n_l), *d, dx=dx, dW=dW)
                    grads += [None] * 6
                    continue
                d, d_pred = _level_rate_bwd(lvj, masks_p, None, x_means, use_clamp, K, g_p, d_masks_p, side is not None, stream)
                if side is not None:
                    side.give(mp if mp is not None else _sub_map(loc, n_l), *d)
                    d = [None] * 4
                grads += [*d, d_pred, None]
        return (dh, d_masks, None, None, *grads)


def rate_all(hsum, masks, x_means, meta, level_tensors):
    """See _RateAll.  level_tensors: flat list (yf, ys, yo, Q, pred, loc) per level.  Returns ((four 0-dim tensors), raw)."""
    o = _RateAll.apply(hsum, masks, x_means, meta, *level_tensors)
    return o[:4], o[4]


class _CtxAssemble(torch.autograd.Function):
    """[anchor[idx] | base_f[pos] | base_s[pos] | own] with the atomics-free CSR backward (cgs_ctx_gather_bwd)."""

    @staticmethod
    def forward(ctx, anchor, base_f, base_s, own, idx, pos, csr):
        anchor, base_f, base_s, own = _c(anchor), _c(base_f), _c(base_s), _c(own)
        _lib.require_device(anchor, base_f, base_s, own)
        n = idx.shape[0]
        srcs, idxs = [anchor, base_f, base_s, own], [idx, pos, pos, None]
        widths = [int(s.shape[1]) for s in srcs]
        out = torch.empty(n, sum(widths), dtype=_f32, device=anchor.device)
        if n > 0:
            _lib.check(_lib.lib().cgs_rowcat_fwd(4, _ptrs(srcs), _ptrs(idxs), _ints(widths), _ints(widths), n,
                                                 _lib.ptr(out), _lib.current_stream()), "cgs_rowcat_fwd")
        ctx.csr, ctx.widths, ctx.n = csr, widths, n
        ctx.rows = (anchor.shape[0], base_f.shape[0])
        return out

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        offs, order, prow = ctx.csr
        wa, DF, DS, WO = ctx.widths
        n_anchor, n_par = ctx.rows
        need = ctx.needs_input_grad
        dev = g.device
        d_anchor = torch.zeros(n_anchor, wa, dtype=_f32, device=dev) if need[0] else None
        d_f = torch.empty(n_par, DF, dtype=_f32, device=dev) if need[1] else None
        d_s = torch.empty(n_par, DS, dtype=_f32, device=dev) if need[2] else None
        d_own = None
        if ctx.n > 0:
            if d_anchor is not None or d_f is not None or d_s is not None:
                _lib.check(_lib.lib().cgs_ctx_gather_bwd(_lib.ptr(g), g.shape[1], n_par, _lib.ptr(offs), _lib.ptr(order),
                                                         _lib.ptr(prow), _lib.ptr(d_anchor), _lib.ptr(d_f), _lib.ptr(d_s),
                                                         wa, DF, DS, _lib.current_stream()), "cgs_ctx_gather_bwd")
            if need[3]:
                d_own = g[:, wa + DF + DS:]          # a column slice: its consumer (the split's cat) takes strided rows
        else:
            d_f = None if d_f is None else d_f.zero_()
            d_s = None if d_s is None else d_s.zero_()
            d_own = torch.zeros(0, WO, dtype=_f32, device=dev) if need[3] else None
        return d_anchor, d_f, d_s, d_own, None, None, None


def ctx_assemble(anchor, base_f, base_s, own, idx, pos, csr):
    """The MLP input rows of a level: parent anchor / coded feature / coded scaling rows + the level's own hyper
    rows.  csr = (offs[n_parents+1], order[n_children], parent_row[n_parents]) lists every parent's children."""
    return _CtxAssemble.apply(anchor, base_f, base_s, own, idx, pos, csr)


def _mask_ste_bwd(x, g):
    d = torch.empty_like(x)
    _lib.check(_lib.lib().cgs_mask_ste_bwd(_lib.ptr(x), _lib.ptr(_c(g)), x.numel(), _lib.ptr(d), _lib.current_stream()),
               "cgs_mask_ste_bwd")
    return d


class _MaskSTE(torch.autograd.Function):
    """get_mask / get_mask_anchor of the model in one launch each way (cgs_mask_ste_*, csrc/mask.hip)."""

    @staticmethod
    def forward(ctx, logits):
        x = _c(logits)
        _lib.require_device(x)
        n, K = x.shape[0], x[0].numel() if x.shape[0] else 1
        mask = torch.empty_like(x)
        alive = torch.empty(n, dtype=torch.bool, device=x.device)
        _lib.check(_lib.lib().cgs_mask_ste_fwd(_lib.ptr(x), n, K, _lib.ptr(mask), _lib.ptr(alive), _lib.current_stream()),
                   "cgs_mask_ste_fwd")
        ctx.save_for_backward(x)
        ctx.mark_non_differentiable(alive)
        ctx.set_materialize_grads(False)       # no zeros [N] for the gradient of the (bool) `alive` output
        return mask, alive

    @staticmethod
    def backward(ctx, g, _g_alive):
        (x,) = ctx.saved_tensors
        return None if g is None else _mask_ste_bwd(x, g)


class _MaskSTEAttach(torch.autograd.Function):
    """The autograd node of mask_ste() created LATER than its values: `values` = the mask mask_ste_values() computed earlier
    in the forward.  The autograd engine runs ready nodes in the reverse order of their creation; a node created at the top of
    render() (where the anchor mask is needed for the level plan) is run after every node of the context model, so `_mask`'s
    gradient — complete once the expansion's and the rate model's backward are done — became final only after the level kernels
    and its all-reduce (dist.GradientSync) could not start beside them."""

    @staticmethod
    def forward(ctx, logits, values):
        ctx.save_for_backward(logits.detach())
        ctx.set_materialize_grads(False)
        return values.view_as(values)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return (None if g is None else _mask_ste_bwd(_c(x), g)), None


def mask_ste_values(logits):
    """(mask, any_alive) of mask_ste() WITHOUT an autograd node (attach one later: mask_ste_attach)."""
    with torch.no_grad():
        m, alive = _MaskSTE.apply(logits.detach())
    return m, alive


def mask_ste_attach(logits, values):
    return _MaskSTEAttach.apply(logits, values)


def mask_ste(logits):
    """(mask, any_alive): mask = ((sigmoid(m) > 0.01) - sigmoid(m)) + sigmoid(m) with the sigmoid's gradient
    (scene/gaussian_model.py:295-299), any_alive[a] = some offset of anchor a has mask > 0 (:302-310)."""
    return _MaskSTE.apply(logits)


_means3_ws = {}


def means3(a, b, c, exp_b=False):
    """float32 [3] = (a.mean(), (exp(b) if exp_b else b).mean(), c.mean()) in one launch, no autograd (the clamp
    centres of the rate model, scene/gaussian_model.py:1664-1668, as the fused rate kernel consumes them)."""
    a, b, c = _c(a.detach()), _c(b.detach()), _c(c.detach())
    _lib.require_device(a, b, c)
    L = _lib.lib()
    ws = _means3_ws.get(a.device)
    if ws is None:
        ws = _means3_ws[a.device] = torch.empty(L.cgs_means3_scratch_bytes(), dtype=torch.uint8, device=a.device)
    out = torch.empty(3, dtype=_f32, device=a.device)
    _lib.check(L.cgs_means3(_lib.ptr(a), a.numel(), _lib.ptr(b), b.numel(), int(bool(exp_b)), _lib.ptr(c), c.numel(),
                            _lib.ptr(ws), ws.numel(), _lib.ptr(out), _lib.current_stream()), "cgs_means3")
    return out


_PINNED_FREE = []
CHOOSE_SLOTS = 32         # `meta` slots the choose kernel's blocks spread their closing atomics over


def _pinned_i32(k):
    """A small pinned int32 buffer from a free list (allocating pinned memory per step would cost more than the read)."""
    while _PINNED_FREE:
        b = _PINNED_FREE.pop()
        if b.numel() >= k:
            return b
    return torch.empty(max(k, 16), dtype=torch.int32, pin_memory=True)


def choose_rows_begin(perm, n, mask, given, seed, thresh, anchor, anchor_ref, mask_ref, bounds):
    """First half of choose_rows: launches the flag / count kernel and returns a handle WITHOUT waiting for it, so that
    the caller can enqueue more work (or reach a synchronisation it has to make anyway) before the counts are read."""
    L = _lib.lib()
    dev = (perm if perm is not None else anchor if anchor is not None else mask).device
    mask_u8, given_u8, mref_u8 = _u8(mask), _u8(given), _u8(mask_ref)
    nlev = len(bounds) - 1
    nblk = int(L.cgs_ctx_choose_blocks(n))
    flags = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    counts = torch.empty(max(nblk, 1), dtype=torch.int32, device=dev)
    # the blocks' closing atomics spread over CHOOSE_SLOTS lines (one counter for ~1000 blocks serialises on its address); the host
    # adds the slots up after the read it makes anyway
    slots, sw = CHOOSE_SLOTS, int(L.cgs_ctx_choose_slot_ints())
    meta = torch.empty(slots * sw, dtype=torch.int32, device=dev)
    b_host = (C.c_int64 * (nlev + 1))(*[int(b) for b in bounds])
    args = (_lib.ptr(perm), n, _lib.ptr(mask_u8), _lib.ptr(given_u8), int(seed), float(thresh),
            _lib.ptr(None if anchor is None else _c(anchor)), _lib.ptr(None if anchor_ref is None else _c(anchor_ref)), _lib.ptr(mref_u8),
            b_host, nlev, _lib.ptr(flags), _lib.ptr(counts), _lib.ptr(meta))
    _lib.check(L.cgs_ctx_choose_flags_slots(*args, slots, _lib.current_stream()), "cgs_ctx_choose_flags_slots")
    # the counts travel to a pinned host buffer behind the kernel, with an event of their own: choose_rows_end waits for
    # THAT copy (long finished by then) instead of draining whatever the caller has queued since
    pinned = _pinned_i32(slots * sw)
    pinned[:slots * sw].copy_(meta, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    return dict(perm=perm, n=n, nlev=nlev, flags=flags, counts=counts, meta=meta, b_host=b_host, dev=dev,
                keep=(mask_u8, given_u8, mref_u8), pinned=pinned, event=ev, slots=(slots, sw))


def choose_rows_end(h):
    """Second half: read the counts (the step's synchronisation of the context model), compact the chosen rows."""
    L = _lib.lib()
    h["event"].synchronize()
    slots, sw = h["slots"]
    k_ = 2 + h["nlev"]
    part = h["pinned"][:slots * sw].view(slots, sw)[:, :k_]
    host = [int(bool(part[:, 0].any()))] + [int(v) for v in part[:, 1:].sum(dim=0).tolist()]
    _PINNED_FREE.append(h.pop("pinned"))
    stale, live, per_level = bool(host[0]), int(host[1]), [int(v) for v in host[2:]]
    total = sum(per_level)
    dev = h["dev"]
    nz = torch.empty(total, dtype=torch.int64, device=dev)
    rows = torch.empty(total, dtype=torch.int64, device=dev)
    loc = torch.empty(total, dtype=torch.int64, device=dev)
    sub_map = None
    if total > 0 and not stale:
        sub_map = torch.empty(max(h["n"], 1), dtype=torch.int32, device=dev)
        c_host = (C.c_int64 * h["nlev"])(*per_level)
        _lib.check(L.cgs_ctx_choose_compact(_lib.ptr(h["flags"]), _lib.ptr(h["counts"]), _lib.ptr(h["perm"]), h["n"],
                                            h["b_host"], h["nlev"], _lib.ptr(nz), _lib.ptr(rows), _lib.ptr(loc),
                                            _lib.ptr(sub_map), c_host, _lib.current_stream()), "cgs_ctx_choose_compact")
    return stale, live, per_level, nz, rows, loc, sub_map


def choose_rows(perm, n, mask, given, seed, thresh, anchor, anchor_ref, mask_ref, bounds):
    """The rate subset of one training step in coding order (csrc/ctx_plan.hip): two launches and ONE host read.

    perm: int64 [n] coding-order permutation (None = identity); mask / given / mask_ref: bool [n] or None; anchor /
    anchor_ref: float32 [n,3] or None (plan-validity check); bounds: python list of the level boundaries in coding
    order.  Returns (stale, live_count, per-level counts, nz, rows, loc, sub_map) — nz / rows / loc hold, for every
    chosen row in coding order, its coding-order position, original anchor index and level-local position; sub_map
    (int32 [n], coding order) is the inverse per level: a row's index in its level's part of the chosen list or -1
    (None when nothing was compacted); `stale` says the
    anchors / mask no longer equal the reference copies (the caller rebuilds its plan and calls again)."""
    return choose_rows_end(choose_rows_begin(perm, n, mask, given, seed, thresh, anchor, anchor_ref, mask_ref, bounds))


# ---- one launch per level and direction for the every-row half of the level loop (csrc/ctx_level.hip) ---------------
# A/B knob, default: the context levels' forward (in_dim 71) hands its hidden layer to the backward (cgs_ctx_level_fwd_h / _bwd_h,
# +416 B per row kept between the two).  CGS_CTXL_KEEP_H=0: the backward recomputes it from X (cgs_ctx_level_bwd2).  The first level
# (in_dim 15) always recomputes: its 28 layer-1 MFMAs per tile cost what the hand-over's bytes do — profiles/ctxl_hidden_handover.txt
KEEP_H = os.environ.get("CGS_CTXL_KEEP_H", "1") != "0"


_LEVEL_DIMS = (50, 6, 30, 12, 100, 175)      # features, scaling, offsets, hyper, hidden, outputs of mlp_grid: the kernels' instance


def level_fused_supported(seq, anchor, hyp, src) -> bool:
    """Shapes / layouts cgs_ctx_level_* are instantiated for: the reference's dimensions (feat 50, scaling 6, 10 offsets,
    hyper 12, mlp_grid {71|15} -> 100 -> 175) read through a RowSource."""
    try:
        l1, l2 = seq[0], seq[2]
        ok = (len(seq) == 3 and l1.out_features == 100 and l2.out_features == 175 and l1.in_features in (71, 15))
    except Exception:
        return False
    return bool(ok and src is not None and src.f.shape[1] == 50 and src.s.shape[1] == 6 and src.o.shape[1] == 30
                and hyp.dim() == 2 and hyp.shape[1] == 12 and hyp.dtype == _f32 and hyp.is_cuda
                and anchor.dtype == _f32 and anchor.is_cuda and anchor.dim() == 2 and anchor.shape[1] == 3)


# What a level's node keeps of level_fused()'s arguments (a_mask: uint8 [N] or None).  `outs` and `pre` travel beside it: they are
# the node's outputs.
_LevelCfg = collections.namedtuple("_LevelCfg", "a_rows a_mask pos n_stat src rows seed q0 csr loc side rate_lazy hyp_direct need_grad",
                                   defaults=(None, None, None, False, None, False))


def _level_bwd_subset(ctx, saved, d_pred):
    """Step 1, the rate subset's branch of mlp_grid: -> ((dW1, db1, dW2, db2) this module's weight gradients so far, dx_sub [m, in]
    the branch's input-row gradient or None).  Its input gradient rides into the level kernel as compact rows."""
    from . import mlp as _mlp
    _X, x_sub, h_sub, W1, _b1, W2, _b2, _H = saved
    n, in_f, hid, out, n_stat, m = ctx.dims
    dev = W1.device
    if ctx.lazy:
        # the rate node's backward (cgs_rate_sub_bwd) already ran: its weight gradients are the start of this module's
        # (no zero fill), its input-row gradient rides along
        dx_sub, dW = ctx.cfg.side.take_branch()
        if dW is not None:
            return dW, dx_sub
    dW = _mlp._zeros_views(dev, (hid, in_f), (hid,), (out, hid), (out,))      # one fill for the module
    dx_sub = None
    if (not ctx.lazy) and d_pred is not None and m > 0:
        ws = _mlp._wgrad_workspace(dev)
        dz1s = torch.empty(m, hid, dtype=_f32, device=dev)
        dx_sub = torch.empty(m, in_f, dtype=_f32, device=dev)
        _lib.check(_lib.lib().cgs_mlp2_backward(
            in_f, hid, out, 0, _lib.ptr(x_sub), in_f, _lib.ptr(W1), None, _lib.ptr(W2), None, _lib.ptr(_c(d_pred)), out, _lib.ptr(h_sub),
            _lib.ptr(dx_sub), in_f, 0, _lib.ptr(dz1s), None, *[_lib.ptr(t) for t in dW], m, _lib.ptr(ws), ws.numel(),
            _lib.current_stream()), "cgs_mlp2_backward")
    return dW, dx_sub


def _level_bwd_launch(ctx, saved, grads, dW, dx_sub):
    """Step 2, the level kernel: parameter-row gradients into the RowSource's buffers (rate gradients added from the RateSide),
    mlp_grid's step-size branch.  -> (dX [n, in], d_hyp: the hyper latents' gradient for autograd, or None when it went direct)"""
    L = _lib.lib()
    X, _xs, _hs, W1, b1, W2, b2, H = saved
    cfg = ctx.cfg
    n, in_f, hid, _out, n_stat, m = ctx.dims
    dev, stream = X.device, _lib.current_stream()
    smap, *sd = cfg.side.take() if cfg.side is not None else RateSide._ABSENT
    if smap is None and dx_sub is not None and not ctx.lazy:
        # no rate side (gradients of y / Q came through autograd) but a subset branch: its rows still need a map
        smap = _sub_map(cfg.loc, n)
        z = torch.zeros(m, 50 + 6 + 30 + 3, dtype=_f32, device=dev)
        sd = [t.contiguous() for t in torch.split(z, [50, 6, 30, 3], dim=1)]
    dxf, dxs, dxo = cfg.src.grad_buffers()
    dX = torch.empty(n, in_f, dtype=_f32, device=dev)
    ws2 = torch.empty(int(L.cgs_ctx_level_bwd_scratch_bytes()), dtype=torch.uint8, device=dev)
    d_hyp_rows = _hyper_rows_direct(cfg.hyp_direct, ctx.needs_input_grad[3], n, int(dxf.shape[0]), dev)
    dW1, db1, dW2, db2 = dW
    # with the forward's hidden layer when it was kept (the recompute's bits, a third fewer matrix products), else from X alone
    bwd_args = (
        in_f, _lib.ptr(X), _lib.ptr(W1), _lib.ptr(b1), W2.data_ptr() + 4 * n_stat * hid, b2.data_ptr() + 4 * n_stat,
        *[_lib.ptr(t) for t in grads], n, cfg.seed, *cfg.q0, _lib.ptr(cfg.rows), int(dxf.shape[0]), _lib.ptr(dxf), _lib.ptr(dxs),
        _lib.ptr(dxo), _lib.ptr(smap), int(sd[0].shape[0]) if sd[0] is not None else 0, *[_lib.ptr(t) for t in sd],
        _lib.ptr(dx_sub), _lib.ptr(dX), _lib.ptr(d_hyp_rows), _lib.ptr(dW1), _lib.ptr(db1), dW2.data_ptr() + 4 * n_stat * hid,
        db2.data_ptr() + 4 * n_stat)
    # (an instrumented cgs_ctx_level_bwd2 — a caller that wrapped the entry to see the level backward start, as the multi-rank
    #  sequence test does — is honoured: the recompute path, the same bits)
    if H is not None and type(L.cgs_ctx_level_bwd2) is type(L.cgs_ctx_level_bwd_h):
        _lib.check(L.cgs_ctx_level_bwd_h(*bwd_args, _lib.ptr(H), _lib.ptr(ws2), ws2.numel(), stream), "cgs_ctx_level_bwd_h")
    else:
        _lib.check(L.cgs_ctx_level_bwd2(*bwd_args, _lib.ptr(ws2), ws2.numel(), stream), "cgs_ctx_level_bwd")
    cfg.src.rows_written += n
    if d_hyp_rows is not None:
        cfg.hyp_direct[0].done.add(cfg.hyp_direct[1])
        return dX, None
    return dX, dX[:, in_f - 12:] if ctx.needs_input_grad[3] else None      # a column slice: its consumer takes strided rows


def _level_bwd_context_inputs(ctx, dX, d_anchor, gf, gs):
    """Step 3, a context level (X = [anchor[a_rows] | base_f[pos] | base_s[pos] | hyper]): the parents' rows, summed over their
    children without atomics.  -> (d_f, d_s) for autograd, None where the sums went into the earlier levels' own gradient rows."""
    cfg, need = ctx.cfg, ctx.needs_input_grad
    _a_shape, f_shape, s_shape = ctx.shapes
    dev = dX.device
    in_f_ = _prefix_inplace(cfg.src, gf, f_shape, need[1])
    in_s_ = _prefix_inplace(cfg.src, gs, s_shape, need[2])
    d_f = in_f_ if in_f_ is not None else (torch.empty(f_shape, dtype=_f32, device=dev) if need[1] else None)
    d_s = in_s_ if in_s_ is not None else (torch.empty(s_shape, dtype=_f32, device=dev) if need[2] else None)
    if d_anchor is not None or d_f is not None or d_s is not None:
        offs, order, prow = cfg.csr
        acc = int(ctx.share_anchor) | (2 if in_f_ is not None else 0) | (4 if in_s_ is not None else 0)
        _lib.check(_lib.lib().cgs_ctx_gather_bwd_acc(
            _lib.ptr(dX), int(dX.shape[1]), int(f_shape[0]), _lib.ptr(offs), _lib.ptr(order), _lib.ptr(prow), _lib.ptr(d_anchor),
            _lib.ptr(d_f), _lib.ptr(d_s), 3, 50, 6, acc, _lib.current_stream()), "cgs_ctx_gather_bwd")
    return None if in_f_ is not None else d_f, None if in_s_ is not None else d_s


def _level_bwd_first_inputs(ctx, dX, d_anchor):
    """Step 4, the first level (X = [anchor[a_rows] * mask | hyper]): the anchor rows."""
    if d_anchor is None:
        return
    cfg = ctx.cfg
    # (the hyper columns of dX leave as a strided slice: mode 0 = no store for that source)
    # (shared buffer: these rows may carry an earlier level's sums — mode 2 adds; the rows are distinct, the atomics uncontended)
    _lib.check(_lib.lib().cgs_rowcat_bwd_masked(
        2, _ptrs([d_anchor, None]), _ptrs([cfg.a_rows, None]), _ptrs([cfg.a_mask, None]), _ints([3, 12]), _ints([3, 12]),
        _ints([2 if ctx.share_anchor else 1, 0]), int(dX.shape[0]), _lib.ptr(dX), _lib.current_stream()), "cgs_rowcat_bwd")


class _LevelFused(torch.autograd.Function):
    """One level of the training level loop (scene/gaussian_model.py:1594-1616) as ONE node and one launch per direction for
    the work that runs on every row: input-row assembly (:1596-1599 / :1711-1724), mlp_grid's hidden layer and three step-size
    outputs (:1600-1608), the noisy values of the level's rows of the three parameter tensors (:1610-1616) — cgs_ctx_level_fwd /
    cgs_ctx_level_bwd (weight gradients of that branch inside the backward kernel) — plus the mean / scale outputs on the rate
    subset `loc` (the same fused MLP kernels as mlp._LevelMLP, on rows of the X the level kernel wrote).

    cfg: a _LevelCfg; outs = (yf, ys, yo) the slices to write — see level_fused()."""

    @staticmethod
    def launch(anchor, base_f, base_s, hyp, W1, b1, W2, b2, cfg, outs):
        """The forward's launch on plain values (no autograd): (X, Q, (W1c, b1c, W2c, b2c), H) — H: the hidden layer's hand-over to
        the backward (a private byte buffer; None when cfg.need_grad is false or KEEP_H is off).  Called by forward(), or EARLIER by
        level_fused_launch() — the level kernels of a step need nothing the host has to wait for, so context_model enqueues them in
        front of the rate subset's read-back and hands the result to forward() as `pre`."""
        from . import mlp as _mlp
        L = _lib.lib()
        _mlp._drop_stale_deferred()
        src, rows, a_rows = cfg.src, cfg.rows, cfg.a_rows
        anchor_c, hyp_c = _c(anchor.detach()), _c(hyp.detach())
        W1c, b1c, W2c, b2c = (t.detach().contiguous() for t in (W1, b1, W2, b2))
        n, in_f = int(rows.shape[0]), int(W1c.shape[1])
        hid, out, n_stat = int(W1c.shape[0]), int(W2c.shape[0]), cfg.n_stat
        assert (hid, out, out - n_stat) == (100, 175, 3) and rows.dtype == torch.int64 and rows.is_contiguous()
        ctxlevel = base_f is not None
        assert in_f == (71 if ctxlevel else 15) and hyp_c.shape == (n, 12)
        bf = _c(base_f.detach()) if ctxlevel else None
        bs = _c(base_s.detach()) if ctxlevel else None
        assert a_rows.dtype == torch.int64 and a_rows.is_contiguous() and int(a_rows.shape[0]) == n
        _lib.require_device(anchor_c, hyp_c, W1c, W2c, src.f)
        dev = anchor_c.device
        src.rows_read += n
        yf, ys, yo = outs
        assert yf.shape == (n, 50) and ys.shape == (n, 6) and yo.shape == (n, 30)
        assert yf.is_contiguous() and ys.is_contiguous() and yo.is_contiguous()
        X = torch.empty(n, in_f, dtype=_f32, device=dev)
        Q = torch.empty(n, 3, dtype=_f32, device=dev)
        H = None
        if KEEP_H and cfg.need_grad and n > 0 and in_f == 71:
            H = torch.empty(int(L.cgs_ctx_level_hidden_bytes(n)), dtype=torch.uint8, device=dev)
        _lib.check(L.cgs_ctx_level_fwd_h(
            in_f, _lib.ptr(anchor_c), int(anchor_c.shape[0]), _lib.ptr(a_rows), _lib.ptr(cfg.a_mask), _lib.ptr(bf), _lib.ptr(bs),
            int(bf.shape[0]) if ctxlevel else 0, _lib.ptr(cfg.pos), _lib.ptr(hyp_c), n, _lib.ptr(W1c), _lib.ptr(b1c), W2c.data_ptr() + 4 * n_stat * hid, b2c.data_ptr() + 4 * n_stat, _lib.ptr(src.f),
            _lib.ptr(src.s), _lib.ptr(src.o), _lib.ptr(rows), cfg.seed, *cfg.q0, _lib.ptr(X), _lib.ptr(yf), _lib.ptr(ys),
            _lib.ptr(yo), _lib.ptr(Q), _lib.ptr(src.sums_buffer()), _lib.ptr(H), _lib.current_stream()), "cgs_ctx_level_fwd_h")
        return X, Q, (W1c, b1c, W2c, b2c), H

    @staticmethod
    def forward(ctx, anchor, base_f, base_s, hyp, W1, b1, W2, b2, _token, cfg, outs, pre):
        if pre is None:
            pre = _LevelFused.launch(anchor, base_f, base_s, hyp, W1, b1, W2, b2,
                                     cfg._replace(need_grad=any(ctx.needs_input_grad)), outs)
        X, Q, (W1c, b1c, W2c, b2c), H = pre
        loc = cfg.loc
        n, in_f = int(cfg.rows.shape[0]), int(W1c.shape[1])
        hid, out = int(W1c.shape[0]), int(W2c.shape[0])
        dev = X.device
        pred = x_sub = h_sub = None
        m = 0 if loc is None else int(loc.shape[0])
        lazy = cfg.rate_lazy and loc is not None and cfg.side is not None
        if lazy:
            # the mean / scale outputs of the chosen rows are formed inside the rate kernels (cgs_rate_sub_*): nothing here
            cfg.side.lend(X, (W1c, b1c, W2c, b2c))
        elif loc is not None:
            x_sub = gather_rows_nograd(X, loc)
            pred = torch.empty(m, out, dtype=_f32, device=dev)
            h_sub = torch.empty(m, hid, dtype=_f32, device=dev)
            _lib.check(_lib.lib().cgs_mlp2_forward(
                in_f, hid, out, 0, _lib.ptr(x_sub), in_f, _lib.ptr(W1c), _lib.ptr(b1c), _lib.ptr(W2c), _lib.ptr(b2c), _lib.ptr(pred),
                out, _lib.ptr(h_sub), m, _lib.current_stream()), "cgs_mlp2_forward")
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(X, x_sub, h_sub, W1c, b1c, W2c, b2c, H)      # (H is no output of this node: no cycle, see below)
        # (`outs` and `pre` stay off ctx: they are this node's OUTPUTS — an output kept on its own ctx is a reference cycle through
        #  the C++ node that Python's collector cannot see: every step's level nodes, RowSource and ~350 MB of level tensors stayed
        #  alive for the life of the process, found in round 5 when the device filled up — tools/leak_probe.py)
        ctx.cfg, ctx.dims, ctx.lazy = cfg, (n, in_f, hid, out, cfg.n_stat, m), lazy
        ctx.shapes = (tuple(anchor.shape), None if base_f is None else tuple(base_f.shape), None if base_s is None else tuple(base_s.shape))
        ctx.share_anchor = _anchor_shared(ctx.needs_input_grad[0])
        if ctx.share_anchor:
            cfg.src.anchor_register()
        if pred is None:
            pred = torch.empty(0, out, dtype=_f32, device=dev)
        return (*outs, Q, pred)

    @staticmethod
    def backward(ctx, gf, gs, go, gQ, d_pred):
        src, need = ctx.cfg.src, ctx.needs_input_grad
        gf, gs, go, gQ = (None if t is None else _c(t) for t in (gf, gs, go, gQ))
        saved = ctx.saved_tensors
        dW, dx_sub = _level_bwd_subset(ctx, saved, d_pred)
        dX, d_hyp = _level_bwd_launch(ctx, saved, (gf, gs, go, gQ), dW, dx_sub)
        a_shape, f_shape, _s_shape = ctx.shapes
        if ctx.share_anchor:
            d_anchor = src.anchor_target(a_shape, dX.device)
        else:
            d_anchor = torch.zeros(a_shape, dtype=_f32, device=dX.device) if need[0] else None
        d_f = d_s = None
        if f_shape is not None:
            d_f, d_s = _level_bwd_context_inputs(ctx, dX, d_anchor, gf, gs)
        else:
            _level_bwd_first_inputs(ctx, dX, d_anchor)
        if ctx.share_anchor:
            d_anchor = src.anchor_release()          # (None unless this is the last level of the backward: that one hands it on)
        return (d_anchor, d_f, d_s, d_hyp, *dW, None, None, None, None)


def level_fused_launch(anchor, base_f, base_s, hyp, seq, n_stat, a_rows, a_mask, pos, src, rows, outs, q0, seed):
    """The launch of level_fused() on plain values, for a caller that creates the node later: returns `pre` for level_fused(pre=)
    (same arguments, same seed).  base_f / base_s: the coded prefix's VALUES (the buffers the earlier levels' launches wrote)."""
    l1, l2 = seq[0], seq[2]
    cfg = _LevelCfg(a_rows=a_rows, a_mask=_u8(a_mask), pos=pos, n_stat=int(n_stat), src=src, rows=rows, seed=int(seed),
                    q0=tuple(float(v) for v in q0), need_grad=torch.is_grad_enabled())
    return _LevelFused.launch(anchor, base_f, base_s, hyp, l1.weight, l1.bias, l2.weight, l2.bias, cfg, outs)


def level_fused(anchor, base_f, base_s, hyp, seq, n_stat, loc, a_rows, a_mask, pos, csr, src, rows, outs, side, q0, seed=None,
                rate_lazy=False, pre=None):
    """One level of the training level loop.  anchor [N,3]; base_f / base_s: the coded prefix (None for the first level);
    hyp [n,12] the level's noisy hyper latents; seq = mlp_grid[level]; loc: level rows of the rate subset (or None);
    a_rows [n]: anchor row of every level row; a_mask: bool [N] (first level from level 1 up) or None; pos [n]: the parents'
    prefix positions; csr: their children lists (cgs_ctx_gather_bwd); src / rows: RowSource and the level's slice of the coding
    permutation; outs = (yf, ys, yo) slices to write; side: RateSide or None.
    rate_lazy (needs side): the mean / scale outputs of the chosen rows are NOT formed here — rate_all() runs them inside
    the fused rate kernels (cgs_rate_sub_*) from the X this node leaves on `side`; pred is then an empty tensor.
    Returns (yf, ys, yo, Q [n,3], pred [len(loc),175] or an empty tensor)."""
    l1, l2 = seq[0], seq[2]
    cfg = _LevelCfg(a_rows=a_rows, a_mask=_u8(a_mask), pos=pos, csr=csr, loc=loc, n_stat=int(n_stat), src=src, rows=rows,
                    seed=next_seed() if seed is None else int(seed), q0=tuple(float(v) for v in q0), side=side,
                    rate_lazy=bool(rate_lazy), hyp_direct=getattr(hyp, "_cgs_hyp_direct", None))
    return _LevelFused.apply(anchor, base_f, base_s, hyp, l1.weight, l1.bias, l2.weight, l2.bias, src.token, cfg, outs, pre)
