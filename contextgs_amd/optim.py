"""`FusedAdam`: the optimizer step of the training iteration in one HIP launch, with a visible-rows sparse mode.

The reference builds `torch.optim.Adam(l, lr=0.0, eps=1e-15)` over 13 parameter groups (scene/gaussian_model.py:475) and
calls `gaussians.optimizer.step()` as the last statement of the loop (train.py:255).  Upstream's rasterizer package
ships a fused `SparseGaussianAdam` next to the rasterizer and gsplat a `SelectiveAdam`; this is that operator for the
anchor model, on `cgs_adam_step` (csrc/adam.hip).

  FusedAdam(params, lr=..., betas=..., eps=..., weight_decay=...)      a torch.optim.Adam subclass: only `step` differs
  opt.step(closure=None, rows="auto")

Everything but `step` is torch's: param groups, `state_dict` / `load_state_dict`, `add_param_group`, the per-group `lr`
that `update_learning_rate` rewrites.  The state layout is torch's too — `state[p] = {"step": CPU float scalar,
"exp_avg", "exp_avg_sq"}`, created on a parameter's first gradient — so densify.py's surgery works unchanged and a
checkpoint moves between the two classes in both directions.

The step.  Parameters with `grad is None` are skipped and their step count does not advance.  All others advance by one
and go to the device as descriptors, 32 per launch, on the current stream; nothing in `step` reads the device back.
Per element, in fp32 (torch's `_single_tensor_adam` without amsgrad; L2 `weight_decay` supported):

  g' = g + weight_decay * p                       m = m + (g' - m) * (1 - beta1)
  v  = v * beta2 + g' * g' * (1 - beta2)          p = p - step_size * (m / (sqrt(v) / bias2_sqrt + eps))

with step_size = lr / (1 - beta1^t) and bias2_sqrt = sqrt(1 - beta2^t) computed on the host in double, as torch does.
There are no atomics: a step is bit-reproducible and does not depend on which tensors share a launch.
`amsgrad`, `maximize`, `capturable`, `differentiable`, `decoupled_weight_decay`, `foreach=True` and `fused=True` are
refused at construction.  A parameter the kernel cannot take (not fp32, not contiguous) is stepped by the parent's
implementation, that parameter alone; a sparse gradient raises as the parent does; a CPU parameter raises
RuntimeError (no CPU fallback), like the package's other operators.

Row-sparse mode.  A param group may carry `"row_sparse": True`.  `rows` is
  a bool [N] device tensor   applied to every row_sparse group (each parameter must have shape[0] == N, else ValueError);
                             groups without the flag are always dense — selection is never by shape;
  None                       dense;
  "auto" (default)           the rows the renderer noted for this view (`dist.touched_rows()`), if the note's counter
                             advanced by exactly one since this optimizer's previous step (two renders before one
                             step: the union is unknown), the note is not None, some group is row_sparse and the world
                             size is 1 (with more ranks every replica must apply the same rows); dense otherwise.
Sparse semantics: rows outside the mask keep p, exp_avg and exp_avg_sq BIT FOR BIT — their moments do not decay and the
parameter does not drift on stale momentum, which is upstream's behaviour — and nothing of them is read or written.  The
step count of the parameter still advances, so the bias correction of a visible row uses the parameter's GLOBAL step,
as gsplat's SelectiveAdam does, not the number of times that row was visible.
"""
from __future__ import annotations

import torch
from torch.optim.adam import adam as _torch_adam

from . import _lib
from . import dist as _dist

MAX_PER_LAUNCH = 32          # CGS_ADAM_MAX
_REFUSED = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay", "foreach", "fused")


def _scalar_dtype():
    return torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32      # torch's dtype of `step`


class FusedAdam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        given = dict(amsgrad=amsgrad, maximize=maximize, capturable=capturable, differentiable=differentiable,
                     decoupled_weight_decay=decoupled_weight_decay, foreach=foreach, fused=fused)
        for name in _REFUSED:
            if given[name]:
                raise ValueError(f"FusedAdam does not support {name}={given[name]!r}")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._note_seen = _dist.touched_rows()[1]

    def load_state_dict(self, state_dict):
        # torch replaces every group's options with the saved ones; a checkpoint of torch.optim.Adam has no row_sparse key
        flags = [g.get("row_sparse", False) for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, f in zip(self.param_groups, flags):
            if f:
                g["row_sparse"] = True

    def resolve_rows(self, rows="auto"):
        """The row mask this step applies to the row_sparse groups (None = dense); consumes the renderer's note."""
        note, count = _dist.touched_rows()
        advanced, self._note_seen = count - self._note_seen, count
        if rows is None:
            return None
        if isinstance(rows, str):
            if rows != "auto":
                raise ValueError(f"rows must be a bool tensor, None or 'auto', not {rows!r}")
            if advanced != 1 or note is None or _dist.world() != 1:
                return None
            rows = note
        if not any(g.get("row_sparse", False) for g in self.param_groups):
            return None
        if rows.dim() != 1 or rows.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"rows must be a bool [N] tensor, not {rows.dtype} {tuple(rows.shape)}")
        return rows

    @torch.no_grad()
    def step(self, closure=None, rows="auto"):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        rows = self.resolve_rows(rows)

        # pass 1: what goes where; every refusal comes before any state changes or any launch
        fused, parent = [], []
        for group in self.param_groups:
            for name in _REFUSED:
                if group.get(name):
                    raise ValueError(f"FusedAdam does not support {name}={group[name]!r} (param group option)")
            if torch.is_tensor(group["lr"]) and group["lr"].is_cuda:
                raise ValueError("FusedAdam: a device tensor lr would need a host read every step")
            sparse = rows is not None and group.get("row_sparse", False)
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                if not p.is_cuda:
                    raise RuntimeError(f"contextgs_amd.optim.FusedAdam runs on the HIP device only (parameter on {p.device}); "
                                       "there is no CPU fallback")
                if sparse and (p.dim() < 1 or p.shape[0] != rows.shape[0]):
                    raise ValueError(f"row_sparse parameter of shape {tuple(p.shape)} in group {group.get('name', '?')!r} "
                                     f"does not have the row mask's {rows.shape[0]} rows")
                st = self.state[p]
                ok = (p.dtype == torch.float32 and g.dtype == torch.float32 and p.is_contiguous() and g.device == p.device
                      and (len(st) == 0 or (st["exp_avg"].is_contiguous() and st["exp_avg_sq"].is_contiguous()
                                            and st["exp_avg"].dtype == torch.float32 and st["exp_avg_sq"].dtype == torch.float32
                                            and not st["step"].is_cuda)))
                (fused if ok else parent).append((group, p, sparse))
        if not fused and not parent:
            return loss

        # pass 2: torch's lazy state, the step counts, the descriptors
        descs, keep = [], []
        for group, p, sparse in fused:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=_scalar_dtype())
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] += 1
            if p.numel() == 0:
                continue
            t = st["step"].item()                  # a CPU scalar: no device read
            beta1, beta2 = group["betas"]
            lr = group["lr"]
            lr = lr.item() if torch.is_tensor(lr) else lr
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            keep.append(g)
            descs.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(),
                          float(beta1), float(beta2), p.numel() // p.shape[0] if sparse else 0,
                          lr / (1 - beta1 ** t), (1 - beta2 ** t) ** 0.5, group["eps"], group["weight_decay"]))
        if descs:
            _lib.require_device(*(p for _, p, _ in fused), rows)
            lib, stream = _lib.lib(), _lib.current_stream()
            if rows is not None:
                rows = rows if rows.is_contiguous() else rows.contiguous()
            rp, nr = (rows.data_ptr(), rows.shape[0]) if rows is not None else (None, 0)
            for at in range(0, len(descs), MAX_PER_LAUNCH):
                part = descs[at:at + MAX_PER_LAUNCH]
                arr = (_lib.AdamTensor * len(part))(*part)
                _lib.check(lib.cgs_adam_step(len(part), arr, rp, nr, stream), "cgs_adam_step")
            # the kernel wrote through raw pointers: tell autograd and the model's version-keyed caches (get_anchor's
            # quantisation, prefilter_voxel's rotation row) what an in-place torch op would have told them
            torch.autograd.graph.increment_version([p for _, p, _ in fused if p.numel()])

        # parameters the kernel does not take: the parent's implementation, one parameter at a time (it advances the step itself)
        for group, p, _ in parent:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=_scalar_dtype())
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            beta1, beta2 = group["betas"]
            _torch_adam([p], [p.grad], [st["exp_avg"]], [st["exp_avg_sq"]], [], [st["step"]], amsgrad=False,
                        has_complex=torch.is_complex(p), beta1=beta1, beta2=beta2, lr=group["lr"],
                        weight_decay=group["weight_decay"], eps=group["eps"], maximize=False,
                        foreach=group["foreach"], capturable=False, differentiable=False, fused=group["fused"],
                        grad_scale=None, found_inf=None, decoupled_weight_decay=False)
        return loss
