"""One optimizer step at the benchmark's size: torch's two Adam paths, FusedAdam dense, FusedAdam row-sparse.

The parameter shapes are the model's own — `make_scene(anchors)` and `training_setup`, all 13 groups — with synthetic gradients
on every parameter (the state of a late training step: every tensor has moments).  Each variant owns a copy of the parameters;
the variants ALTERNATE inside one run (round r times variant 0, 1, 2, ...), one step each between two device events, so that
clock and memory state drift hits all of them alike.  Every step is timed twice: on an IDLE device (the interval then contains
the host's work in front of the first launch) and QUEUED behind ~1.5 ms of fills (the host runs ahead, as it does inside a
training iteration: the interval is the device work alone).  Next to each median: the HBM floor of the elements the step touches,
28 B each (read p, g, m, v; write p, m, v) at the 6.29 TB/s copy rate of the MI355X guide.  For a sparse step the floor counts
the visible rows of the six row-sparse groups, every row of the others, and one byte per row of the mask per sparse tensor.

Usage:  python tools/adam_micro.py [--anchors 1000000] [--rounds 30] [--warmup 5] [--out profiles/fused_adam.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 6.29e12       # B/s
ARGS = dict(
    percent_dense=0.01, position_lr_init=0.0, position_lr_final=0.0, position_lr_delay_mult=0.01, position_lr_max_steps=30000,
    offset_lr_init=0.01, offset_lr_final=0.0001, offset_lr_delay_mult=0.01, offset_lr_max_steps=30000,
    mask_lr_init=0.01, mask_lr_final=0.0001, mask_lr_delay_mult=0.01, mask_lr_max_steps=30000,
    feature_lr=0.0075, hyper_latent_lr=0.0075, opacity_lr=0.02, scaling_lr=0.007, rotation_lr=0.002,
    mlp_opacity_lr_init=0.002, mlp_opacity_lr_final=0.00002, mlp_opacity_lr_delay_mult=0.01, mlp_opacity_lr_max_steps=30000,
    mlp_cov_lr_init=0.004, mlp_cov_lr_final=0.004, mlp_cov_lr_delay_mult=0.01, mlp_cov_lr_max_steps=30000,
    mlp_color_lr_init=0.008, mlp_color_lr_final=0.00005, mlp_color_lr_delay_mult=0.01, mlp_color_lr_max_steps=30000,
    latent_codec_lr_init=0.005, latent_codec_lr_final=0.00001, latent_codec_lr_delay_mult=0.33, latent_codec_lr_max_steps=30000,
    mlp_grid_lr_init=0.005, mlp_grid_lr_final=0.00001, mlp_grid_lr_delay_mult=0.01, mlp_grid_lr_max_steps=30000)


def variant(groups, cls, **kw):
    """A `cls` over fresh copies of the template's parameters, gradients attached."""
    new = []
    for g in groups:
        ps = []
        for p in g["params"]:
            q = torch.nn.Parameter(p.detach().clone())
            q.grad = torch.randn_like(q) * 1e-3
            ps.append(q)
        new.append({**{k: v for k, v in g.items() if k != "params"}, "params": ps})
    return cls(new, lr=0.0, eps=1e-15, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from contextgs_amd.optim import FusedAdam
    from contextgs_amd.synth import make_scene
    torch.manual_seed(0)
    pc = make_scene(a.anchors, seed=0)
    pc.spatial_lr_scale = 1.0
    pc._rotation.requires_grad_(True); pc._opacity.requires_grad_(True)
    opts = {}
    for kind in ("default", "sparse_adam"):
        pc.training_setup(types.SimpleNamespace(optimizer_type=kind, **ARGS))
        opts[kind] = [{k: (list(v) if k == "params" else v) for k, v in g.items()
                       if k in ("params", "lr", "name", "row_sparse")} for g in pc.optimizer.param_groups]
    plain = [{k: v for k, v in g.items() if k != "row_sparse"} for g in opts["default"]]
    N = pc._anchor.shape[0]
    total = sum(p.numel() for g in plain for p in g["params"])
    sparse_el = sum(p.numel() for g in opts["sparse_adam"] if g.get("row_sparse") for p in g["params"])
    n_sparse_t = sum(1 for g in opts["sparse_adam"] if g.get("row_sparse"))
    gen = torch.Generator().manual_seed(1)
    masks = {f: (torch.rand(N, generator=gen) < f).cuda() for f in (0.05, 0.2, 0.5)}

    runs = [("torch default (foreach)", variant(plain, torch.optim.Adam), None, total * 28),
            ("torch fused=True", variant(plain, torch.optim.Adam, fused=True), None, total * 28),
            ("FusedAdam dense", variant(plain, FusedAdam), "dense", total * 28)]
    for f, m in masks.items():
        vis = float(m.float().mean())
        runs.append((f"FusedAdam sparse, {vis:.3f} of the rows visible", variant(opts["sparse_adam"], FusedAdam), m,
                     ((total - sparse_el) + sparse_el * vis) * 28 + n_sparse_t * N))
    times = {mode: [[] for _ in runs] for mode in ("queued", "idle")}
    busy = torch.empty(1 << 28, dtype=torch.float32, device="cuda")          # 1 GiB
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for r in range(a.warmup + a.rounds):
        for mode in ("queued", "idle"):
            for k, (_, opt, rows, _) in enumerate(runs):
                torch.cuda.synchronize()
                if mode == "queued":
                    for _ in range(4):
                        busy.fill_(float(r))
                e0, e1 = ev(), ev()
                e0.record()
                if rows is None:
                    opt.step()
                else:
                    opt.step(rows=None if isinstance(rows, str) else rows)
                e1.record()
                e1.synchronize()
                if r >= a.warmup:
                    times[mode][k].append(e0.elapsed_time(e1))
    lines = [f"adam_micro: {N} anchors, {sum(len(g['params']) for g in plain)} tensors in {len(plain)} groups, {total} elements "
             f"({sparse_el} in the {n_sparse_t} row-sparse groups), {a.rounds} alternating rounds after {a.warmup} warm-up, "
             f"{torch.cuda.get_device_name(0)}"]
    for mode in ("queued", "idle"):
        lines.append(f"-- {mode}: " + ("device work alone (the host ran ahead behind ~1.5 ms of fills)" if mode == "queued" else
                                       "device idle at the first event (host time in front of the first launch included)"))
        lines.append(f"{'variant':58s} {'median ms':>10s} {'min ms':>9s} {'max ms':>9s} {'floor ms':>9s} {'median/floor':>13s}")
        for (name, _, _, nbytes), t in zip(runs, times[mode]):
            floor = nbytes / COPY_RATE * 1e3
            med = statistics.median(t)
            lines.append(f"{name:58s} {med:10.3f} {min(t):9.3f} {max(t):9.3f} {floor:9.3f} {med / floor:13.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
