"""Cost of the per-Gaussian contribution walk (csrc/raster_contrib.hip) at the bench view: the scene bench.py builds (1 M
anchors, seed 0), its first orbit camera, 1920x1080, eval-mode Gaussians.  One process, the cases alternating, after warm-up,
device events around single C-ABI calls on the workspaces one forward left behind:

  cgs_raster_contrib            everything asked (four accumulators, three maps)
  cgs_raster_contrib            the three maps only (no per-entry reduction, no global atomics)
  cgs_raster_contrib            the four accumulators only
  cgs_raster_contrib            everything, through a slot table (identity) instead of NULL
  cgs_raster_render_aux         the yardstick: the same walk, three maps, no reduction (one kernel: aux_fwd)
  cgs_raster_render_features    at C = 1 (one kernel: feat_fwd)

The per-kernel times of the same cases come from running this script under `rocprofv3 --kernel-trace --stats` with
--iters 3 --warmup 1 (no counters in that run).

  python tools/contrib_micro.py [--anchors 1000000] [--iters 10] [--warmup 3] [--out FILE]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", type=int, default=1_000_000)
    ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--H", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contrib_micro: needs the GPU")
    from contextgs_amd import _lib, rasterizer as rz
    from contextgs_amd.renderer import _raster_settings, generate_neural_gaussians, prefilter_voxel
    from contextgs_amd.synth import SynthPipe, make_scene, orbit_cameras

    W, H = a.W, a.H
    pc = make_scene(a.anchors, seed=0)
    pc.eval()
    pipe, bg = SynthPipe(), torch.zeros(3, device="cuda")
    cam = orbit_cameras(8, W, H)[0].to_torch("cuda")
    with torch.no_grad():
        vis = prefilter_voxel(cam, pc, pipe, bg)
        xyz, color, opacity, scaling, rot, _ = generate_neural_gaussians(cam, pc, vis, is_training=False)
        P = int(xyz.shape[0])
        rast = rz.GaussianRasterizer(_raster_settings(cam, pipe, bg, 1.0))
        _, radii, first = rast(means3D=xyz, means2D=torch.zeros_like(xyz), opacities=opacity, colors_precomp=color,
                               scales=scaling, rotations=rot, return_aux=True, contrib=True)
    lc = dict(rz.last_call)
    cfg, geom, binws, img, R = lc["cfg"], lc["geom_ws"], lc["bin_ws"], lc["img_ws"], lc["bin_R"]
    L = _lib.lib()
    p = _lib.ptr
    stream = _lib.current_stream()
    ws = (cfg.ref, P, R, p(geom), geom.numel(), p(binws), binws.numel(), p(img), img.numel())

    dev = "cuda"
    maps = [torch.empty(1, H, W, device=dev) for _ in range(3)]
    ones = torch.ones(P, 1, device=dev)
    fmap = torch.empty(1, H, W, device=dev)
    acc = rz.GaussianContrib.zeros(P, dev)
    top_id = torch.empty(H, W, dtype=torch.int32, device=dev)
    top_w = torch.empty(1, H, W, device=dev)
    count = torch.empty(H, W, dtype=torch.int32, device=dev)
    ident = torch.arange(P, dtype=torch.int32, device=dev)
    A = [p(t) for t in acc.tensors()]
    M = [p(top_id), p(top_w), p(count)]
    N4, N3 = [None] * 4, [None] * 3

    def contrib(accs, outs, slot=None):
        _lib.check(L.cgs_raster_contrib(*ws, slot, P, *accs, *outs, stream), "cgs_raster_contrib")

    cases = {
        "contrib: accumulators + maps": lambda: contrib(A, M),
        "contrib: maps only": lambda: contrib(N4, M),
        "contrib: accumulators only": lambda: contrib(A, N3),
        "contrib: all, identity slot table": lambda: contrib(A, M, p(ident)),
        "aux (depth, invdepth, alpha)": lambda: _lib.check(L.cgs_raster_render_aux(
            *ws, p(maps[0]), p(maps[1]), p(maps[2]), stream), "cgs_raster_render_aux"),
        "features C=1": lambda: _lib.check(L.cgs_raster_render_features(*ws, p(ones), 1, p(fmap), stream),
                                           "cgs_raster_render_features"),
    }
    for _ in range(a.warmup):
        for f in cases.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(a.iters):
        for k, f in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    con = first["contrib"]
    lines = [f"# tools/contrib_micro.py: {a.anchors} anchors, {W}x{H}, P={P} Gaussians, visible {int((radii > 0).sum())}, "
             f"{lc['num_rendered']} pairs, {torch.cuda.get_device_name(0)}, device events, {a.iters} alternating rounds after "
             f"{a.warmup} warm-up rounds",
             f"# one view: {int((con.pixels > 0).sum())} Gaussians contributed, {int(con.pixels.sum())} (pixel, Gaussian) "
             f"contributions, {int((first['top_id'] >= 0).sum())} of {H * W} pixels covered, "
             f"sum of weight {float(con.weight.double().sum()):.1f} vs alpha map {float(first['alpha'].double().sum()):.1f}",
             f"{'case':<36s} {'median ms':>10s} {'min ms':>10s} {'x aux':>8s}"]
    aux = med["aux (depth, invdepth, alpha)"]
    for k, v in times.items():
        lines.append(f"{k:<36s} {med[k]:10.3f} {min(v):10.3f} {med[k] / aux:8.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
