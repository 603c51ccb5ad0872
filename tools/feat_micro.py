"""Cost of the N-channel feature blend (csrc/raster_feat.hip) at the bench view: the scene bench.py builds (1 M anchors,
seed 0), its first orbit camera, 1920x1080, eval-mode Gaussians.  One process, the cases alternating, after warm-up, device
events around single C-ABI calls on the workspaces one forward left behind:

  forward   cgs_raster_render_features at C = 3, 8, 32 (one kernel: feat_fwd)
            cgs_raster_render_aux                      (one kernel: aux_fwd)
            cgs_raster_render                          (binning + blend_fwd: the colour blend is not callable alone)
  backward  cgs_raster_backward_feat with exactly one upstream gradient: none (the zero fill + the per-Gaussian backward, the
            floor every other case contains), the colour image (+ blend_bwd), the three maps (+ aux_bwd + the dz chain), the
            feature map at C = 3, 8, 32 (+ feat_bwd).  The table prints each case and its difference to the floor.

The per-kernel times of the same cases (blend_fwd alone among them) come from running this script under
`rocprofv3 --kernel-trace --stats` with --iters 3 --warmup 1.

  python tools/feat_micro.py [--anchors 1000000] [--iters 10] [--warmup 3] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHANNELS = (3, 8, 32)


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
        raise SystemExit("feat_micro: needs the GPU")
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
        rng = np.random.default_rng(0)
        feats = {C: torch.tensor(rng.normal(size=(P, C)).astype(np.float32), device="cuda") for C in CHANNELS}
        rast = rz.GaussianRasterizer(_raster_settings(cam, pipe, bg, 1.0))
        _, radii, _ = rast(means3D=xyz, means2D=torch.zeros_like(xyz), opacities=opacity, colors_precomp=color, scales=scaling,
                           rotations=rot, features=feats[3], return_aux=True)
    lc = dict(rz.last_call)
    cfg, geom, binws, img, R = lc["cfg"], lc["geom_ws"], lc["bin_ws"], lc["img_ws"], lc["bin_R"]
    L = _lib.lib()
    p = _lib.ptr
    stream = _lib.current_stream()
    ws = (cfg.ref, P, R, p(geom), geom.numel(), p(binws), binws.numel(), p(img), img.numel())

    dev = "cuda"
    out3 = torch.empty(3, H, W, device=dev)
    maps = [torch.empty(1, H, W, device=dev) for _ in range(3)]
    fmap = {C: torch.empty(C, H, W, device=dev) for C in CHANNELS}
    g3 = torch.tensor(rng.normal(size=(3, H, W)).astype(np.float32), device=dev)
    gm = [torch.tensor(rng.normal(size=(1, H, W)).astype(np.float32), device=dev) for _ in range(3)]
    gf = {C: torch.tensor(rng.normal(size=(C, H, W)).astype(np.float32), device=dev) for C in CHANNELS}
    xyz, color, opacity, scaling, rot = (t.contiguous() for t in (xyz, color, opacity, scaling, rot))
    acc = torch.zeros(P * 4, device=dev)                      # dL/dcolor | dL/dopacity (summed atomically: zeroed per call)
    rest = torch.empty(P * 13, device=dev)
    d_feat = {C: torch.zeros(P, C, device=dev) for C in CHANNELS}
    scratch = torch.empty(L.cgs_raster_bwd_aux_scratch_bytes(P), dtype=torch.uint8, device=dev)

    def backward(g_col=None, g_maps=(None, None, None), C=None):
        acc.zero_()
        if C is not None:
            d_feat[C].zero_()
        _lib.check(L.cgs_raster_backward_feat(
            cfg.ref, P, R, p(xyz), p(color), None, 0, 0, p(opacity), p(scaling), p(rot), None, p(radii), p(geom), geom.numel(),
            p(binws), binws.numel(), p(img), img.numel(), p(g_col), p(g_maps[0]), p(g_maps[1]), p(g_maps[2]), p(rest[:3 * P]),
            p(rest[3 * P:6 * P]), p(acc[:3 * P]), p(acc[3 * P:]), None, p(rest[6 * P:9 * P]), p(rest[9 * P:]), None, p(scratch),
            scratch.numel(), stream, 0, p(feats[C]) if C else None, C or 0, p(gf[C]) if C else None,
            p(d_feat[C]) if C else None), "cgs_raster_backward_feat")

    cases = {}
    for C in CHANNELS:
        cases[f"fwd features C={C}"] = (lambda C=C: _lib.check(L.cgs_raster_render_features(
            *ws, p(feats[C]), C, p(fmap[C]), stream), "cgs_raster_render_features"))
    cases["fwd aux (depth, invdepth, alpha)"] = lambda: _lib.check(L.cgs_raster_render_aux(
        *ws, p(maps[0]), p(maps[1]), p(maps[2]), stream), "cgs_raster_render_aux")
    cases["fwd colour: binning + blend"] = lambda: _lib.check(L.cgs_raster_render(*ws, p(out3), stream), "cgs_raster_render")
    cases["bwd floor (no upstream gradient)"] = lambda: backward()
    cases["bwd colour"] = lambda: backward(g_col=g3)
    cases["bwd aux (three maps)"] = lambda: backward(g_maps=gm)
    for C in CHANNELS:
        cases[f"bwd features C={C}"] = (lambda C=C: backward(C=C))

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
    floor = med["bwd floor (no upstream gradient)"]
    lines = [f"# tools/feat_micro.py: {a.anchors} anchors, {W}x{H}, P={P} Gaussians, visible {int((radii > 0).sum())}, "
             f"{lc['num_rendered']} pairs, {torch.cuda.get_device_name(0)}, device events, {a.iters} alternating rounds after "
             f"{a.warmup} warm-up rounds",
             f"{'case':<36s} {'median ms':>10s} {'min ms':>10s} {'- floor':>10s}"]
    for k, v in times.items():
        extra = f"{med[k] - floor:10.3f}" if k.startswith("bwd") and "floor" not in k else ""
        lines.append(f"{k:<36s} {med[k]:10.3f} {min(v):10.3f} {extra}")
    aux_f, aux_b, col_b = med["fwd aux (depth, invdepth, alpha)"], med["bwd aux (three maps)"] - floor, med["bwd colour"] - floor
    for C in CHANNELS:
        f, b = med[f"fwd features C={C}"], med[f"bwd features C={C}"] - floor
        lines.append(f"C={C:<2d}: forward {f / aux_f:.2f} x aux_fwd; backward {b / aux_b:.2f} x aux_bwd (+ dz chain), "
                     f"{b / col_b:.2f} x colour blend_bwd")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
