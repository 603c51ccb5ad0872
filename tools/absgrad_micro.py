"""Cost of the absolute screen-space gradients (`absgrad=True`: the ABS instance of blend_bwd_rows_kernel and the four-column
per-Gaussian backward, csrc/raster_blend_rows.hip / raster_bwd.hip) at the bench view: the scene bench.py builds (1 M anchors,
seed 0), its first orbit camera, 1920x1080, eval-mode Gaussians.  One process, the cases alternating, after warm-up, device
events around single C-ABI calls on the workspaces one forward left behind:

  cgs_raster_backward_feat  without an upstream gradient (zero fill + per-Gaussian backward: the floor) and with the colour
                            image's (+ the default blend_bwd, whose instruction stream is the parent commit's)
  cgs_raster_backward_abs   the same two (+ the ABS blend_bwd)

Case minus its floor is the blend backward of that instance; the table ends with their ratio.  The per-kernel times come from
running this script under `rocprofv3 --kernel-trace --stats` with --iters 3 --warmup 1 (no counters in the same run).

  python tools/absgrad_micro.py [--anchors 1000000] [--iters 10] [--warmup 3] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
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
        raise SystemExit("absgrad_micro: needs the GPU")
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
        rast = rz.GaussianRasterizer(_raster_settings(cam, pipe, bg, 1.0))
        _, radii = rast(means3D=xyz, means2D=torch.zeros_like(xyz), opacities=opacity, colors_precomp=color, scales=scaling,
                        rotations=rot)
    lc = dict(rz.last_call)
    cfg, geom, binws, img, R = lc["cfg"], lc["geom_ws"], lc["bin_ws"], lc["img_ws"], lc["bin_R"]
    L = _lib.lib()
    p = _lib.ptr
    stream = _lib.current_stream()

    dev = "cuda"
    g3 = torch.tensor(rng.normal(size=(3, H, W)).astype(np.float32), device=dev)
    xyz, color, opacity, scaling, rot = (t.contiguous() for t in (xyz, color, opacity, scaling, rot))
    acc = torch.zeros(P * 4, device=dev)                      # dL/dcolor | dL/dopacity (summed atomically: zeroed per call)
    rest = torch.empty(P * 14, device=dev)
    scratch = torch.empty(L.cgs_raster_bwd_abs_scratch_bytes(P), dtype=torch.uint8, device=dev)

    def backward(fn, m2, g_col=None):
        acc.zero_()
        _lib.check(getattr(L, fn)(
            cfg.ref, P, R, p(xyz), p(color), None, 0, 0, p(opacity), p(scaling), p(rot), None, p(radii), p(geom), geom.numel(),
            p(binws), binws.numel(), p(img), img.numel(), p(g_col), None, None, None, p(rest[:3 * P]),
            p(rest[3 * P:(3 + m2) * P]), p(acc[:3 * P]), p(acc[3 * P:]), None, p(rest[7 * P:10 * P]), p(rest[10 * P:]), None,
            p(scratch), scratch.numel(), stream, 0, None, 0, None, None), fn)

    cases = {"default: floor (no upstream gradient)": lambda: backward("cgs_raster_backward_feat", 3),
             "default: colour": lambda: backward("cgs_raster_backward_feat", 3, g3),
             "ABS: floor (no upstream gradient)": lambda: backward("cgs_raster_backward_abs", 4),
             "ABS: colour": lambda: backward("cgs_raster_backward_abs", 4, g3)}

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
    lines = [f"# tools/absgrad_micro.py: {a.anchors} anchors, {W}x{H}, P={P} Gaussians, visible {int((radii > 0).sum())}, "
             f"{lc['num_rendered']} pairs, {torch.cuda.get_device_name(0)}, device events, {a.iters} alternating rounds after "
             f"{a.warmup} warm-up rounds",
             f"{'case':<40s} {'median ms':>10s} {'min ms':>10s}"]
    for k, v in times.items():
        lines.append(f"{k:<40s} {med[k]:10.3f} {min(v):10.3f}")
    d_blend = med["default: colour"] - med["default: floor (no upstream gradient)"]
    a_blend = med["ABS: colour"] - med["ABS: floor (no upstream gradient)"]
    lines.append(f"blend backward (colour - floor): default {d_blend:.3f} ms, ABS {a_blend:.3f} ms, ratio {a_blend / d_blend:.3f}")
    lines.append(f"whole call: default {med['default: colour']:.3f} ms, ABS {med['ABS: colour']:.3f} ms, "
                 f"ratio {med['ABS: colour'] / med['default: colour']:.3f}; floors: ratio "
                 f"{med['ABS: floor (no upstream gradient)'] / med['default: floor (no upstream gradient)']:.3f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
