"""Cost of the bit-reproducible backward (`deterministic=True`: cgs_raster_backward_det, the DET instances of
blend_bwd_rows_kernel and det_sum_kernel, csrc/raster_blend_rows.hip) next to the default backward of the SAME build, at the
bench view (the scene bench.py builds: 1 M anchors, seed 0, first orbit camera, 1920x1080, eval-mode Gaussians) and on the
heavy-pair scene (the same on the 0.01 voxel grid, ~136 M pairs).  One process per scene list, the cases alternating, after
warm-up, device events around single C-ABI calls on the workspaces one forward left behind:

  cgs_raster_backward       the default: zero fills, blend_bwd_rows_kernel<false> (float atomics), per-Gaussian backward
  cgs_raster_backward_det   scan of tiles[], zero fill of the slot array, blend_bwd_rows_det_kernel<false>, det_sum_kernel,
                            per-Gaussian backward; and the same without an upstream gradient (det_sum_kernel over no slots +
                            per-Gaussian backward: the floor)
  zero fill                 a fill of the slot array's bytes alone (torch's, as a stand-in for the call's hipMemsetAsync)

It prints the times, their ratio, the workspace bytes and the slot traffic, checks that two det calls give the same bits, and
writes the table to --out.  The per-kernel times (zero fill, DET blend, sum kernel) come from running this script under
`rocprofv3 --kernel-trace --stats` with --iters 3 --warmup 1 (no counters in the same run).

  python tools/det_micro.py [--anchors 1000000] [--scenes headline,heavy] [--iters 7] [--warmup 2] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_scene(a, name, voxel):
    from contextgs_amd import _lib, rasterizer as rz
    from contextgs_amd.renderer import _raster_settings, generate_neural_gaussians, prefilter_voxel
    from contextgs_amd.synth import SynthPipe, make_scene, orbit_cameras

    W, H = a.W, a.H
    pc = make_scene(a.anchors, seed=0, **({} if voxel is None else dict(voxel_size=voxel)))
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
    acc = torch.zeros(P * 4, device=dev)                      # dL/dcolor | dL/dopacity (default: summed atomically, zeroed per call)
    rest = torch.empty(P * 13, device=dev)
    scratch = torch.empty(L.cgs_raster_bwd_abs_scratch_bytes(P), dtype=torch.uint8, device=dev)
    det_bytes = int(L.cgs_raster_bwd_det_bytes(P, R, 3))
    det_ws = torch.empty(det_bytes, dtype=torch.uint8, device=dev)
    slot_bytes = 48 * int(R)
    grads = (p(rest[:3 * P]), p(rest[3 * P:6 * P]), p(acc[:3 * P]), p(acc[3 * P:]))
    tail = (p(rest[6 * P:9 * P]), p(rest[9 * P:]))

    def default():
        acc.zero_()
        _lib.check(L.cgs_raster_backward(
            cfg.ref, P, R, p(xyz), p(color), p(opacity), p(scaling), p(rot), p(radii), p(geom), geom.numel(), p(binws),
            binws.numel(), p(img), img.numel(), p(g3), *grads, *tail, p(scratch), scratch.numel(), stream), "cgs_raster_backward")

    def det(g_col=g3):
        _lib.check(L.cgs_raster_backward_det(
            cfg.ref, P, R, p(xyz), p(color), None, 0, 0, p(opacity), p(scaling), p(rot), None, p(radii), p(geom), geom.numel(),
            p(binws), binws.numel(), p(img), img.numel(), p(g_col), None, None, None, *grads, None, *tail, None, p(scratch),
            scratch.numel(), stream, 0, 3, p(det_ws), det_bytes), "cgs_raster_backward_det")

    cases = {"default: cgs_raster_backward": default,
             "det: cgs_raster_backward_det": det,
             "det: floor (no upstream gradient)": lambda: det(None),
             "zero fill of the slot array alone": lambda: det_ws[det_bytes - slot_bytes:].zero_()}

    for _ in range(a.warmup):
        for f in cases.values():
            f()
    torch.cuda.synchronize()
    det()
    first = (rest.clone(), acc.clone())
    det_ws.fill_(0xFF)
    det()
    torch.cuda.synchronize()
    same_bits = torch.equal(first[0], rest) and torch.equal(first[1], acc)
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
    pairs = int(lc["num_rendered"])
    lines = [f"# tools/det_micro.py, {name}: {a.anchors} anchors, {W}x{H}, P={P} Gaussians, visible {int((radii > 0).sum())}, "
             f"{pairs} pairs (workspaces carved for {R}), {torch.cuda.get_device_name(0)}, device events, {a.iters} alternating "
             f"rounds after {a.warmup} warm-up rounds",
             f"{'case':<40s} {'median ms':>10s} {'min ms':>10s} {'max ms':>10s}"]
    for k, v in times.items():
        lines.append(f"{k:<40s} {med[k]:10.3f} {min(v):10.3f} {max(v):10.3f}")
    d, t = med["default: cgs_raster_backward"], med["det: cgs_raster_backward_det"]
    lines.append(f"whole call: default {d:.3f} ms, det {t:.3f} ms, ratio {t / d:.3f}")
    lines.append(f"det_ws {det_bytes} B ({det_bytes / 2 ** 20:.1f} MiB), of which slots {slot_bytes} B; slot traffic per call: "
                 f"{slot_bytes} B zero fill + <= {48 * pairs} B stored + {48 * pairs} B read by the sum kernel")
    lines.append(f"two det calls (the second on a det_ws filled with 0xFF bytes) gave the same bits: {same_bits}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", type=int, default=1_000_000)
    ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--H", type=int, default=1080)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scenes", default="headline,heavy")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("det_micro: needs the GPU")
    lines = []
    for name in a.scenes.split(","):
        lines += one_scene(a, name, {"headline": None, "heavy": 0.01}[name]) + [""]
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
