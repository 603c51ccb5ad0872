"""Cost of the depth-distortion / median-depth walk (csrc/raster_geom_maps.hip) next to the depth / inverse-depth / alpha walk
(csrc/raster_aux.hip) at the bench view: the scene bench.py builds (1 M anchors, seed 0), its first orbit camera, 1920x1080,
eval-mode Gaussians.  One process, the cases alternating, after warm-up, device events around single C-ABI calls on the
workspaces one forward left behind:

  forward   cgs_raster_render_geom (one kernel: geom_maps_fwd) next to cgs_raster_render_aux (one kernel: aux_fwd)
  backward  cgs_raster_backward_geom with the two new gradients only (geom_maps_bwd + the dz chain) next to
            cgs_raster_backward_feat with the three map gradients only (aux_bwd + the dz chain), each minus its own floor: the
            same entry point without any upstream gradient (the zero fill + the per-Gaussian backward)

The file records both pairs and their ratios; no time is fixed anywhere.

  python tools/geom_micro.py [--anchors 1000000] [--iters 10] [--warmup 3] [--out profiles/raster_geom.txt]
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
        raise SystemExit("geom_micro: needs the GPU")
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
        _, radii, ex = rast(means3D=xyz, means2D=torch.zeros_like(xyz), opacities=opacity, colors_precomp=color, scales=scaling,
                            rotations=rot, return_aux=True, return_geometry=True)
    lc = dict(rz.last_call)
    cfg, geom, binws, img, R = lc["cfg"], lc["geom_ws"], lc["bin_ws"], lc["img_ws"], lc["bin_R"]
    L = _lib.lib()
    p = _lib.ptr
    stream = _lib.current_stream()
    ws = (cfg.ref, P, R, p(geom), geom.numel(), p(binws), binws.numel(), p(img), img.numel())

    dev = "cuda"
    maps = [torch.empty(1, H, W, device=dev) for _ in range(3)]
    gmaps = [torch.empty(1, H, W, device=dev) for _ in range(2)]
    med_id = torch.empty(H, W, dtype=torch.int32, device=dev)
    moments = torch.empty(2, H, W, device=dev)
    gm = [torch.tensor(rng.normal(size=(1, H, W)).astype(np.float32), device=dev) for _ in range(3)]
    gg = [torch.tensor(rng.normal(size=(1, H, W)).astype(np.float32), device=dev) for _ in range(2)]
    xyz, color, opacity, scaling, rot = (t.contiguous() for t in (xyz, color, opacity, scaling, rot))
    acc = torch.zeros(P * 4, device=dev)                      # dL/dcolor | dL/dopacity (summed atomically: zeroed per call)
    rest = torch.empty(P * 14, device=dev)
    scratch = torch.empty(L.cgs_raster_bwd_abs_scratch_bytes(P), dtype=torch.uint8, device=dev)

    def backward(name, g_maps=(None, None, None), g_geom=None):
        m2 = 4 if name.endswith("_geom") else 3
        acc.zero_()
        tail = (p(moments), p(med_id), p(g_geom[0]) if g_geom else None, p(g_geom[1]) if g_geom else None) if m2 == 4 else ()
        _lib.check(getattr(L, name)(
            cfg.ref, P, R, p(xyz), p(color), None, 0, 0, p(opacity), p(scaling), p(rot), None, p(radii), p(geom), geom.numel(),
            p(binws), binws.numel(), p(img), img.numel(), None, p(g_maps[0]), p(g_maps[1]), p(g_maps[2]), p(rest[:3 * P]),
            p(rest[3 * P:(3 + m2) * P]), p(acc[:3 * P]), p(acc[3 * P:]), None, p(rest[7 * P:10 * P]), p(rest[10 * P:]), None,
            p(scratch), scratch.numel(), stream, 0, None, 0, None, None, *tail), name)

    cases = {
        "fwd geom (distortion, median)": lambda: _lib.check(L.cgs_raster_render_geom(
            *ws, p(gmaps[0]), p(gmaps[1]), p(med_id), p(moments), stream), "cgs_raster_render_geom"),
        "fwd aux (depth, invdepth, alpha)": lambda: _lib.check(L.cgs_raster_render_aux(
            *ws, p(maps[0]), p(maps[1]), p(maps[2]), stream), "cgs_raster_render_aux"),
        "bwd geom floor (no gradient)": lambda: backward("cgs_raster_backward_geom"),
        "bwd geom (distortion, median)": lambda: backward("cgs_raster_backward_geom", g_geom=gg),
        "bwd aux floor (no gradient)": lambda: backward("cgs_raster_backward_feat"),
        "bwd aux (three maps)": lambda: backward("cgs_raster_backward_feat", g_maps=gm),
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
    lines = [f"# tools/geom_micro.py: {a.anchors} anchors, {W}x{H}, P={P} Gaussians, visible {int((radii > 0).sum())}, "
             f"{lc['num_rendered']} pairs, {torch.cuda.get_device_name(0)}, device events, {a.iters} alternating rounds after "
             f"{a.warmup} warm-up rounds",
             f"# the view: distortion max {float(ex['distortion'].max()):.4g}, median found on "
             f"{int((ex['median_id'] >= 0).sum())} of {H * W} pixels",
             f"{'case':<36s} {'median ms':>10s} {'min ms':>10s}"]
    for k, v in times.items():
        lines.append(f"{k:<36s} {med[k]:10.3f} {min(v):10.3f}")
    f_geom, f_aux = med["fwd geom (distortion, median)"], med["fwd aux (depth, invdepth, alpha)"]
    b_geom = med["bwd geom (distortion, median)"] - med["bwd geom floor (no gradient)"]
    b_aux = med["bwd aux (three maps)"] - med["bwd aux floor (no gradient)"]
    lines.append(f"forward:  geom_maps_fwd {f_geom:.3f} ms, aux_fwd {f_aux:.3f} ms, ratio {f_geom / f_aux:.2f}")
    lines.append(f"backward: geom_maps_bwd + dz chain {b_geom:.3f} ms, aux_bwd + dz chain {b_aux:.3f} ms (each minus its floor), "
                 f"ratio {b_geom / b_aux:.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
