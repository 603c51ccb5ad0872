"""BASELINE.json's configurations c1, c2, c3 and c5 at FULL size on one MI355X (c4's single-GPU training step runs in
tests/test_training_gpu.py, its 8-GPU half is the driver's scaling run).

c1: 10 k anchors, 256x256, forward only: prefilter -> expansion -> rasterizer forward against the CPU oracles (the
    configuration the reference itself can run on the CPU: BASELINE.md section 3 "report c1 always"); the CPU oracle is timed.

c2: ~100 k anchors, 800x800, forward + backward: the visibility filter, the anchor -> Gaussian expansion and the
    rasterizer (image + six gradient tensors) against the CPU oracles on the SAME full-size inputs.
c3: ~500 k anchors, 1920x1080, 3-level context entropy encode + decode: every decoded attribute equals the encoder's
    quantised value bit for bit, and the decoded model renders the encoder-side image.
c5: ~3 M anchors, rate sweep (feature spread as the lambda proxy), encode -> files -> decode round trip.
"""
import os

import numpy as np
import pytest
import torch

from raster_harness import settings

pytestmark = pytest.mark.gpu


def test_c1_10k_anchors_256x256_vs_oracle(oracle32):
    """BASELINE configs[0]: the whole forward path (a1 prefilter, a2 expansion, a4 rasterizer forward) at the size of the
    reference's CPU-runnable case, every stage against its oracle; prints the CPU oracle's time next to the device's."""
    import time
    from contextgs_amd.rasterizer import GaussianRasterizer
    from contextgs_amd.renderer import generate_neural_gaussians, prefilter_voxel
    from contextgs_amd.synth import SynthPipe, make_scene, orbit_cameras
    from oracle import context_ref as cr
    N, W, H = 10_000, 256, 256
    pc = make_scene(N, seed=0)
    pc.eval()
    cam_np = orbit_cameras(8, W, H)[1]
    cam = cam_np.to_torch("cuda")
    bg = torch.zeros(3, device="cuda")
    f = lambda t: t.detach().cpu().numpy()
    with torch.no_grad():
        vis = prefilter_voxel(cam, pc, SynthPipe(), bg)
        rot0 = pc.get_rotation[[0], :].repeat(N, 1)
        t0 = time.perf_counter()
        ref_r = oracle32.visible_filter(cam_np.oracle_dict(), f(pc.get_anchor), f(pc.get_scaling[:, :3]), f(rot0))
        t_filter = time.perf_counter() - t0
        assert np.array_equal(f(vis), ref_r > 0) and int(vis.sum()) > N // 4
        xyz, color, opacity, scaling, rot, neural_opacity, mask = generate_neural_gaussians(
            cam, pc, vis, is_training=True, step=1000)[:7]
        Wd = {k: f(v) for k, v in pc.state_dict().items()}
        v = f(vis)
        t0 = time.perf_counter()
        o_xyz, o_color, o_op, o_sc, o_rot, o_no, o_sel = cr.expand(
            Wd, f(pc.get_anchor)[v], f(pc._anchor_feat)[v], f(pc._offset)[v], f(pc.get_scaling)[v], f(pc.get_mask)[v],
            f(cam.camera_center))
        t_expand = time.perf_counter() - t0
        flips = int((f(mask) != o_sel).sum())
        assert flips <= 1, flips
        if flips == 0:
            for a, b in ((xyz, o_xyz), (color, o_color), (opacity, o_op), (scaling, o_sc), (rot, o_rot)):
                assert np.allclose(f(a), b, rtol=1e-4, atol=3e-6)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img, radii = GaussianRasterizer(settings(cam_np, bg=bg))(
            means3D=xyz, means2D=torch.zeros_like(xyz), shs=None, colors_precomp=color, opacities=opacity, scales=scaling,
            rotations=rot, cov3D_precomp=None)
        torch.cuda.synchronize()
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        ref = oracle32.render(cam_np.oracle_dict(bg=(0, 0, 0)), f(xyz), f(color), f(opacity), f(scaling), f(rot))
        t_raster = time.perf_counter() - t0
    assert np.array_equal(f(radii), ref["radii"])
    d = np.abs(f(img) - ref["color"])
    assert float(np.sqrt((d ** 2).mean())) <= 1e-5 and float((d > 2e-5).mean()) <= 1e-4 and d.max() <= 1 / 255 + 1e-4
    print(f"[c1] 10k anchors 256x256 forward: {int(vis.sum())} visible anchors, {xyz.shape[0]} Gaussians; CPU oracle "
          f"filter {t_filter * 1e3:.1f} ms + expansion {t_expand * 1e3:.1f} ms + rasterizer {t_raster * 1e3:.1f} ms; "
          f"device rasterizer call (incl. host) {t_dev * 1e3:.2f} ms")


def test_c2_100k_anchors_800x800_forward_backward_vs_oracles(oracle32):
    from contextgs_amd.rasterizer import GaussianRasterizer
    from contextgs_amd.renderer import generate_neural_gaussians, prefilter_voxel
    from contextgs_amd.synth import SynthPipe, make_scene, orbit_cameras
    from oracle import context_ref as cr
    N, W, H = 100_000, 800, 800
    pc = make_scene(N, seed=0)
    pc.train()
    cam_np = orbit_cameras(8, W, H)[3]
    cam = cam_np.to_torch("cuda")
    bg = torch.zeros(3, device="cuda")
    f = lambda t: t.detach().cpu().numpy()

    # a1: anchor-level cull, bit-exact radii>0 against the oracle's preprocess on all 100 k anchors
    vis = prefilter_voxel(cam, pc, SynthPipe(), bg)
    with torch.no_grad():
        rot0 = pc.get_rotation[[0], :].repeat(N, 1)
        ref_r = oracle32.visible_filter(cam_np.oracle_dict(), f(pc.get_anchor), f(pc.get_scaling[:, :3]), f(rot0))
    assert np.array_equal(f(vis), ref_r > 0) and 0.5 * N < int(vis.sum()) <= N

    # a2: expansion (training phase, step <= 3000) against the numpy oracle on every visible anchor
    xyz, color, opacity, scaling, rot, neural_opacity, mask = generate_neural_gaussians(
        cam, pc, vis, is_training=True, step=1000)[:7]
    Wd = {k: f(v) for k, v in pc.state_dict().items()}
    v = f(vis)
    o_xyz, o_color, o_op, o_sc, o_rot, o_no, o_sel = cr.expand(
        Wd, f(pc.get_anchor)[v], f(pc._anchor_feat)[v], f(pc._offset)[v], f(pc.get_scaling)[v], f(pc.get_mask)[v],
        f(cam.camera_center))
    flips = int((f(mask) != o_sel).sum())
    assert flips <= 2, flips                                   # sign of a tanh output sitting at 0
    P = xyz.shape[0]
    assert 0.4e6 < P < 0.8e6, P
    if flips == 0:
        for a, b in ((xyz, o_xyz), (color, o_color), (opacity, o_op), (scaling, o_sc), (rot, o_rot)):
            assert np.allclose(f(a), b, rtol=1e-4, atol=3e-6)

    # a4/a5: rasterizer forward + backward on these P Gaussians at 800x800 against the C oracle
    leaves = [t.detach().clone().requires_grad_(True) for t in (xyz, color, opacity, scaling, rot)]
    m2d = torch.zeros_like(leaves[0], requires_grad=True)
    img, radii = GaussianRasterizer(settings(cam_np, bg=bg))(
        means3D=leaves[0], means2D=m2d, shs=None, colors_precomp=leaves[1], opacities=leaves[2], scales=leaves[3],
        rotations=leaves[4], cov3D_precomp=None)
    w = np.random.default_rng(2).normal(size=(3, H, W)).astype(np.float32)
    (img * torch.from_numpy(w).cuda()).sum().backward()
    ref = oracle32.render(cam_np.oracle_dict(bg=(0, 0, 0)), f(leaves[0]), f(leaves[1]), f(leaves[2]), f(leaves[3]),
                          f(leaves[4]), dL_dout=w)
    assert np.array_equal(f(radii), ref["radii"])
    d = np.abs(f(img) - ref["color"])
    assert float(np.sqrt((d ** 2).mean())) <= 1e-5 and float((d > 2e-5).mean()) <= 1e-4 and d.max() <= 1 / 255 + 1e-4
    got = dict(dL_dmeans3D=leaves[0].grad, dL_dmeans2D=m2d.grad, dL_dcolors=leaves[1].grad,
               dL_dopacities=leaves[2].grad.reshape(-1), dL_dscales=leaves[3].grad, dL_drotations=leaves[4].grad)
    for k, a in got.items():
        b = ref[k]
        err = np.abs(f(a) - b) / max(1e-6, float(np.abs(b).max()))
        assert float((err > 2e-4).mean()) <= 2e-3 and float(np.median(err)) <= 1e-6, (k, float(err.max()))


def _roundtrip(pc, tmpdir, render_check=None, version=1):
    """conduct_encoding -> files -> conduct_decoding on a fresh model; value-level equality of every attribute."""
    from contextgs_amd import context_model as cm
    from contextgs_amd.codec_driver import conduct_encoding
    from contextgs_amd.synth import make_scene
    pc.eval()
    d = str(tmpdir)
    conduct_encoding(pc, d, container_version=version)
    size = sum(os.path.getsize(os.path.join(d, x)) for x in os.listdir(d))
    N = pc._anchor.shape[0]
    dec = make_scene(N, seed=0, voxel_size=pc.voxel_size, requires_grad=False)
    with torch.no_grad():           # scramble: everything must come from the files
        dec._anchor_feat.zero_(); dec._offset.zero_(); dec._hyper_latent.zero_(); dec._scaling.zero_(); dec._anchor.zero_()
        for p in dec.mlp_grid.parameters():
            p.zero_()
    dec.eval()
    dec.conduct_decoding(d)
    assert dec.decoded_version
    with torch.no_grad():
        m = pc.get_mask_anchor
        nv = int(m.sum())
        anchor = pc.get_anchor[m]
        fq, sq, oq = cm.multi_scale_generating(pc, anchor, pc._hyper_latent[m], pc._anchor_feat[m], pc._offset[m],
                                               pc.get_scaling[m], pc.get_mask[m], None, predict_bpp=False, training=False)
        assert torch.equal(dec._anchor[:nv], anchor)
        assert torch.equal(dec._mask[:nv], pc.get_mask[m])
        assert torch.equal(dec._hyper_latent[:nv], torch.round(pc._hyper_latent[m]))
        assert torch.equal(dec._anchor_feat[:nv], fq)
        assert torch.equal(dec._scaling[:nv], sq)
        assert torch.equal(dec._offset[:nv], oq * pc.get_mask[m])
        if render_check is not None:
            render_check(pc, dec)
    return size, nv


def test_c3_500k_anchors_1080p_encode_decode(tmp_path):
    from contextgs_amd.renderer import prefilter_voxel, render
    from contextgs_amd.synth import SynthPipe, make_scene, orbit_cameras
    pc = make_scene(500_000, seed=0, requires_grad=False)
    cam = orbit_cameras(8, 1920, 1080)[1].to_torch("cuda")
    bg = torch.zeros(3, device="cuda")

    def render_check(enc, dec):
        # The decoded model (decoded_version: parameters ARE the transmitted values) against the encoder-side model
        # rendered through its context model (gaussian_renderer/__init__.py:83-101).  NOT the same numbers, in the
        # reference either: the eval render levels the anchors with the masked ones ZEROED (quirk Q4,
        # scene/gaussian_model.py:1758-1759) while the encoder DROPS them first (:1031-1043), so a few anchors sit in
        # another level, see another context and get another step size.  The value-level equality above is the
        # bit-exact statement; this only bounds the visible effect (RMSE 5e-3 = 46 dB).
        # (same visible set for both: prefilter_voxel reads get_scaling, which is exp(_scaling) before and the
        # QUANTISED scaling after decoding, so its own answer differs for anchors on the frustum border)
        vis = prefilter_voxel(cam, enc, SynthPipe(), bg)
        keep = enc.get_mask_anchor
        vis_dec = torch.zeros(dec._anchor.shape[0], dtype=torch.bool, device="cuda")
        vis_dec[:int(keep.sum())] = vis[keep]
        imgs = [render(cam, enc, SynthPipe(), bg, visible_mask=vis)["render"],
                render(cam, dec, SynthPipe(), bg, visible_mask=vis_dec)["render"]]
        d = (imgs[0] - imgs[1]).abs()
        assert float(d.pow(2).mean().sqrt()) <= 5e-3, float(d.pow(2).mean().sqrt())

    size, nv = _roundtrip(pc, tmp_path / "c3", render_check)
    assert nv > 400_000 and 20e6 < size < 120e6
    size2, _ = _roundtrip(pc, tmp_path / "c3v2", None, version=2)          # version 2: same symbols, shorter streams
    # + 128-byte block headers and 64 stream ends per block: ~0.6 % at 32 768-symbol blocks, the two small levels' shorter
    # blocks (codec_driver._block_for: their launches are a quarter / half as long) add ~0.15 %
    print(f"[c3] container version 2: {size2} bytes against {size} (+{(size2 - size) / size * 100:.2f} %)")
    assert abs(size2 - size) < 0.008 * size, (size, size2)


def test_c5_3M_anchors_rate_sweep_roundtrip(tmp_path):
    from contextgs_amd.synth import make_scene
    pc = make_scene(3_000_000, seed=0, requires_grad=False)
    rng = torch.Generator(device="cuda").manual_seed(11)
    import shutil
    sizes = []
    # feature spread as the rate proxy of the five-point lambda sweep (scripts/train_blending.py:3)
    for k, sigma in enumerate((1.0, 2.0, 3.0, 5.0, 8.0)):
        with torch.no_grad():
            pc._anchor_feat.copy_(torch.round(torch.randn(pc._anchor_feat.shape, device="cuda", generator=rng) * sigma))
        size, nv = _roundtrip(pc, tmp_path / f"c5_{k}", version=1 + (k % 2))      # both container versions along the sweep
        shutil.rmtree(tmp_path / f"c5_{k}", ignore_errors=True)
        assert nv > 2_400_000
        sizes.append(size)
    assert all(b > 1.03 * a for a, b in zip(sizes, sizes[1:])), sizes            # more spread -> more bits, monotonically
    assert sizes[-1] > 1.3 * sizes[0], sizes
