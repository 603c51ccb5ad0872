"""GPU parity of the rasterizer in the regimes the mild scenes of tests/test_raster_gpu.py never reach, against the CPU
oracle (oracle/raster_ref.c): saturated stacks (early termination at T < 1e-4, the 0.99 alpha clamp, a terminating entry
in a later 256-record batch), needles (100:1 .. 1000:1 on screen, the octagon's diagonal cut of rb_block_mask, fp16
diagonal extents beyond 1024 pixels), long lists (one tile in the top class of tile_order_kernel, a view whose mean list
keeps the raster order), borders (ragged images, centres on tile borders and outside the image, the near plane) and exact
depth ties.

Tolerances are those of tests/test_raster_gpu.py, unchanged: radii bit-exact; image RMSE <= 1e-5, at most 1e-4 of the
values beyond 2e-5, max-abs <= 1/255 + 1e-4; every gradient within 2e-4 of its tensor's maximum on all but 2e-3 of the
entries, median <= 1e-6.  The precomputed-covariance form keeps tests/test_raster_sh_cov_gpu.py's allowance: radii equal on
all but 1e-4 of the Gaussians, gradients compared on the rows whose radii agree.

Every scene asserts that its regime was reached (the oracle's final_T, the pair count of the last forward, or the scene's
own geometry restated in fp64 below), so that a scene that drifts out of its regime fails instead of passing quietly.
"""
import math

import numpy as np
import pytest
import torch

from contextgs_amd.synth import look_at_camera
from raster_harness import cov6_torch, settings
from raster_units_ref import geom64 as _geom64, t_no_termination as _t_no_termination

pytestmark = pytest.mark.gpu

BG = (0.1, 0.25, 0.4)
GRADS = ["dL_dmeans3D", "dL_dmeans2D", "dL_dcolors", "dL_dopacities", "dL_dscales", "dL_drotations"]
T_EPS = np.float32(1e-4)             # RB_T_EPS / the oracle's termination threshold
TAU2_MIN = 9.0                       # (3 sigma)^2: beyond it the alpha >= 1/255 ellipse reaches past the 3-sigma radius


@pytest.fixture
def bin_mode(request):
    """cgs_debug_set_bin_mode for one test: 1 = radix passes over (tile, Gaussian) pairs, 2 = two-level (bucket) binning"""
    from contextgs_amd import _lib
    L = _lib.lib()
    _lib.check(L.cgs_debug_set_bin_mode(request.param), "cgs_debug_set_bin_mode")
    yield request.param
    _lib.check(L.cgs_debug_set_bin_mode(0), "cgs_debug_set_bin_mode")


# ---------------------------------------------------------------------------------------------------------------------
# cameras and geometry

def _cam(W, H, fovx=60.0):
    """view = identity: world coordinates are camera coordinates (x right, y down, z forward)"""
    return look_at_camera((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), W, H, fovx_deg=fovx, up=(0.0, -1.0, 0.0))


def _focal(cam):
    return cam.image_width / (2 * math.tan(cam.FoVx / 2)), cam.image_height / (2 * math.tan(cam.FoVy / 2))


def _unproject(cam, u, v, z):
    """camera-space x, y of the point at depth z whose pixel centre is (u, v)"""
    fx, fy = _focal(cam)
    return (np.asarray(u, np.float64) + 0.5 - cam.image_width / 2) * z / fx, \
        (np.asarray(v, np.float64) + 0.5 - cam.image_height / 2) * z / fy


def _qmul(a, b):
    w1, x1, y1, z1 = a.T
    w2, x2, y2, z2 = b.T
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=1)


def _qaxis(axis, ang):
    ang = np.asarray(ang, np.float64)
    q = np.zeros((ang.size, 4))
    q[:, 0] = np.cos(ang / 2)
    q[:, 1 + axis] = np.sin(ang / 2)
    return q


def _gaussians(means, scales, quats, opac, colors):
    f = lambda a: np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))
    return dict(means3D=f(means), scales=f(scales), rotations=f(quats), colors=f(colors),
                opacities=f(np.asarray(opac).reshape(-1, 1)))


# (the fp64 restatement of the preprocess and of the dense alpha: tests/raster_units_ref.py)


def _tile_counts(cam, geo, radii):
    """Per-tile list lengths of the GPU binning (3-sigma rectangle cut to the box of the alpha >= 1/255 ellipse),
    restated in fp64: exact up to decisions on the last ulp of a rectangle edge."""
    W, H = cam.image_width, cam.image_height
    gx, gy = (W + 15) // 16, (H + 15) // 16
    cnt = np.zeros((gy, gx), np.int64)
    for i in np.nonzero((radii > 0) & (geo["tau2"] > 0))[0]:
        px, py, r, hx, hy = geo["px"][i], geo["py"][i], radii[i], geo["hx"][i], geo["hy"][i]
        x0 = max(int(np.clip(math.floor((px - r) / 16), 0, gx)), max(0, math.ceil(px - hx)) // 16)
        y0 = max(int(np.clip(math.floor((py - r) / 16), 0, gy)), max(0, math.ceil(py - hy)) // 16)
        x1 = min(int(np.clip((px + r + 15) // 16, 0, gx)), min(W - 1, math.floor(px + hx)) // 16 + 1)
        y1 = min(int(np.clip((py + r + 15) // 16, 0, gy)), min(H - 1, math.floor(py + hy)) // 16 + 1)
        if x1 > x0 and y1 > y0:
            cnt[y0:y1, x0:x1] += 1
    return cnt


# ---------------------------------------------------------------------------------------------------------------------
# scenes: (camera, Gaussians, regime check).  The check gets the oracle's result, the fp64 geometry and the pair count of
# the GPU forward, asserts the regime and returns a one-line description of it.

def _colors(rng, n):
    return rng.random((n, 3))


def _layers(rng, cam, n, z_lo, z_hi, sig_lo, sig_hi, op_lo, op_hi, margin=8.0):
    """n roughly round splats facing the camera, centres uniform over the image (and a margin around it)"""
    W, H = cam.image_width, cam.image_height
    fx, _ = _focal(cam)
    z = rng.uniform(z_lo, z_hi, n)
    u, v = rng.uniform(-margin, W + margin, n), rng.uniform(-margin, H + margin, n)
    x, y = _unproject(cam, u, v, z)
    s = np.exp(rng.uniform(np.log(sig_lo), np.log(sig_hi), n)) * z / fx
    scales = np.stack([s, s * rng.uniform(0.5, 1.0, n), np.full(n, 1e-4)], 1)
    return _gaussians(np.stack([x, y, z], 1), scales, _qaxis(2, rng.uniform(0, np.pi, n)),
                      rng.uniform(op_lo, op_hi, n), _colors(rng, n))


def _cat(*gs):
    return {k: np.ascontiguousarray(np.concatenate([g[k] for g in gs])) for k in gs[0]}


def _terminated(min_frac):
    def check(cam, g, ref, geo, R):
        tn = _t_no_termination(cam, g, geo, ref["radii"])
        term = tn < 0.5 * T_EPS                      # (a factor 2 from the threshold: decisions on the last ulp do not count)
        frac = float(term.mean())
        assert frac >= min_frac, f"only {frac:.3f} of the pixels terminate"
        assert (ref["final_T"][term] >= T_EPS * 0.999).all()          # the oracle stopped there, it did not go below
        return f"{frac:.3f} of the pixels terminate early"
    return check


def scene_sat_stack(op_lo, op_hi, W=96, H=64, n=600, seed=0):
    """six depth slabs of splats with opacity in [op_lo, op_hi] (1.0: alpha is the 0.99 clamp wherever G >= 0.99)"""
    cam = _cam(W, H)
    rng = np.random.default_rng(seed)
    g = _cat(*[_layers(rng, cam, n // 6, 2 + k, 2.5 + k, 8, 24, op_lo, op_hi) for k in range(6)])
    return cam, g, _terminated(0.5)


def scene_sat_boundary(W=40, H=24):
    """four screen-filling layers of opacity 1 (alpha = the 0.99 clamp everywhere): after the first T = 1 - 0.99, and the
    second's test T (1 - 0.99) = 0.01 * 0.01 is the threshold 1e-4 itself in real arithmetic (in fp32 it rounds to 26 ulps
    below it: the second layer is not added).  The layers have different colours, so either decision shows in the image."""
    cam = _cam(W, H)
    fx, _ = _focal(cam)
    z = np.array([2.0, 3.0, 4.0, 5.0])
    x, y = _unproject(cam, np.full(4, W / 2 - 0.5), np.full(4, H / 2 - 0.5), z)
    s = 2000.0 * z / fx                              # sigma 2000 pixels: G >= 0.99 over the whole image
    g = _gaussians(np.stack([x, y, z], 1), np.stack([s, s, np.full(4, 1e-3)], 1), _qaxis(2, np.zeros(4)), np.ones(4),
                   [[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]])

    def check(cam, g, ref, geo, R):
        one_minus = np.float32(1) - np.float32(0.99)
        t1, t2 = one_minus, np.float32(one_minus * one_minus)
        assert abs(float(t2) - float(T_EPS)) <= 1e-5 * float(T_EPS), (t2, T_EPS)    # on the boundary up to fp32 rounding
        ft = ref["final_T"]
        want = t1 if t2 < T_EPS else t2
        assert (ft == want).all(), np.unique(ft)
        return f"second layer's T {t2!r} vs eps {T_EPS!r}: {'stops at' if t2 < T_EPS else 'takes'} the second layer"
    return cam, g, check


def scene_sat_late_batch(W=48, H=48, n_faint=320, n_opaque=300, seed=1):
    """320 faint screen-filling splats in front of every tile (opacity ~0.01: T ~ 0.04 behind them), opaque splats
    (0.98 .. 1.0) behind: the terminating entry of a pixel sits in the second 256-record batch or later."""
    cam = _cam(W, H)
    rng = np.random.default_rng(seed)
    fx, _ = _focal(cam)
    z = rng.uniform(1.0, 1.5, n_faint)
    x, y = _unproject(cam, rng.uniform(0, W, n_faint), rng.uniform(0, H, n_faint), z)
    s = 400.0 * z / fx
    faint = _gaussians(np.stack([x, y, z], 1), np.stack([s, s, np.full(n_faint, 1e-3)], 1),
                       _qaxis(2, np.zeros(n_faint)), rng.uniform(0.008, 0.012, n_faint), _colors(rng, n_faint))
    opaque = _cat(*[_layers(rng, cam, n_opaque // 3, 3 + k, 3.5 + k, 6, 14, 0.98, 1.0) for k in range(3)])
    g = _cat(faint, opaque)
    term = _terminated(0.5)

    def check(cam, g, ref, geo, R):
        gx, gy = (W + 15) // 16, (H + 15) // 16
        # every faint splat is in every tile's list, in front of every opaque one
        assert (geo["radius"][:n_faint] > 2 * (W + H)).all() and geo["z"][:n_faint].max() < geo["z"][n_faint:].min()
        assert int(ref["stats"][0]) >= n_faint * gx * gy
        return term(cam, g, ref, geo, R) + f", behind {n_faint} entries per tile (batch 2 and later)"
    return cam, g, check


def _needles(rng, cam, n, sig_lo, sig_hi, margin, aniso_lo, aniso_hi):
    W, H = cam.image_width, cam.image_height
    fx, _ = _focal(cam)
    z = rng.uniform(2.0, 5.0, n)
    x, y = _unproject(cam, rng.uniform(-margin, W + margin, n), rng.uniform(-margin, H + margin, n), z)
    s_long = np.exp(rng.uniform(np.log(sig_lo), np.log(sig_hi), n)) * z / fx
    aniso = np.exp(rng.uniform(np.log(aniso_lo), np.log(aniso_hi), n))
    s_short = s_long / aniso
    theta = rng.uniform(0, np.pi, n)
    k = np.arange(n)
    theta[k % 3 == 0] = np.pi / 4 + rng.uniform(-0.02, 0.02, n)[k % 3 == 0]          # near 45 degrees on screen
    theta[k % 6 == 1] = 3 * np.pi / 4 + rng.uniform(-0.02, 0.02, n)[k % 6 == 1]      # near 135 degrees
    q = _qmul(_qaxis(2, theta), _qaxis(1, np.where(k % 2 == 0, rng.uniform(-0.3, 0.3, n), 0.0)))   # tilted out of the plane
    rnd = k % 5 == 4                                                                   # some: random 3-D orientation
    qr = rng.normal(size=(n, 4))
    q[rnd] = qr[rnd] / np.linalg.norm(qr[rnd], axis=1, keepdims=True)
    return _gaussians(np.stack([x, y, z], 1), np.stack([s_long, s_short, s_short], 1), q, rng.uniform(0.9, 1.0, n),
                      _colors(rng, n))


def scene_needles(W=128, H=96, n=240, seed=2):
    """100:1 .. 1000:1 needles (scales), 6 .. 12 pixels sigma, many near 45 / 135 degrees on screen, opacity 0.9 .. 1.0.

    On screen the 0.3 dilation floors the short variance, so the eigenvalue ratio is 100 .. ~500.  Longer needles of the same
    thinness reach ratios of 1e4 .. 1e5, where det = a c - b^2 of the fp32 preprocess (kernel and oracle alike: the published
    algorithm) keeps 1 .. 3 digits and the fp32 oracle itself lies up to 1e-3 per pixel from fp64: no fp32 code can be held
    to these tolerances there, so the scenes stay where the conic is well conditioned."""
    cam = _cam(W, H)
    g = _needles(np.random.default_rng(seed), cam, n, 6.0, 12.0, 20.0, 100.0, 1000.0)

    def check(cam, g, ref, geo, R):
        live = ref["radii"] > 0
        thin = geo["ratio"][live] >= 100
        assert thin.mean() >= 0.5, thin.mean()
        cut = (np.minimum(geo["hu"], geo["hv"]) < 0.5 * (geo["hx"] + geo["hy"]))[live]       # the diagonals cut the box
        assert cut.sum() >= 40, cut.sum()
        assert (geo["tau2"][live] > TAU2_MIN).all()
        return f"{int(thin.sum())} of {int(live.sum())} with eigenvalue ratio >= 100 (max {geo['ratio'][live].max():.0f}), " \
               f"{int(cut.sum())} cut by the diagonals"
    return cam, g, check


def scene_needles_long(W=256, H=256, n=30, seed=3):
    """needles of 330 .. 500 pixels sigma: diagonal half extents above 1024 pixels, where fp16 has a spacing of 1.  12:1 .. 20:1
    in scale (eigenvalue ratio 100 .. 400 on screen): thinner at this length is ill-conditioned in fp32 (scene_needles)."""
    cam = _cam(W, H)
    g = _needles(np.random.default_rng(seed), cam, n, 330.0, 500.0, 0.0, 12.0, 20.0)

    def check(cam, g, ref, geo, R):
        live = ref["radii"] > 0
        big = np.maximum(geo["hu"], geo["hv"])[live] > 1024
        assert big.sum() >= n // 2, big.sum()
        assert (geo["ratio"][live] >= 100).mean() >= 0.5
        return f"{int(big.sum())} of {int(live.sum())} with a diagonal half extent above 1024 pixels"
    return cam, g, check


def scene_long_top(W=128, H=128, heavy=6000, light=800, seed=4, tile=(3, 2)):
    """one tile with about 5000 faint entries (opacity 0.002 .. 0.02) among light tiles: the top class (>= 4096) of the tile
    order; nothing terminates, every entry of the long list is walked"""
    cam = _cam(W, H)
    rng = np.random.default_rng(seed)
    fx, _ = _focal(cam)
    z = rng.uniform(2.0, 4.0, heavy)
    x, y = _unproject(cam, rng.uniform(16 * tile[0], 16 * tile[0] + 15, heavy), rng.uniform(16 * tile[1], 16 * tile[1] + 15, heavy), z)
    s = rng.uniform(1.0, 2.5, heavy) * z / fx
    hv = _gaussians(np.stack([x, y, z], 1), np.stack([s, s * rng.uniform(0.6, 1.0, heavy), s], 1),
                    _qaxis(2, rng.uniform(0, np.pi, heavy)), rng.uniform(0.002, 0.02, heavy), _colors(rng, heavy))
    g = _cat(hv, _layers(rng, cam, light, 2.0, 4.0, 2.0, 6.0, 0.002, 0.02))

    def check(cam, g, ref, geo, R):
        cnt = _tile_counts(cam, geo, ref["radii"])
        top, rest = int(cnt.max()), np.sort(cnt.ravel())[:-1]
        assert top >= 4096 * 1.05 and np.unravel_index(cnt.argmax(), cnt.shape) == tile[::-1], (top, cnt.argmax())
        assert rest.max() < 1024, rest.max()
        assert float(ref["final_T"].min()) >= 1e-3, ref["final_T"].min()                    # nothing terminates
        return f"top tile {top} entries, the others at most {int(rest.max())}; min final_T {ref['final_T'].min():.2e}"
    return cam, g, check


def scene_long_dense(W=64, H=64, n=70000, seed=5):
    """64 x 64 pixels, 70 000 faint splats: the mean list is above TO_DENSE = 4096 entries (the view keeps the raster order)"""
    cam = _cam(W, H)
    g = _layers(np.random.default_rng(seed), cam, n, 2.0, 4.0, 1.5, 3.0, 0.002, 0.02, margin=2.0)

    def check(cam, g, ref, geo, R):
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        assert R / tiles >= 4096 * 1.1, R / tiles
        assert float(ref["final_T"].min()) >= 1e-3, ref["final_T"].min()
        return f"mean list {R / tiles:.0f} entries ({R} pairs, {tiles} tiles); min final_T {ref['final_T'].min():.2e}"
    return cam, g, check


def scene_borders(W, H, seed=6):
    """centres on tile borders (x = 16 k - 0.5 .. 16 k) and on pixel centres, outside the image but reaching in, just
    beyond the 0.2 near plane, and splats larger than the image"""
    cam = _cam(W, H)
    rng = np.random.default_rng(seed + W * 1000 + H)
    fx, _ = _focal(cam)
    us = np.concatenate([np.arange(0, W + 16, 16) - 0.5, np.arange(0, W + 16, 16).astype(np.float64), [W - 1.0, -0.5]])
    vs = np.concatenate([np.arange(0, H + 16, 16) - 0.5, np.arange(0, H + 16, 16).astype(np.float64), [H - 1.0, -0.5]])
    uu, vv = np.meshgrid(us, vs)
    uu, vv = uu.ravel(), vv.ravel()
    n1 = uu.size
    z1 = rng.uniform(2.0, 4.0, n1)
    parts = []
    x, y = _unproject(cam, uu, vv, z1)
    s = rng.uniform(2.0, 7.0, n1) * z1 / fx
    parts.append(_gaussians(np.stack([x, y, z1], 1), np.stack([s, s * 0.7, s], 1), _qaxis(2, rng.uniform(0, np.pi, n1)),
                            rng.uniform(0.3, 1.0, n1), _colors(rng, n1)))
    # outside the image, the footprint reaching in (up to 1.5 sigma inside the edge)
    n2 = 16
    z2 = rng.uniform(2.0, 4.0, n2)
    side = np.arange(n2) % 4
    sig = rng.uniform(4.0, 10.0, n2)
    off = sig * rng.uniform(0.3, 1.5, n2)
    u2 = np.where(side == 0, -off, np.where(side == 1, W - 1 + off, rng.uniform(0, W, n2)))
    v2 = np.where(side == 2, -off, np.where(side == 3, H - 1 + off, rng.uniform(0, H, n2)))
    x, y = _unproject(cam, u2, v2, z2)
    s = sig * z2 / fx
    parts.append(_gaussians(np.stack([x, y, z2], 1), np.stack([s, s, s], 1), _qaxis(2, np.zeros(n2)),
                            rng.uniform(0.5, 1.0, n2), _colors(rng, n2)))
    # just beyond the near plane (z = 0.2 + 1e-4 .. 0.21), and one just before it (culled)
    n3 = 8
    z3 = np.r_[0.2 + 1e-4, rng.uniform(0.2005, 0.21, n3 - 2), 0.2 - 1e-4]
    x, y = _unproject(cam, rng.uniform(0, W, n3), rng.uniform(0, H, n3), z3)
    s = rng.uniform(2.0, 6.0, n3) * z3 / fx
    parts.append(_gaussians(np.stack([x, y, z3], 1), np.stack([s, s, s], 1), _qaxis(2, np.zeros(n3)),
                            rng.uniform(0.3, 0.7, n3), _colors(rng, n3)))
    # screen radius beyond the image, behind everything else
    n4 = 3
    z4 = np.full(n4, 6.0)
    x, y = _unproject(cam, rng.uniform(0, W, n4), rng.uniform(0, H, n4), z4)
    s = 3.0 * max(W, H) * z4 / fx
    parts.append(_gaussians(np.stack([x, y, z4], 1), np.stack([s, s * 0.5, s], 1), _qaxis(2, [0.3, 1.0, 2.0]),
                            [0.4, 0.5, 0.6], _colors(rng, n4)))
    g = _cat(*parts)

    def check(cam, g, ref, geo, R):
        rad = ref["radii"]
        near = slice(n1 + n2, n1 + n2 + n3)
        assert (rad[near][:-1] > 0).all() and rad[near][-1] == 0, rad[near]
        outside = slice(n1, n1 + n2)
        px, py = geo["px"][outside], geo["py"][outside]
        out = (px < -0.5) | (px > W - 0.5) | (py < -0.5) | (py > H - 0.5)
        assert out.sum() >= n2 // 2 and (rad[outside][out] > 0).all()
        assert (rad[-n4:] > max(W, H)).all()
        return f"{n1} on tile borders / pixel centres, {int(out.sum())} outside reaching in, {n3 - 1} beyond the near plane"
    return cam, g, check


def scene_ties(W=96, H=64, n=300, seed=7):
    """coplanar splats facing the camera on two planes (z = 2 and z = 3 exactly), a third of them duplicated at the same
    position with another colour and opacity: exact depth ties everywhere, the ids decide the order"""
    cam = _cam(W, H)
    rng = np.random.default_rng(seed)
    fx, _ = _focal(cam)
    z = np.where(np.arange(n) % 2 == 0, 2.0, 3.0)
    x, y = _unproject(cam, rng.uniform(0, W, n), rng.uniform(0, H, n), z)
    s = rng.uniform(4.0, 12.0, n) * z / fx
    g = _gaussians(np.stack([x, y, z], 1), np.stack([s, s * rng.uniform(0.4, 1.0, n), np.full(n, 1e-4)], 1),
                   _qaxis(2, rng.uniform(0, np.pi, n)), rng.uniform(0.3, 0.9, n), _colors(rng, n))
    d = g["means3D"][: n // 3]
    dup = _gaussians(d, g["scales"][: n // 3], g["rotations"][: n // 3], rng.uniform(0.3, 0.9, n // 3),
                     _colors(rng, n // 3))
    g = _cat(g, dup)

    def check(cam, g, ref, geo, R):
        live = ref["radii"] > 0
        assert set(np.unique(g["means3D"][live, 2]).tolist()) == {2.0, 3.0}
        assert (np.asarray(geo["z"])[live] == np.where(g["means3D"][live, 2] == 2.0, 2.0, 3.0)).all()
        return f"{int(live.sum())} Gaussians on 2 depths, {n // 3} exact duplicates"
    return cam, g, check


SCENES = {
    "sat_opacity_1": lambda: scene_sat_stack(1.0, 1.0),
    "sat_opacity_098": lambda: scene_sat_stack(0.98, 1.0, seed=10),
    "sat_boundary": scene_sat_boundary,
    "sat_late_batch": scene_sat_late_batch,
    "needles": scene_needles,
    "needles_long": scene_needles_long,
    "long_top_class": scene_long_top,
    "long_dense": scene_long_dense,
    "ties": scene_ties,
}
BORDER_SIZES = [(15, 16), (16, 17), (17, 15), (31, 33), (33, 31), (255, 257), (257, 255)]
for _W, _H in BORDER_SIZES:
    SCENES[f"border_{_W}x{_H}"] = (lambda W=_W, H=_H: scene_borders(W, H))
COV_FORM = ["sat_opacity_1", "sat_opacity_098", "sat_boundary", "sat_late_batch", "needles", "needles_long"]

# Open findings, strict xfails (an XPASS fails: the mark goes with the fix).  The images of these scenes pass (forward
# tests); what fails is named per case.
_NEEDLE_GRAD = ("needle gradients: dL/dscales (dL/dmeans3D beyond 1024 px) of 1 .. 3 % of the needles beyond 2e-4 of the "
                "maximum: the conic's derivative carries 1 / det^2 of the cancelling det = a c - b^2")
KNOWN = {"needles": _NEEDLE_GRAD, "needles_long": _NEEDLE_GRAD}
KNOWN_FORWARD = {"border_257x255": "12 pixels differ from the oracle by up to 6.4e-4 (allowance: 6); cause not found"}


def _params(names, known):
    return [pytest.param(n, marks=pytest.mark.xfail(strict=True, reason=known[n])) if n in known else n for n in names]


# small versions of every regime for the fp64 comparison
SMALL = {
    "sat_opacity_098": lambda: scene_sat_stack(0.98, 1.0, W=48, H=32, n=150, seed=11),
    "sat_late_batch": lambda: scene_sat_late_batch(W=32, H=32, n_faint=300, n_opaque=150, seed=12),
    "needles": lambda: scene_needles(W=64, H=48, n=120, seed=13),
    "long_top_class": lambda: scene_long_top(W=48, H=48, heavy=5200, light=100, seed=14, tile=(1, 1)),
    "border_17x15": lambda: scene_borders(17, 15, seed=15),
    "ties": lambda: scene_ties(W=48, H=32, n=120, seed=16),
}


# ---------------------------------------------------------------------------------------------------------------------
# rendering and checks

_SCENE_CACHE = {}


def _scene(name, table=SCENES):
    """(camera, Gaussians, check, weights, fp32 oracle forward + backward, fp64 geometry): one oracle run per scene"""
    key = (name, table is SMALL)
    if key not in _SCENE_CACHE:
        from oracle.raster_oracle import RasterOracle
        cam, g, check = table[name]()
        w = np.random.default_rng(len(name)).normal(size=(3, cam.image_height, cam.image_width)).astype(np.float32)
        ref = RasterOracle(np.float32).render(cam.oracle_dict(bg=BG), **_kw(g), dL_dout=w)
        _SCENE_CACHE[key] = (cam, g, check, w, ref, _geom64(cam, g))
    return _SCENE_CACHE[key]


def _kw(g):
    return dict(means3D=g["means3D"], colors=g["colors"], opacities=g["opacities"], scales=g["scales"],
                rots=g["rotations"])


def _run_gpu(cam, g, w=None, cov=False):
    """forward (+ backward with dL/dimage = w) through the drop-in GaussianRasterizer with the image size's pair capacity
    reset (the first view of a size sorts with the count known on the host); returns numpy arrays and the pair count"""
    from contextgs_amd import rasterizer as rz
    H, W = cam.image_height, cam.image_width
    grad = w is not None
    t = {k: torch.tensor(v, device="cuda", requires_grad=grad) for k, v in g.items()}
    means2D = torch.zeros_like(t["means3D"], requires_grad=grad)
    kw = dict(means3D=t["means3D"], means2D=means2D, shs=None, colors_precomp=t["colors"], opacities=t["opacities"])
    if cov:
        kw["cov3D_precomp"] = cov6_torch(t["scales"], t["rotations"])
    else:
        kw.update(scales=t["scales"], rotations=t["rotations"])
    rz._pair_capacity.pop((H, W), None)
    try:
        color, radii = rz.GaussianRasterizer(settings(cam, debug=True))(**kw)
        R = int(rz.last_call["num_rendered"])
        out = {"color": color.detach().cpu().numpy(), "radii": radii.cpu().numpy(), "R": R}
        if grad:
            (color * torch.tensor(w, device="cuda")).sum().backward()
            torch.cuda.synchronize()
            out.update(dL_dmeans3D=t["means3D"].grad, dL_dmeans2D=means2D.grad, dL_dcolors=t["colors"].grad,
                       dL_dopacities=t["opacities"].grad.reshape(-1), dL_dscales=t["scales"].grad,
                       dL_drotations=t["rotations"].grad)
            for k in GRADS:
                out[k] = out[k].cpu().numpy()
    finally:
        rz._pair_capacity.pop((H, W), None)
    return out


def _check_image(a, b, what):
    d = np.abs(a - b)
    rmse = float(np.sqrt((d ** 2).mean()))
    n_out = int((d > 2e-5).sum())
    print(f"[allowance] {what}: {n_out} of {d.size} pixel values differ by more than 2e-5 (allowed {1e-4 * d.size:.0f}), max {d.max():.2e}, rmse {rmse:.2e}")
    assert rmse <= 1e-5, (what, rmse)
    assert n_out / d.size <= 1e-4, (what, n_out, d.max())
    assert d.max() <= 1.0 / 255 + 1e-4, (what, d.max())


def _check_grads(out, ref, what, rows=None):
    for k in GRADS:
        a, b = out[k], ref[k]
        if rows is not None:
            a, b = a[rows], b[rows]
        scale = max(1e-6, float(np.abs(b).max()))
        err = np.abs(a - b) / scale
        n_out = int((err > 2e-4).sum())
        print(f"[allowance] {k} {what}: {n_out} of {err.size} entries beyond 2e-4 of the maximum (allowed {2e-3 * err.size:.0f}), worst {err.max():.2e}")
        assert float((err > 2e-4).mean()) <= 2e-3, (k, what, float(err.max()), n_out)
        assert float(np.median(err)) <= 1e-6, (k, what, float(np.median(err)))


def _regime(name, table=SCENES, R=None):
    cam, g, check, w, ref, geo = _scene(name, table)
    msg = check(cam, g, ref, geo, R)
    print(f"[regime] {name}: {msg}")


@pytest.mark.parametrize("bin_mode", [1, 2], indirect=True)
@pytest.mark.parametrize("name", _params(SCENES, KNOWN_FORWARD))
def test_forward_matches_oracle(name, bin_mode):
    cam, g, check, w, ref, geo = _scene(name)
    out = _run_gpu(cam, g)
    _regime(name, R=out["R"])
    assert (out["radii"] == ref["radii"]).all(), np.nonzero(out["radii"] != ref["radii"])
    _check_image(out["color"], ref["color"], f"forward {name} mode {bin_mode}")


@pytest.mark.parametrize("name", _params(SCENES, {**KNOWN, **KNOWN_FORWARD}))
def test_backward_matches_oracle(name):
    cam, g, check, w, ref, geo = _scene(name)
    out = _run_gpu(cam, g, w)
    _regime(name, R=out["R"])
    assert (out["radii"] == ref["radii"]).all()
    _check_image(out["color"], ref["color"], f"backward-run image {name}")
    _check_grads(out, ref, name)


@pytest.mark.parametrize("name", _params(COV_FORM, {"needles": _NEEDLE_GRAD}))
def test_cov3d_precomp_matches_oracle(name):
    """the cov3D_precomp form (csrc/raster_forms.h repeats the preprocess tail) on the saturation and needle scenes:
    cov3D built in torch from the same scales and rotations, gradients of scales / rotations through torch"""
    cam, g, check, w, ref, geo = _scene(name)
    out = _run_gpu(cam, g, w, cov=True)
    same = out["radii"] == ref["radii"]
    print(f"[allowance] cov3D {name}: {int((~same).sum())} of {same.size} radii differ (allowed {1e-4 * same.size:.0f})")
    assert (~same).sum() <= int(1e-4 * same.size), np.nonzero(~same)
    _check_image(out["color"], ref["color"], f"cov3D image {name}")
    _check_grads(out, ref, f"cov3D {name}", rows=same)


@pytest.mark.parametrize("name", _params(SMALL, {"needles": _NEEDLE_GRAD}))
def test_error_against_fp64_is_that_of_the_fp32_oracle(name, oracle64):
    """The GPU kernels' error against the fp64 oracle, next to the plain fp32 oracle's error.

    Statistic: the 99.9th percentile of |x - x64| over the image values, and of |x - x64| / max |x64| over each gradient's
    entries; the GPU's may be at most 2x the fp32 oracle's plus 1e-6.  A percentile and not the maximum, because the fp32
    codes and the fp64 code take some alpha >= 1/255 and termination decisions differently on the last ulp, and one such
    flip moves a pixel by up to 1/255 and the gradients of every Gaussian on that pixel.  Those values are excluded
    outright: the image values where either fp32 code differs from the other or from fp64 by more than 2e-5, the gradient
    entries where they differ by more than 2e-4 of the maximum - the oracle32 comparisons bound how many there can be,
    and they are asserted below to stay under 1e-3 of the values.  What is left is rounding: a kernel whose sums drift
    with the list length (v_exp_f32 through the prescaled conic, sums reassociated in LDS and DPP) shows up in it even
    where it stays within the oracle32 tolerance."""
    cam, g, check, w, ref32, geo = _scene(name, SMALL)
    _regime(name, SMALL)
    ref64 = oracle64.render(cam.oracle_dict(bg=BG), **_kw(g), dL_dout=w)
    out = _run_gpu(cam, g, w)
    assert (out["radii"] == ref32["radii"]).all()

    def compare(what, gpu, o32, o64, scale, flip_tol):
        e_gpu, e_32 = np.abs(gpu - o64) / scale, np.abs(o32 - o64) / scale
        flip = (np.abs(gpu - o32) / scale > flip_tol) | (e_32 > flip_tol)
        keep = ~flip
        assert flip.mean() <= 1e-3 or flip.sum() <= 2, (what, int(flip.sum()))
        p_gpu = float(np.percentile(e_gpu[keep], 99.9)) if keep.any() else 0.0
        p_32 = float(np.percentile(e_32[keep], 99.9)) if keep.any() else 0.0
        print(f"[fp64] {name} {what}: p99.9 error gpu {p_gpu:.2e}, oracle32 {p_32:.2e} ({int(flip.sum())} flipped excluded)")
        assert p_gpu <= 2 * p_32 + 1e-6, (what, p_gpu, p_32)

    compare("image", out["color"], ref32["color"], ref64["color"], 1.0, 2e-5)
    for k in GRADS:
        compare(k, out[k], ref32[k], ref64[k], max(1e-6, float(np.abs(ref64[k]).max())), 2e-4)
