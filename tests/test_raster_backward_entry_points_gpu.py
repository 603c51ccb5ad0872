"""The two places where the one driver behind the seven cgs_raster_backward* entry points (csrc/api.hip, raster_backward_run) can
go wrong without any of the value tests noticing, on the C-ABI directly:

  * a view whose Gaussians are all culled (R == 0): no blend runs, and what the caller reads is what the zero fill (or, for
    _det, the sum kernel over no slots) and the per-Gaussian backward wrote.  include/cgs.h promises exact zeros for culled
    Gaussians and full-row writes from _det; here every output starts as NaN (dL_dcolors / dL_dopacities as zeros where the
    contract has the caller zero them) and the scratch and det_ws as 0xFF bytes;
  * the size of the zero fill: an entry point fills its own scratch layout and not the largest one's."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from contextgs_amd.synth import look_at_camera
from raster_backward_entries import ENTRIES, MAPS

pytestmark = pytest.mark.gpu

H = W = 16
FORMS = ("colours + scales / rotations", "SH degree 1 + cov3D")
COLS = {"cgs_raster_backward_abs": (4,), "cgs_raster_backward_det": (3, 4)}       # every other entry point: 3


def _bytes(n, value):
    return torch.full((max(int(n), 256),), value, dtype=torch.uint8, device="cuda")


def _view(means3D, sh_cov):
    """The forward of one view through the C-ABI, with the view's true pair count R: the arguments of the backward by name."""
    from contextgs_amd import _lib
    from contextgs_amd import rasterizer as rz
    L, p = _lib.lib(), _lib.ptr
    cam = look_at_camera((0.0, -3.0, 0.0), (0, 0, 0), W, H, fovx_deg=60.0).to_torch("cuda")
    rs = rz.GaussianRasterizationSettings(H, W, math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), torch.zeros(3, device="cuda"), 1.0,
                                          cam.world_view_transform, cam.full_proj_transform, 1, cam.camera_center, False, False)
    cfg = rz._Cfg(rs)
    rng = np.random.default_rng(0)
    P = len(means3D)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device="cuda")
    k = dict(means3D=t(means3D), opacities=t(np.full((P, 1), 0.8)), colors=None, shs=None, scales=None, rotations=None, cov3D=None)
    if sh_cov:
        k.update(shs=t(rng.normal(size=(P, 4, 3))), cov3D=t(np.tile([0.09, 0.0, 0.0, 0.09, 0.0, 0.09], (P, 1))))
    else:
        k.update(colors=t(rng.uniform(size=(P, 3))), scales=t(np.full((P, 3), 0.3)), rotations=t(np.tile([1.0, 0, 0, 0], (P, 1))))
    D, M = (1, 4) if sh_cov else (0, 0)
    stream = _lib.current_stream()
    radii = torch.empty(P, dtype=torch.int32, device="cuda")
    geom, img = _bytes(L.cgs_raster_geom_bytes(P), 0), _bytes(L.cgs_raster_img_bytes(H, W), 0)
    ticket, n = C.c_uint64(0), C.c_int64(0)
    _lib.check(L.cgs_raster_preprocess_launch_ex(cfg.ref, P, p(k["means3D"]), p(k["colors"]), p(k["shs"]), D, M, p(k["opacities"]),
                                                 p(k["scales"]), p(k["rotations"]), p(k["cov3D"]), p(geom), geom.numel(), p(radii),
                                                 stream, C.byref(ticket)), "cgs_raster_preprocess_launch_ex")
    _lib.check(L.cgs_raster_preprocess_wait(ticket, C.byref(n)), "cgs_raster_preprocess_wait")
    R = int(n.value)
    binws = _bytes(L.cgs_raster_bin_bytes(P, R), 0)
    color = torch.empty(3, H, W, device="cuda")
    _lib.check(L.cgs_raster_render(cfg.ref, P, R, p(geom), geom.numel(), p(binws), binws.numel(), p(img), img.numel(), p(color),
                                   stream), "cgs_raster_render")
    k.update(cfg=cfg, P=P, R=R, sh_degree=D, sh_coeffs=M, radii=radii, geom_ws=geom, geom_bytes=geom.numel(), bin_ws=binws,
             bin_bytes=binws.numel(), img_ws=img, img_bytes=img.numel(), stream=stream,
             dL_dout=t(rng.normal(size=(3, H, W))), opts=0, features=None, C=0, dL_dfeatures_map=None, dL_dfeatures=None)
    k.update({m: t(rng.normal(size=(H, W))) for m in MAPS})
    return k


def _backward(entry, k, outs, scratch, cols=3, det_ws=None):
    from contextgs_amd import _lib
    L = _lib.lib()
    a = dict(k, **outs, scratch=scratch, scratch_bytes=scratch.numel(), means2D_cols=cols, det_ws=det_ws,
             det_bytes=det_ws.numel() if det_ws is not None else 0)
    if entry == "cgs_raster_backward_det":      # (it refuses the map gradients)
        a.update({m: None for m in MAPS})
    args = []
    for name in ENTRIES[entry][0]:
        v = a[name]
        args.append(v.ref if name == "cfg" else v if name == "stream" else _lib.ptr(v) if isinstance(v, torch.Tensor) else v)
    _lib.check(getattr(L, entry)(*args), entry)
    torch.cuda.synchronize()


ALL_CULLED = [(e, f, c) for f in FORMS for e in ENTRIES for c in COLS.get(e, (3,))
              if not (f == FORMS[1] and e == "cgs_raster_backward")]       # (cgs_raster_backward has the first form only)


@pytest.mark.parametrize("entry,form,cols", ALL_CULLED,
                         ids=[f"{e[11:]}-{'sh_cov' if f == FORMS[1] else 'plain'}-{c}" for e, f, c in ALL_CULLED])
def test_all_culled_view_gives_exact_zeros(entry, form, cols):
    """8 Gaussians behind the camera: R == 0, every gradient exactly zero, dL_dmeans2D written in the entry point's column count
    (the floats behind 3 columns keep their NaN)."""
    from contextgs_amd import _lib
    L = _lib.lib()
    sh_cov = form == FORMS[1]
    P = 8
    k = _view([(0.1 * i - 0.4, -6.0 - 0.2 * i, 0.05 * i) for i in range(P)], sh_cov)
    assert k["R"] == 0 and int((k["radii"] != 0).sum()) == 0
    det = entry == "cgs_raster_backward_det"
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    acc = nan if det else (lambda *s: torch.zeros(*s, device="cuda"))      # _det overwrites them; the others add into zeros
    outs = dict(dL_dmeans3D=nan(P, 3), dL_dmeans2D=nan(P * 4), dL_dcolors=acc(P, 3), dL_dopacities=acc(P, 1),
                dL_dshs=nan(P, 4, 3) if sh_cov else None, dL_dscales=None if sh_cov else nan(P, 3),
                dL_drotations=None if sh_cov else nan(P, 4), dL_dcov3D=nan(P, 6) if sh_cov else None)
    scratch = _bytes(getattr(L, ENTRIES[entry][1])(P), 0xFF)
    det_ws = _bytes(L.cgs_raster_bwd_det_bytes(P, 0, cols), 0xFF) if det else None
    _backward(entry, k, outs, scratch, cols, det_ws)
    m2 = outs.pop("dL_dmeans2D")
    assert torch.equal(m2[:P * cols], torch.zeros(P * cols, device="cuda")), m2
    assert bool(torch.isnan(m2[P * cols:]).all()), m2
    for name, v in outs.items():
        if v is not None:
            assert torch.equal(v, torch.zeros_like(v)), (name, v)


@pytest.mark.parametrize("entry", ["cgs_raster_backward", "cgs_raster_backward_ex", "cgs_raster_backward_aux"])
def test_zero_fill_is_the_entry_points_own_size(entry):
    """One visible Gaussian, the scratch 256 guard bytes longer than the entry point's own query says: the guard is intact."""
    from contextgs_amd import _lib
    L = _lib.lib()
    k = _view([(0.0, 0.0, 0.0)], False)
    assert k["R"] > 0
    P = 1
    need = getattr(L, ENTRIES[entry][1])(P)
    scratch = _bytes(need + 256, 0xA5)
    outs = dict(dL_dmeans3D=torch.empty(P, 3, device="cuda"), dL_dmeans2D=torch.empty(P, 3, device="cuda"),
                dL_dcolors=torch.zeros(P, 3, device="cuda"), dL_dopacities=torch.zeros(P, 1, device="cuda"), dL_dshs=None,
                dL_dscales=torch.empty(P, 3, device="cuda"), dL_drotations=torch.empty(P, 4, device="cuda"), dL_dcov3D=None)
    _backward(entry, k, outs, scratch)
    assert need % 256 == 0 and bool((scratch[need:] == 0xA5).all()), scratch[need:]
    assert bool(torch.isfinite(outs["dL_dmeans3D"]).all()) and float(outs["dL_dcolors"].abs().sum()) > 0
