"""The rasterizer's image and gradients per element against the fp64 oracle (tests/raster_units_ref.py: the reference, the
error unit of every element, the decision-free scenes), through the drop-in GaussianRasterizer: the default backward (float
atomics), deterministic=True (store-and-sum), both binnings (cgs_debug_set_bin_mode 1 and 2), absgrad=True, and the
precomputed-covariance form on `open` and `terminating`.

Every image value and every gradient entry is within UNITS_KERNEL[scene][tensor] = 2 UNITS_LITERAL[scene][tensor] units of
the fp64 value, an element whose unit is 0 is exactly 0, and the radii are the oracle's: no percentile, nothing left out.
UNITS_LITERAL is what the fp32 oracle needs (tests/test_raster_units.py); neither number is taken from the kernels' results.

Largest error in units per scene and tensor (fp32 oracle: the literal, on the CPU, rounded up; the other rows on an MI355X,
the maximum over both binnings and the runs with and without absgrad; the cap of a row is twice its scene's first row):
                                    image   means3D   means2D    colors opacities    scales rotations   absgrad
  open         fp32 oracle              8       2.2       1.3       3.8       2.5       2.5       2.4       6.9
               default               8.00      2.05      1.52      1.26      1.14      2.16      2.33      5.37
               deterministic         8.00      1.92      1.52      1.26      1.31      1.77      1.93      4.63
               cov3D_precomp         8.09      2.05      1.52      1.61      1.31      2.06      2.33         -
  open3        fp32 oracle            7.7       1.3       1.2       1.5      0.97       1.9         2       2.1
               default               7.51      1.21      1.18      1.94      1.32      2.26      1.86      2.69
               deterministic         7.51      1.14      1.13      1.65      1.32      2.26      1.86      2.69
  long         fp32 oracle             29       5.5         4       1.9       2.9       180       5.9        28
               default              28.69      3.20      2.66      1.20      2.58     27.00     10.16     10.30
               deterministic        28.69      3.08      2.77      1.08      2.58     27.00      8.17      9.45
  terminating  fp32 oracle             11        21       9.9        17       6.4        11       8.5        27
               default              12.21     18.24      9.83     14.88      6.38     10.61      9.05     27.33
               deterministic        12.21     18.24      9.83     15.53      6.38     10.61      9.05     25.43
               cov3D_precomp        10.37     19.08     10.55     16.83      7.19     10.10      8.46         -
  clamp        fp32 oracle            8.2        11       9.3       6.8       7.3       5.4       7.5        11
               default               6.65     10.41      9.14      6.72      9.28      4.98      7.73     11.06
               deterministic         6.65     10.41      9.14      6.72      9.28      4.98      7.73     11.06
  borders      fp32 oracle            6.3        41        42       8.9        11        80        40        42
               default               5.57     40.46     41.57      8.84     10.69     81.02     39.36     41.57
               deterministic         5.57     40.46     41.57      8.84     10.69     81.02     39.36     41.57
  thin_1x1     fp32 oracle            2.4        26        23       2.4        16        82        30        23
               default               2.34     30.48     31.12      2.32     24.45     61.75     30.84     31.12
               deterministic         2.34     30.48     31.12      2.32     24.45     61.75     30.84     31.12
  thin_16x1    fp32 oracle            2.4        12        11       7.1       4.5        77       5.8        12
               default               2.50     10.06      8.28      5.69      4.43     19.80      3.80      9.54
               deterministic         2.50     10.06      8.28      5.69      4.43     19.80      3.80      9.54
  thin_1x17    fp32 oracle            3.8       6.3       6.3       2.3       2.6       4.5        28       6.2
               default               3.71      6.22      6.80      3.21      2.19      6.75     25.75      5.02
               deterministic         3.71      6.22      6.80      3.21      2.19      6.75     25.75      5.02
The image column does not depend on the backward.  In twenty further runs of the default backward per scene (float atomics: the
order of a Gaussian's per-tile sums differs from run to run) only dL_drotations of `long` came beyond 0.8 of its cap (4.4 .. 10.2 of
11.8); the deterministic backward repeats its figures bit for bit.

What the unit had to learn.  With u = 2^-24 M alone (M: the sum of the per-pixel magnitudes) the default backward reached 46.4
units on one dL_dscales entry of `terminating` against a literal of 23 (the deterministic one 20 on the same entry), and 5.4 ..
6.4 on dL_dopacities of a 1 x 17 image against 2.3.  The exponent's share E (tests/raster_units_ref.py: the kernels' prescaled
conic and v_exp_f32 put G up to 20 times 2^-24 off where the exponent's terms sum to 21, by an fp32 emulation on the CPU) went
into the unit for it, as the sigmoid's |s| did in tests/expand_ref.py; literal and caps above are in that unit.  Not explained by
it, and left as an observation: with 60 degrees across the single pixel column of a 1 x 17 image (168 degrees down it) the kernels'
dL_dopacities, dL_dscales and dL_drotations stayed at 3 .. 3.6 times the literal (5.6 / 1.6, 20 / 8.7, 22 / 7.4 units), while the same
C text compiled with fused multiply-adds exceeded twice the literal as well (dL_dscales of the 1 x 1 image, 173 / 83): at that
field of view the perspective terms of the Jacobian carry the covariance (variances of 70 .. 740 square pixels from Gaussians of
1 .. 5 pixels) and the largest entry of six Gaussians says little.  The thin scenes' camera is capped at 100 degrees down the
height instead; no cap was moved.

That the tests bite (each alteration built once into a copy of the library, arithmetic only, never committed; this file, then
tests/test_raster_gpu.py::test_backward_matches_oracle and all of tests/test_raster_regimes_gpu.py run once on it; 47 tests here):
  T = T * inv_om for the division: 5 of 47 fail, all of them `long` (every path; dL_dcolors 19.8 units against a cap of 3.8,
      dL_dopacities 25.4 / 5.8, dL_dmeans3D 38 / 11, absgrad 265 / 56: the 5 .. 8 times of the kernel's comment).  The drift needs
      the 540-entry lists; in the other scenes the two forms differ by an ulp on a few entries and stay inside.
      test_backward_matches_oracle passes; of the regimes file only the fp64 percentile test notices (2 of its 6 cases).
  the bound passed to rb_list_build one lower: 47 of 47 fail (a block loses its last contribution).  This one the old tests see
      too: test_backward_matches_oracle fails in 3 + 13 cases, the regimes' cov3D and fp64 tests in 5 + 5.
  v[3] (the conic gradient's off-diagonal term) times 1 + 1e-4: 47 of 47 fail, by 5 .. 100 000 units (dL_dmeans3D, dL_dscales,
      dL_drotations).  Both test_backward_matches_oracle pass; the fp64 percentile test fails in 5 cases, the cov3D test in 1.
  the background term neg_bg_T * inv_om dropped: 47 of 47 fail; so do the old tests (3 + 13, 5, 5 as above).
  in the preprocess backward (raster_bwd.hip), the r = 0 term of ds[k] times 1 + 1e-4: 45 of 47 fail (dL_dscales); the two that
      pass are the cov3D_precomp tests, whose scale gradient goes through torch and not through that line.
      The regimes' test_backward_matches_oracle passes; test_raster_gpu.py's fails in 1 of its cases, the fp64 test in 5.
"""
import types

import numpy as np
import pytest
import torch

import raster_units_ref as ru
from raster_harness import cov6_torch, settings
from raster_units_ref import UNITS_KERNEL, UNITS_LITERAL

pytestmark = pytest.mark.gpu


@pytest.fixture
def bin_mode(request):
    """cgs_debug_set_bin_mode for one test: 1 = radix passes over (tile, Gaussian) pairs, 2 = two-level (bucket) binning"""
    from contextgs_amd import _lib
    L = _lib.lib()
    _lib.check(L.cgs_debug_set_bin_mode(request.param), "cgs_debug_set_bin_mode")
    yield request.param
    _lib.check(L.cgs_debug_set_bin_mode(0), "cgs_debug_set_bin_mode")


def _run(sc, w, deterministic=False, absgrad=False, cov=False):
    """Forward and the backward of sum(image * w) on fresh leaves, with the image size's pair capacity reset (the first view of
    a size sorts with the count known on the host) -> numpy arrays under the reference's names."""
    from contextgs_amd import rasterizer as rz
    H, W = sc.cam.image_height, sc.cam.image_width
    t = {k: torch.tensor(v, device="cuda", requires_grad=True) for k, v in sc.g.items()}
    P = t["means3D"].shape[0]
    m2 = torch.zeros(P, 4 if absgrad else 3, device="cuda", requires_grad=True)
    kw = dict(means3D=t["means3D"], means2D=m2, shs=None, colors_precomp=t["colors"], opacities=t["opacities"],
              deterministic=deterministic)
    if absgrad:
        kw["absgrad"] = True
    if cov:
        kw["cov3D_precomp"] = cov6_torch(t["scales"], t["rotations"])
    else:
        kw.update(scales=t["scales"], rotations=t["rotations"])
    rz._pair_capacity.pop((H, W), None)
    try:
        image, radii = rz.GaussianRasterizer(settings(sc.cam, bg=sc.bg))(**kw)
        (image * torch.tensor(w, device="cuda")).sum().backward()
        torch.cuda.synchronize()
    finally:
        rz._pair_capacity.pop((H, W), None)
    n = lambda a: a.detach().cpu().numpy()
    g2 = n(m2.grad)
    out = dict(image=n(image), radii=n(radii), dL_dmeans3D=n(t["means3D"].grad), dL_dcolors=n(t["colors"].grad),
               dL_dopacities=n(t["opacities"].grad).reshape(-1), dL_dscales=n(t["scales"].grad),
               dL_drotations=n(t["rotations"].grad), means2D_grad=g2)
    if absgrad:
        assert g2.shape == (P, 4)
        out["dL_dmeans2D"] = np.concatenate([g2[:, :2], np.zeros((P, 1), np.float32)], axis=1)
        out["absgrad"] = g2[:, 2:4]
    else:
        assert g2.shape == (P, 3)
        out["dL_dmeans2D"] = g2
    return out


def _check(sc, ref, out, what, rows=None):
    """Every tensor of `out` within its cap, unit-0 elements exactly 0 (`units_error`); rows: the Gaussians compared (the image
    always is)."""
    tensors = [k for k in ru.TENSORS if k in out]
    got = {k: out[k] for k in tensors}
    if rows is not None:
        got = {k: (v if k == "image" else v[rows]) for k, v in got.items()}
        ref = _select(ref, rows)
    measured = ru.compare(ref, got, tensors)
    print(f"[raster-units] {sc.name} {what}, units gpu / literal: " +
          ", ".join(f"{k.replace('dL_d', '')} {measured[k]:.3g} / {UNITS_LITERAL[sc.name][k]:g}" for k in tensors))
    over = {k: (round(v, 2), UNITS_KERNEL[sc.name][k]) for k, v in measured.items() if v > UNITS_KERNEL[sc.name][k]}
    assert not over, (sc.name, what, "beyond the cap (measured, cap)", over)
    return measured


def _select(ref, rows):
    """The reference restricted to the Gaussians `rows` (the image untouched)."""
    return types.SimpleNamespace(image=ref.image, absgrad=ref.absgrad[rows], grads={k: v[rows] for k, v in ref.grads.items()},
                                 units={k: (v if k == "image" else v[rows]) for k, v in ref.units.items()})


@pytest.mark.parametrize("bin_mode", [1, 2], indirect=True)
@pytest.mark.parametrize("path", ["default", "deterministic"])
@pytest.mark.parametrize("name", ru.SCENES)
def test_every_element_within_the_cap(name, path, bin_mode, oracle64):
    sc = ru.scene(name)
    ref = ru.reference(oracle64, sc)
    out = _run(sc, ref.w, deterministic=(path == "deterministic"))
    assert np.array_equal(out["radii"], ref.radii), np.nonzero(out["radii"] != ref.radii)[0]
    _check(sc, ref, out, f"{path}, bin mode {bin_mode}")


@pytest.mark.parametrize("name", ru.SCENES)
def test_absgrad_is_the_sum_of_magnitudes(name, oracle64):
    """Columns 2:4 of the means2D gradient against M of columns 0:2 (the fp64 sum of the per-pixel magnitudes itself) within
    the cap, on both backwards; with deterministic=True everything else is the call without the flag bit for bit (the default
    path's float atomics have no order to repeat: there every tensor meets its cap instead)."""
    sc = ru.scene(name)
    ref = ru.reference(oracle64, sc)
    for det in (False, True):
        out = _run(sc, ref.w, deterministic=det, absgrad=True)
        assert np.array_equal(out["radii"], ref.radii)
        _check(sc, ref, out, f"absgrad, {'deterministic' if det else 'default'}")
        assert (out["absgrad"] >= 0).all()
    plain = _run(sc, ref.w, deterministic=True)
    for k in ("image",) + ru.GRADS:
        cols = slice(0, 2) if k == "dL_dmeans2D" else slice(None)         # (with the flag the z column makes way for 2:4)
        a, b = (np.ascontiguousarray(o[k][..., cols]).view(np.uint32) for o in (out, plain))
        assert np.array_equal(a, b), (name, k, "absgrad changed bits of the deterministic backward")


@pytest.mark.parametrize("name", ru.COV_FORM)
def test_cov3d_precomp_within_the_cap(name, oracle64):
    """The cov3D_precomp form (cov3D built in torch from the same scales and rotations, their gradients through torch),
    compared when its radii are the oracle's: the allowance of tests/test_raster_regimes_gpu.py for this form, unchanged
    (radii equal on all but 1e-4 of the Gaussians, which is none of so few; gradients on the rows whose radii agree)."""
    sc = ru.scene(name)
    ref = ru.reference(oracle64, sc)
    out = _run(sc, ref.w, cov=True)
    same = out["radii"] == ref.radii
    print(f"[allowance] cov3D {name}: {int((~same).sum())} of {same.size} radii differ (allowed {1e-4 * same.size:.0f})")
    assert (~same).sum() <= int(1e-4 * same.size), np.nonzero(~same)[0]
    _check(sc, ref, out, "cov3D_precomp", rows=same)
