"""The argument checks of the seven cgs_raster_backward* entry points, one table: every entry point times every fault its
signature can express, with stand-in pointers (tests/test_raster_absgrad.py), so that nothing is launched and no device is
needed.  The seven share one driver (csrc/api.hip, raster_backward_run); the expected (return code, message) pairs below were
recorded from a build of the commit BEFORE that driver existed, where the checks were written out four times, and pin that the
merge moved no check, no code and no text.  The entries that differ from what that build returned on purpose carry a comment:

  * `was unprefixed`: the two oldest entry points said "backward scratch too small", "workspace too small" and "binning
    workspace missing or too small" without their name; they take the common wording of the others now.
  * `was enqueued`: cgs_raster_backward / _ex had no check of P < 0 or R < 0 and zero-filled the scratch before looking at the
    binning workspace, so these calls reached the device (here, without one: CGS_ERR_HIP); now they are refused first."""
import ctypes as C

import pytest

from raster_backward_entries import ENTRIES, MAPS

CGS_OK, CGS_ERR_ARG, CGS_ERR_WORKSPACE = 0, 1, 3
P1 = 4096       # a non-NULL stand-in: the checks only look at which pointers are given
BIG = 1 << 40

# one Gaussian, no pair, colours + scales / rotations, every pointer the form needs given
BASE = dict(P=1, R=0, means3D=P1, colors=P1, shs=None, sh_degree=0, sh_coeffs=0, opacities=P1, scales=P1, rotations=P1, cov3D=None,
            radii=P1, geom_ws=P1, geom_bytes=BIG, bin_ws=None, bin_bytes=0, img_ws=P1, img_bytes=BIG, dL_dout=P1, dL_ddepth=None,
            dL_dinvdepth=None, dL_dalpha=None, dL_dmeans3D=P1, dL_dmeans2D=P1, dL_dcolors=P1, dL_dopacities=P1, dL_dshs=None,
            dL_dscales=P1, dL_drotations=P1, dL_dcov3D=None, scratch=P1, scratch_bytes=BIG, stream=None, opts=0, features=None, C=0,
            dL_dfeatures_map=None, dL_dfeatures=None, means2D_cols=3, det_ws=P1, det_bytes=BIG)
SH_COV = dict(colors=None, shs=P1, sh_degree=1, sh_coeffs=4, scales=None, rotations=None, cov3D=P1, dL_dshs=P1, dL_dscales=None,
              dL_drotations=None, dL_dcov3D=P1)       # SH degree 1 + cov3D
POINTERS = [k for k, v in BASE.items() if v in (P1, None) and k != "stream"]
SHORT, SMALLER = "one byte short", "the next smaller layout"        # resolved per entry point by _call


def _faults(entry):
    """name -> overrides of BASE: every fault of the list that `entry` accepts as an argument."""
    names, _, smaller = ENTRIES[entry]
    oldest = entry in ("cgs_raster_backward", "cgs_raster_backward_ex")
    f = {"cfg NULL": dict(cfg=None), "image height 0": dict(H=0), "P = -1": dict(P=-1), "R = -1": dict(R=-1),
         "P = 0, every pointer NULL": dict(P=0, geom_bytes=0, img_bytes=0, scratch_bytes=0, det_bytes=0, **{k: None for k in POINTERS})}
    if "shs" in names:
        f["colours and SH"] = dict(shs=P1, sh_degree=1, sh_coeffs=4)
        f["neither colours nor SH"] = dict(colors=None)
        f["scales / rotations and cov3D"] = dict(cov3D=P1)
        f["neither scales / rotations nor cov3D"] = dict(scales=None, rotations=None)
        for g in ("dL_dshs", "dL_dcov3D", "dL_dmeans3D", "dL_dmeans2D"):
            f[f"SH + cov3D, {g} NULL"] = dict(SH_COV, **{g: None})
    for g in ("dL_dmeans3D", "dL_dmeans2D", "dL_dcolors", "dL_dopacities", "dL_dscales", "dL_drotations"):
        f[f"{g} NULL"] = {g: None}
    # where dL_dout may be NULL a short scratch stands behind it: its message says that the NULL was let through
    f["dL_dout NULL"] = dict(dL_dout=None) if oldest else dict(dL_dout=None, scratch_bytes=SHORT)
    for w in ("geom_ws", "img_ws", "scratch"):
        f[f"{w} NULL"] = {w: None}
    f["bin_ws NULL with R = 1"] = dict(R=1)
    f["scratch one byte short"] = dict(scratch_bytes=SHORT)
    if smaller:
        f["scratch of the next smaller layout"] = dict(P=1000, scratch_bytes=SMALLER)
    if "opts" in names:
        f["unknown opts bit"] = dict(opts=4)
        f["CGS_RASTER_ANTIALIAS without opacities"] = dict(opts=1, opacities=None)
    if "features" in names:
        f["features without dL_dfeatures"] = dict(features=P1, C=5, dL_dfeatures_map=P1)
        f["dL_dfeatures without features"] = dict(dL_dfeatures=P1, C=5, dL_dfeatures_map=P1)
        f["C = 0"] = dict(features=P1, dL_dfeatures=P1, dL_dfeatures_map=P1, C=0)
        f["C = 33"] = dict(features=P1, dL_dfeatures=P1, dL_dfeatures_map=P1, C=33)
    if "det_ws" in names:
        for m in MAPS:
            f[f"{m} given"] = {m: P1}
        f["means2D_cols = 2"] = dict(means2D_cols=2)
        f["det_ws NULL"] = dict(det_ws=None)
        f["det_ws one byte short"] = dict(R=1, bin_ws=P1, bin_bytes=BIG, det_bytes=SHORT)
    return f


def _call(entry, fault):
    from contextgs_amd import _lib
    L = _lib.lib()
    names, query, smaller = ENTRIES[entry]
    a = dict(BASE, **fault)
    fake = C.c_void_p(256)      # never dereferenced: every call fails its checks first, or returns at P == 0
    cfg = _lib.RasterCfg(image_height=a.pop("H", 16), image_width=16, tanfovx=0.5, tanfovy=0.5, scale_modifier=1.0, prefiltered=0,
                         debug=0, viewmatrix=fake, projmatrix=fake, campos=fake, bg=fake)
    a["cfg"] = C.byref(cfg) if a.get("cfg", True) is not None else None
    if a["scratch_bytes"] == SHORT:
        a["scratch_bytes"] = getattr(L, query)(a["P"]) - 1
    elif a["scratch_bytes"] == SMALLER:
        a["scratch_bytes"] = getattr(L, smaller)(a["P"])
    if a["det_bytes"] == SHORT:
        a["det_bytes"] = L.cgs_raster_bwd_det_bytes(a["P"], a["R"], a["means2D_cols"]) - 1
    rc = getattr(L, entry)(*(a[n] for n in names))
    return rc, L.cgs_last_error().decode()


# (return code, message) per entry point and fault, recorded from the parent build (module docstring)
EXPECTED = {
    "cgs_raster_backward": {
        "cfg NULL": (1, "cfg is NULL"),
        "image height 0": (1, "bad image size 16x0"),
        "P = -1": (1, "cgs_raster_backward: P < 0 or R < 0"),      # was enqueued
        "R = -1": (1, "cgs_raster_backward: P < 0 or R < 0"),      # was enqueued
        "P = 0, every pointer NULL": (0, ""),
        "dL_dmeans3D NULL": (1, "cgs_raster_backward: NULL input"),
        "dL_dmeans2D NULL": (1, "cgs_raster_backward: NULL input"),
        "dL_dcolors NULL": (1, "cgs_raster_backward: NULL input"),
        "dL_dopacities NULL": (1, "cgs_raster_backward: NULL input"),
        "dL_dscales NULL": (1, "cgs_raster_backward: NULL input"),
        "dL_drotations NULL": (1, "cgs_raster_backward: NULL input"),
        "dL_dout NULL": (1, "cgs_raster_backward: NULL input"),
        "geom_ws NULL": (3, "cgs_raster_backward: workspace too small"),      # was unprefixed
        "img_ws NULL": (3, "cgs_raster_backward: workspace too small"),      # was unprefixed
        "scratch NULL": (1, "cgs_raster_backward: NULL input"),
        "bin_ws NULL with R = 1": (3, "cgs_raster_backward: workspace too small"),      # was enqueued
        "scratch one byte short": (3, "cgs_raster_backward: scratch too small: 511 < 512"),      # was unprefixed
    },
    "cgs_raster_backward_ex": {
        "cfg NULL": (1, "cfg is NULL"),
        "image height 0": (1, "bad image size 16x0"),
        "P = -1": (1, "cgs_raster_backward: P < 0 or R < 0"),      # was enqueued
        "R = -1": (1, "cgs_raster_backward: P < 0 or R < 0"),      # was enqueued
        "P = 0, every pointer NULL": (0, ""),
        "colours and SH": (1, "cgs_raster_backward_ex: please provide exactly one of either SHs or precomputed colors"),
        "neither colours nor SH": (1, "cgs_raster_backward_ex: please provide exactly one of either SHs or precomputed colors"),
        "scales / rotations and cov3D": (1, "cgs_raster_backward_ex: please provide exactly one of either scale/rotation pair or precomputed 3D covariance"),
        "neither scales / rotations nor cov3D": (1, "cgs_raster_backward_ex: please provide exactly one of either scale/rotation pair or precomputed 3D covariance"),
        "SH + cov3D, dL_dshs NULL": (1, "cgs_raster_backward_ex: NULL input"),
        "SH + cov3D, dL_dcov3D NULL": (1, "cgs_raster_backward_ex: NULL input"),
        "SH + cov3D, dL_dmeans3D NULL": (1, "cgs_raster_backward_ex: NULL input"),
        "SH + cov3D, dL_dmeans2D NULL": (1, "cgs_raster_backward_ex: NULL input"),
        "dL_dmeans3D NULL": (1, "cgs_raster_backward: NULL input"),
        "dL_dmeans2D NULL": (1, "cgs_raster_backward: NULL input"),
        "dL_dcolors NULL": (1, "cgs_raster_backward: NULL input"),
        "dL_dopacities NULL": (1, "cgs_raster_backward: NULL input"),
        "dL_dscales NULL": (1, "cgs_raster_backward: NULL input"),
        "dL_drotations NULL": (1, "cgs_raster_backward: NULL input"),
        "dL_dout NULL": (1, "cgs_raster_backward: NULL input"),
        "geom_ws NULL": (3, "cgs_raster_backward: workspace too small"),      # was unprefixed
        "img_ws NULL": (3, "cgs_raster_backward: workspace too small"),      # was unprefixed
        "scratch NULL": (1, "cgs_raster_backward: NULL input"),
        "bin_ws NULL with R = 1": (3, "cgs_raster_backward: workspace too small"),      # was enqueued
        "scratch one byte short": (3, "cgs_raster_backward: scratch too small: 511 < 512"),      # was unprefixed
    },
    "cgs_raster_backward_aux": {
        "cfg NULL": (1, "cfg is NULL"),
        "image height 0": (1, "bad image size 16x0"),
        "P = -1": (1, "cgs_raster_backward_aux: P < 0 or R < 0"),
        "R = -1": (1, "cgs_raster_backward_aux: P < 0 or R < 0"),
        "P = 0, every pointer NULL": (0, ""),
        "colours and SH": (1, "cgs_raster_backward_aux: please provide exactly one of either SHs or precomputed colors"),
        "neither colours nor SH": (1, "cgs_raster_backward_aux: please provide exactly one of either SHs or precomputed colors"),
        "scales / rotations and cov3D": (1, "cgs_raster_backward_aux: please provide exactly one of either scale/rotation pair or precomputed 3D covariance"),
        "neither scales / rotations nor cov3D": (1, "cgs_raster_backward_aux: please provide exactly one of either scale/rotation pair or precomputed 3D covariance"),
        "SH + cov3D, dL_dshs NULL": (1, "cgs_raster_backward_aux: NULL input"),
        "SH + cov3D, dL_dcov3D NULL": (1, "cgs_raster_backward_aux: NULL input"),
        "SH + cov3D, dL_dmeans3D NULL": (1, "cgs_raster_backward_aux: NULL input"),
        "SH + cov3D, dL_dmeans2D NULL": (1, "cgs_raster_backward_aux: NULL input"),
        "dL_dmeans3D NULL": (1, "cgs_raster_backward_aux: NULL input"),
        "dL_dmeans2D NULL": (1, "cgs_raster_backward_aux: NULL input"),
        "dL_dcolors NULL": (1, "cgs_raster_backward_aux: NULL input"),
        "dL_dopacities NULL": (1, "cgs_raster_backward_aux: NULL input"),
        "dL_dscales NULL": (1, "cgs_raster_backward_aux: NULL input"),
        "dL_drotations NULL": (1, "cgs_raster_backward_aux: NULL input"),
        "dL_dout NULL": (3, "cgs_raster_backward_aux: scratch too small: 767 < 768"),
        "geom_ws NULL": (1, "cgs_raster_backward_aux: NULL input"),
        "img_ws NULL": (1, "cgs_raster_backward_aux: NULL input"),
        "scratch NULL": (1, "cgs_raster_backward_aux: NULL input"),
        "bin_ws NULL with R = 1": (1, "cgs_raster_backward_aux: NULL input"),
        "scratch one byte short": (3, "cgs_raster_backward_aux: scratch too small: 767 < 768"),
        "scratch of the next smaller layout": (3, "cgs_raster_backward_aux: scratch too small: 20224 < 24320"),
    },
    "cgs_raster_backward_opt": {
        "cfg NULL": (1, "cfg is NULL"),
        "image height 0": (1, "bad image size 16x0"),
        "P = -1": (1, "cgs_raster_backward_opt: P < 0 or R < 0"),
        "R = -1": (1, "cgs_raster_backward_opt: P < 0 or R < 0"),
        "P = 0, every pointer NULL": (0, ""),
        "colours and SH": (1, "cgs_raster_backward_opt: please provide exactly one of either SHs or precomputed colors"),
        "neither colours nor SH": (1, "cgs_raster_backward_opt: please provide exactly one of either SHs or precomputed colors"),
        "scales / rotations and cov3D": (1, "cgs_raster_backward_opt: please provide exactly one of either scale/rotation pair or precomputed 3D covariance"),
        "neither scales / rotations nor cov3D": (1, "cgs_raster_backward_opt: please provide exactly one of either scale/rotation pair or precomputed 3D covariance"),
        "SH + cov3D, dL_dshs NULL": (1, "cgs_raster_backward_opt: NULL input"),
        "SH + cov3D, dL_dcov3D NULL": (1, "cgs_raster_backward_opt: NULL input"),
        "SH + cov3D, dL_dmeans3D NULL": (1, "cgs_raster_backward_opt: NULL input"),
        "SH + cov3D, dL_dmeans2D NULL": (1, "cgs_raster_backward_opt: NULL input"),
        "dL_dmeans3D NULL": (1, "cgs_raster_backward_opt: NULL input"),
        "dL_dmeans2D NULL": (1, "cgs_raster_backward_opt: NULL input"),
        "dL_dcolors NULL": (1, "cgs_raster_backward_opt: NULL input"),
        "dL_dopacities NULL": (1, "cgs_raster_backward_opt: NULL input"),
        "dL_dscales NULL": (1, "cgs_raster_backward_opt: NULL input"),
        "dL_drotations NULL": (1, "cgs_raster_backward_opt: NULL input"),
        "dL_dout NULL": (3, "cgs_raster_backward_opt: scratch too small: 767 < 768"),
        "geom_ws NULL": (1, "cgs_raster_backward_opt: NULL input"),
        "img_ws NULL": (1, "cgs_raster_backward_opt: NULL input"),
        "scratch NULL": (1, "cgs_raster_backward_opt: NULL input"),
        "bin_ws NULL with R = 1": (1, "cgs_raster_backward_opt: NULL input"),
        "scratch one byte short": (3, "cgs_raster_backward_opt: scratch too small: 767 < 768"),
        "scratch of the next smaller layout": (3, "cgs_raster_backward_opt: scratch too small: 20224 < 24320"),
        "unknown opts bit": (1, "cgs_raster_backward_opt: unknown option bits 0x4 (known: CGS_RASTER_ANTIALIAS = 0x1)"),
        "CGS_RASTER_ANTIALIAS without opacities": (1, "cgs_raster_backward_opt: NULL input"),
    },
    "cgs_raster_backward_feat": {
        "cfg NULL": (1, "cfg is NULL"),
        "image height 0": (1, "bad image size 16x0"),
        "P = -1": (1, "cgs_raster_backward_feat: P < 0 or R < 0"),
        "R = -1": (1, "cgs_raster_backward_feat: P < 0 or R < 0"),
        "P = 0, every pointer NULL": (0, ""),
        "colours and SH": (1, "cgs_raster_backward_feat: please provide exactly one of either SHs or precomputed colors"),
        "neither colours nor SH": (1, "cgs_raster_backward_feat: please provide exactly one of either SHs or precomputed colors"),
        "scales / rotations and cov3D": (1, "cgs_raster_backward_feat: please provide exactly one of either scale/rotation pair or precomputed 3D covariance"),
        "neither scales / rotations nor cov3D": (1, "cgs_raster_backward_feat: please provide exactly one of either scale/rotation pair or precomputed 3D covariance"),
        "SH + cov3D, dL_dshs NULL": (1, "cgs_raster_backward_feat: NULL input"),
        "SH + cov3D, dL_dcov3D NULL": (1, "cgs_raster_backward_feat: NULL input"),
        "SH + cov3D, dL_dmeans3D NULL": (1, "cgs_raster_backward_feat: NULL input"),
        "SH + cov3D, dL_dmeans2D NULL": (1, "cgs_raster_backward_feat: NULL input"),
        "dL_dmeans3D NULL": (1, "cgs_raster_backward_feat: NULL input"),
        "dL_dmeans2D NULL": (1, "cgs_raster_backward_feat: NULL input"),
        "dL_dcolors NULL": (1, "cgs_raster_backward_feat: NULL input"),
        "dL_dopacities NULL": (1, "cgs_raster_backward_feat: NULL input"),
        "dL_dscales NULL": (1, "cgs_raster_backward_feat: NULL input"),
        "dL_drotations NULL": (1, "cgs_raster_backward_feat: NULL input"),
        "dL_dout NULL": (3, "cgs_raster_backward_feat: scratch too small: 767 < 768"),
        "geom_ws NULL": (1, "cgs_raster_backward_feat: NULL input"),
        "img_ws NULL": (1, "cgs_raster_backward_feat: NULL input"),
        "scratch NULL": (1, "cgs_raster_backward_feat: NULL input"),
        "bin_ws NULL with R = 1": (1, "cgs_raster_backward_feat: NULL input"),
        "scratch one byte short": (3, "cgs_raster_backward_feat: scratch too small: 767 < 768"),
        "scratch of the next smaller layout": (3, "cgs_raster_backward_feat: scratch too small: 20224 < 24320"),
        "unknown opts bit": (1, "cgs_raster_backward_feat: unknown option bits 0x4 (known: CGS_RASTER_ANTIALIAS = 0x1)"),
        "CGS_RASTER_ANTIALIAS without opacities": (1, "cgs_raster_backward_feat: NULL input"),
        "features without dL_dfeatures": (1, "cgs_raster_backward_feat: features and dL_dfeatures go together (one of them is NULL)"),
        "dL_dfeatures without features": (1, "cgs_raster_backward_feat: features and dL_dfeatures go together (one of them is NULL)"),
        "C = 0": (1, "cgs_raster_backward_feat: 0 feature channels outside 1..32"),
        "C = 33": (1, "cgs_raster_backward_feat: 33 feature channels outside 1..32"),
    },
    "cgs_raster_backward_abs": {
        "cfg NULL": (1, "cfg is NULL"),
        "image height 0": (1, "bad image size 16x0"),
        "P = -1": (1, "cgs_raster_backward_abs: P < 0 or R < 0"),
        "R = -1": (1, "cgs_raster_backward_abs: P < 0 or R < 0"),
        "P = 0, every pointer NULL": (0, ""),
        "colours and SH": (1, "cgs_raster_backward_abs: please provide exactly one of either SHs or precomputed colors"),
        "neither colours nor SH": (1, "cgs_raster_backward_abs: please provide exactly one of either SHs or precomputed colors"),
        "scales / rotations and cov3D": (1, "cgs_raster_backward_abs: please provide exactly one of either scale/rotation pair or precomputed 3D covariance"),
        "neither scales / rotations nor cov3D": (1, "cgs_raster_backward_abs: please provide exactly one of either scale/rotation pair or precomputed 3D covariance"),
        "SH + cov3D, dL_dshs NULL": (1, "cgs_raster_backward_abs: NULL input"),
        "SH + cov3D, dL_dcov3D NULL": (1, "cgs_raster_backward_abs: NULL input"),
        "SH + cov3D, dL_dmeans3D NULL": (1, "cgs_raster_backward_abs: NULL input"),
        "SH + cov3D, dL_dmeans2D NULL": (1, "cgs_raster_backward_abs: NULL input"),
        "dL_dmeans3D NULL": (1, "cgs_raster_backward_abs: NULL input"),
        "dL_dmeans2D NULL": (1, "cgs_raster_backward_abs: NULL input"),
        "dL_dcolors NULL": (1, "cgs_raster_backward_abs: NULL input"),
        "dL_dopacities NULL": (1, "cgs_raster_backward_abs: NULL input"),
        "dL_dscales NULL": (1, "cgs_raster_backward_abs: NULL input"),
        "dL_drotations NULL": (1, "cgs_raster_backward_abs: NULL input"),
        "dL_dout NULL": (3, "cgs_raster_backward_abs: scratch too small: 1023 < 1024"),
        "geom_ws NULL": (1, "cgs_raster_backward_abs: NULL input"),
        "img_ws NULL": (1, "cgs_raster_backward_abs: NULL input"),
        "scratch NULL": (1, "cgs_raster_backward_abs: NULL input"),
        "bin_ws NULL with R = 1": (1, "cgs_raster_backward_abs: NULL input"),
        "scratch one byte short": (3, "cgs_raster_backward_abs: scratch too small: 1023 < 1024"),
        "scratch of the next smaller layout": (3, "cgs_raster_backward_abs: scratch too small: 24320 < 32512"),
        "unknown opts bit": (1, "cgs_raster_backward_abs: unknown option bits 0x4 (known: CGS_RASTER_ANTIALIAS = 0x1)"),
        "CGS_RASTER_ANTIALIAS without opacities": (1, "cgs_raster_backward_abs: NULL input"),
        "features without dL_dfeatures": (1, "cgs_raster_backward_abs: features and dL_dfeatures go together (one of them is NULL)"),
        "dL_dfeatures without features": (1, "cgs_raster_backward_abs: features and dL_dfeatures go together (one of them is NULL)"),
        "C = 0": (1, "cgs_raster_backward_abs: 0 feature channels outside 1..32"),
        "C = 33": (1, "cgs_raster_backward_abs: 33 feature channels outside 1..32"),
    },
    "cgs_raster_backward_det": {
        "cfg NULL": (1, "cfg is NULL"),
        "image height 0": (1, "bad image size 16x0"),
        "P = -1": (1, "cgs_raster_backward_det: P < 0 or R < 0"),
        "R = -1": (1, "cgs_raster_backward_det: P < 0 or R < 0"),
        "P = 0, every pointer NULL": (0, ""),
        "colours and SH": (1, "cgs_raster_backward_det: please provide exactly one of either SHs or precomputed colors"),
        "neither colours nor SH": (1, "cgs_raster_backward_det: please provide exactly one of either SHs or precomputed colors"),
        "scales / rotations and cov3D": (1, "cgs_raster_backward_det: please provide exactly one of either scale/rotation pair or precomputed 3D covariance"),
        "neither scales / rotations nor cov3D": (1, "cgs_raster_backward_det: please provide exactly one of either scale/rotation pair or precomputed 3D covariance"),
        "SH + cov3D, dL_dshs NULL": (1, "cgs_raster_backward_det: NULL input"),
        "SH + cov3D, dL_dcov3D NULL": (1, "cgs_raster_backward_det: NULL input"),
        "SH + cov3D, dL_dmeans3D NULL": (1, "cgs_raster_backward_det: NULL input"),
        "SH + cov3D, dL_dmeans2D NULL": (1, "cgs_raster_backward_det: NULL input"),
        "dL_dmeans3D NULL": (1, "cgs_raster_backward_det: NULL input"),
        "dL_dmeans2D NULL": (1, "cgs_raster_backward_det: NULL input"),
        "dL_dcolors NULL": (1, "cgs_raster_backward_det: NULL input"),
        "dL_dopacities NULL": (1, "cgs_raster_backward_det: NULL input"),
        "dL_dscales NULL": (1, "cgs_raster_backward_det: NULL input"),
        "dL_drotations NULL": (1, "cgs_raster_backward_det: NULL input"),
        "dL_dout NULL": (3, "cgs_raster_backward_det: scratch too small: 1023 < 1024"),
        "geom_ws NULL": (1, "cgs_raster_backward_det: NULL input"),
        "img_ws NULL": (1, "cgs_raster_backward_det: NULL input"),
        "scratch NULL": (1, "cgs_raster_backward_det: NULL input"),
        "bin_ws NULL with R = 1": (1, "cgs_raster_backward_det: NULL input"),
        "scratch one byte short": (3, "cgs_raster_backward_det: scratch too small: 1023 < 1024"),
        "scratch of the next smaller layout": (3, "cgs_raster_backward_det: scratch too small: 24320 < 32512"),
        "unknown opts bit": (1, "cgs_raster_backward_det: unknown option bits 0x4 (known: CGS_RASTER_ANTIALIAS = 0x1)"),
        "CGS_RASTER_ANTIALIAS without opacities": (1, "cgs_raster_backward_det: NULL input"),
        "dL_ddepth given": (1, "cgs_raster_backward_det: dL_ddepth, dL_dinvdepth and dL_dalpha must be NULL (the map blends' backward sums with float atomics and is not covered by the deterministic mode)"),
        "dL_dinvdepth given": (1, "cgs_raster_backward_det: dL_ddepth, dL_dinvdepth and dL_dalpha must be NULL (the map blends' backward sums with float atomics and is not covered by the deterministic mode)"),
        "dL_dalpha given": (1, "cgs_raster_backward_det: dL_ddepth, dL_dinvdepth and dL_dalpha must be NULL (the map blends' backward sums with float atomics and is not covered by the deterministic mode)"),
        "means2D_cols = 2": (1, "cgs_raster_backward_det: means2D_cols = 2, must be 3 or 4"),
        "det_ws NULL": (1, "cgs_raster_backward_det: NULL input"),
        "det_ws one byte short": (3, "cgs_raster_backward_det: det_ws too small: 767 < 768"),
    },
}


CASES = [(e, n) for e in ENTRIES for n in _faults(e)]


def test_the_table_names_every_fault_of_every_entry_point():
    assert {(e, n) for e in EXPECTED for n in EXPECTED[e]} == set(CASES)
    assert len(ENTRIES) == 7 and all(EXPECTED[e]["P = 0, every pointer NULL"] == (CGS_OK, "") for e in ENTRIES)
    assert all(rc in (CGS_ERR_ARG, CGS_ERR_WORKSPACE) for e in EXPECTED for n, (rc, _) in EXPECTED[e].items() if not n.startswith("P = 0"))


@pytest.mark.parametrize("entry,fault", CASES, ids=[f"{e[11:]}-{n}" for e, n in CASES])
def test_backward_argument_checks(entry, fault):
    rc, msg = _call(entry, _faults(entry)[fault])
    want = EXPECTED[entry][fault]
    assert (rc, msg if rc else "") == want, (entry, fault)
