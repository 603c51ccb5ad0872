"""The signatures of the seven cgs_raster_backward* entry points (include/cgs.h), as data: the argument checks of
tests/test_raster_backward_checks.py and the C-ABI runs of tests/test_raster_backward_entry_points_gpu.py both read it."""
COMMON = ["cfg", "P", "R", "means3D", "colors", "shs", "sh_degree", "sh_coeffs", "opacities", "scales", "rotations", "cov3D",
          "radii", "geom_ws", "geom_bytes", "bin_ws", "bin_bytes", "img_ws", "img_bytes", "dL_dout"]
MAPS = ["dL_ddepth", "dL_dinvdepth", "dL_dalpha"]
GRADS = ["dL_dmeans3D", "dL_dmeans2D", "dL_dcolors", "dL_dopacities", "dL_dshs", "dL_dscales", "dL_drotations", "dL_dcov3D"]
TAIL = ["scratch", "scratch_bytes", "stream"]
FEAT = ["features", "C", "dL_dfeatures_map", "dL_dfeatures"]
NO_FORMS = ("shs", "sh_degree", "sh_coeffs", "cov3D", "dL_dshs", "dL_dcov3D")
ENTRIES = {     # name -> (argument names in order, the size query of its scratch, the query of the next smaller layout)
    "cgs_raster_backward": ([a for a in COMMON + GRADS + TAIL if a not in NO_FORMS], "cgs_raster_bwd_scratch_bytes", None),
    "cgs_raster_backward_ex": (COMMON + GRADS + TAIL, "cgs_raster_bwd_scratch_bytes", None),
    "cgs_raster_backward_aux": (COMMON + MAPS + GRADS + TAIL, "cgs_raster_bwd_aux_scratch_bytes", "cgs_raster_bwd_scratch_bytes"),
    "cgs_raster_backward_opt": (COMMON + MAPS + GRADS + TAIL + ["opts"], "cgs_raster_bwd_aux_scratch_bytes",
                                "cgs_raster_bwd_scratch_bytes"),
    "cgs_raster_backward_feat": (COMMON + MAPS + GRADS + TAIL + ["opts"] + FEAT, "cgs_raster_bwd_aux_scratch_bytes",
                                 "cgs_raster_bwd_scratch_bytes"),
    "cgs_raster_backward_abs": (COMMON + MAPS + GRADS + TAIL + ["opts"] + FEAT, "cgs_raster_bwd_abs_scratch_bytes",
                                "cgs_raster_bwd_aux_scratch_bytes"),
    "cgs_raster_backward_det": (COMMON + MAPS + GRADS + TAIL + ["opts", "means2D_cols", "det_ws", "det_bytes"],
                                "cgs_raster_bwd_abs_scratch_bytes", "cgs_raster_bwd_aux_scratch_bytes"),
}
