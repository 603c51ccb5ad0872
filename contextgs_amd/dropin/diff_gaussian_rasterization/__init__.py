"""Shim with the import name the reference uses (gaussian_renderer/__init__.py:20)."""
from contextgs_amd.rasterizer import (GaussianContrib, GaussianRasterizationSettings, GaussianRasterizer,  # noqa: F401
                                     rasterize_gaussians)
