"""Per-view exposure for the training image loss (contextgs_amd/loss_utils.py).

Upstream 3DGS answers auto-exposure and white-balance drift between the training images with one 3x4 affine colour transform
per image, applied to the render before the loss: with E = `exposure[i]`,

  image'_c = sum_k image_k E[k, c] + E[c, 3]       (= matmul(image.permute(1, 2, 0), E[:3, :3]).permute(2, 0, 1) + E[:3, 3, None, None])

`ViewExposure(n_views)` holds the [n_views, 3, 4] parameter, initialised to [I | 0] (no change).  In training the row goes into the
fused loss, which applies it where it loads the image and returns the row's gradient through autograd:

  exposures = ViewExposure(len(train_cameras)).cuda()
  optimizer = torch.optim.Adam(exposures.parameters(), lr=1e-3)        # its own optimizer, or one more group of the scene's
  loss, l1, ssim = training_image_loss(image, gt, 0.2, exposure=exposures(cam.uid))
  loss.backward(); optimizer.step()

Only the row that was used receives a gradient; the others see zeros (a dense [n_views, 3, 4] gradient: 48 bytes per view).
For evaluation, `apply(image, i)` is the same transform in plain torch.  Learning-rate schedules are the caller's.
"""
from __future__ import annotations

import torch
import torch.nn as nn


class ViewExposure(nn.Module):
    """See the module docstring.  `exposure` [n_views, 3, 4] is the only parameter."""

    def __init__(self, n_views: int, dtype=torch.float32, device=None):
        super().__init__()
        if n_views < 1:
            raise ValueError("ViewExposure needs at least one view")
        self.exposure = nn.Parameter(torch.eye(3, 4, dtype=dtype, device=device).repeat(n_views, 1, 1))

    def forward(self, i: int) -> torch.Tensor:
        """The [3,4] row of view i, through autograd: what `training_image_loss(..., exposure=)` takes."""
        return self.exposure[i]

    def apply(self, image, i=None):
        """image' of a [3,H,W] image for view i (the module docstring's formula), in plain torch.  (`apply(fn)` stays
        nn.Module's own: a parent module's `apply(init_fn)` reaches its children through this name.)"""
        if i is None and callable(image) and not isinstance(image, torch.Tensor):
            return super().apply(image)
        E = self.exposure[i].to(image.dtype)
        return torch.matmul(image.permute(1, 2, 0), E[:, :3]).permute(2, 0, 1) + E[:, 3, None, None]
