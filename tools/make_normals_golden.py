"""Golden vectors for the depth normals from the reference's own Python (utils/visualize_utils.py: depthImgToPosCam_Batched and
computeNormalsFromPosCam_Batched), run on the CPU.  Writes tests/golden/depth_normals.npz: three 24x40 float32 depth maps (a
smooth one with a zero hole in rows 5-8, columns 10-19, a rough one, a constant one: tests/normals_ref.py depth_case), tanfovx,
tanfovy, and the reference's [3,24,40] output for each, with the focal length and principal point of INTEGRATION.md's recipe.

The reference module imports cv2 for its drawing helpers, which the two functions never touch: an empty stand-in module is
registered before the import when cv2 is not installed.  Nothing of the reference is copied.
Usage: python tools/make_normals_golden.py <reference checkout>"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import normals_ref  # noqa: E402

try:
    import cv2  # noqa: F401
except ImportError:
    sys.modules["cv2"] = types.ModuleType("cv2")
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = os.path.join(sys.argv[1], "utils", "visualize_utils.py")
spec = importlib.util.spec_from_file_location("ref_visualize_utils", REF)
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

H, W = 24, 40
tanfovx, tanfovy = normals_ref.TAN
fx, fy = W / (2 * tanfovx), H / (2 * tanfovy)
focal = torch.tensor([[[fx, 0.0], [0.0, fy]]])
princpt = torch.tensor([[W / 2, H / 2]])
uv = torch.stack(torch.meshgrid(torch.arange(W), torch.arange(H), indexing="xy"), dim=0)[None].float()
out = {"tanfovx": np.float64(tanfovx), "tanfovy": np.float64(tanfovy)}
for kind in ("smooth", "rough", "constant"):
    depth = normals_ref.depth_case(kind, H, W)
    pos = ref.depthImgToPosCam_Batched(torch.from_numpy(depth)[None], uv, focal, princpt)
    out[kind + "_depth"] = depth
    out[kind + "_normals"] = ref.computeNormalsFromPosCam_Batched(pos)[0].numpy()
path = os.path.join(ROOT, "tests", "golden", "depth_normals.npz")
np.savez_compressed(path, **out)
print(path, {k: getattr(v, "shape", v) for k, v in out.items()})
