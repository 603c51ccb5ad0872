"""What the drop-in rasterizer asks of libcgs_hip.so, call by call: the cases, the recording proxy and the writer of
tests/golden/raster_calls.json, which tests/test_raster_calls_gpu.py compares the tree under test with.

    python tools/raster_call_record.py OUT.json       (on the MI355X, at the commit whose behaviour is to be kept)

The fixture is recorded at the PARENT of a change that must keep the host side as it is, never from the changed tree.  Only the
public surface is used (GaussianRasterizer, GaussianRasterizationSettings, GaussianContrib, rasterizer._pair_capacity and
_lib.lib / _lib.SIGNATURES), so the same file runs on both sides of such a change.

A recorded call is [entry point, argument, ...].  An argument whose type in _lib.SIGNATURES is an integer is noted by value (P,
R, D, M, opts, C, means2D_cols, every byte size), a pointer as "ptr" or "null" (which gradients and which optional inputs are
NULL), a float by value.  The one exception is the first argument of the *_wait entry points: the ticket of a *_launch / *_wait
pair, a process-wide counter that depends on what ran before, noted as "ticket".
"""
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_INTS = (C.c_int, C.c_int32, C.c_int64, C.c_size_t, C.c_uint32)
_FLOATS = (C.c_float, C.c_double)


def _note(argtype, value):
    value = getattr(value, "value", value)
    if argtype in _INTS:
        return int(value)
    if argtype in _FLOATS:
        return float(value)
    return "null" if value is None or (isinstance(value, int) and value == 0) else "ptr"


class CallRecorder:
    """Stands in for the library handle (`_lib.lib = lambda: CallRecorder(handle, calls)`): every call made through it is
    appended to `calls` and handed on unchanged."""

    def __init__(self, handle, calls):
        self._handle, self._calls = handle, calls

    def __getattr__(self, name):
        from contextgs_amd import _lib
        fn, argtypes = getattr(self._handle, name), _lib.SIGNATURES[name][1]

        def call(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            noted = [_note(t, a) for t, a in zip(argtypes, args)]
            if name.endswith(("_wait", "_wait2")):
                noted[0] = "ticket"
            self._calls.append([name] + noted)
            return fn(*args)
        return call


# ---- the scenes ----------------------------------------------------------------------------------------------------------------
W, H = 80, 64       # 5 x 4 tiles, the right edge ragged
SCENES = ("visible", "behind", "none")      # 64 Gaussians in view; all of them behind the camera (R = 0); P = 0


def scene(name):
    from contextgs_amd.synth import look_at_camera, random_gaussians
    cam = look_at_camera((0.0, -3.0, 0.0), (0, 0, 0), W, H, fovx_deg=50.0)
    g = random_gaussians(64, seed=6)
    rng = np.random.default_rng(6)
    g["shs"] = rng.normal(scale=0.3, size=(64, 4, 3)).astype(np.float32)
    g["features"] = rng.normal(size=(64, 2)).astype(np.float32)
    if name == "behind":
        g["means3D"][:, 1] -= 20.0
    if name == "none":
        g = {k: v[:0] for k, v in g.items()}
    return cam, g


def _cov6(scales, rotations):
    """Upper triangle of R S S^T R^T (quaternion w, x, y, z, normalised)."""
    q = rotations / np.maximum(np.linalg.norm(rotations, axis=1, keepdims=True), 1e-12)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    M = R * scales[:, None, :]
    S = M @ M.transpose(0, 2, 1)
    return np.ascontiguousarray(S[:, (0, 0, 0, 1, 1, 2), (0, 1, 2, 1, 2, 2)].astype(np.float32))


# ---- the cases -----------------------------------------------------------------------------------------------------------------
# name -> (keywords of GaussianRasterizer.forward, options of the call); "loss": which outputs the loss reads (default: every
# differentiable one)
_COMBINED = dict(return_aux=True, features=True, contrib="slots", absgrad=True, return_geometry=True, return_normals=True)
CASES = {
    "plain": ({}, {}),
    "return_aux": (dict(return_aux=True), {}),
    "features": (dict(features=True), {}),
    "contrib": (dict(contrib=True), {}),
    "contrib_slots": (dict(contrib="slots"), {}),
    "absgrad": (dict(absgrad=True), {}),
    "deterministic": (dict(deterministic=True), {}),
    "return_geometry": (dict(return_geometry=True), {}),
    "return_normals": (dict(return_normals=True), {}),
    "antialiasing": ({}, dict(antialiasing=True)),
    "shs_cov": ({}, dict(shs=True, cov=True)),
    "combined": (_COMBINED, dict(antialiasing=True, shs=True)),
    "combined_distortion_only": (_COMBINED, dict(antialiasing=True, shs=True, loss=("distortion",))),
    "combined_features_only": (_COMBINED, dict(antialiasing=True, shs=True, loss=("features",))),
    "viewmatrix_grad": ({}, dict(camera_grad=("viewmatrix",))),
    "camera_grad": (dict(return_aux=True), dict(shs=True, camera_grad=("viewmatrix", "projmatrix", "campos"))),
}
_NON_DIFFERENTIABLE = ("radii", "top_id", "top_weight", "count", "median_id", "contrib")


def build_call(case, scene_name):
    """(the GaussianRasterizer, its keywords on fresh leaves, the outputs the loss reads or None for every differentiable one)"""
    import torch
    from contextgs_amd.rasterizer import GaussianContrib, GaussianRasterizationSettings, GaussianRasterizer
    kw, opt = CASES[case]
    cam, g = scene(scene_name)
    P = g["means3D"].shape[0]
    leaf = lambda a: torch.tensor(a, device="cuda", requires_grad=True)
    c = cam.to_torch("cuda")
    camera = dict(viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform, campos=c.camera_center)
    for k in opt.get("camera_grad", ()):
        camera[k].requires_grad_(True)
    rs = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
        bg=torch.tensor((0.1, 0.25, 0.4), dtype=torch.float32, device="cuda"), scale_modifier=1.0, sh_degree=1,
        prefiltered=False, debug=False, antialiasing=bool(opt.get("antialiasing")), **camera)
    kw = dict(kw)
    if kw.get("features"):
        kw["features"] = leaf(g["features"])
    if kw.get("contrib") == "slots":      # three rows shared by all Gaussians
        kw["contrib"] = GaussianContrib.zeros(3, "cuda")
        kw["contrib_slots"] = (torch.arange(P, dtype=torch.int32, device="cuda") % 3).contiguous()
    if opt.get("shs"):
        kw["shs"] = leaf(g["shs"])
    else:
        kw["colors_precomp"] = leaf(g["colors"])
    if opt.get("cov"):
        kw["cov3D_precomp"] = leaf(_cov6(g["scales"], g["rotations"]))
    else:
        kw["scales"], kw["rotations"] = leaf(g["scales"]), leaf(g["rotations"])
    kw.update(means3D=leaf(g["means3D"]), opacities=leaf(g["opacities"]),
              means2D=torch.zeros(P, 4 if kw.get("absgrad") else 3, device="cuda", requires_grad=True))
    return GaussianRasterizer(rs), kw, opt.get("loss")


def run_call(rasterizer, kw, loss=None, sync=True):
    """One forward + backward.  Returns the outputs by name (color, radii and the extras but the GaussianContrib)."""
    import torch
    res = rasterizer(**kw)
    out = {"color": res[0], "radii": res[1], **(res[2] if len(res) > 2 else {})}
    read = loss or [k for k in out if k not in _NON_DIFFERENTIABLE]
    sum((out[k] * (0.5 + 0.25 * i)).sum() for i, k in enumerate(read)).backward()
    if sync:
        torch.cuda.synchronize()
    return {k: v.detach() for k, v in out.items() if k != "contrib"}


def record(case, scene_name):
    """(the calls of two runs in a row from an empty pair capacity: the first takes bin_and_blend's non-speculative path, the
    second the speculative one; the outputs of the two runs)"""
    from contextgs_amd import _lib, rasterizer
    rasterizer._pair_capacity.clear()
    calls, real = [], _lib.lib
    handle = real()
    _lib.lib = lambda: CallRecorder(handle, calls)
    try:
        outs = [run_call(*build_call(case, scene_name)) for _ in range(2)]
    finally:
        _lib.lib = real
    return calls, outs


def key(case, scene_name):
    return f"{case}/{scene_name}"


def dump(path, library, calls):
    """JSON with one recorded call per line, so that a difference reads as a line."""
    one = lambda c: "   " + json.dumps(c, separators=(",", ":"))
    body = ",\n".join(f"  {json.dumps(k)}: [\n" + ",\n".join(map(one, v)) + "\n  ]" for k, v in calls.items())
    with open(path, "w") as f:
        f.write(f'{{\n "generator": "tools/raster_call_record.py (MI355X, gfx950)",\n "library": {json.dumps(library)},\n'
                f' "calls": {{\n{body}\n }}\n}}\n')


def main():
    from contextgs_amd import _lib
    calls = {key(case, s): record(case, s)[0] for case in CASES for s in SCENES}
    dump(sys.argv[1], (_lib.lib().cgs_build_info() or b"").decode(), calls)
    print(sys.argv[1], {k: len(v) for k, v in calls.items()})


if __name__ == "__main__":
    main()
