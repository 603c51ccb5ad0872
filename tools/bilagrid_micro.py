"""Cost of the per-view bilateral grid (csrc/bilagrid.hip, contextgs_amd/bilagrid.py) at 3x1080x1920 with the default grid
(12 x 8 x 16 x 16), alternating in one run, device events after a warm-up; forward and backward timed apart:
  the fused slice                       bilagrid_slice(grid, image) with d grid only, d image only, both
  the same maths composed in torch      a 5-D grid_sample (bilinear, align_corners, border padding) and the affine apply, autograd
  the TV term at N = 200 views          BilateralGrid.tv_loss() and torch.diff / pow / mean per axis
next to the bytes each call must move (fp32) and the share of HBM bandwidth (6.29 TB/s) that makes:
  forward            image read, out written (12 + 12 B per pixel); the 98 KB grid is noise
  backward, d image  image and dout read, d image written (36 B per pixel)
  backward, d grid   image and dout read once (24 B per pixel) — the kernel reads them once per z node of the cell (L times,
                     from the caches): what bounds that pass is said in DESIGN.md
  TV                 the grids read once forward; read and written backward
The comparison partner of a fused call is the torch composition of the same run, never an earlier number.
Usage: python tools/bilagrid_micro.py [iters] -> stdout (kept in profiles/bilagrid.txt).  GPU box."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from contextgs_amd.bilagrid import BilateralGrid, bilagrid_slice, bilagrid_tv

ITERS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
H, W = 1080, 1920
L, GH, GW = 8, 16, 16
N_TV = 200
HBM = 6.29e12
dev = "cuda"
gen = torch.Generator(device=dev).manual_seed(0)
image = (torch.rand(3, H, W, device=dev, generator=gen) * 1.2 - 0.1)
dout = torch.randn(3, H, W, device=dev, generator=gen)
grid = (torch.eye(3, 4, device=dev).reshape(12, 1, 1, 1) + 0.1 * torch.randn(12, L, GH, GW, device=dev, generator=gen)).contiguous()
grids = (torch.eye(3, 4, device=dev).reshape(1, 12, 1, 1, 1) + 0.1 * torch.randn(N_TV, 12, L, GH, GW, device=dev, generator=gen)).contiguous()
GX = ((torch.arange(W, device=dev) + 0.5) / W * 2 - 1)[None, :].expand(H, W)
GY = ((torch.arange(H, device=dev) + 0.5) / H * 2 - 1)[:, None].expand(H, W)


def torch_slice(g, x):
    z = 0.299 * x[0] + 0.587 * x[1] + 0.114 * x[2]
    coords = torch.stack([GX, GY, z * 2 - 1], dim=-1)[None, None]
    A = F.grid_sample(g[None], coords, mode="bilinear", align_corners=True, padding_mode="border")[0, :, 0].reshape(3, 4, H, W)
    return (A[:, :3] * x[None]).sum(dim=1) + A[:, 3]


def torch_tv(g):
    return sum(torch.diff(g, dim=a).pow(2).mean(dim=(1, 2, 3, 4)).sum() for a in (2, 3, 4)) / g.shape[0]


PIX = H * W * 4 * 3                                  # one [3,H,W] array in bytes
GRIDS = grids.numel() * 4


def slice_variant(fn, need_g, need_x):
    def make():
        g, x = grid.detach().requires_grad_(need_g), image.detach().requires_grad_(need_x)
        return fn(g, x), dout
    return make


def tv_variant(fn):
    def make():
        return fn(grids.detach().requires_grad_()), None
    return make


# (name, make() -> (output, upstream gradient), bytes forward, bytes backward)
VARIANTS = []
for label, ng, nx, bb in (("d grid", True, False, 2 * PIX), ("d image", False, True, 3 * PIX), ("both", True, True, 3 * PIX)):
    VARIANTS.append((f"fused slice, {label}", slice_variant(bilagrid_slice, ng, nx), 2 * PIX, bb))
    VARIANTS.append((f"torch slice, {label}", slice_variant(torch_slice, ng, nx), None, None))
VARIANTS.append((f"fused TV, N = {N_TV}", tv_variant(bilagrid_tv), GRIDS, 2 * GRIDS))
VARIANTS.append((f"torch TV, N = {N_TV}", tv_variant(torch_tv), None, None))


def run(make, timed):
    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    a.record()
    out, up = make()
    b.record()
    if up is None:
        out.backward()
    else:
        out.backward(up)
    c.record()
    c.synchronize()
    if timed is not None:
        timed[0] += a.elapsed_time(b)
        timed[1] += b.elapsed_time(c)
    return out.detach()


for _, make, _, _ in VARIANTS:
    for _ in range(3):
        run(make, None)
torch.cuda.synchronize()
total = {name: [0.0, 0.0] for name, _, _, _ in VARIANTS}
for _ in range(ITERS):                              # alternating: every variant sees the same clocks
    for name, make, _, _ in VARIANTS:
        run(make, total[name])
print(f"# image 3x{H}x{W}, grid 12x{L}x{GH}x{GW}, TV over {N_TV} views, {ITERS} iterations, device events around the forward call and "
      "around .backward(), alternating")
makes = {name: make for name, make, _, _ in VARIANTS}
d = (run(makes["fused slice, both"], None) - run(makes["torch slice, both"], None)).abs().max().item()
print(f"# max |fused - torch| of the sliced image: {d:.2e}")
d = (run(makes[f"fused TV, N = {N_TV}"], None) - run(makes[f"torch TV, N = {N_TV}"], None)).abs().item()
print(f"# |fused - torch| of the TV term: {d:.2e}")
slower = []
for name, _, fb, bb in VARIANTS:
    for i, (what, nbytes) in enumerate((("forward ", fb), ("backward", bb))):
        us = total[name][i] / ITERS * 1e3
        tail = f"  must move {nbytes / 1e6:.1f} MB = {nbytes / (us * 1e-6) / HBM * 100:.1f} % of {HBM / 1e12:.2f} TB/s" if nbytes else ""
        print(f"{name}, {what}: {us:.1f} us{tail}")
        partner = name.replace("fused", "torch")
        if name.startswith("fused") and total[name][i] > total[partner][i]:
            slower.append(f"{name}, {what.strip()}")
print("# fused calls slower than their torch composition: " + (", ".join(slower) if slower else "none"))

# The rows above time a call as a training step sees it on an idle device: at these sizes mostly the host's path to the launch.
# The kernels alone: C-ABI calls queued back to back (QUEUE per event pair), so the device never waits for the host.
from contextgs_amd import _lib

QUEUE = 20
Lb, p, st = _lib.lib(), _lib.ptr, _lib.current_stream()
out, dimg, dgrid, dgrids = torch.empty_like(image), torch.empty_like(image), torch.empty_like(grid), torch.empty_like(grids)
sb = int(Lb.cgs_bilagrid_bwd_scratch_bytes(L, GH, GW, H, W))
scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
tv_out, tv_g = torch.empty(1, device=dev), torch.ones(1, device=dev)
tv_scratch = torch.empty(int(Lb.cgs_bilagrid_tv_scratch_bytes(N_TV, L, GH, GW)), dtype=torch.uint8, device=dev)
ABI = [
    ("cgs_bilagrid_slice_fwd", 2 * PIX,
     lambda: Lb.cgs_bilagrid_slice_fwd(p(grid), L, GH, GW, p(image), H, W, p(out), st)),
    ("cgs_bilagrid_slice_bwd, d image (1 launch)", 3 * PIX,
     lambda: Lb.cgs_bilagrid_slice_bwd(p(grid), L, GH, GW, p(image), p(dout), H, W, p(dimg), None, None, 0, st)),
    ("cgs_bilagrid_slice_bwd, d grid (2 launches)", 2 * PIX,
     lambda: Lb.cgs_bilagrid_slice_bwd(p(grid), L, GH, GW, p(image), p(dout), H, W, None, p(dgrid), p(scratch), sb, st)),
    ("cgs_bilagrid_slice_bwd, both (3 launches)", 3 * PIX,
     lambda: Lb.cgs_bilagrid_slice_bwd(p(grid), L, GH, GW, p(image), p(dout), H, W, p(dimg), p(dgrid), p(scratch), sb, st)),
    (f"cgs_bilagrid_tv_fwd, N = {N_TV} (2 launches)", GRIDS,
     lambda: Lb.cgs_bilagrid_tv_fwd(p(grids), N_TV, L, GH, GW, p(tv_out), p(tv_scratch), st)),
    (f"cgs_bilagrid_tv_bwd, N = {N_TV}", 2 * GRIDS,
     lambda: Lb.cgs_bilagrid_tv_bwd(p(grids), N_TV, L, GH, GW, p(tv_g), p(dgrids), st)),
]
abi_ms = {name: 0.0 for name, _, _ in ABI}
for rep in range(1 + ITERS // 5):                   # the first round warms up; the entries alternate
    for name, _, call in ABI:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(QUEUE):
            assert call() == 0
        b.record()
        b.synchronize()
        if rep:
            abi_ms[name] += a.elapsed_time(b)
print(f"# kernels alone: {QUEUE} C-ABI calls queued between two device events, {ITERS // 5} rounds, entries alternating; the scratch of d grid "
      f"is {sb / 1e6:.2f} MB")
for name, nbytes, _ in ABI:
    us = abi_ms[name] / (ITERS // 5) / QUEUE * 1e3
    print(f"{name}: {us:.1f} us  must move {nbytes / 1e6:.1f} MB = {nbytes / (us * 1e-6) / HBM * 100:.1f} % of {HBM / 1e12:.2f} TB/s")
