"""Cost of the training image loss with a per-pixel weight and / or a per-view exposure (csrc/loss.hip, `l1_ssim_w_*`) at
3x1080x1920, alternating in one run, device events after a warm-up; forward and backward timed apart:
  the plain node                              training_image_loss(x, gt)
  the node with weight / exposure / both      one node, the keywords
  the same maths composed in torch            exposure: the permute / matmul / permute / add chain in front of the plain node;
                                              weight (and both): SSIM from five grouped conv2d with the map weighted
next to the bytes each variant must move (fp32: reads of x, gt, w and E, the three maps written and read back, the gradient
written) and the share of HBM bandwidth (6.29 TB/s) that makes.  What the kernels request beyond that: with an exposure the
forward's patch reads all three channels for each channel's tile (16 + 12 B per pixel and channel instead of 8 + 12), and the
weight is read once per channel.  The comparison partner of a fused variant is the torch composition of the same run, never an
earlier number.  The plain node is also timed on its own, back to back, before the alternation: that row means the same on a
build without the keywords (where the tool times nothing else), so it is the one to compare between two builds on one box;
between the other variants the plain node finds the caches as they leave them (~100 MB of inputs and maps otherwise stay in the
256 MB last-level cache from one call to the next).  Usage: python tools/loss_weighted_micro.py [iters] [--plain-only: what a build without the
keywords runs, for the comparison of two builds] -> stdout (kept in profiles/loss_weighted.txt).  GPU box."""
import inspect
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from contextgs_amd.loss_utils import training_image_loss

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
ITERS = int(ARGS[0]) if ARGS else 50
C, H, W = 3, 1080, 1920
HBM = 6.29e12
LAM = 0.2
dev = "cuda"
HAS_KEYWORDS = "weight" in inspect.signature(training_image_loss).parameters and "--plain-only" not in sys.argv
g = torch.Generator(device=dev).manual_seed(0)
gt = torch.rand(C, H, W, device=dev, generator=g)
x = (gt + 0.1 * torch.randn(C, H, W, device=dev, generator=g)).clamp(0, 1).requires_grad_()
w = torch.rand(H, W, device=dev, generator=g)
E = torch.tensor([[1.10, -0.07, 0.04, 0.03], [0.06, 0.92, -0.09, -0.02], [-0.05, 0.08, 1.05, 0.01]], device=dev).requires_grad_()
k1 = torch.exp(-(torch.arange(11, device=dev, dtype=torch.float32) - 5) ** 2 / (2 * 1.5 ** 2))
k1 = k1 / k1.sum()
WIN = (k1[:, None] * k1[None, :]).expand(C, 1, 11, 11).contiguous()


def expose(img):
    return torch.matmul(img.permute(1, 2, 0), E[:, :3]).permute(2, 0, 1) + E[:, 3, None, None]


def torch_weighted(img, weight):
    """(loss, L1, SSIM) with the SSIM map and |x - y| weighted: utils/loss_utils.py:43-63 of the reference plus the weight."""
    a, b = img[None], gt[None]
    mu1, mu2 = F.conv2d(a, WIN, padding=5, groups=C), F.conv2d(b, WIN, padding=5, groups=C)
    s1 = F.conv2d(a * a, WIN, padding=5, groups=C) - mu1 * mu1
    s2 = F.conv2d(b * b, WIN, padding=5, groups=C) - mu2 * mu2
    s12 = F.conv2d(a * b, WIN, padding=5, groups=C) - mu1 * mu2
    m = ((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    cs = C * weight.sum()
    l1, s = (weight * (img - gt).abs()).sum() / cs, (weight * m[0]).sum() / cs
    return (1 - LAM) * l1 + LAM * (1 - s), l1, s


PLANE = H * W * 4                                    # one channel, or the weight, in bytes
FWD, BWD = C * 5 * PLANE, C * 6 * PLANE              # x, gt read + three maps written (8 + 12 B); three maps, x, gt read + the gradient written (20 + 4 B)
VARIANTS = [("plain node", lambda: training_image_loss(x, gt, LAM), FWD, BWD)]
if HAS_KEYWORDS:
    VARIANTS += [
        ("node, weight", lambda: training_image_loss(x, gt, LAM, weight=w), FWD + PLANE, BWD + PLANE),
        ("node, exposure", lambda: training_image_loss(x, gt, LAM, exposure=E), FWD, BWD),
        ("node, weight + exposure", lambda: training_image_loss(x, gt, LAM, weight=w, exposure=E), FWD + PLANE, BWD + PLANE),
        ("torch: exposure chain + plain node", lambda: training_image_loss(expose(x), gt, LAM), None, None),
        ("torch: weighted SSIM from conv2d", lambda: torch_weighted(x, w), None, None),
        ("torch: exposure chain + weighted SSIM from conv2d", lambda: torch_weighted(expose(x), w), None, None),
    ]


def run(fn, timed):
    x.grad = E.grad = None
    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    a.record()
    loss = fn()[0]
    b.record()
    loss.backward()
    c.record()
    c.synchronize()
    if timed is not None:
        timed[0] += a.elapsed_time(b)
        timed[1] += b.elapsed_time(c)
    return float(loss.detach())


def report(name, t, fb, bb):
    for what, ms, nbytes in (("forward ", t[0], fb), ("backward", t[1], bb)):
        us = ms / ITERS * 1e3
        tail = f"  must move {nbytes / 1e6:.1f} MB = {nbytes / (us * 1e-6) / HBM * 100:.1f} % of {HBM / 1e12:.2f} TB/s" if nbytes else ""
        print(f"{name}, {what}: {us:.1f} us{tail}")


for _, fn, _, _ in VARIANTS:
    for _ in range(3):
        run(fn, None)
torch.cuda.synchronize()
# the plain node on its own, back to back: the one row that means the same on a build without the keywords (between the other
# variants it finds the caches as they leave them: a different number, below)
alone = [0.0, 0.0]
for _ in range(ITERS):
    run(VARIANTS[0][1], alone)
total = {name: [0.0, 0.0] for name, _, _, _ in VARIANTS}
for _ in range(ITERS):              # alternating: every variant sees the same clocks
    for name, fn, _, _ in VARIANTS:
        run(fn, total[name])
print(f"# {C}x{H}x{W}, {ITERS} iterations, device events around the forward call and around .backward(); "
      f"keywords {'present' if HAS_KEYWORDS else 'absent: plain node only'}")
if HAS_KEYWORDS:
    pairs = [("node, exposure", "torch: exposure chain + plain node"), ("node, weight", "torch: weighted SSIM from conv2d"),
             ("node, weight + exposure", "torch: exposure chain + weighted SSIM from conv2d")]
    fns = {name: fn for name, fn, _, _ in VARIANTS}
    for a, b in pairs:
        print(f"# |fused - torch| of the loss, {a}: {abs(run(fns[a], None) - run(fns[b], None)):.2e}")
report("plain node alone (back to back)", alone, FWD, BWD)
print("# alternating:")
for name, _, fb, bb in VARIANTS:
    report(name, total[name], fb, bb)
