"""Cost of the depth-prior losses (csrc/depth_prior.hip, contextgs_amd/depth_prior.py) at 1x1080x1920, alternating in one run, device
events after a warm-up; forward and backward timed apart:
  the fused nodes                       l1 with a given affine, l1 / l2 with align="lstsq", Pearson; mask none / float / bool
  the same maths composed in torch      selection by torch.where, the moments in float64 (in float32 they cancel and the composition
                                        would compute something else), the fit detached, the residual pass in float32
next to the bytes each call must move and the share of HBM bandwidth (6.29 TB/s) that makes:
  forward            x and y read once per pass over the planes (8 B per pixel; l1 with the fit makes two passes), plus the mask
                     (4 B per pixel as float, 1 B as bool)
  backward           the same planes read once, d x written (+ 4 B per pixel)
and, with --count-launches (a run of its own: the profiler slows the host), the kernel launches of each fused call as the
profiler sees them, next to the budget in the module's docstring.
The comparison partner of a fused call is the torch composition of the same run, never an earlier number.
Usage: python tools/depth_prior_micro.py [iters] [--count-launches] -> stdout (kept in profiles/depth_prior.txt).  GPU box."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from contextgs_amd.depth_prior import depth_prior_loss, pearson_depth_loss

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
ITERS = int(ARGS[0]) if ARGS else 50
H, W = 1080, 1920
N = H * W
HBM = 6.29e12
AFFINE = (0.0069, 4.0004)
dev = "cuda"
gen = torch.Generator(device=dev).manual_seed(0)
prior = torch.rand(1, H, W, device=dev, generator=gen) * 1.9 + 0.1
render = 4.0 + 0.01 * (0.7 * prior + 0.3 * torch.randn(1, H, W, device=dev, generator=gen))
keep = torch.rand(1, H, W, device=dev, generator=gen) > 0.3
MASKS = {"none": None, "float": keep.float() * (torch.rand(1, H, W, device=dev, generator=gen) + 0.5), "bool": keep}
MASK_BYTES = {"none": 0, "float": 4, "bool": 1}


# ---- the torch compositions ---------------------------------------------------------------------------------------------------------
def _selected(x, y, m):
    """(w, x, y) in float64 with the pixels of m = 0 selected out (w None without a mask)."""
    xd, yd = x.double(), y.double()
    if m is None:
        return None, xd, yd
    sel = m != 0
    return (m.double() if m.is_floating_point() else sel.double()), torch.where(sel, xd, 0.0), torch.where(sel, yd, 0.0)


def _moments(w, xd, yd):
    if w is None:
        return float(N), xd.sum(), yd.sum(), (xd * xd).sum(), (yd * yd).sum(), (xd * yd).sum()
    wx, wy = w * xd, w * yd
    return w.sum(), wx.sum(), wy.sum(), (wx * xd).sum(), (wy * yd).sum(), (wx * yd).sum()


def _residual_loss(x, y, m, a, b, kind):
    r = x - (a * y + b)
    e = r.abs() if kind == "l1" else r * r
    if m is None:
        return e.mean()
    sel = m != 0
    w = m if m.is_floating_point() else sel.float()
    return (w * torch.where(sel, e, 0.0)).sum() / w.sum()


def torch_given(kind):
    return lambda x, y, m: _residual_loss(x, y, m, AFFINE[0], AFFINE[1], kind)


def torch_lstsq(kind):
    def f(x, y, m):
        with torch.no_grad():
            M, Sx, Sy, Sxx, Syy, Sxy = _moments(*_selected(x, y, m))
            a = (M * Sxy - Sx * Sy) / (M * Syy - Sy * Sy)
            b = (Sx - a * Sy) / M
        return _residual_loss(x, y, m, a.float(), b.float(), kind)
    return f


def torch_pearson(x, y, m):
    M, Sx, Sy, Sxx, Syy, Sxy = _moments(*_selected(x, y, m))
    return (1.0 - (M * Sxy - Sx * Sy) / torch.sqrt((M * Sxx - Sx * Sx) * (M * Syy - Sy * Sy))).float()


FORMS = (      # name, fused, torch, passes over the planes in the forward, launch budget forward
    ("l1, given affine", lambda x, y, m: depth_prior_loss(x, y, m, kind="l1", affine=AFFINE), torch_given("l1"), 1, 2),
    ("l1, lstsq", lambda x, y, m: depth_prior_loss(x, y, m, kind="l1", align="lstsq"), torch_lstsq("l1"), 2, 4),
    ("l2, lstsq", lambda x, y, m: depth_prior_loss(x, y, m, kind="l2", align="lstsq"), torch_lstsq("l2"), 1, 2),
    ("pearson", pearson_depth_loss, torch_pearson, 1, 2),
)


def variant(fn, m):
    def make():
        return fn(render.detach().requires_grad_(), prior, m)
    return make


# (name, make() -> loss, bytes forward, bytes backward, launch budget or None)
VARIANTS = []
for mname, m in MASKS.items():
    px = 8 + MASK_BYTES[mname]
    for fname, fused, composed, passes, budget in FORMS:
        VARIANTS.append((f"fused {fname}, mask {mname}", variant(fused, m), passes * px * N, (px + 4) * N, budget))
        VARIANTS.append((f"torch {fname}, mask {mname}", variant(composed, m), None, None, None))


def run(make, timed):
    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    a.record()
    out = make()
    b.record()
    out.backward()
    c.record()
    c.synchronize()
    if timed is not None:
        timed[0] += a.elapsed_time(b)
        timed[1] += b.elapsed_time(c)
    return out.detach()


if "--count-launches" in sys.argv:
    from torch.profiler import ProfilerActivity, profile

    for name, make, _, _, budget in VARIANTS:
        if budget is None:
            continue
        run(make, None)
        counts = []
        for phase in ("forward", "backward"):
            x = render.detach().requires_grad_()
            out = None if phase == "forward" else make()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                if phase == "forward":
                    out = make()
                else:
                    out.backward()
                torch.cuda.synchronize()
            names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "dp_" in e.name]
            counts.append(len(names))
        print(f"{name}: launches of depth-prior kernels forward {counts[0]} (budget {budget}), backward {counts[1]} (budget 1)")
    sys.exit(0)

for _, make, _, _, _ in VARIANTS:
    for _ in range(3):
        run(make, None)
torch.cuda.synchronize()
total = {name: [0.0, 0.0] for name, *_ in VARIANTS}
for _ in range(ITERS):                              # alternating: every variant sees the same clocks
    for name, make, *_ in VARIANTS:
        run(make, total[name])
print(f"# render and prior 1x{H}x{W}, {ITERS} iterations, device events around the forward call and around .backward(), alternating; "
      "the torch compositions take their moments in float64")
makes = {name: make for name, make, *_ in VARIANTS}
for name in makes:
    if name.startswith("fused"):
        d = (run(makes[name], None) - run(makes[name.replace("fused", "torch")], None)).abs().item()
        print(f"# |fused - torch| of {name[6:]}: {d:.2e}")
slower = []
for name, _, fb, bb, _ in VARIANTS:
    for i, (what, nbytes) in enumerate((("forward ", fb), ("backward", bb))):
        us = total[name][i] / ITERS * 1e3
        tail = f"  must move {nbytes / 1e6:.1f} MB = {nbytes / (us * 1e-6) / HBM * 100:.1f} % of {HBM / 1e12:.2f} TB/s" if nbytes else ""
        print(f"{name}, {what}: {us:.1f} us{tail}")
        if name.startswith("fused") and total[name][i] > total[name.replace("fused", "torch")][i]:
            slower.append(f"{name}, {what.strip()}")
print("# fused calls slower than their torch composition: " + (", ".join(slower) if slower else "none"))

# The rows above time a call as a training step sees it on an idle device: at these sizes mostly the host's path to the launch.
# The kernels alone: C-ABI calls queued back to back (QUEUE per event pair), so the device never waits for the host.
from contextgs_amd import _lib

QUEUE = 20
Lb, p, st = _lib.lib(), _lib.ptr, _lib.current_stream()
x, y = render.contiguous(), prior.contiguous()
out, dx, g = torch.empty(1, device=dev), torch.empty_like(x), torch.ones(1, device=dev)
coef = torch.zeros(8, dtype=torch.float64, device=dev)
sb = int(Lb.cgs_depth_prior_scratch_bytes(H, W))
scratch = torch.empty(sb // 8, dtype=torch.float64, device=dev)
ABI = []
for mname, m in MASKS.items():
    mt = {"none": 0, "float": 1, "bool": 2}[mname]
    mm = None if m is None else (m.view(torch.uint8) if m.dtype == torch.bool else m.contiguous())
    px = 8 + MASK_BYTES[mname]
    for fname, kind, align, passes, launches in (("l1 given", 0, 0, 1, 2), ("l1 lstsq", 0, 1, 2, 4), ("l2 lstsq", 1, 1, 1, 2), ("pearson", 2, 0, 1, 2)):
        ABI.append((f"cgs_depth_prior_fwd {fname}, mask {mname} ({launches} launches)", passes * px * N,
                    lambda mm=mm, mt=mt, kind=kind, align=align: Lb.cgs_depth_prior_fwd(
                        p(x), p(y), p(mm), mt, H, W, kind, align, 0, AFFINE[0], AFFINE[1], None, None, p(out), p(coef), p(scratch), sb, st)))
    ABI.append((f"cgs_depth_prior_bwd l1, mask {mname} (1 launch)", (px + 4) * N,
                lambda mm=mm, mt=mt: Lb.cgs_depth_prior_bwd(p(x), p(y), p(mm), mt, H, W, 0, p(coef), p(g), p(dx), st)))
    ABI.append((f"cgs_depth_prior_bwd pearson, mask {mname} (1 launch)", (px + 4) * N,
                lambda mm=mm, mt=mt: Lb.cgs_depth_prior_bwd(p(x), p(y), p(mm), mt, H, W, 2, p(coef), p(g), p(dx), st)))
# The scalar instances: what a call pays when H W is no multiple of 4 or a plane is off its 16-byte alignment (a sliced view).
# The same planes one float off the alignment; the same four pixels per lane, by 4-byte accesses.
def _off(t):
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    big[1:] = t.reshape(-1)
    return big[1:]


xo, yo, dxo = _off(x), _off(y), _off(dx)
assert xo.data_ptr() % 16 and yo.data_ptr() % 16 and dxo.data_ptr() % 16
for fname, kind, align, passes, launches in (("l1 given", 0, 0, 1, 2), ("pearson", 2, 0, 1, 2)):
    ABI.append((f"cgs_depth_prior_fwd {fname}, mask none, planes off alignment: scalar instance ({launches} launches)", passes * 8 * N,
                lambda kind=kind, align=align: Lb.cgs_depth_prior_fwd(
                    p(xo), p(yo), None, 0, H, W, kind, align, 0, AFFINE[0], AFFINE[1], None, None, p(out), p(coef), p(scratch), sb, st)))
ABI.append(("cgs_depth_prior_bwd l1, mask none, planes off alignment: scalar instance (1 launch)", 12 * N,
            lambda: Lb.cgs_depth_prior_bwd(p(xo), p(yo), None, 0, H, W, 0, p(coef), p(g), p(dxo), st)))
abi_ms = {name: 0.0 for name, _, _ in ABI}
ROUNDS = max(1, ITERS // 5)
for rep in range(1 + ROUNDS):                       # the first round warms up; the entries alternate
    for name, _, call in ABI:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(QUEUE):
            assert call() == 0
        b.record()
        b.synchronize()
        if rep:
            abi_ms[name] += a.elapsed_time(b)
print(f"# kernels alone: {QUEUE} C-ABI calls queued between two device events, {ROUNDS} rounds, entries alternating; fp64 accumulation "
      f"in every reduction; scratch {sb} B")
for name, nbytes, _ in ABI:
    us = abi_ms[name] / ROUNDS / QUEUE * 1e3
    print(f"{name}: {us:.1f} us  must move {nbytes / 1e6:.1f} MB = {nbytes / (us * 1e-6) / HBM * 100:.1f} % of {HBM / 1e12:.2f} TB/s")
