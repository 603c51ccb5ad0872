"""Anchor position codec (container version 3) on the bench scene's 1 M anchors and on a shell set of the same size:
bytes of anchor.b against the raw 6 N, device-event times of the order, of pack + class coding and of the decode (single calls,
cases alternating), then conduct_encoding / conduct_decoding in container version 2 and 3 alternately (version 2 is the
yardstick) with the CGS_CODEC_TRACE milestones.  Writes profiles/anchor_code.txt (or argv: --out FILE, --anchors N, --rounds R).

The bench scene's positions are synthetic (contextgs_amd.synth.make_scene); no trained scene is coded here."""
import argparse
import contextlib
import io
import os
import re
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["CGS_CODEC_TRACE"] = "1"

import numpy as np
import torch

from contextgs_amd import _lib, codec
from contextgs_amd.codec_driver import conduct_encoding
from contextgs_amd.encodings import Quantize_anchor
from contextgs_amd.synth import make_scene


def shells(n, seed=1):
    """Three thin spherical shells (radii 0.2 / 0.35 / 0.5 of the half-extent, relative radial jitter 0.002) in the 65536^3 grid."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    r = np.array([0.2, 0.35, 0.5])[rng.integers(0, 3, n)] * (1.0 + 0.002 * rng.normal(size=n))
    return np.clip(np.floor(32768.0 + 32768.0 * r[:, None] * v), 0, 65535).astype(np.int32)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def order_call(q):
    L = _lib.lib()
    n = int(q.shape[0])
    order = torch.empty(n, dtype=torch.int64, device="cuda")
    keys = torch.empty(n, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(int(L.cgs_anchor_order_scratch_bytes(n)), dtype=torch.uint8, device="cuda")

    def call():
        _lib.check(L.cgs_anchor_order(_lib.ptr(q), n, _lib.ptr(order), _lib.ptr(keys), _lib.ptr(status), _lib.ptr(scratch),
                                      scratch.numel(), _lib.current_stream()), "cgs_anchor_order")
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_code.txt"))
    ap.add_argument("--anchors", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--containers", type=int, default=5)
    args = ap.parse_args()
    lines = []
    say = lambda s="": (print(s, flush=True), lines.append(s))

    N = args.anchors
    pc = make_scene(N, seed=0, requires_grad=False)
    pc.eval()
    with torch.no_grad():
        m = pc.get_mask_anchor
        q_scene = Quantize_anchor.apply(pc._anchor[m], pc.x_bound_min, pc.x_bound_max)[1].to(torch.int32).contiguous()
    cases = {"bench scene (synthetic positions)": q_scene, "three thin shells": torch.from_numpy(shells(int(q_scene.shape[0]))).cuda()}
    say(f"anchor_code_micro: {int(q_scene.shape[0])} valid anchors of {N}, {torch.cuda.get_device_name(0)}; the bench scene's positions "
        "are synthetic, no trained scene was coded")
    say("-- size of anchor.b")
    streams = {}
    for name, q in cases.items():
        order, stream = codec.anchor_encode(q)
        assert torch.equal(codec.anchor_decode(stream, "cuda"), q[order])
        streams[name] = stream
        n = int(q.shape[0])
        say(f"{name:36s} {len(stream):9d} B = {len(stream) / n:.3f} B/anchor = {len(stream) / (6 * n):.4f} of the raw {6 * n} B")
    say(f"-- device events around single calls, {args.rounds} alternating rounds after 2 warm-up; encode and decode include their host "
        "read-backs (status + histogram, block lengths, bytes) and the header validation")
    t = {name: {"order": [], "encode": [], "decode": []} for name in cases}
    calls = {name: order_call(q) for name, q in cases.items()}
    for r in range(args.rounds + 2):
        for name, q in cases.items():
            a = timed(calls[name])[0]
            b = timed(lambda: codec.anchor_encode(q))[0]
            c = timed(lambda: codec.anchor_decode(streams[name], "cuda"))[0]
            if r >= 2:
                t[name]["order"].append(a); t[name]["encode"].append(b); t[name]["decode"].append(c)
    say(f"{'case':36s} {'call':36s} {'median ms':>10s} {'min ms':>8s} {'max ms':>8s}")
    for name in cases:
        o, e, d = t[name]["order"], t[name]["encode"], t[name]["decode"]
        rest = [x - y for x, y in zip(e, o)]
        for label, v in (("cgs_anchor_order", o), ("anchor_encode (all)", e), ("  pack + class coding (all - order)", rest),
                         ("anchor_decode", d)):
            say(f"{name:36s} {label:36s} {statistics.median(v):10.3f} {min(v):8.3f} {max(v):8.3f}")

    say(f"-- conduct_encoding / conduct_decoding, versions 2 and 3 alternating, {args.containers} each after one warm-up pair")
    root = tempfile.mkdtemp(prefix="cgs_anchor_micro_")
    res = {2: {"enc": [], "dec": [], "plan": [], "size": None}, 3: {"enc": [], "dec": [], "plan": [], "size": None}}
    try:
        for r in range(args.containers + 1):
            for v in (2, 3):
                d = os.path.join(root, f"v{v}")
                torch.cuda.synchronize(); t0 = time.perf_counter()
                with contextlib.redirect_stderr(io.StringIO()), contextlib.redirect_stdout(io.StringIO()):
                    conduct_encoding(pc, d, container_version=v)
                torch.cuda.synchronize(); te = time.perf_counter() - t0
                dec = make_scene(N, seed=0, requires_grad=False); dec.eval()
                err = io.StringIO()
                torch.cuda.synchronize(); t0 = time.perf_counter()
                with contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
                    dec.conduct_decoding(d)
                torch.cuda.synchronize(); td = time.perf_counter() - t0
                plan = re.search(r"\+\s*([0-9.]+) ms\] level plan built", err.getvalue())
                if r >= 1:
                    res[v]["enc"].append(te); res[v]["dec"].append(td); res[v]["plan"].append(float(plan.group(1)))
                res[v]["size"] = {f: os.path.getsize(os.path.join(d, f)) for f in sorted(os.listdir(d))}
                res[v]["trace"] = err.getvalue()
                del dec
    finally:
        shutil.rmtree(root, ignore_errors=True)
    nv = int(q_scene.shape[0])
    for v in (2, 3):
        e, d, p = res[v]["enc"], res[v]["dec"], res[v]["plan"]
        say(f"version {v}: encode {statistics.median(e) * 1e3:6.1f} ms = {nv / statistics.median(e) / 1e6:5.1f} M anchors/s "
            f"({' / '.join(f'{x * 1e3:.1f}' for x in e)}); decode {statistics.median(d) * 1e3:6.1f} ms = "
            f"{nv / statistics.median(d) / 1e6:5.1f} M anchors/s ({' / '.join(f'{x * 1e3:.1f}' for x in d)}); decoder start -> "
            f"\"level plan built\" {statistics.median(p):5.1f} ms ({' / '.join(f'{x:.1f}' for x in p)})")
    s2, s3 = res[2]["size"], res[3]["size"]
    say(f"container bytes: version 2 {sum(s2.values())} (anchor.npy {s2.get('anchor.npy')}), version 3 {sum(s3.values())} "
        f"(anchor.b {s3.get('anchor.b')}); the other files: {sum(v for k, v in s2.items() if k != 'anchor.npy')} -> "
        f"{sum(v for k, v in s3.items() if k != 'anchor.b')}")
    say("-- decoder milestones of the last version-3 container")
    for ln in res[3]["trace"].splitlines():
        say("   " + ln)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
