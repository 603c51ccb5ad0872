"""Bitstream container: `conduct_encoding`, `conduct_decoding`, `estimate_final_bits`,
`save/load_mlp_checkpoints` (scene/gaussian_model.py:912-951,
980-1004, 1007-1295, 1299-1539 — cited lines are that file).

Same container as the reference — anchor.npy (uint16 [N_valid,3]), hyper.b,
feat{l}.b / scaling{l}.b / offsets{l}.b (1000-anchor chunk streams concatenated,
byte lengths in meta), masks.b, meta.b (a torch.save'd 14-item list, :1277), mlp.pt —
and the same level / chunk / mask order.  What differs is how it is scheduled: instead
of a Python loop of ~3 N/1000 serial torchac calls, each shipping a [50 000, L] float
table over PCIe (:1192-1232), chunk streams are coded concurrently by device launches,
one wave per stream (codec.gaussian_encode_groups / gaussian_decode_groups):
  * encoding never reads coded bytes back, so the level loop only predicts and
    quantises, and ALL streams (3 levels x feat/scaling/offsets) go through one launch
    whose duration is that of its longest stream;
  * decoding needs level l's feat+scaling before level l+1's context, so those are one
    launch per level; offsets feed no context and are decoded for all levels at the end;
  * the format's serial host streams (the mask stream, the 10 000-anchor hyper rANS
    strings) run on host threads next to the device work (codec.host_pool).

Container version 3 (opt-in) is version 2 with the anchors coded: anchor.b (codec.anchor_encode: Morton-ordered positions, gap
classes through the table coder, raw low bits) replaces anchor.npy, and every per-anchor tensor is coded in that sorted order, so
the decoded model's rows come back sorted by Morton key.

Layout of the code: `ContainerLayout` is the one record of what a container version means.  Built when writing (requested version,
module constants) or when reading (the header: `ContainerMeta` is meta.b by name), it alone says where streams and blocks are cut,
which files are staged in which order and what the header's 15th item holds: both directions must agree on that byte for byte.
`conduct_encoding` / `conduct_decoding` read top to bottom as the schedule: one function per stage, one `_Coding` object carrying the
buffers; a stage that differs by version (masks, hyper, anchors, the offsets' launch) is listed per version in `_ENCODE` / `_DECODE`.

Deliberate deviation: the reference's decoder raises IndexError when fewer
than 10 000 anchors are valid (:1322-1331); this one decodes any size.
"""
from __future__ import annotations

import os
import re
import time
from collections import namedtuple
from functools import partial
from typing import NamedTuple

import numpy as np
import torch
import torch.nn as nn

from . import codec
from . import dist as mgpu
from .context_model import context_rows, find_divide_scale, grid_mlp, level_plan, multi_scale_generating, split_prediction
from .encodings import Q_anchor, Quantize_anchor, STE_multistep

bit2MB_scale = 8 * 1024 * 1024
MAX_BATCH = 1_000                                              # :1071

# Container versions.  1 = the reference's container (default): one serial arithmetic-coded mask stream, 10 000-anchor hyper
# strings, 1000-anchor chunk streams for every Gaussian-coded attribute, a 14-item meta list.  2 = the same files, symbols,
# order and coder, re-cut for a device: the masks are 1000-anchor chunk streams coded by the device coder
# (codec.BernoulliEncodeJob; no serial host stream is left on either critical chain), the hyper latents go through the device
# table coder instead of host rANS strings (EntropyBottleneck.compress_lanes: same tables), and feat / scaling / offsets are cut
# into BLOCKS of V2_BLOCK consecutive symbols, each coded as 64 interleaved lane streams by one wave (csrc/codec.hip,
# "Lane-parallel Gaussian codec": the coder arithmetic runs 64-wide in vector registers instead of one serial chain per
# wave on the scalar unit).  meta.b gets a 15th item {"version": 2, "block_symbols": ..., "chunk": {"masks": ...},
# "bit_masks": [...]}; the per-stream lists of the header (bits, min, max) are per block; a 14-item list is version 1.
# 3 = version 2 with the anchor positions coded without loss: anchor.b (codec.anchor_encode / anchor_decode, csrc/anchor_code.hip;
# byte format in INTEGRATION.md) instead of anchor.npy.  The valid anchors are coded in the stable ascending order of their
# 48-bit Morton keys — the selection of every per-anchor tensor is nonzero(mask)[order] instead of [mask] — so the level plan,
# the contexts and every other stream live in that order, and so do the rows of the decoded model.  meta.b's 15th item says
# "version": 3 and adds "anchor": {"scheme": "morton-gap", "block": B, "bytes": len(anchor.b)}.  One rank only.
CONTAINER_VERSION = 1
V2_BLOCK = 64 * 512                      # symbols per block: 512 per lane stream
V2_CHUNK = {"masks": 1000}               # anchors per mask chunk stream
V2_HYPER_BLOCK = 64 * 512                # anchors of one channel per hyper.b block (lane-parallel table coder)


def default_container_version():
    return int(os.environ.get("CGS_CONTAINER_VERSION", CONTAINER_VERSION))


def save_mlp_checkpoints(pc, path):                            # :912-936
    pc.latent_codec.update()
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    torch.save({"opacity_mlp": pc.mlp_opacity.state_dict(), "cov_mlp": pc.mlp_cov.state_dict(),
                "color_mlp": pc.mlp_color.state_dict(), "latent_codec": pc.latent_codec.state_dict(),
                "grid_mlp": pc.mlp_grid.state_dict(), "bound": [pc.x_bound_min, pc.x_bound_max],
                "level_scale": pc.level_scale}, path)


def load_mlp_checkpoints(pc, path, ck=None, tr=None, stored_tables=False):          # :939-950
    """ck: an already loaded checkpoint dict; tr: the driver's tracer (CGS_CODEC_TRACE).
    stored_tables (container version 2): take the hyper prior's integer CDF tables the ENCODER used from the checkpoint
    (`_quantized_cdf` / `_cdf_length` / `_offset`: buffers of the state dict torch.save wrote) instead of rebuilding them with
    update(force=True) as the reference does (:946-947) — the decoder then codes with exactly the encoder's tables whatever
    device evaluated the density, and skips ~2 ms of its prologue.  A checkpoint without them falls back to update()."""
    tr = tr or (lambda label: None)
    if ck is None:
        ck = read_mlp_checkpoint(path)
        tr("mlp.pt unpickled")
    # restored on the HOST, then every tensor of the checkpoint goes to the device in ONE pinned non-blocking copy
    # (restoring ~70 small tensors on the device is ~70 blocking pageable copies: 3 ms of the decoder's prologue)
    ck = _tensors_to_device(ck, pc.x_bound_min.device)
    tr("mlp.pt on the device")
    pc.mlp_opacity.load_state_dict(ck["opacity_mlp"])
    pc.mlp_cov.load_state_dict(ck["cov_mlp"])
    pc.mlp_color.load_state_dict(ck["color_mlp"])
    _load_latent_codec(pc.latent_codec, ck["latent_codec"])
    tr("mlp.pt: state dicts loaded")
    lc, eb = ck["latent_codec"], pc.latent_codec
    tabs = [lc.get(k) for k in ("_quantized_cdf", "_cdf_length", "_offset")] if stored_tables else [None]
    if all(isinstance(t, torch.Tensor) and t.numel() > 0 for t in tabs) and tabs[0].dim() == 2 \
            and tabs[0].shape[0] == tabs[1].numel() == tabs[2].numel() == eb.channels:
        dev = eb.quantiles.device
        eb._quantized_cdf, eb._cdf_length, eb._offset = (t.to(device=dev, dtype=torch.int32) for t in tabs)
        tr("prior tables taken from the checkpoint")
    else:
        eb.update(force=True)
        tr("prior tables rebuilt")
    pc.mlp_grid.load_state_dict(ck["grid_mlp"])
    pc.x_bound_min, pc.x_bound_max = ck["bound"]
    pc.level_scale = ck["level_scale"]


_STORAGE_DTYPES = {"FloatStorage": torch.float32, "DoubleStorage": torch.float64, "HalfStorage": torch.float16,
                   "BFloat16Storage": torch.bfloat16, "LongStorage": torch.int64, "IntStorage": torch.int32,
                   "ShortStorage": torch.int16, "CharStorage": torch.int8, "ByteStorage": torch.uint8, "BoolStorage": torch.bool}


class _StorageRef:
    __slots__ = ("dtype", "key", "numel")

    def __init__(self, dtype, key, numel):
        self.dtype, self.key, self.numel = dtype, key, numel


def _zip_members(buf):
    """{name: (data offset, size)} of an uncompressed, non-zip64 archive held in `buf` — the layout torch.save writes.
    (zipfile.ZipFile takes 1.2 ms for the 80 members of mlp.pt; this is two struct reads per member.)"""
    import struct
    eocd = buf.rfind(b"PK\x05\x06")
    if eocd < 0:
        raise ValueError("no end-of-central-directory record")
    n_ent, cd_size, cd_off = struct.unpack_from("<HII", buf, eocd + 10)
    if n_ent == 0xFFFF or cd_size == 0xFFFFFFFF or cd_off == 0xFFFFFFFF:
        raise ValueError("zip64 archive")
    out, p = {}, cd_off
    for _ in range(n_ent):
        if buf[p:p + 4] != b"PK\x01\x02":
            raise ValueError("bad central directory")
        method, = struct.unpack_from("<H", buf, p + 10)
        csize, usize, nlen, elen, clen = struct.unpack_from("<IIHHH", buf, p + 20)
        hoff, = struct.unpack_from("<I", buf, p + 42)
        name = bytes(buf[p + 46:p + 46 + nlen]).decode("utf-8")
        if method != 0 or csize != usize or 0xFFFFFFFF in (csize, hoff):
            raise ValueError("compressed or zip64 member")
        lnlen, lelen = struct.unpack_from("<HH", buf, hoff + 26)          # the LOCAL header's own name / extra lengths
        out[name] = (hoff + 30 + lnlen + lelen, usize)
        p += 46 + nlen + elen + clen
    return out


def _fast_checkpoint_load(path):
    """torch.load(path, map_location="cpu") for the files THIS container holds (mlp.pt, meta.b: nested dicts / lists of
    tensors, numpy arrays and Python numbers), without torch's per-tensor Python path (~60 us a tensor: 4.6 ms of the
    decoder's 23 for mlp.pt's 74): the archive is mapped once, tensors are views into the mapping.  Only the globals such a
    file needs are resolved; anything else raises and the caller falls back to torch.load."""
    import collections
    import io
    import pickle
    import mmap
    with open(path, "rb") as f:
        buf = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_COPY)       # private pages: the tensors below keep it alive
    members = _zip_members(buf)
    pkl = [n for n in members if n.endswith("/data.pkl")]
    if len(pkl) != 1:
        raise ValueError("not a torch.save archive")
    root = pkl[0][:-len("data.pkl")]

    def rebuild(st, storage_offset, size, stride, requires_grad=False, backward_hooks=None, metadata=None):
        off, nbytes = members[root + "data/" + st.key]
        if st.numel * torch.empty(0, dtype=st.dtype).element_size() > nbytes:
            raise ValueError("storage shorter than its tensor")
        if st.numel == 0:
            return torch.empty(tuple(size), dtype=st.dtype)
        return torch.frombuffer(buf, dtype=st.dtype, count=st.numel, offset=off).as_strided(tuple(size), tuple(stride),
                                                                                           storage_offset)

    class Unpickler(pickle.Unpickler):
        def find_class(self, module, name):
            if module == "torch._utils" and name == "_rebuild_tensor_v2":
                return rebuild
            if module == "torch._utils" and name == "_rebuild_parameter":
                return lambda data, requires_grad, backward_hooks: data
            if module == "torch" and name in _STORAGE_DTYPES:
                return _STORAGE_DTYPES[name]
            if module == "collections" and name == "OrderedDict":
                return collections.OrderedDict
            if module.split(".")[0] == "numpy" or (module, name) == ("_codecs", "encode") or (
                    module in ("builtins", "__builtin__") and name in ("bytes", "bytearray", "complex", "set", "frozenset")):
                return super().find_class(module, name)                     # numpy arrays (protocol 2) and plain containers
            raise pickle.UnpicklingError(f"global {module}.{name} is not one this loader resolves")

        def persistent_load(self, pid):
            if not (isinstance(pid, tuple) and len(pid) >= 5 and pid[0] == "storage" and isinstance(pid[1], torch.dtype)):
                raise pickle.UnpicklingError("unexpected persistent id")
            return _StorageRef(pid[1], str(pid[2]), int(pid[4]))

    off, nbytes = members[pkl[0]]
    return Unpickler(io.BytesIO(bytes(buf[off:off + nbytes]))).load()


def read_mlp_checkpoint(path):
    """mlp.pt -> the checkpoint dict with HOST tensors: _fast_checkpoint_load, else torch.load (mapped: it copies every
    storage out of the zip otherwise; a legacy non-zip file cannot be mapped and loads the plain way)."""
    try:
        return _fast_checkpoint_load(path)
    except Exception:
        pass
    try:
        return torch.load(path, map_location="cpu", weights_only=False, mmap=True)
    except (RuntimeError, ValueError):
        return torch.load(path, map_location="cpu", weights_only=False)


def _tensors_to_device(obj, dev):
    """Nested dict / list / tuple of CPU tensors -> the same structure of device tensors, one upload for all of them."""
    flat = []

    def collect(o):
        if isinstance(o, torch.Tensor):
            if o.device.type == "cpu":
                flat.append(o)
        elif isinstance(o, dict):
            for v in o.values():
                collect(v)
        elif isinstance(o, (list, tuple)):
            for v in o:
                collect(v)
    collect(obj)
    if not flat or dev.type != "cuda":
        return obj
    up = iter(codec._upload_small([t.detach().contiguous() for t in flat], dev, key="checkpoint"))

    def rebuild(o):
        if isinstance(o, torch.Tensor):
            return next(up) if o.device.type == "cpu" else o
        if isinstance(o, dict):
            return type(o)((k, rebuild(v)) for k, v in o.items())
        if isinstance(o, (list, tuple)):
            return type(o)(rebuild(v) for v in o)
        return o
    return rebuild(obj)


_LEGACY_EB_KEY = re.compile(r"^_?(matrix|bias|factor)(\d+)$")


def _load_latent_codec(codec, state):
    """load_state_dict for the hyper prior that refuses a checkpoint without its density parameters.

    strict=False stays (the reference loads that way, :946: buffers such as the quantised CDF tables are rebuilt by
    update()), but a checkpoint whose density parameters do not land — e.g. one written by a compressai release that
    names them `_matrix0` / `_bias0` / `_factor0` instead of `matrices.0` ... — would leave the prior at its random
    initialisation and decode garbage without a word.  Legacy names are remapped; anything still missing raises."""
    own = set(codec.state_dict().keys())
    remapped = {}
    for k, v in state.items():
        if k in ("_quantized_cdf", "_offset", "_cdf_length"):
            continue      # derived tables with data-dependent shapes: rebuilt from the parameters by update(force=True)
        m = _LEGACY_EB_KEY.match(k)
        if m and k not in own:
            k = {"matrix": "matrices", "bias": "biases", "factor": "factors"}[m.group(1)] + "." + m.group(2)
        remapped[k] = v
    res = codec.load_state_dict(remapped, strict=False)
    density = [k for k in res.missing_keys if k.split(".")[0] in ("matrices", "biases", "factors", "quantiles")]
    if density:
        raise RuntimeError("latent_codec checkpoint lacks the density parameters " + ", ".join(density) +
                           (f" (unexpected keys: {', '.join(res.unexpected_keys)})" if res.unexpected_keys else ""))
    return res


@torch.no_grad()
def estimate_final_bits(pc):                                   # :980-1004
    m = pc.get_mask_anchor
    sums = multi_scale_generating(pc, pc.get_anchor[m], pc._hyper_latent[m], pc._anchor_feat[m], pc._offset[m],
                                  pc.get_scaling[m], binary_grid_masks=pc.get_mask[m], predict_bpp=True,
                                  return_sum_bits=True)
    a, h, f, s, o, mk = sums
    mlp = pc.get_mlp_size()[0]
    r = lambda v: round(v / bit2MB_scale, 4)
    return (f"\nEstimated sizes in MB: anchor {r(a)}, feat {r(f)}, scaling {r(s)}, offsets {r(o)}, hyper {r(h)}, "
            f"masks {r(mk)}, MLPs {r(mlp)}, Total {r(a + f + s + o + h + mk + mlp)}")


V2_BLOCK_MIN = 64 * 128                  # shortest block of the per-group policy: 128 symbols per lane stream
V2_BLOCK_POLICY = 2                      # 0 / absent: every group in blocks of "block_symbols"; 1, 2: ContainerLayout.block_symbols


# ---- the header by name -------------------------------------------------------------------------------------------------------
# meta.b: the reference's 14-item list (:1277) in its order, and the 15th item of container versions 2 and 3 (None: absent).
# n_anchors counts every anchor of the model, valid or not; n_levels the valid ones per level, in the order the levels are coded;
# the per-level dicts map a level to its per-stream (version 1) or per-block lists; bit_hyper is per hyper string / block.
ContainerMeta = namedtuple("ContainerMeta", "n_anchors max_batch min_feat max_feat min_scaling max_scaling min_offsets max_offsets "
                           "prob_masks bit_hyper bit_feat bit_scaling bit_offsets n_levels extra", defaults=[None])


def _pack_meta(meta):
    # ContainerMeta -> the list torch.save writes as meta.b.
    return list(meta[:14]) + ([meta.extra] if meta.extra is not None else [])


def _unpack_meta(items):
    return ContainerMeta(*items[:14], items[14] if len(items) > 14 else None)


# ---- the layout: what a container version means -----------------------------------------------------------------------------
def _edges(n, step):
    # 0, step, 2 step, ..., n: the element offsets of the blocks (or chunks) of n symbols (or rows)
    return torch.tensor(list(range(0, n, int(step))) + [n] if n > 0 else [0], dtype=torch.int64)


class ContainerLayout(NamedTuple):
    """How one container is cut.  Built in two places only: for_writing and from_header."""
    # The encoder and the decoder answer every question about streams, blocks and files through it, with the same code.  Nothing
    # outside this class looks at the version number; the stage functions further down are picked by it once per call.
    version: int                         # as stored: 1, 2 or 3
    max_batch: int                       # anchors per version-1 chunk stream (x 10: per hyper string)
    mask_chunk: int                      # anchors per mask chunk stream
    block: int                           # "block_symbols": the block size the policy starts from
    policy: int                          # "block_policy"
    hyper_block: int                     # anchors of one channel per hyper.b block
    block_min: int                       # where the halving of block_symbols stops (not stored: both sides take the module's)

    @staticmethod
    def _check_version(version, unknown, role):
        if version not in (1, 2, 3):
            raise unknown
        if version == 3 and mgpu.world() > 1:
            raise NotImplementedError(f"container version 3 (anchors coded in Morton order) is {role} by one rank only")

    @classmethod
    def for_writing(cls, version=None):
        # (the module's constants as they are at the call)
        version = default_container_version() if version is None else int(version)
        cls._check_version(version, ValueError(f"container version {version}: 1 (the reference's container), 2 or 3"), "written")
        mask_chunk = V2_CHUNK["masks"] if version > 1 else MAX_BATCH
        return cls(version, MAX_BATCH, mask_chunk, V2_BLOCK, V2_BLOCK_POLICY, V2_HYPER_BLOCK, V2_BLOCK_MIN)

    @classmethod
    def from_header(cls, meta):
        # (meta: a ContainerMeta.  14 items are version 1; a 15th item without "block_policy" was cut by policy 0)
        extra = meta.extra if meta.extra is not None else {}
        version = int(extra.get("version", 1))
        cls._check_version(version, RuntimeError(f"meta.b: container version {version} is newer than this decoder (1, 2, 3)"), "decoded")
        max_batch, mask_chunk = int(meta.max_batch), int(extra["chunk"]["masks"] if version > 1 else meta.max_batch)
        return cls(version, max_batch, mask_chunk, int(extra.get("block_symbols", V2_BLOCK)), int(extra.get("block_policy", 0)),
                   int(extra.get("hyper_block", V2_HYPER_BLOCK)), V2_BLOCK_MIN)

    # feat / scaling / offsets are blocks of 64 interleaved lane streams (else 1000-anchor chunk streams)
    lanes = property(lambda self: self.version >= 2)
    # masks and hyper latents go through the device coders (else: a serial host stream, host rANS strings)
    device_coders = property(lambda self: self.version >= 2)
    # anchor.b in Morton order (else anchor.npy in the model's order)
    anchors_coded = property(lambda self: self.version == 3)

    def block_symbols(self, n_level, n_group, D):
        # Symbols per block of a group of n_group symbols in a level of n_level anchors with D features each.
        # A coder launch lasts as long as its longest lane stream (block / 64 serial symbols), and the decoder's three level
        # launches depend on each other: the two small levels would occupy a few dozen waves for 512-symbol chains.
        # Policy 2 (what the encoder writes): ONE block size per LEVEL — from the level's feature symbols (anchors x D), the same
        # size for its scaling and offset groups, which ride in the same launch — halved until the level's features make >= 256
        # blocks (one wave per CU) or lane streams are 128 symbols long: at 1 M and at 500 k anchors the big level keeps
        # 32 768-symbol blocks, the middle one gets 16 384, the small one 8 192 (a block costs a 128-byte header and 64 stream
        # ends, ~0.6 % of its bytes at 32 768 symbols: +0.15 % of the container for the shorter blocks).
        # Policy 1 (containers written earlier): per GROUP, from the group's own symbols, halved until >= 1024 blocks.
        # Policy 0 / absent: every group in blocks of "block_symbols".  The size follows from the counts in the header alone.
        if not self.policy:
            return self.block
        n_sym, want = (n_group, 1024) if self.policy == 1 else (n_level * D, 256)
        b = self.block
        while b > self.block_min and n_sym // b < want:
            b //= 2
        return b

    def mask_edges(self, N_valid, K):
        # Symbol edges of the mask streams of N_valid anchors with K offsets each (version 1: the one serial stream).
        return _edges(N_valid, self.mask_chunk if self.device_coders else max(N_valid, 1)) * K

    def group_edges(self, n_level, width, D):
        # Symbol edges of a level's feature (width = D) or scaling (width = 6) group: n_level x width symbols.
        if self.lanes:
            return _edges(n_level * width, self.block_symbols(n_level, n_level * width, D))
        return _edges(n_level, self.max_batch) * width

    def offset_edges(self, n_level, D, live):
        # Host symbol edges of a level's offsets group, which holds the live slots only.
        # live: the running count of live slots in front of every anchor row and behind the last, int64 [n_level + 1] on any
        # device (lane blocks need its last entry alone and take a plain count as well)
        if self.lanes:
            n_live = int(live[-1]) if isinstance(live, torch.Tensor) else int(live)
            return _edges(n_live, self.block_symbols(n_level, n_live, D))
        return live[_edges(n_level, self.max_batch).to(live.device)].cpu()

    def staged_files(self, n_levels):
        # (the files the decoder stages on the device, in the order the coder launches consume them; how many are read at once)
        # Lane containers: masks first (their launch runs beside the prologue), then level by level incl. the offsets — version 3:
        # anchor.b in front of them, because the anchors gate the level plan.  Version 1: its offsets are one launch at the end.
        # Only the leading files start at once: the checkpoint is read first, on a quiet interpreter — beside eight reader threads
        # that read took 4-8 ms instead of 0.3; the other files are released right after it, still early for the first level.
        levels = list(reversed(range(n_levels)))
        if not self.lanes:
            return [f"{a}{l}.b" for l in levels for a in ("feat", "scaling")] + [f"offsets{l}.b" for l in levels], 0
        lead = ["anchor.b"] if self.anchors_coded else []
        return lead + ["masks.b", "hyper.b"] + [f"{a}{l}.b" for l in levels for a in ("feat", "scaling", "offsets")], len(lead) + 1

    def stream_records(self, lens, mn, mx):
        # A file's per-stream (bits, min, max) as the header stores them.
        if self.lanes:   # arrays: thousands of blocks as Python ints cost the decoder's unpickling a garbage-collector pass
            return lens * 8, mn.astype(np.int32), mx.astype(np.int32)
        return (lens * 8).tolist(), mn.astype(np.int64).tolist(), mx.astype(np.int64).tolist()

    def header_item(self, bit_masks, anchor_bytes):
        # The 15th item of meta.b (None: version 1 keeps the reference's 14).
        if not self.device_coders:
            return None
        item = {"version": 2, "block_symbols": self.block, "block_policy": self.policy, "hyper_block": self.hyper_block,
                "chunk": {"masks": self.mask_chunk}, "bit_masks": bit_masks}
        if self.anchors_coded:
            item.update(version=3, anchor={"scheme": "morton-gap", "block": codec._ANCHOR_BLOCK, "bytes": anchor_bytes})
        return item


def _predict(pc, level, feat_in):
    (mean_feat, scale_feat, mean_scaling, scale_scaling, mean_offsets, scale_offsets, Qf, Qs, Qo) = \
        split_prediction(pc, grid_mlp(pc, level, feat_in))
    c = lambda t: torch.clamp(t, min=1e-9).contiguous()
    return (mean_feat.contiguous(), c(scale_feat), mean_scaling.contiguous(), c(scale_scaling),
            mean_offsets.contiguous(), c(scale_offsets), Qf.reshape(-1).contiguous(), Qs.reshape(-1).contiguous(),
            Qo.reshape(-1).contiguous())


_SIDE = {}


def _side_stream(dev, tag=""):
    # one side stream per device (and purpose) for the life of the process (a fresh stream per container costs the caching
    # allocator a fresh pool, see codec.StagedFiles)
    key = str(dev) + tag
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=dev)
    return _SIDE[key]


def _tracer(name):
    """CGS_CODEC_TRACE=1: wall-clock milestones of the container driver on stderr (host time, no extra synchronisation)."""
    if not os.environ.get("CGS_CODEC_TRACE"):
        return lambda label: None
    import sys
    sync = os.environ.get("CGS_CODEC_TRACE") == "2"       # 2: drain the device at every milestone (attributes device time)
    t0 = time.perf_counter()

    def mark(label):
        if sync:
            torch.cuda.synchronize()
        print(f"[{name} +{(time.perf_counter() - t0) * 1e3:7.1f} ms] {label}", file=sys.stderr)
    return mark


# ---- what both directions share ---------------------------------------------------------------------------------------------
class _Coding:
    """What one conduct_encoding / conduct_decoding call hands from stage to stage."""
    # the valid anchors' tensors as far as they are known (the encoder has anchors, hyper and masks from the start, the decoder
    # fills them in): anchors [N_valid, 3] dequantised; hyper [N_valid, H] as the context MLP is fed it (the encoder's symbols,
    # the decoder's rows); masks [N_valid, K, 1]; context: the rows gathered for the level about to be coded (None: the first)
    anchors = hyper = masks = feat_after_Q = scaling_after_Q = offsets_after_Q = already_coded = None
    context = inverse_indices = mapping = None
    # the decoder's: the unpacked header, the codec.StagedFiles, anchor.npy on its way into pinned memory; version 1: the serial
    # mask stream's host job, the main stream's event in front of the last level's launch; lane containers: the side stream's
    # event behind the mask launch
    meta = staged = anchor_job = mask_job = fork = masks_ready = None

    def __init__(self, layout, directory, pc, **decoder):
        self.layout, self.K, self.D = layout, pc.n_offsets, pc.feat_dim
        self.path = lambda name: os.path.join(directory, name)
        self.pending_offsets, self.live_ahead = [], {}
        self.__dict__.update(decoder)


def _skip(*args):
    pass              # a stage this container version does not have


def _plan_levels(pc, st, tr):
    if pc.level_scale is None:
        pc.level_scale = find_divide_scale(pc, st.anchors, pc.target_ratio, pc.level_num)
    plan, st.inverse_indices, st.mapping = level_plan(pc, st.anchors, None)
    tr("level plan built")
    return plan


def _predict_level(pc, st, level, orig, tr, mark_rows=False):
    # a level's input rows — the anchors themselves for the first level, then the context gathered from the levels already
    # coded; the hyper latents beside either — through the context MLP
    feat_in = torch.cat([st.anchors[orig] if st.context is None else st.context, st.hyper[orig].float()], dim=1)
    if mark_rows:
        tr(f"level {level}: input rows assembled")
    pred = _predict(pc, level, feat_in)
    tr(f"level {level}: predicted (enqueued)")
    return pred


def _gather_next_context(pc, st, level, tr):
    st.context = context_rows(pc, st.anchors, st.feat_after_Q, st.scaling_after_Q, st.already_coded, st.inverse_indices,
                              st.mapping, level)
    tr(f"level {level}: context of the next level gathered")


def _live_mask(st, orig, n):
    # [n, 3K] bool: the offset slots that are transmitted (:1222-1223).
    return st.masks[orig].repeat(1, 1, 3).reshape(n, 3 * st.K).to(torch.bool)


def _live_index(m30):
    # ONE compaction index of the live slots for every operand of the offsets group (and the decoder's fill).
    return torch.nonzero(m30.reshape(-1))[:, 0]


def _live_running_count(m30):
    cnt = torch.zeros(m30.shape[0] + 1, dtype=torch.int64, device=m30.device)
    cnt[1:] = torch.cumsum(m30.sum(1), 0)
    return cnt


def _place_offsets(st, fills, values):
    for (orig, n, live), off_vals in zip(fills, values):
        off_dec = torch.zeros(n * 3 * st.K, device=off_vals.device)
        off_dec.index_copy_(0, live, off_vals)
        st.offsets_after_Q[orig] = off_dec.view(n, st.K, 3)


# ---- encoder stages -----------------------------------------------------------------------------------------------------------
def _anchors_in_model_order(pc, tr):
    return pc.get_mask_anchor, None


def _anchors_in_morton_order(pc, tr):
    # version 3: the valid anchors in the stable ascending order of their Morton keys (an index selection; the model itself
    # is neither permuted nor modified).  Everything after it is defined on whatever order this selection produces.
    mask_anchor = pc.get_mask_anchor
    q = Quantize_anchor.apply(pc._anchor[mask_anchor], pc.x_bound_min, pc.x_bound_max)[1]
    anchor_order, anchor_stream = codec.anchor_encode(q.to(torch.int32))
    tr("anchors ordered and coded (device)")
    return torch.nonzero(mask_anchor.reshape(-1))[:, 0][anchor_order], anchor_stream


def _mask_symbols(st):
    return torch.floor(((st.masks * 2 - 1).view(-1) + 1) / 2)


def _mask_stream_on_host(sym, prob):
    return codec.bernoulli_encode_host(sym, prob), None


def _encode_masks_host(st, prob_masks, tr):
    # Version 1: ONE serial stream on a host thread -> a job whose result is (bytes, None).
    mask_sym = codec.to_host_pinned(_mask_symbols(st).to(torch.int16), "mask symbols")
    tr("mask symbols on the host")
    return codec.host_pool().submit(_mask_stream_on_host, mask_sym, prob_masks)


def _encode_masks_device(st, prob_masks, tr):
    # lane containers: the same symbols as chunk streams, one device launch on a side stream beside everything that follows
    # -> a job whose result is (uint8 array, per-stream byte lengths)
    job = codec.BernoulliEncodeJob(_mask_symbols(st), prob_masks, st.layout.mask_edges(int(st.masks.shape[0]), st.K),
                                   _side_stream(st.masks.device))
    tr("mask chunk streams enqueued (device)")
    return job


def _write_anchor_npy(st, quantized_anchor, anchor_stream):
    # -> (write jobs, bits)
    anchor_u16 = quantized_anchor.cpu().numpy().astype(np.uint16)                           # :1100-1101
    return [codec.host_pool().submit(np.save, st.path("anchor.npy"), anchor_u16)], anchor_u16.size * 16


def _write_anchor_b(st, quantized_anchor, anchor_stream):
    return codec.write_file(st.path("anchor.b"), anchor_stream), len(anchor_stream) * 8


def _encode_hyper_rans(pc, st, hyper_latent, tr):
    jobs = pc.latent_codec.compress_chunks(hyper_latent.t(), st.layout.max_batch * 10, lazy=True)
    tr("hyper symbols on the host, rANS jobs submitted")
    return jobs


def _finish_hyper_rans(st, jobs, writes, tr):
    # Version 1: 10 000-anchor rANS strings (:1082-1098) from host threads -> the header's bit list.
    hyper_bytes = [j.result() for j in jobs]
    tr("hyper rANS jobs done")
    with open(st.path("hyper.b"), "wb") as f:
        f.write(b"".join(hyper_bytes))
    return [len(b) * 8 for b in hyper_bytes]


def _encode_hyper_lanes(pc, st, hyper_latent, tr):
    coded = pc.latent_codec.compress_lanes(hyper_latent.t().contiguous(), st.layout.hyper_block)
    tr("hyper blocks coded (device) and on the host")
    return coded


def _finish_hyper_lanes(st, coded, writes, tr):
    writes += codec.write_file(st.path("hyper.b"), coded[0])
    return coded[1] * 8


_EncodeStages = namedtuple("_EncodeStages", "select_anchors start_masks write_anchors start_hyper finish_hyper")
_ENCODE = {1: _EncodeStages(_anchors_in_model_order, _encode_masks_host, _write_anchor_npy, _encode_hyper_rans, _finish_hyper_rans),
           2: _EncodeStages(_anchors_in_model_order, _encode_masks_device, _write_anchor_npy, _encode_hyper_lanes, _finish_hyper_lanes),
           3: _EncodeStages(_anchors_in_morton_order, _encode_masks_device, _write_anchor_b, _encode_hyper_lanes, _finish_hyper_lanes)}
# the valid anchors' rows of the model, as the encoder codes them
_Source = namedtuple("_Source", "quantized_anchor feat offsets scaling hyper_latent")


def _gather_valid_anchors(pc, st, mask_anchor, tr):
    # -> (_Source, level plan); st gets the anchors, the hyper symbols and the zeroed buffers of the level loop.
    pc.latent_codec.update(force=True)
    tr("tables updated")
    st.anchors, quantized_anchor = Quantize_anchor.apply(pc._anchor[mask_anchor], pc.x_bound_min, pc.x_bound_max)
    src = _Source(quantized_anchor, pc._anchor_feat[mask_anchor], pc._offset[mask_anchor], pc.get_scaling[mask_anchor],
                  pc._hyper_latent[mask_anchor])
    tr("valid anchors gathered")
    # Q3: the encoder feeds integer SYMBOLS to the context MLP (:1040,1164)
    st.hyper = pc.latent_codec.quantize(src.hyper_latent, "symbols", means=pc.latent_codec._get_medians().permute(1, 2, 0)[0])
    plan = _plan_levels(pc, st, tr)
    st.feat_after_Q = torch.zeros_like(src.feat)
    st.scaling_after_Q = torch.zeros_like(src.scaling)
    st.already_coded = torch.zeros(src.feat.shape[0], dtype=torch.bool, device=src.feat.device)
    return src, plan


def _encode_level(pc, st, src, level, orig, tr):
    # Predict and quantise one level (:1112-1242) -> its feat / scaling / offsets groups for the coder launch.
    n_l, K, D, layout = int(orig.shape[0]), st.K, st.D, st.layout
    (mean_feat, scale_feat, mean_scaling, scale_scaling, mean_offsets, scale_offsets, Qf, Qs, Qo) = \
        _predict_level(pc, st, level, orig, tr)
    edges_f, edges_s = layout.group_edges(n_l, D, D), layout.group_edges(n_l, 6, D)
    tr(f"level {level}: chunk rows")
    feat_q = STE_multistep.apply(src.feat[orig], Qf.unsqueeze(1))
    scal_q = STE_multistep.apply(src.scaling[orig], Qs.unsqueeze(1))
    off_q = STE_multistep.apply(src.offsets[orig].reshape(n_l, 3 * K), Qo.unsqueeze(1))
    tr(f"level {level}: quantised")
    m30 = _live_mask(st, orig, n_l)
    off_edges = layout.offset_edges(n_l, D, _live_running_count(m30))
    tr(f"level {level}: offset stream edges on the host")
    live = _live_index(m30)
    pick = lambda t: t.reshape(-1).index_select(0, live)
    groups = [(feat_q, mean_feat, scale_feat, Qf, edges_f, D),
              (scal_q, mean_scaling, scale_scaling, Qs, edges_s, 6),
              (pick(off_q), pick(mean_offsets), pick(scale_offsets), Qo.index_select(0, live // (3 * K)), off_edges, 1)]
    tr(f"level {level}: groups built")

    st.feat_after_Q[orig] = feat_q                                                       # :1240-1242
    st.scaling_after_Q[orig] = scal_q
    st.already_coded.index_fill_(0, orig, True)    # (x[idx] = True uploads its scalar through a blocking pageable copy)
    if level != 0:
        _gather_next_context(pc, st, level, tr)
    return groups


def _write_mlp(pc, st):
    # mlp.pt on THIS thread while the coder launch runs (its small device-to-host copies on a side stream, not behind the
    # launch).  A host thread of its own was tried: torch.save holds the GIL for milliseconds at a time and the level loop
    # stretched from 8 to 10-35 ms waiting for it.
    with torch.cuda.stream(_side_stream(st.masks.device, "mlp")):
        save_mlp_checkpoints(pc, st.path("mlp.pt"))


def _write_streams(st, tags, coded, ready, writes):
    # Submit the file writes of the coded groups (:1235-1238) -> the header's {attribute: {level: list}} of bits, min, max.
    bits, mins, maxs = ({"feat": {}, "scaling": {}, "offsets": {}} for _ in range(3))
    for (name, level), (blob, lens, mn, mx) in zip(tags, coded):
        writes += codec.write_file(st.path(f"{name}{level}.b"), blob, ready=ready)
        bits[name][level], mins[name][level], maxs[name][level] = st.layout.stream_records(lens, mn, mx)
    return bits, mins, maxs


def _finish_masks(st, mask_job, tr):
    # masks.b, written on this thread -> (its bits, the header's per-stream bits or None).
    mask_bytes, mask_lens = mask_job.result()
    tr("mask stream done")
    with open(st.path("masks.b"), "wb") as f:
        f.write(mask_bytes)
    return len(mask_bytes) * 8, None if mask_lens is None else mask_lens * 8


def _write_header(pc, st, meta, bit_anchor, bit_masks, seconds):
    # meta.b (:1276-1277) -> the encoder's summary line.
    torch.save(_pack_meta(meta), st.path("meta.b"))
    total = lambda d: sum(int(np.sum(v)) for v in d.values())
    sizes = {"meta": os.path.getsize(st.path("meta.b")) * 8, "hyper": int(np.sum(meta.bit_hyper)), "anchor": bit_anchor,
             "feat": total(meta.bit_feat), "scaling": total(meta.bit_scaling), "offsets": total(meta.bit_offsets),
             "masks": bit_masks, "MLPs": pc.get_mlp_size()[0]}
    r = lambda v: round(v / bit2MB_scale, 4)
    return ("\nEncoded sizes in MB: " + ", ".join(f"{k} {r(v)}" for k, v in sizes.items()) +
            f", Total {r(sum(sizes.values()))}, EncTime {round(seconds, 4)}")


@torch.no_grad()
def conduct_encoding(pc, pre_path_name, container_version=None):   # :1007-1295
    layout = ContainerLayout.for_writing(container_version)
    stages = _ENCODE[layout.version]
    torch.cuda.synchronize(); t1 = time.time()
    tr = _tracer("encode")
    print("Start encoding ...")
    root = mgpu.rank() == 0          # multi-GPU: every rank predicts/quantises, codes its block of streams; rank 0 writes
    os.makedirs(pre_path_name, exist_ok=True)
    st = _Coding(layout, pre_path_name, pc)

    # the mask stream (:1265-1269) is the longest chain of the version-1 encoder (ONE serial arithmetic-coded stream, 10 M
    # symbols on a host thread): it is started FIRST, before the prior tables and the other per-anchor gathers
    mask_anchor, anchor_stream = stages.select_anchors(pc, tr)
    st.masks = pc.get_mask[mask_anchor]
    prob_masks = (st.masks.sum() / st.masks.numel()).item() if st.masks.numel() else 0.5
    mask_job = stages.start_masks(st, prob_masks, tr) if root else None
    src, plan = _gather_valid_anchors(pc, st, mask_anchor, tr)
    # file writes run on host threads while the device predicts / codes
    writes, bit_anchor = stages.write_anchors(st, src.quantized_anchor, anchor_stream) if root else ([], 0)

    n_levels, groups, tags = [], [], []
    for (level, _to_code, orig, _hybrid_anchor) in plan:                                 # :1112
        n_levels.append(int(orig.shape[0]))
        groups += _encode_level(pc, st, src, level, orig, tr)
        tags += [("feat", level), ("scaling", level), ("offsets", level)]
    tr("levels enqueued")
    # the hyper latents only AFTER the level loop has been enqueued: ~100 short rANS jobs finishing on the pool make the main
    # thread queue for the GIL, which stretched the 7 ms of launch code above to 38 ms when they ran beside it
    hyper_job = stages.start_hyper(pc, st, src.hyper_latent, tr) if root else None
    torch.cuda.synchronize(); t0 = time.time()
    tr("levels done on the device")
    # ALL streams in one launch; the blobs alias the pinned buffer and their download is still in flight when this returns:
    # the file writers wait for it piece by piece (`ready`)
    coded, ready = codec.gaussian_encode_groups(groups, staging=True, lanes=layout.lanes, deferred=True,
                                                overlap=partial(_write_mlp, pc, st) if root else None)
    tr("coder launch done, download queued")
    if not root:
        torch.cuda.synchronize()
        return mgpu.broadcast_object(None)            # the summary string of rank 0

    bits, mins, maxs = _write_streams(st, tags, coded, ready, writes)
    tr("file writes submitted")
    torch.cuda.synchronize(); t_codec = time.time() - t0
    tr("bitstream on the host")
    bit_hyper = stages.finish_hyper(st, hyper_job, writes, tr)
    bit_masks, bit_mask_streams = _finish_masks(st, mask_job, tr)
    for w in writes:
        w.result()                    # every file is on disk before the encoder reports (and raises here if one failed)
    tr("files written")

    torch.cuda.synchronize(); t2 = time.time()
    print("encoding time:", t2 - t1)
    print("codec time:", t_codec)
    meta = ContainerMeta(pc._anchor.shape[0], layout.max_batch, mins["feat"], maxs["feat"], mins["scaling"], maxs["scaling"],
                         mins["offsets"], maxs["offsets"], prob_masks, bit_hyper, bits["feat"], bits["scaling"], bits["offsets"],
                         n_levels, layout.header_item(bit_mask_streams, bit_anchor // 8))
    return mgpu.broadcast_object(_write_header(pc, st, meta, bit_anchor, bit_masks, t2 - t1))


# ---- decoder stages -----------------------------------------------------------------------------------------------------------
def _read_anchor_npy(path):
    # anchor.npy -> a pinned int32 tensor, or None: version 3 has anchor.b, staged and decoded on the device.
    if not os.path.exists(path):
        return None
    a = np.load(path)
    pinned = codec._pinned_staging(a.size * 4, "anchors")[:a.size * 4].view(torch.int32).view(a.shape)
    np.copyto(pinned.numpy(), a, casting="unsafe")
    return pinned


def _stage_files(st, dev, tr):
    # all coded streams: file -> pinned buffer -> device by the staging threads on a side stream; started before anything
    # else is loaded (reading ~120 MB is the longest chain of the prologue)
    names, start = st.layout.staged_files(len(st.meta.n_levels))
    st.staged = codec.StagedFiles([st.path(f_) for f_ in names if os.path.exists(st.path(f_))], dev, start=start)
    codec.decode_status(dev, reset=True)     # the lane decoders report a malformed block here (read once, after the last launch)
    tr("file staging prepared")
    # (whatever tensors a header holds — the reference stores its minima / maxima as device tensors — are only ever read as
    #  Python numbers here: restoring them on the device would cost a copy each and a stream drain per .item())
    tr("meta.b loaded")


def _decode_group(st, name, level, mean, scale, Q, edges, q_div):
    # a group of the decoder launch: the prediction, the cut, and what the header and the staged file hold for it
    header = st.meta._asdict()
    blob = st.staged.get(st.path(f"{name}{level}.b"))                                    # device bytes
    lens = np.asarray(header["bit_" + name][level], dtype=np.int64) // 8
    assert int(lens.sum()) == int(blob.numel())                                          # :1479-1481
    return (mean, scale, Q, edges, header["min_" + name][level], header["max_" + name][level], blob, lens, q_div)


def _masks_from_host_job(st, dev):
    return torch.from_numpy(st.mask_job.result()).to(dev).to(torch.float32).view(-1, st.K, 1)


def _submit_mask_job(st, N_valid, dev, tr):
    # version 1: the mask stream (:1348-1353) is serial and only the offsets need it: a host thread decodes it meanwhile
    st.mask_job = codec.host_pool().submit(codec.bernoulli_decode_host, np.fromfile(st.path("masks.b"), dtype=np.uint8),
                                           N_valid * st.K, float(st.meta.prob_masks))
    tr("mask job submitted")


def _launch_masks(st, N_valid, dev, tr):
    # lane containers: chunk streams, one device launch on the side stream.  It needs the header and masks.b only — staged by
    # the time the checkpoint is unpickled — so its ~3 ms run beside the rest of the prologue, not in front of the first level.
    side_stream = _side_stream(dev)
    with torch.cuda.stream(side_stream):
        mask_lens = np.asarray(st.meta.extra["bit_masks"], dtype=np.int64) // 8
        blob = st.staged.get(st.path("masks.b"))
        assert int(mask_lens.sum()) == int(blob.numel())
        st.masks = codec.bernoulli_decode_packed(float(st.meta.prob_masks), st.layout.mask_edges(N_valid, st.K), blob,
                                                 mask_lens).view(-1, st.K, 1)
        st.masks_ready = side_stream.record_event()
    tr("mask chunk streams: device launch enqueued")


def _join_mask_launch(st, dev):
    torch.cuda.current_stream().wait_event(st.masks_ready)
    st.masks.record_stream(torch.cuda.current_stream())


def _masks_of_a_model_without_levels(st, dev):
    # no level at all (empty model): nothing has asked for the mask job's result
    st.masks = st.masks if st.masks is not None else _masks_from_host_job(st, dev)


def _anchors_from_npy(st, N_valid, dev, tr):
    return st.anchor_job.result().to(dev, non_blocking=True)     # :1340-1342 (pinned: the copy is queued, not waited for)


def _anchors_from_anchor_b(st, N_valid, dev, tr):
    q = codec.anchor_decode(st.staged.get(st.path("anchor.b")))  # int32 [N_valid, 3], rows in Morton order
    if int(q.shape[0]) != N_valid:
        raise RuntimeError(f"anchor.b holds {int(q.shape[0])} anchors, meta.b's levels {N_valid}")
    tr("anchor.b decoded (device)")
    return q


def _decode_hyper_rans(pc, st, N_valid, tr):
    # version 1: the hyper strings are decoded by host threads (straight into a pinned [N_valid, H] buffer); the first level's
    # prediction waits for them
    with open(st.path("hyper.b"), "rb") as f:
        hyper_stream = f.read()
    ends = np.cumsum(np.asarray(st.meta.bit_hyper, dtype=np.int64) // 8).tolist()
    per = st.layout.max_batch * 10                                                       # :1326-1336 (any N_valid, Q2)
    sizes = [min(per, N_valid - s0) for s0 in range(0, N_valid, per)]
    strings = [hyper_stream[e0:e1] for e0, e1 in zip([0] + ends, ends[:len(sizes)])]
    job = pc.latent_codec.decompress_chunks_rows(strings, sizes)
    tr("hyper rANS jobs submitted")
    return job()


def _decode_hyper_lanes(pc, st, N_valid, tr):
    # lane-parallel table blocks, one device launch (EntropyBottleneck.decompress_lanes_rows)
    rows = pc.latent_codec.decompress_lanes_rows(st.staged.get(st.path("hyper.b")), np.asarray(st.meta.bit_hyper, dtype=np.int64) // 8,
                                                 N_valid, st.layout.hyper_block)
    tr("hyper blocks: device launch enqueued")
    return rows


def _live_slots(st, level, orig, n, by_row=True):
    # -> (host stream edges, live index) of a level's offsets from the decoded masks; by_row: the edges want every row's count.
    m30 = _live_mask(st, orig, n)
    live = _live_index(m30)
    return st.layout.offset_edges(n, st.D, _live_running_count(m30) if by_row else int(live.numel())), live


def _read_offset_edges_ahead(st, plan, tr):
    # lane containers: the offsets' stream edges of EVERY level in one host read, before the first coder launch is queued (a
    # read inside the level loop would drain the previous level's launch and leave the device idle while the next one is built)
    _join_mask_launch(st, None)
    for (level, _to_code, orig, _hybrid_anchor) in plan:
        st.live_ahead[level] = _live_slots(st, level, orig, int(orig.shape[0]), by_row=False)
    tr("offset blocks of all levels on the host")


def _offset_groups(st, pending, live_slots):
    # -> (the coder groups of the pending levels' offsets, where their values go).
    groups, fills = [], []
    for (level, orig, n, mean_o, scale_o, Qo) in pending:
        off_edges, live = live_slots(st, level, orig, n)
        groups.append(_decode_group(st, "offsets", level, mean_o.reshape(-1).index_select(0, live),
                                    scale_o.reshape(-1).index_select(0, live), Qo.index_select(0, live // (3 * st.K)), off_edges, 1))
        fills.append((orig, n, live))
    return groups, fills


def _offsets_ride_with_their_level(st, last):
    # lane containers: the masks are on the device long before the first level is predicted, so a level's offsets ride in
    # that level's launch (their streams are not longer than the feature streams beside them)
    return _offset_groups(st, st.pending_offsets[-1:], lambda st, level, orig, n: st.live_ahead[level])


def _fork_before_the_last_level(st, last):
    if last:
        st.fork = torch.cuda.current_stream().record_event()        # everything the offsets need exists before this point
    return [], []


def _launch_offsets_beside_the_last_level(st, last, dev, tr):
    # version 1: the offsets of ALL levels as their own launch on a side stream, forked BEFORE the last feature launch: they
    # need the mask stream (a serial host job of ~70 ms that ends about now), the features do not, and a coder launch keeps few
    # SIMDs busy (one wave per stream), so the two launches run side by side instead of the last one waiting for the masks
    if not last:
        return
    main, side_stream = torch.cuda.current_stream(), _side_stream(dev)
    with torch.cuda.stream(side_stream):
        side_stream.wait_event(st.fork)
        tr("waiting for the mask stream")
        st.masks = _masks_from_host_job(st, dev)
        tr("mask stream decoded")
        og, fills = _offset_groups(st, st.pending_offsets, _live_slots)
        _place_offsets(st, fills, codec.gaussian_decode_groups(og, lanes=st.layout.lanes))
        tr("offsets launch enqueued")
    main.wait_stream(side_stream)


# submit_masks: before the checkpoint is read, launch_masks: after it; level_offsets: in front of a level's launch -> (groups to
# add to it, where their values go), offsets_launch: behind it
_DecodeStages = namedtuple("_DecodeStages", "submit_masks launch_masks anchors hyper offset_edges_ahead level_offsets offsets_launch "
                           "masks_joined status_check")
_DECODE_V1 = _DecodeStages(_submit_mask_job, _skip, _anchors_from_npy, _decode_hyper_rans, _skip, _fork_before_the_last_level,
                           _launch_offsets_beside_the_last_level, _masks_of_a_model_without_levels, _skip)
_DECODE_V2 = _DecodeStages(_skip, _launch_masks, _anchors_from_npy, _decode_hyper_lanes, _read_offset_edges_ahead,
                           _offsets_ride_with_their_level, _skip, _join_mask_launch, codec.decode_status_check)
_DECODE = {1: _DECODE_V1, 2: _DECODE_V2, 3: _DECODE_V2._replace(anchors=_anchors_from_anchor_b)}


def _decode_level(pc, st, stages, level, orig, last, dev, tr):
    # One level: predict, ONE coder launch for its features and scaling (and whatever offsets the container version lets ride
    # along), place the decoded rows, gather the next level's context.  Coder launches last as long as their LONGEST stream (a
    # 1000-anchor feature chunk: 50 000 serial symbols at ~0.4 us each) however many streams they hold, so the fewer the better:
    # version 1 codes the offsets of all levels in ONE more launch beside the last level's — 3 serial launches for 3 levels.
    n_l, D, layout = int(orig.shape[0]), st.D, st.layout
    (mean_feat, scale_feat, mean_scaling, scale_scaling, mean_offsets, scale_offsets, Qf, Qs, Qo) = \
        _predict_level(pc, st, level, orig, tr, mark_rows=True)
    st.pending_offsets.append((level, orig, n_l, mean_offsets, scale_offsets, Qo))
    groups = [_decode_group(st, "feat", level, mean_feat, scale_feat, Qf, layout.group_edges(n_l, D, D), D),
              _decode_group(st, "scaling", level, mean_scaling, scale_scaling, Qs, layout.group_edges(n_l, 6, D), 6)]
    offset_groups, fills = stages.level_offsets(st, last)
    decoded = codec.gaussian_decode_groups(groups + offset_groups, lanes=layout.lanes)
    tr(f"level {level}: coder launch enqueued")
    _place_offsets(st, fills, decoded[2:])
    stages.offsets_launch(st, last, dev, tr)
    tr(f"level {level}: offsets placed")
    st.feat_after_Q[orig] = decoded[0].view(n_l, D)
    st.scaling_after_Q[orig] = decoded[1].view(n_l, 6)
    tr(f"level {level}: decoded rows placed")
    if level != 0:
        st.already_coded.index_fill_(0, orig, True)    # (x[idx] = True uploads its scalar through a blocking pageable copy)
        _gather_next_context(pc, st, level, tr)


def _install_decoded(pc, st, N_valid, dev):
    # The decoded rows in front of zeroed rows for the anchors that were not valid (:1503-1533).
    rows = {"_hyper_latent": st.hyper, "_anchor": st.anchors, "_anchor_feat": st.feat_after_Q, "_offset": st.offsets_after_Q,
            "_scaling": st.scaling_after_Q, "_mask": st.masks}
    full = {name: torch.zeros(st.meta.n_anchors, *r.shape[1:], device=dev) for name, r in rows.items()}
    for name in ("_anchor", "_hyper_latent", "_anchor_feat", "_offset", "_scaling", "_mask"):
        full[name][:N_valid] = rows[name]
    for name, t in full.items():
        setattr(pc, name, nn.Parameter(t))
    pc.decoded_version = True
    if hasattr(pc, "_level_cache"):
        pc._level_cache = None
    pc._anchor_q_cache = None


@torch.no_grad()
def conduct_decoding(pc, pre_path_name):                       # :1299-1539
    torch.cuda.synchronize(); t1 = time.time()
    tr = _tracer("decode")
    print("Start decoding ...")
    # anchor.npy (12 MB at 1 M anchors) is read and converted on a host thread while this one loads the header, the MLPs and
    # the prior tables: the level plan — the first thing the device chain waits for — needs nothing else from the files.
    # (Submitted before the header says which container this is: a version-3 directory has no such file.)
    anchor_job = codec.host_pool().submit(_read_anchor_npy, os.path.join(pre_path_name, "anchor.npy"))
    meta = _unpack_meta(read_mlp_checkpoint(os.path.join(pre_path_name, "meta.b")))   # (the same loader: lists / dicts of numbers, arrays)
    tr("meta.b unpickled")
    layout = ContainerLayout.from_header(meta)
    stages = _DECODE[layout.version]
    st = _Coding(layout, pre_path_name, pc, meta=meta, anchor_job=anchor_job)
    dev = pc.x_bound_min.device
    _stage_files(st, dev, tr)
    n_levels = list(reversed(meta.n_levels))
    N_valid = sum(n_levels)
    stages.submit_masks(st, N_valid, dev, tr)
    # mlp.pt gates everything below (bounds -> anchors -> level plan; prior tables -> hyper launch) and unpickling it is the
    # longest host step of the prologue (on a host thread it only moved the time: unpickling holds the GIL), so it is read on
    # THIS thread, before the other files' reads are released
    ck = read_mlp_checkpoint(st.path("mlp.pt"))
    tr("mlp.pt unpickled")
    st.staged.release()
    stages.launch_masks(st, N_valid, dev, tr)
    load_mlp_checkpoints(pc, st.path("mlp.pt"), ck=ck, tr=tr, stored_tables=layout.device_coders)   # (incl. the hyper prior's CDF tables)
    # the level plan (sorts and compactions: milliseconds of device work) needs the anchors and the checkpoint's bounds only:
    # queued now, it runs while the host goes on with the hyper launch
    q = stages.anchors(st, N_valid, dev, tr)
    st.anchors = q * ((pc.x_bound_max - pc.x_bound_min) * Q_anchor + 1e-6) + pc.x_bound_min
    tr("anchors on the device")
    plan = _plan_levels(pc, st, tr)
    st.hyper = stages.hyper(pc, st, N_valid, tr)                                         # [N_valid, H]
    tr("hyper latents decoded (host rANS) and on the device")

    st.feat_after_Q = torch.zeros(N_valid, st.D, device=dev)
    st.scaling_after_Q = torch.zeros(N_valid, 6, device=dev)
    st.offsets_after_Q = torch.zeros(N_valid, st.K, 3, device=dev)
    st.already_coded = torch.zeros(N_valid, dtype=torch.bool, device=dev)
    stages.offset_edges_ahead(st, plan, tr)
    for (level, _to_code, orig, _hybrid_anchor) in plan:
        assert int(orig.shape[0]) == n_levels[level]
        _decode_level(pc, st, stages, level, orig, level == plan[-1][0], dev, tr)
    stages.masks_joined(st, dev)
    tr("levels enqueued")
    torch.cuda.synchronize(); t2 = time.time()
    tr("device done")
    stages.status_check(dev)                     # (after the synchronize: no extra wait)
    print("decoding time:", t2 - t1)
    _install_decoded(pc, st, N_valid, dev)
    return f"\nDecTime {round(t2 - t1, 4)}"
