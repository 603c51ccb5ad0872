"""numpy restatement of the anchor position code of container version 3 (a helper, not a test).

Written from the format's definition, not from the kernels:
  1. key: 48-bit Morton key of a grid index (qx, qy, qz), each in [0, 65535]: bit b of qx -> key bit 3b+2, of qy -> 3b+1, of
     qz -> 3b;
  2. order: the stable ascending sort of the keys;
  3. blocks of B sorted keys: the first key raw (48 bits), every other key as the gap d >= 0 to its predecessor, sent as the class
     c = bit length of d (0 for d = 0; 0..48) and the c - 1 low bits of d (the top bit is implied by the class);
and the ideal code length of that scheme: -sum log2 p(class) over the gap classes (empirical distribution of the whole stream)
+ sum max(c - 1, 0) + 48 per block.
"""
import numpy as np

B_DEFAULT = 1024


def keys_of(q):
    q = np.asarray(q).astype(np.uint64).reshape(-1, 3)
    key = np.zeros(q.shape[0], dtype=np.uint64)
    for b in range(16):
        for col, shift in ((0, 2), (1, 1), (2, 0)):
            key |= ((q[:, col] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + shift)
    return key


def positions_of(key):
    key = np.asarray(key, dtype=np.uint64)
    q = np.zeros((key.shape[0], 3), dtype=np.int64)
    for b in range(16):
        for col, shift in ((0, 2), (1, 1), (2, 0)):
            q[:, col] |= (((key >> np.uint64(3 * b + shift)) & np.uint64(1)) << np.uint64(b)).astype(np.int64)
    return q


def order_of(key):
    return np.argsort(np.asarray(key, dtype=np.uint64), kind="stable")


def bit_length(d):
    """Bit length of every uint64 in d (0 for 0), exact (no floating point)."""
    d = np.asarray(d, dtype=np.uint64)
    c = np.zeros(d.shape, dtype=np.int64)
    for b in range(64):
        c[(d >> np.uint64(b)) != 0] = b + 1
    return c


def blocks_of(sorted_keys, B=B_DEFAULT):
    """-> dict(first uint64 [n_blocks], classes int64 [N - n_blocks] block after block, mantissas uint64 (same shape),
    block_of int64 (same shape: the block each gap belongs to))."""
    k = np.asarray(sorted_keys, dtype=np.uint64)
    N = k.shape[0]
    starts = np.arange(0, N, B)
    first = k[starts]
    is_gap = np.ones(N, dtype=bool)
    is_gap[starts] = False
    d = np.zeros(N, dtype=np.uint64)
    d[1:] = k[1:] - k[:-1]
    d = d[is_gap]
    c = bit_length(d)
    low = np.where(c > 1, np.uint64(1) << np.maximum(c - 1, 0).astype(np.uint64), np.uint64(1)) - np.uint64(1)
    return {"N": N, "B": B, "first": first, "classes": c, "mantissas": d & low, "block_of": (np.arange(N) // B)[is_gap]}


def keys_from_blocks(blk):
    """Inverse of blocks_of."""
    N, B = blk["N"], blk["B"]
    c, m = blk["classes"], blk["mantissas"]
    d = np.where(c > 0, (np.uint64(1) << np.maximum(c - 1, 0).astype(np.uint64)) | m, np.uint64(0)).astype(np.uint64)
    keys = np.zeros(N, dtype=np.uint64)
    starts = np.arange(0, N, B)
    is_gap = np.ones(N, dtype=bool)
    is_gap[starts] = False
    keys[is_gap] = d
    for s in starts:                               # a running sum per block on top of its first key
        e = min(N, s + B)
        keys[s] = blk["first"][s // B]
        keys[s:e] = np.cumsum(keys[s:e], dtype=np.uint64)
    return keys


def mantissa_bytes(blk):
    """Bytes of every block's bit-packed mantissas (LSB first, each block from a byte boundary) -> int64 [n_blocks]."""
    nb = blk["first"].shape[0]
    bits = np.zeros(nb, dtype=np.int64)
    np.add.at(bits, blk["block_of"], np.maximum(blk["classes"] - 1, 0))
    return (bits + 7) // 8


def ideal_bits(blk):
    c = blk["classes"]
    total = float(np.maximum(c - 1, 0).sum()) + 48.0 * blk["first"].shape[0]
    if c.size:
        cnt = np.bincount(c, minlength=49).astype(np.float64)
        p = cnt[cnt > 0] / c.size
        total += float(-(cnt[cnt > 0] * np.log2(p)).sum())
    return total


def encode(q, B=B_DEFAULT):
    """q [N, 3] -> (order, blocks dict)."""
    key = keys_of(q)
    order = order_of(key)
    return order, blocks_of(key[order], B)


def decode(blk):
    return positions_of(keys_from_blocks(blk))


# ---- point sets -------------------------------------------------------------------------------------------------------
def uniform(n, seed):
    return np.random.default_rng(seed).integers(0, 65536, size=(n, 3), dtype=np.int64)


def shells(n, seed):
    """Three thin spherical shells: radii 0.2, 0.35 and 0.5 of the half-extent, relative radial jitter 0.002."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    r = np.array([0.2, 0.35, 0.5])[rng.integers(0, 3, n)] * (1.0 + 0.002 * rng.normal(size=n))
    half = 32768.0
    return np.clip(np.floor(half + half * r[:, None] * v), 0, 65535).astype(np.int64)


def edge_sets():
    """name -> int64 [N, 3]: the sets the order and the round trip are checked on."""
    sets = {f"uniform{n}": uniform(n, 100 + n) for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)}
    rng = np.random.default_rng(7)
    # keys that differ only in their high 24 bits (index bits 8..15) / only in their low 24 bits (index bits 0..7)
    sets["high_bits_only"] = rng.integers(0, 256, size=(1500, 3), dtype=np.int64) << 8
    sets["low_bits_only"] = rng.integers(0, 256, size=(1500, 3), dtype=np.int64) + (0x5A << 8)
    u = uniform(1500, 11)
    srt = u[order_of(keys_of(u))]
    sets["sorted"] = srt
    sets["reverse_sorted"] = srt[::-1].copy()
    d = uniform(2000, 12)
    dup = rng.random(2000) < 0.3
    d[dup] = d[rng.integers(0, 200, int(dup.sum()))]             # 30 % of the rows repeat one of the first 200
    sets["duplicates"] = d
    sets["all_identical"] = np.tile(np.array([[1234, 40000, 77]], dtype=np.int64), (1300, 1))
    sets["all_max"] = np.full((70, 3), 65535, dtype=np.int64)
    sets["two_corners"] = np.array([[0, 0, 0], [65535, 65535, 65535]], dtype=np.int64)
    far = np.tile(np.array([[3, 3, 3]], dtype=np.int64), (1025, 1))
    far[500] = (65535, 65535, 65535)                             # sorts last: the first key of the second block, never a gap
    sets["gap_at_block_boundary"] = far
    sets["empty"] = np.zeros((0, 3), dtype=np.int64)
    return sets
