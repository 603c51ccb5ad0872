"""Anchor position code of container version 3, without a GPU: the C-ABI exports its entry points, the numpy restatement
(tests/anchor_code_ref.py) round-trips its own arrays on the edge sets, its ideal code length matches the figures the scheme
was proposed with, and the host-side header validation of codec.anchor_decode refuses malformed streams."""
import os
import re

import numpy as np
import pytest

import anchor_code_ref as acr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["cgs_anchor_order", "cgs_anchor_order_scratch_bytes", "cgs_anchor_pack", "cgs_anchor_pack_slot_bytes",
               "cgs_anchor_unpack"]


def test_anchor_entry_points_are_declared_and_exported():
    from contextgs_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cgs.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cgs_[a-z0-9_]+)\s*\(", src))
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/cgs.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
    # size queries are host functions: a block of B anchors holds B - 1 mantissas of at most 47 bits
    for B in (64, 1024, 4096):
        assert lib.cgs_anchor_pack_slot_bytes(B) >= ((B - 1) * 47 + 7) // 8
        assert lib.cgs_anchor_pack_slot_bytes(B) % 16 == 0
    assert lib.cgs_anchor_order_scratch_bytes(1 << 20) >= 8 * 4 * (1 << 20)
    # argument errors come back as return codes
    assert lib.cgs_anchor_pack(None, 10, 32, None, None, None, None, None, None) != 0
    assert lib.cgs_anchor_unpack(None, 10, 8192, None, None, None, None, None, None) != 0
    assert lib.cgs_anchor_order(None, -1, None, None, None, None, 0, None) != 0


def test_keys_follow_the_bit_layout():
    q = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0x8000, 0, 0], [65535, 65535, 65535], [2, 0, 0]], dtype=np.int64)
    assert acr.keys_of(q).tolist() == [4, 2, 1, 1 << 47, (1 << 48) - 1, 4 << 3]
    assert np.array_equal(acr.positions_of(acr.keys_of(q)), q)


@pytest.mark.parametrize("name", sorted(acr.edge_sets()))
@pytest.mark.parametrize("B", [64, 1024])
def test_reference_round_trips_its_own_arrays(name, B):
    q = acr.edge_sets()[name]
    order, blk = acr.encode(q, B)
    key = acr.keys_of(q)
    assert np.array_equal(np.sort(order), np.arange(q.shape[0]))
    ks = key[order]
    assert np.all(ks[1:] >= ks[:-1])
    same = ks[1:] == ks[:-1]
    assert np.all(order[1:][same] > order[:-1][same])            # stable: equal keys keep their input order
    assert blk["classes"].shape[0] == q.shape[0] - blk["first"].shape[0]
    if blk["classes"].size:
        assert 0 <= blk["classes"].min() and blk["classes"].max() <= 48
        assert np.all(blk["mantissas"] < (np.uint64(1) << np.maximum(blk["classes"] - 1, 0).astype(np.uint64)))
    assert np.array_equal(acr.keys_from_blocks(blk), ks)
    assert np.array_equal(acr.decode(blk), q[order])


def test_edge_sets_hit_the_cases_they_are_named_for():
    sets = acr.edge_sets()
    k = acr.keys_of(sets["high_bits_only"])
    assert np.all(k & np.uint64(0xFFFFFF) == 0) and np.unique(k >> np.uint64(24)).size > 1000
    k = acr.keys_of(sets["low_bits_only"])
    assert np.unique(k >> np.uint64(24)).size == 1 and np.unique(k).size > 1000
    _, blk = acr.encode(sets["all_identical"])
    assert set(blk["classes"].tolist()) == {0}
    _, blk = acr.encode(sets["two_corners"])
    assert blk["classes"].tolist() == [48] and int(blk["mantissas"][0]) == (1 << 47) - 1
    _, blk = acr.encode(sets["gap_at_block_boundary"])
    assert blk["first"].tolist() == [int(acr.keys_of(np.array([[3, 3, 3]]))[0]), (1 << 48) - 1]
    assert set(blk["classes"].tolist()) == {0}                   # the largest gap is a block's first key: not coded
    d = sets["duplicates"]
    assert 0.25 < 1 - np.unique(d, axis=0).shape[0] / d.shape[0] < 0.4
    assert np.array_equal(acr.order_of(acr.keys_of(sets["sorted"])), np.arange(1500))


def test_ideal_length_matches_the_proposal():
    """Bytes per anchor of the ideal code at N = 100 000: 4.12 uniform, 3.36 on three thin shells (and the information bound
    (48 - log2 N + 1.44) / 8 for the uniform set, within 1 %)."""
    N = 100_000
    _, blk = acr.encode(acr.uniform(N, 1))
    per = acr.ideal_bits(blk) / 8 / N
    assert abs(per - 4.12) < 0.03
    assert abs(per / ((48 - np.log2(N) + 1.44) / 8) - 1) < 0.01
    _, blk = acr.encode(acr.shells(N, 1))
    assert abs(acr.ideal_bits(blk) / 8 / N - 3.36) < 0.08
    assert int(acr.mantissa_bytes(blk).sum()) * 8 >= int(np.maximum(blk["classes"] - 1, 0).sum())


def _host_stream(q, B=1024, cls_block=32768):
    """A stream with a valid header for q (placeholder class stream: the host validation never looks inside the payload)."""
    from contextgs_amd import codec
    _, blk = acr.encode(q, B)
    nb = blk["first"].shape[0]
    n_cls = q.shape[0] - nb
    ncb = -(-n_cls // cls_block)
    cdf = codec._anchor_cdf(np.bincount(blk["classes"], minlength=49))
    mant_len = acr.mantissa_bytes(blk)
    cls_len = np.full(ncb, 200, dtype=np.int64)
    first = np.ascontiguousarray(blk["first"].astype("<u8").view(np.uint8).reshape(nb, 8)[:, :6])
    head = (np.array([codec._ANCHOR_MAGIC, q.shape[0], B, cls_block], dtype="<u4").tobytes() + cdf.astype("<u4").tobytes()
            + first.tobytes() + mant_len.astype("<u2").tobytes() + cls_len.astype("<u4").tobytes())
    return head + bytes(int(cls_len.sum()) + int(mant_len.sum())), len(head), nb


def test_class_cdf_totals_2_16_and_keeps_every_class_that_occurs():
    from contextgs_amd import codec
    for hist in ([0] * 49, [5] + [0] * 48, [0] * 48 + [1], [10 ** 9, 1] + [0] * 46 + [1], list(range(49)), [1] * 49):
        cdf = codec._anchor_cdf(np.array(hist))
        assert cdf[0] == 0 and cdf[-1] == 1 << 16 and np.all(np.diff(cdf) >= 0)
        assert np.all(np.diff(cdf)[np.array(hist) > 0] >= 1)
        assert np.all(np.diff(cdf)[np.array(hist) == 0] == 0) or sum(hist) == 0


def test_header_validation_on_the_host():
    from contextgs_amd import codec
    stream, hdr, nb = _host_stream(acr.uniform(3000, 3))
    h = codec._anchor_header(stream, len(stream))
    assert (h["N"], h["B"], h["n_blocks"], h["header_bytes"]) == (3000, 1024, 3, hdr)
    _, blk = acr.encode(acr.uniform(3000, 3))
    assert np.array_equal(h["first_key"], blk["first"])

    def refused(buf, match):
        with pytest.raises(RuntimeError, match=match):
            codec._anchor_header(bytes(buf), len(buf))

    refused(stream[:-1], "do not add up")
    refused(stream + b"\0", "do not add up")
    b = bytearray(stream); b[0] ^= 1
    refused(b, "magic")
    b = bytearray(stream); b[codec._ANCHOR_FIXED + nb * 6] += 1           # a mantissa-length entry raised by one
    refused(b, "do not add up")
    for bad_B in (32, 8192):
        b = bytearray(stream); b[8:12] = np.array([bad_B], dtype="<u4").tobytes()
        refused(b, "block size")
    b = bytearray(stream); b[16 + 4 * 49:16 + 4 * 50] = np.array([65535], dtype="<u4").tobytes()
    refused(b, "CDF")
    b = bytearray(stream); b[16 + 4 * 3:16 + 4 * 4] = np.array([70000], dtype="<u4").tobytes()
    refused(b, "CDF")
    refused(stream[:100], "shorter")
