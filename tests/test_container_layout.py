"""codec_driver.ContainerLayout and the named header (no device): the cut the encoder and the decoder must agree on —
block sizes per policy, stream edges, the staged files and their order, what a header reads as."""
import pytest
import torch

from contextgs_amd import codec_driver as cd


def _layout(version, policy=2, **kw):
    return cd.ContainerLayout.for_writing(version)._replace(policy=policy, **kw)


# block sizes of the groups of 50 n / 6 n / 17 n symbols in a level of n anchors, with the shipped constants
# (32 768 halving to 8 192): worked out from the policies' definitions, not read off the code
BLOCKS = {700_000: {0: (32768, 32768, 32768), 1: (32768, 8192, 8192), 2: (32768, 32768, 32768)},
          100_000: {0: (32768, 32768, 32768), 1: (8192, 8192, 8192), 2: (16384, 16384, 16384)},
          20_000: {0: (32768, 32768, 32768), 1: (8192, 8192, 8192), 2: (8192, 8192, 8192)}}


@pytest.mark.parametrize("n", sorted(BLOCKS))
@pytest.mark.parametrize("policy", [0, 1, 2])
def test_block_sizes_per_policy(n, policy):
    assert (cd.V2_BLOCK, cd.V2_BLOCK_MIN) == (32768, 8192)
    layout = _layout(2, policy)
    assert tuple(layout.block_symbols(n, n * w, 50) for w in (50, 6, 17)) == BLOCKS[n][policy]
    # the edges are that size's multiples and the group's end
    for w in (50, 6, 17):
        B = layout.block_symbols(n, n * w, 50)
        e = (layout.group_edges(n, w, 50) if w != 17 else layout.offset_edges(n, 50, n * w)).tolist()
        assert e == list(range(0, n * w, B)) + [n * w]


def test_constants_are_read_when_the_layout_is_built(monkeypatch):
    monkeypatch.setattr(cd, "V2_BLOCK", 4096)
    monkeypatch.setattr(cd, "V2_BLOCK_MIN", 512)
    monkeypatch.setattr(cd, "V2_BLOCK_POLICY", 1)
    monkeypatch.setattr(cd, "V2_HYPER_BLOCK", 640)
    layout = cd.ContainerLayout.for_writing(2)
    assert (layout.block, layout.block_min, layout.policy, layout.hyper_block) == (4096, 512, 1, 640)
    assert layout.block_symbols(10_000, 60_000, 50) == 512 and layout.block_symbols(10_000, 5_000_000, 50) == 4096


def test_version_1_edges():
    layout = cd.ContainerLayout.for_writing(1)
    assert not (layout.lanes or layout.device_coders or layout.anchors_coded)
    D = 50
    assert layout.group_edges(2500, D, D).tolist() == [0, 1000 * D, 2000 * D, 2500 * D]
    assert layout.group_edges(2500, 6, D).tolist() == [0, 6000, 12000, 15000]
    assert layout.group_edges(1000, 6, D).tolist() == [0, 6000]
    # offsets: a chunk stream holds the live slots of its 1000 anchor rows
    per_row = torch.arange(2500) % 31
    running = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(per_row, 0)])
    want = [0, int(per_row[:1000].sum()), int(per_row[:2000].sum()), int(per_row.sum())]
    assert layout.offset_edges(2500, D, running).tolist() == want
    assert layout.mask_edges(2500, 10).tolist() == [0, 25000]                   # ONE serial stream


@pytest.mark.parametrize("version", [1, 2, 3])
def test_edges_of_an_empty_group(version):
    layout = cd.ContainerLayout.for_writing(version)
    assert layout.group_edges(0, 50, 50).tolist() == [0]
    assert layout.offset_edges(0, 50, torch.zeros(1, dtype=torch.int64)).tolist() == [0]
    # a level whose masks are all off: anchors, but no offset symbol
    edges = layout.offset_edges(1500, 50, torch.zeros(1501, dtype=torch.int64)).tolist()
    assert edges == ([0] if layout.lanes else [0, 0, 0])
    if layout.lanes:
        assert layout.offset_edges(1500, 50, 0).tolist() == [0]
        assert layout.mask_edges(0, 10).tolist() == [0]


def test_mask_chunk_streams():
    layout = cd.ContainerLayout.for_writing(2)
    assert layout.mask_edges(2500, 10).tolist() == [0, 10000, 20000, 25000]
    assert layout.lanes and layout.device_coders and not layout.anchors_coded
    assert cd.ContainerLayout.for_writing(3).anchors_coded


def test_staged_files_in_order():
    streams = [f"{a}{l}.b" for l in (2, 1, 0) for a in ("feat", "scaling", "offsets")]
    assert cd.ContainerLayout.for_writing(1).staged_files(3) == (
        ["feat2.b", "scaling2.b", "feat1.b", "scaling1.b", "feat0.b", "scaling0.b", "offsets2.b", "offsets1.b", "offsets0.b"], 0)
    assert cd.ContainerLayout.for_writing(2).staged_files(3) == (["masks.b", "hyper.b"] + streams, 1)
    assert cd.ContainerLayout.for_writing(3).staged_files(3) == (["anchor.b", "masks.b", "hyper.b"] + streams, 2)


def _header(extra=None):
    items = [12000, 1000, {0: [-3]}, {0: [4]}, {0: [-1]}, {0: [2]}, {0: [-5]}, {0: [6]}, 0.37, [800, 808], {0: [64]}, {0: [32]},
             {0: [16]}, [7000, 2000, 1000]]
    return items + ([extra] if extra is not None else [])


def test_header_reads():
    v1 = cd.ContainerLayout.from_header(cd._unpack_meta(_header()))
    assert v1.version == 1 and v1.max_batch == v1.mask_chunk == 1000 and not v1.lanes
    assert v1 == cd.ContainerLayout.for_writing(1)._replace(policy=0)
    old = cd.ContainerLayout.from_header(cd._unpack_meta(_header({"version": 2, "block_symbols": 16384, "chunk": {"masks": 500},
                                                                  "bit_masks": [8]})))
    assert (old.version, old.block, old.policy, old.mask_chunk, old.hyper_block) == (2, 16384, 0, 500, cd.V2_HYPER_BLOCK)
    assert old.block_symbols(100, 5000, 50) == 16384
    new = cd.ContainerLayout.from_header(cd._unpack_meta(_header({"version": 3, "block_symbols": 32768, "block_policy": 2,
                                                                  "hyper_block": 4096, "chunk": {"masks": 1000}, "bit_masks": [8]})))
    assert (new.version, new.policy, new.hyper_block, new.anchors_coded) == (3, 2, 4096, True)
    with pytest.raises(RuntimeError, match=r"meta\.b: container version 4 is newer than this decoder \(1, 2, 3\)"):
        cd.ContainerLayout.from_header(cd._unpack_meta(_header({"version": 4})))
    with pytest.raises(ValueError, match=r"container version 4: 1 \(the reference's container\), 2 or 3"):
        cd.ContainerLayout.for_writing(4)


def test_header_names_and_round_trip():
    extra = {"version": 2, "block_symbols": 32768, "block_policy": 2, "hyper_block": 32768, "chunk": {"masks": 1000}, "bit_masks": [8]}
    for items in (_header(), _header(extra)):
        meta = cd._unpack_meta(items)
        assert (meta.n_anchors, meta.max_batch, meta.prob_masks, meta.bit_hyper, meta.n_levels) == (12000, 1000, 0.37, [800, 808],
                                                                                                   [7000, 2000, 1000])
        assert (meta.min_feat, meta.max_offsets, meta.bit_feat, meta.bit_offsets) == (items[2], items[7], items[10], items[12])
        back = cd._pack_meta(meta)
        assert type(back) is list and len(back) == len(items) and all(a is b for a, b in zip(back, items))
    assert cd._unpack_meta(_header()).extra is None and cd._unpack_meta(_header(extra)).extra is extra


def test_the_header_item_a_layout_writes_reads_back_as_that_layout():
    assert cd.ContainerLayout.for_writing(1).header_item(None, 0) is None
    for version in (2, 3):
        layout = cd.ContainerLayout.for_writing(version)
        item = layout.header_item([8, 16], 4321)
        assert item["version"] == version and item["bit_masks"] == [8, 16] and ("anchor" in item) == (version == 3)
        if version == 3:
            assert item["anchor"]["bytes"] == 4321 and item["anchor"]["scheme"] == "morton-gap"
        assert cd.ContainerLayout.from_header(cd._unpack_meta(_header(item))) == layout
