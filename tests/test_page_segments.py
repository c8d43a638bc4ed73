"""Segmented pages without a GPU: the geometry predicate
(csrc/core/page_codec.h, `segments_legal`) over its rule table, the packed
wire framing with and without the segment extension (csrc/core/protocol.h),
and the refusals the Python layers raise before anything is sent. What needs a
GPU tensor (write_pages / read_pages themselves) is in
tests/test_gpu_segments.py."""

import struct

import numpy as np
import pytest
import torch

from infinistore_amd import _native
from infinistore_amd.lib import InfinityConnection, ClientConfig, TYPE_RDMA
from infinistore_amd.vllm_adapter import InfiniStoreKVAdapter

NONE, FP8, MXFP4 = 0, 1, 2  # codec ids (PageCodec)
CODECS = [NONE, FP8, MXFP4]
SEG_MULTIPLE = {NONE: 1, FP8: 16, MXFP4: 64}  # bytes a segment is a multiple of
MAX_SEG = 1024
legal = _native._dbg_segments_legal


def test_constants_agree():
    assert _native._MAX_PAGE_SEGMENTS == MAX_SEG == InfinityConnection.MAX_PAGE_SEGMENTS
    rows = _native._page_codec_rows()
    # a segment obeys the codec's own page multiple (bf16 elements -> bytes)
    assert [2 * r[2] if r[1] else 1 for r in rows] == [SEG_MULTIPLE[c] for c in CODECS]


# --- segments_legal: each rule, just legal and just illegal, per codec -------
@pytest.mark.parametrize("codec", CODECS)
def test_segment_count_bounds(codec):
    seg = 64
    assert not legal(codec, seg * 2, 0, seg)
    assert legal(codec, seg, 1, 0)
    assert legal(codec, seg * 2, 2, seg)
    assert legal(codec, seg * MAX_SEG, MAX_SEG, seg)
    assert not legal(codec, seg * (MAX_SEG + 1), MAX_SEG + 1, seg)


@pytest.mark.parametrize("codec", CODECS)
def test_page_divides_into_segments(codec):
    assert legal(codec, 192, 3, 64)
    assert not legal(codec, 192 + 64, 3, 128)  # 256 % 3 != 0
    assert not legal(codec, 193, 3, 128)


@pytest.mark.parametrize("codec", CODECS)
def test_segments_never_overlap(codec):
    assert legal(codec, 256, 2, 128)  # stride == segment: the contiguous page
    assert not legal(codec, 256, 2, 112)  # 16-byte multiple, one step short
    assert not legal(codec, 256, 2, 0)
    # one segment is the contiguous page: the stride is not looked at
    assert legal(codec, 256, 1, 0) and legal(codec, 256, 1, 7)


@pytest.mark.parametrize("codec", [FP8, MXFP4])
def test_transforming_codecs_segment_size(codec):
    m = SEG_MULTIPLE[codec]
    for s in (2, 3):
        assert legal(codec, s * m, s, m)
        assert legal(codec, s * 2 * m, s, 2 * m + 16)
        # half a lane unit short of / past a whole number of groups
        assert not legal(codec, s * (m - 8), s, 1024)
        assert not legal(codec, s * (m + 8), s, 1024)
    if codec == MXFP4:  # 32 bytes: fine for fp8, half a group for mxfp4
        assert legal(FP8, 64, 2, 32) and not legal(MXFP4, 64, 2, 32)
        assert not legal(MXFP4, 2 * 48, 2, 64)


@pytest.mark.parametrize("codec", [FP8, MXFP4])
def test_transforming_codecs_stride_alignment(codec):
    m = SEG_MULTIPLE[codec]
    assert legal(codec, 2 * m, 2, m + 16)
    for off in (1, 2, 8, 15):
        assert not legal(codec, 2 * m, 2, m + off)
        assert not legal(codec, 2 * m, 2, m + 16 + off)


def test_plain_takes_any_segment_and_stride():
    assert legal(NONE, 2, 2, 1)
    assert legal(NONE, 3 * 513, 3, 516)
    assert legal(NONE, 2 * 17, 2, 17 + 3)
    assert legal(NONE, 2 * 16, 2, 16 + 1)


def test_unknown_codec_id():
    with pytest.raises(ValueError):
        legal(3, 64, 2, 32)


# --- packed framing ----------------------------------------------------------
IPC = bytes(range(64))
HDR = 104
FLAG_SYNC, FLAG_FP8, FLAG_MXFP4, FLAG_SEG = 1, 2, 4, 8


def _build(keys, offsets, block_size=256, flags=0, **kw):
    return _native._dbg_build_packed_local(3, 1234, 0x7000_0000_0000, 4096, block_size, flags,
                                           17, IPC, offsets, keys, **kw)


def test_contiguous_body_is_todays_bytes():
    keys, offs = ["alpha", "b", "gamma-3"], [0, 256, 1 << 33]
    body = _build(keys, offs, flags=FLAG_SYNC)
    want = struct.pack("<iiQQIIII", 3, 1234, 0x7000_0000_0000, 4096, 256, 3, FLAG_SYNC, 17)
    want += IPC + struct.pack("<3Q", *offs) + b"alpha\0b\0gamma-3"
    assert body == want
    # n_segments == 1, with any stride, is byte-identical: no flag, no extension
    assert _build(keys, offs, flags=FLAG_SYNC, n_segments=1, segment_stride=0) == want
    assert _build(keys, offs, flags=FLAG_SYNC, n_segments=1, segment_stride=4096) == want
    for op in ("w", "r"):
        got = _native._dbg_parse_packed_local(op, body)
        assert got["keys"] == keys and got["offsets"] == offs
        assert (got["n_segments"], got["segment_stride"]) == (1, 0)
        assert got["flags"] == FLAG_SYNC and got["alloc_mb"] == 17
        assert (got["device"], got["pid"], got["block_size"]) == (3, 1234, 256)
        assert (got["base_ptr"], got["base_offset"]) == (0x7000_0000_0000, 4096)


def test_extension_present_iff_flag():
    keys, offs = ["k0", "k1"], [0, 128]
    plain = _build(keys, offs)
    seg = _build(keys, offs, n_segments=2, segment_stride=1 << 20)
    assert len(seg) == len(plain) + 16
    flags = struct.unpack_from("<I", seg, 32)[0]
    assert flags & FLAG_SEG and not struct.unpack_from("<I", plain, 32)[0] & FLAG_SEG
    assert seg[HDR:HDR + 16] == struct.pack("<IIQ", 2, 0, 1 << 20)
    assert seg[HDR + 16:] == plain[HDR:]  # offsets and keys follow unchanged
    assert seg[:32] == plain[:32] and seg[36:HDR] == plain[36:HDR]
    for op in ("w", "r"):
        got = _native._dbg_parse_packed_local(op, seg)
        assert (got["n_segments"], got["segment_stride"]) == (2, 1 << 20)
        assert got["keys"] == keys and got["offsets"] == offs


def _seg_body(n_segments, stride, rsvd=0, block_size=256, flags=0):
    body = bytearray(_build(["k"], [0], block_size=block_size, flags=flags,
                            n_segments=2, segment_stride=4096))
    body[HDR:HDR + 16] = struct.pack("<IIQ", n_segments, rsvd, stride)
    return bytes(body)


def _refused(op, body):
    with pytest.raises(ValueError, match="INVALID_REQ"):
        _native._dbg_parse_packed_local(op, body)


@pytest.mark.parametrize("op", ["w", "r"])
def test_parse_refusals(op):
    good = _seg_body(2, 4096)
    assert _native._dbg_parse_packed_local(op, good)["n_segments"] == 2
    for cut in (HDR, HDR + 1, HDR + 8, HDR + 15):  # truncated inside the extension
        _refused(op, good[:cut])
    _refused(op, good[:HDR + 16 + 7])  # extension whole, offsets cut
    _refused(op, _seg_body(0, 4096))
    assert _native._dbg_parse_packed_local(op, _seg_body(MAX_SEG, 4096, block_size=2048))
    _refused(op, _seg_body(MAX_SEG + 1, 4096, block_size=2050))
    _refused(op, _seg_body(2, 4096, rsvd=1))
    _refused(op, _seg_body(3, 4096))  # 256 % 3
    _refused(op, _seg_body(2, 127))  # overlap
    # flag set but no room for the extension at all
    hdr_only = bytearray(_build([], []))
    struct.pack_into("<I", hdr_only, 32, FLAG_SEG)
    _refused(op, bytes(hdr_only))


def test_parse_applies_the_request_codec_on_write_only():
    # 32-byte segments with an 8-byte-misaligned stride: legal for plain pages
    body = _seg_body(2, 40, block_size=64)
    assert _native._dbg_parse_packed_local("w", body)["segment_stride"] == 40
    for flag in (FLAG_FP8, FLAG_MXFP4):
        bad = _seg_body(2, 72, block_size=128, flags=flag)  # stride % 16
        _refused("w", bad)
        # a read carries no codec: the server checks each entry's own
        assert _native._dbg_parse_packed_local("r", bad)["n_segments"] == 2
    _refused("w", _seg_body(2, 64, block_size=64, flags=FLAG_MXFP4))  # 32-byte segments
    assert _native._dbg_parse_packed_local("w", _seg_body(2, 64, block_size=64, flags=FLAG_FP8))
    _refused("w", _seg_body(2, 4096, flags=FLAG_FP8 | FLAG_MXFP4))


# --- Python refusals, before anything is sent --------------------------------
check = InfinityConnection._check_segments


def test_check_segments_accepts_the_legal():
    check(4096, 2, [0, 64], 128, 1, 0)  # contiguous: nothing looked at
    check(4096, 2, [0, 64], 128, 2, 2048)
    check(4096, 2, np.array([0, 64], dtype=np.uint64), 128, 2, 2048, "fp8")
    check(4096, 2, [0, 64], 128, 2, 2048, "mxfp4")
    check(4096, 2, [4096 - 2048 - 64], 128, 2, 2048)  # ends exactly at numel
    check(4096, 1, [0], 3 * 513, 3, 516)
    check(4096, 2, [0], 16, 2, 64, "fp8")  # 8-element segments
    check(4096, 2, [0], 64, 2, 64, "mxfp4")  # 32-element segments


@pytest.mark.parametrize("args", [
    (4096, 2, [0], 128, 0, 64),  # no segments
    (1 << 22, 2, [0], 2 * 1025, 1025, 2),  # too many
    (4096, 2, [0], 128, 3, 64),  # does not divide
    (4096, 2, [0], 128, 2, 63),  # overlap
    (4096, 2, [0], 128, 2, 0),
    (4096, 2, [0], 24, 2, 64, "fp8"),  # 12-element segments
    (4096, 2, [0], 64, 4, 64, "mxfp4"),  # 16-element segments
    (4096, 2, [0], 128, 2, 68, "fp8"),  # stride 136 bytes
    (4096, 2, [0], 128, 2, 68, "mxfp4"),
    (4096, 2, [4096 - 2048 - 64 + 1], 128, 2, 2048),  # one element past numel
    (4096, 2, [0, 1985], 128, 2, 2048),
])
def test_check_segments_refuses(args):
    with pytest.raises(ValueError):
        check(*args)


class _NoTraffic:
    """Stands in for the native connection: any use is a test failure."""

    def __getattr__(self, name):
        raise AssertionError(f"connection used: {name}")


def _fabric_conn():
    c = InfinityConnection(ClientConfig(host_addr="127.0.0.1", service_port=1,
                                        connection_type=TYPE_RDMA))
    c.conn = _NoTraffic()
    c.rdma_connected = True  # as after connect() on the fabric path
    return c


def test_segments_on_a_fabric_connection_are_refused():
    c = _fabric_conn()
    t = torch.zeros(4096, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="local"):
        c.write_pages(t, ["k"], [0], 128, segments=2, segment_stride=2048)
    with pytest.raises(ValueError, match="local"):
        c.read_pages(t, ["k"], [0], 128, segments=2, segment_stride=2048)
    with pytest.raises(ValueError, match="local"):
        c.read_pages_async(t, ["k"], [0], 128, segments=2, segment_stride=2048)


def test_kv_major_needs_the_local_path():
    # refused at construction, before any connection is made (port 1)
    with pytest.raises(ValueError, match="kv_major"):
        InfiniStoreKVAdapter("127.0.0.1", 1, "m", 2, 16, 4096, local=False,
                             kv_layout="kv_major")
    with pytest.raises(ValueError, match="kv_layout"):
        InfiniStoreKVAdapter("127.0.0.1", 1, "m", 2, 16, 4096, kv_layout="kv-major")
