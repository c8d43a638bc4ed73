"""Sliced reads without a GPU: the geometry predicate (csrc/core/page_codec.h,
`slice_legal`) against an independent Python statement of its rules, the
packed wire framing with and without the slice extension
(csrc/core/protocol.h), the refusals the Python layers raise before anything
is sent, and plain sliced jobs through a CPU `Shard`.

The local path itself (OP_R_FAST through a server) needs a GPU on both ends:
a CPU-only server answers every packed op with SYSTEM_ERROR and the client
refuses CPU tensors. So the server-level cases (INVALID_REQ for a key written
with another page_size, KEY_NOT_FOUND with the destination untouched) are in
tests/test_gpu_slices.py, and what runs here is the CPU shard's own sliced
copy, the code a CPU pool would execute."""

import struct

import numpy as np
import pytest
import torch

import infinistore_amd
from infinistore_amd import _native, PageSlice
from infinistore_amd.lib import InfinityConnection, ClientConfig, TYPE_RDMA
from infinistore_amd.kv_connector import PagedKVConnector
from infinistore_amd.vllm_adapter import InfiniStoreKVAdapter

NONE, FP8, MXFP4 = 0, 1, 2  # codec ids (PageCodec)
CODECS = [NONE, FP8, MXFP4]
MULTIPLE = {NONE: 1, FP8: 16, MXFP4: 64}  # page_multiple, bytes
MAX_PIECES = 4096
MAX_SEG = 1024
U64 = (1 << 64) - 1


def legal(codec, n, page, offset, piece, stride, S=1, seg_stride=0):
    return _native._dbg_slice_legal(codec, (n, page, offset, piece, stride), S, seg_stride)


# --- the rules, stated independently (Python integers never overflow) --------
def segments_ok(codec, page, S, seg_stride):
    if not 1 <= S <= MAX_SEG or page % S:
        return False
    if S == 1:
        return True
    seg = page // S
    if seg == 0 or seg_stride < seg:
        return False
    if codec != NONE and (seg % MULTIPLE[codec] or seg_stride % 16):
        return False
    return True


def slice_ok(codec, n, page, offset, piece, stride, S=1, seg_stride=0):
    if not 1 <= n <= MAX_PIECES or piece <= 0:
        return False
    if n > 1 and stride < piece:
        return False
    span = (n - 1) * stride if n > 1 else 0  # the stride of one piece is ignored
    if offset + span + piece > page:
        return False
    m = MULTIPLE[codec]
    if codec != NONE:
        if page % m or offset % m or piece % m or (n > 1 and stride % m):
            return False
    if S != 1:
        if S < 1 or n % S:
            return False
        if not segments_ok(codec, n * piece, S, seg_stride):
            return False
    return True


def check(codec, *args, want=None):
    """Native and Python agree; `want`, when given, pins the answer too."""
    ref = slice_ok(codec, *args)
    assert legal(codec, *args) == ref, (codec, args, ref)
    if want is not None:
        assert ref == want, (codec, args)


def test_constants_agree():
    assert _native._MAX_SLICE_PIECES == MAX_PIECES == InfinityConnection.MAX_SLICE_PIECES
    assert infinistore_amd.PageSlice is PageSlice
    assert PageSlice(64, 0, 8) == (64, 0, 8, 0, 1)  # stride and count default


@pytest.mark.parametrize("codec", CODECS)
def test_exact_fit_and_one_over(codec):
    m = MULTIPLE[codec]
    piece, stride, n, off = 2 * m, 5 * m, 7, 3 * m
    end = off + (n - 1) * stride + piece
    page = -(-end // 64) * 64 + 64  # a legal page for every codec, with room
    check(codec, n, page, off, piece, stride, want=True)
    # ends exactly on the page's last byte
    off_fit = page - ((n - 1) * stride + piece)
    check(codec, n, page, off_fit, piece, stride, want=True)
    check(codec, n, page, off_fit + m, piece, stride, want=False)
    check(NONE, n, page, off_fit + 1, piece, stride, want=False)  # one byte over
    check(NONE, n, end, off, piece, stride, want=True)
    check(NONE, n, end - 1, off, piece, stride, want=False)
    # one piece as large as the page, and one byte larger
    check(NONE, 1, 256, 0, 256, 0, want=True)
    check(NONE, 1, 256, 0, 257, 0, want=False)
    check(NONE, 1, 256, 1, 256, 0, want=False)


@pytest.mark.parametrize("codec", CODECS)
def test_stride_against_piece(codec):
    m = MULTIPLE[codec]
    piece = 4 * m
    check(codec, 4, 64 * m, 0, piece, piece, want=True)  # stride == piece: contiguous
    check(NONE, 4, 64 * m, 0, piece, piece - 1, want=False)  # pieces would overlap
    check(codec, 4, 64 * m, 0, piece, piece - m, want=False)
    check(codec, 4, 64 * m, 0, piece, 0, want=False)
    # one piece: the stride is not looked at
    check(codec, 1, 64 * m, 0, piece, 0, want=True)
    check(codec, 1, 64 * m, 0, piece, 7, want=True)
    check(codec, 1, 64 * m, 0, piece, U64, want=True)


@pytest.mark.parametrize("codec", CODECS)
def test_piece_count_bounds(codec):
    m = MULTIPLE[codec]
    page = (MAX_PIECES + 1) * m
    check(codec, 0, page, 0, m, m, want=False)
    check(codec, 1, page, 0, m, m, want=True)
    check(codec, MAX_PIECES, page, 0, m, m, want=True)
    check(codec, MAX_PIECES + 1, page, 0, m, m, want=False)
    check(codec, 2, page, 0, 0, m, want=False)  # empty pieces


@pytest.mark.parametrize("codec", [FP8, MXFP4])
def test_codec_multiple_on_each_value(codec):
    m = MULTIPLE[codec]
    page, off, piece, stride = 64 * m, 2 * m, 2 * m, 6 * m
    check(codec, 4, page, off, piece, stride, want=True)
    for d in sorted({1, 2, 8, m // 2, m - 1}):
        check(codec, 4, page, off + d, piece, stride, want=False)
        check(codec, 4, page, off, piece + d, stride, want=False)
        check(codec, 4, page, off, piece, stride + d, want=False)
        check(NONE, 4, page, off + d, piece + d, stride + d, want=True)
    # the written page itself must be legal for the codec
    check(codec, 4, page + m // 2, off, piece, stride, want=False)
    if codec == MXFP4:  # 16-byte steps: whole lanes for fp8, part groups for mxfp4
        check(FP8, 4, 4096, 16, 32, 48, want=True)
        check(MXFP4, 4, 4096, 16, 64, 128, want=False)
        check(MXFP4, 4, 4096, 64, 32, 128, want=False)
        check(MXFP4, 4, 4096, 64, 64, 144, want=False)


@pytest.mark.parametrize("codec", CODECS)
def test_client_segments(codec):
    m = MULTIPLE[codec]
    page, piece, stride = 256 * m, m, 4 * m
    # kv-major: 2 * T pieces into 2 segments
    check(codec, 8, page, 0, piece, stride, 2, 1 << 20, want=True)
    check(codec, 8, page, 0, piece, stride, 8, 1 << 20, want=True)  # S == n
    check(codec, 8, page, 0, piece, stride, 3, 1 << 20, want=False)  # n % S
    check(codec, 9, page, 0, piece, stride, 2, 1 << 20, want=False)
    check(codec, 8, page, 0, piece, stride, 0, 1 << 20, want=False)
    check(codec, 8, page, 0, piece, stride, 16, 1 << 20, want=False)
    # the sliced page obeys segments_legal: segments must not overlap
    check(codec, 8, page, 0, piece, stride, 2, 4 * piece, want=True)
    check(codec, 8, page, 0, piece, stride, 2, 4 * piece - min(m, 16), want=False)
    if codec != NONE:  # and the client stride keeps 16-byte alignment
        check(codec, 8, page, 0, piece, stride, 2, (1 << 20) + 8, want=False)
    check(NONE, 8, page, 0, piece, stride, 2, (1 << 20) + 1, want=True)
    check(codec, MAX_SEG * 2, MAX_PIECES * 4 * m, 0, m, 4 * m, MAX_SEG, 1 << 20, want=True)
    check(codec, MAX_PIECES, MAX_PIECES * 4 * m, 0, m, 4 * m, 2 * MAX_SEG, 1 << 20,
          want=False)


def test_values_near_2_to_64():
    check(NONE, 1, U64, U64 - 256, 256, 0, want=True)
    check(NONE, 1, U64, U64 - 255, 256, 0, want=False)  # offset + piece wraps to 0
    check(NONE, 1, U64, U64, 1, 0, want=False)
    check(NONE, 2, U64, 0, 1 << 63, 1 << 63, want=False)  # ends at 2^64: wraps to 0
    check(NONE, 2, U64, 0, (1 << 63) - 1, 1 << 63, want=True)
    check(NONE, MAX_PIECES, U64, 0, 1, 1 << 53, want=False)  # 4095 * stride > 2^64
    check(NONE, MAX_PIECES, U64, 0, 1, U64 // 4095, want=True)
    assert U64 % 4095 == 15  # so 14 more bytes of offset fit, 15 do not
    check(NONE, MAX_PIECES, U64, 14, 1, U64 // 4095, want=True)
    check(NONE, MAX_PIECES, U64, 15, 1, U64 // 4095, want=False)
    check(NONE, 3, 1 << 20, U64 - 10, 16, 16, want=False)
    check(NONE, 2, 1 << 20, 0, 16, U64, want=False)
    check(FP8, 1, U64 - 15, U64 - 15 - 256, 256, 0, want=True)
    check(MXFP4, 2, (1 << 64) - 64, 0, 64, (1 << 64) - 128, want=True)
    check(MXFP4, 2, (1 << 64) - 64, 64, 64, (1 << 64) - 128, want=False)


def test_random_geometries_agree():
    rs = np.random.RandomState(5)
    n_legal = 0
    for _ in range(4000):
        codec = int(rs.randint(3))
        unit = int(rs.choice([1, 8, 16, 32, 64]))
        n = int(rs.choice([1, 2, 3, 4, 8, 16]))
        piece = unit * int(rs.randint(0, 6))
        stride = unit * int(rs.randint(0, 12))
        off = unit * int(rs.randint(0, 6))
        page = unit * int(rs.randint(1, 200))
        S = int(rs.choice([1, 1, 2, 4]))
        args = (n, page, off, piece, stride, S, int(rs.choice([0, 64, 1024, 1032])))
        check(codec, *args)
        n_legal += slice_ok(codec, *args)
    assert 200 < n_legal < 3800  # the table exercises both answers


def test_unknown_codec_id_and_shape():
    with pytest.raises(ValueError):
        legal(3, 1, 64, 0, 64, 0)
    with pytest.raises(ValueError):
        _native._dbg_slice_legal(NONE, (1, 64, 0, 64))


# --- packed framing ----------------------------------------------------------
IPC = bytes(range(64))
HDR = 104
FLAG_SYNC, FLAG_FP8, FLAG_MXFP4, FLAG_SEG, FLAG_SLICED = 1, 2, 4, 8, 16
SLICE = (8, 4096, 128, 64, 512)  # n_pieces, page_bytes, offset, piece_bytes, stride
SLICE_EXT = struct.pack("<IIQQQQ", 8, 0, 4096, 128, 64, 512)


def _build(keys, offsets, block_size=512, flags=0, **kw):
    return _native._dbg_build_packed_local(3, 1234, 0x7000_0000_0000, 4096, block_size, flags,
                                           17, IPC, offsets, keys, **kw)


def _hdr(block_size, n, flags):
    return struct.pack("<iiQQIIII", 3, 1234, 0x7000_0000_0000, 4096, block_size, n, flags,
                       17) + IPC


def test_unsliced_bodies_are_the_parents_bytes():
    keys, offs = ["alpha", "b", "gamma-3"], [0, 256, 1 << 33]
    tail = struct.pack("<3Q", *offs) + b"alpha\0b\0gamma-3"
    # contiguous, as the builder made it before slices existed
    want = _hdr(512, 3, FLAG_SYNC) + tail
    assert _build(keys, offs, flags=FLAG_SYNC) == want
    assert _build(keys, offs, flags=FLAG_SYNC, slice=None) == want
    # with the segment extension in front
    want_seg = _hdr(512, 3, FLAG_SYNC | FLAG_SEG) + struct.pack("<IIQ", 2, 0, 1 << 20) + tail
    assert _build(keys, offs, flags=FLAG_SYNC, n_segments=2, segment_stride=1 << 20) == want_seg
    assert _build(keys, offs, flags=FLAG_SYNC, n_segments=2, segment_stride=1 << 20,
                  slice=None) == want_seg
    for op in ("w", "r"):
        for body in (want, want_seg):
            got = _native._dbg_parse_packed_local(op, body)
            assert got["slice"] is None and got["keys"] == keys and got["offsets"] == offs


@pytest.mark.parametrize("seg", [False, True])
def test_slice_extension_follows_header_and_segments(seg):
    keys, offs = ["k0", "k1"], [0, 1024]
    kw = dict(n_segments=2, segment_stride=1 << 20) if seg else {}
    plain = _build(keys, offs, **kw)
    body = _build(keys, offs, slice=SLICE, **kw)
    pos = HDR + (16 if seg else 0)
    assert len(body) == len(plain) + 40
    flags = struct.unpack_from("<I", body, 32)[0]
    assert flags == (FLAG_SLICED | (FLAG_SEG if seg else 0))
    assert body[:32] == plain[:32] and body[36:pos] == plain[36:pos]
    assert body[pos:pos + 40] == SLICE_EXT
    assert body[pos + 40:] == plain[pos:]  # offsets and keys follow unchanged
    got = _native._dbg_parse_packed_local("r", body)
    assert got["slice"] == SLICE and got["block_size"] == 512
    assert got["keys"] == keys and got["offsets"] == offs
    assert (got["n_segments"], got["segment_stride"]) == ((2, 1 << 20) if seg else (1, 0))


def _refused(op, body):
    with pytest.raises(ValueError, match="INVALID_REQ"):
        _native._dbg_parse_packed_local(op, body)


def _with_ext(body, pos, **fields):
    """`body` with fields of its slice extension (at `pos`) replaced."""
    names = ["n_pieces", "rsvd", "page_bytes", "offset", "piece_bytes", "stride"]
    vals = dict(zip(names, struct.unpack_from("<IIQQQQ", body, pos)))
    vals.update(fields)
    out = bytearray(body)
    struct.pack_into("<IIQQQQ", out, pos, *(vals[k] for k in names))
    return bytes(out)


@pytest.mark.parametrize("seg", [False, True])
def test_parse_refusals(seg):
    kw = dict(n_segments=2, segment_stride=1 << 20) if seg else {}
    pos = HDR + (16 if seg else 0)
    good = _build(["k"], [0], slice=SLICE, **kw)
    assert _native._dbg_parse_packed_local("r", good)["slice"] == SLICE
    _refused("w", good)  # a slice is a read-side geometry
    for cut in (pos, pos + 1, pos + 8, pos + 39):  # truncated inside the extension
        _refused("r", good[:cut])
    _refused("r", good[:pos + 40 + 7])  # extension whole, offsets cut
    _refused("r", _with_ext(good, pos, rsvd=1))
    _refused("r", _with_ext(good, pos, n_pieces=0))
    _refused("r", _with_ext(good, pos, n_pieces=4))  # block_size != n * piece
    _refused("r", _with_ext(good, pos, piece_bytes=32))
    _refused("r", _with_ext(good, pos, page_bytes=128 + 7 * 512 + 63))  # one byte short
    assert _native._dbg_parse_packed_local("r", _with_ext(good, pos, page_bytes=128 + 7 * 512 + 64))
    _refused("r", _with_ext(good, pos, stride=63))  # overlap
    _refused("r", _with_ext(good, pos, offset=U64 - 8))
    if seg:  # 8 pieces do not split into 3 segments; 512 % 3 != 0 either way
        three = bytearray(good)
        struct.pack_into("<IIQ", three, HDR, 3, 0, 1 << 20)
        _refused("r", bytes(three))
    # the flag set with no room for the extension at all
    hdr_only = bytearray(_build([], []))
    struct.pack_into("<I", hdr_only, 32, FLAG_SLICED)
    _refused("r", bytes(hdr_only))
    # too many pieces (block_size agrees, so only the bound refuses)
    many = _build(["k"], [0], block_size=(MAX_PIECES + 1) * 16,
                  slice=(MAX_PIECES + 1, 1 << 20, 0, 16, 16))
    _refused("r", many)
    assert _native._dbg_parse_packed_local(
        "r", _build(["k"], [0], block_size=MAX_PIECES * 16,
                    slice=(MAX_PIECES, 1 << 20, 0, 16, 16)))


def test_parse_applies_plain_rules_on_read():
    # 8-byte pieces at odd offsets: fine for plain pages; a compressed entry is
    # refused by the read sweep, which knows what the key holds
    body = _build(["k"], [0], block_size=24, slice=(3, 1000, 5, 8, 11))
    assert _native._dbg_parse_packed_local("r", body)["slice"] == (3, 1000, 5, 8, 11)


# --- Python refusals, before anything is sent --------------------------------
chk = InfinityConnection._check_slice


def test_check_slice_accepts_the_legal():
    offs = np.array([0, 512], dtype=np.uint64)
    chk(4096, offs, 512, PageSlice(4096, 128, 64, 512, 8))
    chk(4096, offs, 512, (4096, 128, 64, 512, 8))  # a plain tuple too
    chk(4096, offs, 512, PageSlice(4096, 128 + 320, 64, 512, 8))  # ends on the last element
    chk(4096, [4096 - 512], 512, PageSlice(4096, 0, 64, 64, 8))  # ends exactly at numel
    chk(4096, [0], 64, PageSlice(4096, 4032, 64))  # one piece, stride unused
    chk(4096, offs, 512, PageSlice(4096, 0, 64, 512, 8), 2, 2048)
    chk(4096, offs, 512, PageSlice(4096, 0, 64, 512, 8), 8, 64)


@pytest.mark.parametrize("args", [
    (4096, [0], 0, PageSlice(4096, 0, 64, 512, 0)),  # no pieces
    (1 << 20, [0], 4097, PageSlice(1 << 20, 0, 1, 1, 4097)),  # too many
    (4096, [0], 0, PageSlice(4096, 0, 0, 512, 8)),  # empty pieces
    (4096, [0], 512, PageSlice(4096, 0, 64, 63, 8)),  # overlap
    (4096, [0], 512, PageSlice(4096, 0, 64, 0, 8)),
    (4096, [0], 512, PageSlice(4096, 128 + 321, 64, 512, 8)),  # leaves the stored page
    (4096, [0], 512, PageSlice(4095, 128 + 320, 64, 512, 8)),
    (4096, [0], 512, PageSlice(4096, -64, 64, 512, 8)),
    (4096, [0], 576, PageSlice(4096, 0, 64, 512, 8)),  # page_size != count * piece
    (4096, [0], 448, PageSlice(4096, 0, 64, 512, 8)),
    (4096, [0], 512, PageSlice(4096, 0, 64, 512, 8), 3, 1024),  # count % segments
    (4096, [4096 - 511], 512, PageSlice(4096, 0, 64, 512, 8)),  # leaves the tensor
])
def test_check_slice_refuses(args):
    with pytest.raises(ValueError):
        chk(*args)


class _NoTraffic:
    """Stands in for the native connection: any use is a test failure."""

    def __getattr__(self, name):
        raise AssertionError(f"connection used: {name}")


def _conn(local):
    c = InfinityConnection(ClientConfig(host_addr="127.0.0.1", service_port=1,
                                        connection_type=TYPE_RDMA))
    c.conn = _NoTraffic()
    c.local_connected, c.rdma_connected = local, not local
    c._verify = lambda cache: None  # a CPU tensor stands in for the cache
    return c


SL = PageSlice(4096, 128, 64, 512, 8)


def test_reads_refuse_before_anything_is_sent():
    c = _conn(local=True)
    t = torch.zeros(4096, dtype=torch.bfloat16)
    for read in (c.read_pages, c.read_pages_async):
        with pytest.raises(ValueError, match="count"):
            read(t, ["k"], [0], 512, page_slice=SL._replace(count=0))
        with pytest.raises(ValueError, match="page_size"):
            read(t, ["k"], [0], 256, page_slice=SL)
        with pytest.raises(ValueError, match="stored page"):
            read(t, ["k"], [0], 512, page_slice=SL._replace(page_size=2048))
        with pytest.raises(ValueError, match="tensor"):
            read(t, ["k"], [4096 - 256], 512, page_slice=SL)
        # combined with segments: the second segment leaves the tensor
        with pytest.raises(ValueError, match="tensor"):
            read(t, ["k"], [0], 512, segments=2, segment_stride=4096 - 255, page_slice=SL)
        with pytest.raises(ValueError, match="segments"):
            read(t, ["k"], [0], 512, segments=3, segment_stride=1024, page_slice=SL)


def test_slices_on_a_fabric_connection_are_refused():
    c = _conn(local=False)
    t = torch.zeros(4096, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="local"):
        c.read_pages(t, ["k"], [0], 512, page_slice=SL)
    with pytest.raises(ValueError, match="local"):
        c.read_pages_async(t, ["k"], [0], 512, page_slice=SL)


@pytest.mark.parametrize("local", [True, False])
def test_write_pages_takes_no_slice(local):
    c = _conn(local)
    t = torch.zeros(4096, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="read-only"):
        c.write_pages(t, ["k"], [0], 512, page_slice=SL)
    with pytest.raises(TypeError):
        c.write_pages(t, ["k"], [0], 512, page_slice_typo=SL)


def test_connector_passes_the_refusals_through():
    kc = PagedKVConnector.__new__(PagedKVConnector)  # no connection is made
    kc.model_tag, kc.n_layers, kc.quant, kc.local = "m", 1, None, True
    kc.conn = _conn(local=True)
    t = torch.zeros(4096, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="page_size"):
        kc.load_layer(0, t, ["k"], [0], 256, page_slice=SL)
    with pytest.raises(ValueError, match="page_size"):
        kc.load_layer_async(0, t, ["k"], [0], 256, page_slice=SL)
    kc.local = False
    with pytest.raises(ValueError, match="local"):
        kc.load_layer(0, t, ["k"], [0], 512, page_slice=SL)
    with pytest.raises(ValueError, match="local"):
        kc.load_layer_async(0, t, ["k"], [0], 512, page_slice=SL)


def test_adapter_head_range_arguments():
    # all refused at construction, before any connection is made (port 1)
    mk = lambda **kw: InfiniStoreKVAdapter("127.0.0.1", 1, "m", 2, 4, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="stored_kv_heads"):
        mk(page_elems=512, head_range=(2, 4))
    with pytest.raises(ValueError, match="page_elems"):
        mk(page_elems=1024, stored_kv_heads=4, head_range=(2, 4), head_dim=32)
    with pytest.raises(ValueError, match="head_range"):
        mk(page_elems=512, stored_kv_heads=4, head_range=(2, 5), head_dim=32)
    with pytest.raises(ValueError, match="head_range"):
        mk(page_elems=512, stored_kv_heads=4, head_range=(2, 2), head_dim=32)
    with pytest.raises(ValueError, match="local"):
        mk(page_elems=512, stored_kv_heads=4, head_range=(2, 4), head_dim=32, local=False)
    with pytest.raises(ValueError, match="head_range"):
        mk(page_elems=512, stored_kv_heads=4)


# --- plain sliced jobs through a CPU shard -----------------------------------
PAGE, GUARD = 2 * 4 * 4 * 32 * 2, 64  # [2, T=4, H=4, hd=32] bf16 pages, bytes


def _stored(n_blocks, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (n_blocks, PAGE), dtype=np.uint8)


def _run(jobs, slices):
    return _native._dbg_shard_run_sliced(-1, 1, 2, 16, jobs, slices, 1, 30.0)


def _job(src, dst_ptrs, nbytes, S=1, seg_stride=0, codec=NONE, store=False):
    return ([int(src[i].ctypes.data) for i in range(len(src))], dst_ptrs, nbytes, codec, store,
            S, seg_stride, None, 0)


@pytest.mark.parametrize("heads", [(0, 2), (2, 4), (1, 2)])
def test_cpu_shard_head_slice_contiguous(heads):
    h0, h1 = heads
    T, H, hd = 4, 4, 32
    src = _stored(5)
    piece = (h1 - h0) * hd * 2
    sliced = 2 * T * piece
    dst = np.full((5, GUARD + sliced + GUARD), 0xA5, dtype=np.uint8)
    sl = (2 * T, PAGE, h0 * hd * 2, piece, H * hd * 2)
    res = _run([_job(src, [int(dst[i].ctypes.data) + GUARD for i in range(5)], sliced)], [sl])
    assert res[0]["submitted"] and res[0]["done_calls"] == 1 and res[0]["ok"]
    want = src.reshape(5, 2 * T, H, hd * 2)[:, :, h0:h1].reshape(5, sliced)
    assert np.array_equal(dst[:, GUARD:GUARD + sliced], want)
    assert (dst[:, :GUARD] == 0xA5).all() and (dst[:, GUARD + sliced:] == 0xA5).all()


def test_cpu_shard_head_slice_into_two_segments():
    T, H, hd, h0, h1 = 4, 4, 32, 2, 4
    n = 3
    src = _stored(n, seed=1)
    piece = (h1 - h0) * hd * 2
    half = T * piece  # the K half, then the V half a plane further
    plane = n * half + 48
    dst = np.full(GUARD + 2 * plane + GUARD, 0xA5, dtype=np.uint8)
    base = int(dst.ctypes.data) + GUARD
    sl = (2 * T, PAGE, h0 * hd * 2, piece, H * hd * 2)
    res = _run([_job(src, [base + i * half for i in range(n)], 2 * half, 2, plane)], [sl])
    assert res[0]["submitted"] and res[0]["ok"]
    want = src.reshape(n, 2, T, H, hd * 2)[:, :, :, h0:h1].reshape(n, 2, half)
    body = dst[GUARD:GUARD + 2 * plane].reshape(2, plane)
    assert np.array_equal(body[:, :n * half].reshape(2, n, half), want.transpose(1, 0, 2))
    assert (body[:, n * half:] == 0xA5).all()
    assert (dst[:GUARD] == 0xA5).all() and (dst[-GUARD:] == 0xA5).all()


def test_cpu_shard_refusals_leave_the_destination_alone():
    src = _stored(2, seed=2)
    dst = np.full((2, 512), 0xA5, dtype=np.uint8)
    ptrs = [int(dst[i].ctypes.data) for i in range(2)]
    sl = (8, PAGE, 0, 64, 256)
    cases = [
        (_job(src, ptrs, 512, store=True), sl),  # a slice is valid only for loads
        (_job(src, ptrs, 512), (8, PAGE, 0, 64, 63)),  # illegal geometry
        (_job(src, ptrs, 512), (8, 7 * 256 + 63, 0, 64, 256)),  # leaves the page
        (_job(src, ptrs, 256), sl),  # the job's page is not n * piece
        (_job(src, ptrs, 512, 3, 1024), sl),  # 8 % 3
        (_job(src, ptrs, 512, codec=FP8), sl),  # compressed jobs stay GPU-only
    ]
    res = _run([c[0] for c in cases], [c[1] for c in cases])
    for r in res:
        assert not r["submitted"] and r["done_calls"] == 0
    assert (dst == 0xA5).all()
    # and the unsliced entry of the same binding still copies whole pages
    whole = np.full((2, PAGE), 0xA5, dtype=np.uint8)
    res = _run([_job(src, [int(whole[i].ctypes.data) for i in range(2)], PAGE)], [None])
    assert res[0]["ok"] and np.array_equal(whole, src)
