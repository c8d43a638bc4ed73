"""Permuted pages without a GPU: permute_legal against its rules written out
here, the wire extension byte for byte, the parser's refusals, every Python
ValueError, and plain permuted jobs through a CPU Shard."""

import struct

import numpy as np
import pytest
import torch

from infinistore_amd import PagePermute, PageSlice, _native
from infinistore_amd.lib import ClientConfig, InfinityConnection, TensorSet, TYPE_RDMA
from infinistore_amd.vllm_adapter import InfiniStoreKVAdapter

NONE, FP8, MXFP4 = 0, 1, 2
MULTIPLE = {NONE: 1, FP8: 16, MXFP4: 64}  # page multiple in bytes
MAX_PIECES = 1 << 20
IPC = bytes(range(64))
HDR = 104
FLAG_SYNC, FLAG_FP8, FLAG_MXFP4, FLAG_SEG, FLAG_PERM = 1, 2, 4, 8, 64


def legal_ref(codec, page, perm, S, stride):
    o, r, c, piece = perm
    pieces = o * r * c  # Python integers do not wrap
    if min(o, r, c, piece) < 1 or pieces > MAX_PIECES or pieces * piece != page:
        return False
    if piece % MULTIPLE[codec]:
        return False
    return S == 1 or (S >= 1 and pieces % S == 0 and
                      _native._dbg_segments_legal(codec, page, S, stride))


def test_permute_legal_matches_its_rules():
    assert _native._MAX_PERM_PIECES == MAX_PIECES == InfinityConnection.MAX_PERM_PIECES
    big = 1 << 64
    cases = [(o, r, c, p) for o, r, c in [(2, 5, 3), (0, 5, 3), (2, 0, 3), (2, 5, 0), (1, 1, 1),
                                          (2, 1, 7), (2, 7, 1)] for p in (0, 16, 24, 96, 128)]
    cases += [(1 << 10, 1 << 10, 1, 64), (1 << 10, 1 << 10, 2, 64),
              ((1 << 32) - 1, (1 << 32) - 1, (1 << 32) - 1, 64),  # the count wraps 64 bits
              (1 << 16, 1 << 16, 1, 128),  # 2^32 pieces: wraps 32 bits
              (2, 5, 3, big - 1), (2, 5, 3, (big + 3840) // 30), (1, 1, 2, 1 << 63)]
    for codec in (NONE, FP8, MXFP4):
        for perm in cases:
            for page in [0, 480, 3840, 1 << 26, big - 1, perm[0] * perm[1] * perm[2] * perm[3] % big]:
                for S, stride in ((1, 0), (2, 1 << 30), (3, 1 << 30), (2, 8), (0, 0)):
                    got = _native._dbg_permute_legal(codec, page, perm, S, stride)
                    assert got == legal_ref(codec, page, perm, S, stride), (codec, page, perm, S)


def _build(keys, offsets, block_size=3840, flags=0, **kw):
    return _native._dbg_build_packed_local(3, 1234, 0x7000_0000_0000, 4096, block_size, flags,
                                           17, IPC, offsets, keys, **kw)


def test_framing_and_parser_refusals():
    keys, offs = ["alpha", "b", "gamma-3"], [0, 256, 1 << 33]
    hdr = struct.pack("<iiQQIIII", 3, 1234, 0x7000_0000_0000, 4096, 3840, 3, FLAG_SYNC, 17) + IPC
    tail = struct.pack("<3Q", *offs) + b"alpha\0b\0gamma-3"
    assert _build(keys, offs, flags=FLAG_SYNC) == hdr + tail
    assert _build(keys, offs, flags=FLAG_SYNC, permute=None) == hdr + tail
    flagged = struct.pack("<iiQQIIII", 3, 1234, 0x7000_0000_0000, 4096, 3840, 3,
                          FLAG_SYNC | FLAG_SEG | FLAG_PERM, 17) + IPC
    body = _build(keys, offs, flags=FLAG_SYNC, n_segments=2, segment_stride=4096,
                  permute=(2, 5, 3, 128))
    assert body == (flagged + struct.pack("<IIQ", 2, 0, 4096)
                    + struct.pack("<IIIIQ", 2, 5, 3, 0, 128) + tail)
    good = _build(["k"], [0], permute=(2, 5, 3, 128))
    zero = bytearray(good)
    struct.pack_into("<I", zero, HDR + 4, 0)  # flag set, rows == 0
    bad = [good[:cut] for cut in (HDR, HDR + 1, HDR + 23, HDR + 24 + 7)] + [
        bytes(zero),
        _build(["k"], [0], permute=(2, 5, 3, 128, 9)),  # rsvd
        _build(["k"], [0], permute=(2, 5, 3, 64)),  # cut for another page size
        _build(["k"], [0], permute=(1 << 16, 1 << 16, 1, 128)),
        _build(["k"], [0], n_segments=4, segment_stride=4096, permute=(2, 5, 3, 128)),
        # next to the slice or the tensor-set flag
        _build(["k"], [0], block_size=256, slice=(2, 1024, 0, 128, 512), permute=(1, 2, 1, 128)),
        _build(["k"], [0], n_segments=2, tensor_set=(1, 2), permute=(2, 5, 3, 128))]
    for op in ("w", "r"):
        assert _native._dbg_parse_packed_local(op, hdr + tail)["permute"] is None
        got = _native._dbg_parse_packed_local(op, body)
        assert got["permute"] == (2, 5, 3, 128) and got["keys"] == keys and got["offsets"] == offs
        assert (got["n_segments"], got["segment_stride"]) == (2, 4096)
        for b in bad:
            with pytest.raises(ValueError, match="INVALID_REQ"):
                _native._dbg_parse_packed_local(op, b)
    for flag, piece in ((FLAG_FP8, 24), (FLAG_MXFP4, 96)):  # the request's codec: writes only
        b = _build(["k"], [0], block_size=30 * piece, flags=flag, permute=(2, 5, 3, piece))
        assert _native._dbg_parse_packed_local("r", b)["permute"] == (2, 5, 3, piece)
        with pytest.raises(ValueError, match="INVALID_REQ"):
            _native._dbg_parse_packed_local("w", b)


def _conn(local):
    c = InfinityConnection(ClientConfig(host_addr="127.0.0.1", service_port=1,
                                        connection_type=TYPE_RDMA))
    c.conn = None  # any use of the native connection fails the test
    c.local_connected, c.rdma_connected = local, not local
    c._verify = lambda cache: None  # a CPU tensor stands in for the cache
    return c


def test_python_refusals():
    cache = torch.zeros(8192, dtype=torch.bfloat16)
    pm = PagePermute(2, 5, 3)
    for call in (_conn(False).write_pages, _conn(False).read_pages, _conn(False).read_pages_async):
        with pytest.raises(ValueError, match="local"):
            call(cache, ["k"], [0], 1920, page_permute=pm)
    c = _conn(True)
    ts = TensorSet(c, 1, [torch.zeros(4096, dtype=torch.bfloat16) for _ in range(2)])
    for call in (c.write_pages, c.read_pages, c.read_pages_async):
        for bad, page in ((PagePermute(2, 0, 3), 1920), (PagePermute(0, 5, 3), 1920),
                          (PagePermute(2, 5, -1), 1920), (pm, 1921), (pm, 0),
                          (PagePermute(1 << 10, 1 << 10, 2), 1 << 21)):
            with pytest.raises(ValueError):
                call(cache, ["k"], [0], page, page_permute=bad)
        for S in (4, 0):
            with pytest.raises(ValueError, match="segments"):
                call(cache, ["k"], [0], 1920, segments=S, segment_stride=2048, page_permute=pm)
        with pytest.raises(ValueError, match="tensor_set"):
            call(None, ["k"], [0], 1920, tensor_set=ts, page_permute=pm)
    for call in (c.read_pages, c.read_pages_async):
        with pytest.raises(ValueError, match="page_slice"):
            call(cache, ["k"], [0], 256, page_slice=PageSlice(1024, 0, 128, 512, 2),
                 page_permute=PagePermute(1, 2, 1))
    for quant, page in (("fp8", 30 * 12), ("mxfp4", 30 * 48)):  # pieces of half a unit
        with pytest.raises(ValueError, match="pieces"):
            c.write_pages(cache, ["k"], [0], page, quant=quant, page_permute=pm)
    hnd = dict(host="127.0.0.1", port=1, model_tag="m", n_layers=2, block_tokens=4,
               page_elems=2 * 4 * 3 * 16, cache_layout="hnd", cache_kv_heads=3)
    for kw in (dict(cache_kv_heads=None), dict(local=False), dict(layer_pages="fused"),
               dict(cache_kv_heads=5), dict(cache_layout="dhn"), dict(cache_layout="nhd"),
               dict(page_elems=2 * 4 * 16, stored_kv_heads=3, head_range=(0, 1), head_dim=16)):
        with pytest.raises(ValueError):
            InfiniStoreKVAdapter(**{**hnd, **kw})


@pytest.mark.parametrize("store", [True, False])
@pytest.mark.parametrize("geo,piece,S", [((2, 5, 3), 7, 1), ((1, 3, 5), 16, 1), ((2, 5, 3), 4, 2),
                                         ((2, 1, 7), 5, 1), ((2, 4, 3), 1, 24)])
def test_cpu_shard_copies_permuted_pages(geo, piece, S, store):
    o, r, c = geo
    n, page = 3, o * r * c * piece
    seg, stride = page // S, page // S + 5
    client = np.full((n, S * stride + 8), 0xA5, dtype=np.uint8)
    pool = np.full((n, page + 8), 0xA5, dtype=np.uint8)
    data = np.random.RandomState(page + S).randint(0, 256, (n, page)).astype(np.uint8)
    segs = [slice(s * stride, s * stride + seg) for s in range(S)]
    if store:
        for s in range(S):
            client[:, segs[s]] = data[:, s * seg:(s + 1) * seg]
    else:
        pool[:, :page] = data
    cp, pp = [client[i].ctypes.data for i in range(n)], [pool[i].ctypes.data for i in range(n)]
    job = (cp if store else pp, pp if store else cp, page, NONE, store, S, stride, None, 0)
    res = _native._dbg_shard_run_perm(-1, 1, 1, 16, [job], [(o, r, c, piece)], 1, 10.0)
    assert res[0]["submitted"] and res[0]["done_calls"] == 1 and res[0]["ok"]
    got_client = np.concatenate([client[:, sl] for sl in segs], axis=1)
    canon = got_client.reshape(n, o, c, r, piece).transpose(0, 1, 3, 2, 4).reshape(n, page)
    assert (pool[:, :page] == canon).all() and (pool[:, page:] == 0xA5).all()
    for s in range(S):
        assert (client[:, s * stride + seg:(s + 1) * stride] == 0xA5).all()
    assert ((got_client if store else pool[:, :page]) == data).all(), "the source was modified"
