"""Transposed pages without a GPU: transpose_legal against its rules written out here,
the framing, the parser's refusals, every new ValueError, and a CPU Shard's jobs."""

import struct
from math import prod

import numpy as np
import pytest
import torch

from infinistore_amd import PagePermute, PageSlice, PageTranspose, _native
from infinistore_amd.kv_connector import PagedKVConnector
from infinistore_amd.lib import TensorSet
from infinistore_amd.vllm_adapter import InfiniStoreKVAdapter

from test_gpu_xpose_kernels import canonical
from test_page_permute import HDR, IPC, _conn

MULTIPLE, MAX_TILE = {0: 1, 1: 16, 2: 64}, 32 << 10  # codec id -> page multiple in bytes
FLAG_SYNC, FLAG_FP8, FLAG_MXFP4, FLAG_SEG, FLAG_PERM, FLAG_XPOSE = 1, 2, 4, 8, 64, 128
GOOD = (2, 16, 3, 64, 2, 8, 1)  # a 12288-byte bf16 page


def legal_ref(codec, page, x, S, stride):
    outer, T, H, C, eb, *inner = x  # Python integers do not wrap
    if min(outer, T, H, C) < 1 or outer > 2 or eb not in (1, 2, 4) or (codec and eb != 2):
        return False
    for xo in inner:
        if xo < 1 or xo & (xo - 1) or C % xo or xo * eb > 16 or T % (16 // (xo * eb)):
            return False
    row = C * eb
    if row % 16 or row % MULTIPLE[codec] or outer * T * H * row != page or T * row > MAX_TILE:
        return False
    return S == 1 or (S >= 1 and outer * H % S == 0 and
                      _native._dbg_segments_legal(codec, page, S, stride))


def test_transpose_legal_matches_its_rules():
    assert _native._MAX_TRANSPOSE_TILE == MAX_TILE
    cases = [GOOD[:i] + (v,) + GOOD[i + 1:] for i in range(7) for v in (0, 1, 2, 3, 4, 12, 16, 32)]
    cases += [(2, 8, 1, 32, 2, 8, 1), (1, 24, 2, 96, 4, 4, 2), (2, 128, 1, 128, 2, 8, 1),
              (2, 136, 1, 128, 2, 8, 1), (2, 129, 1, 128, 2, 8, 8), (2, 16, 12, 16, 2, 8, 1),
              (2, 1 << 16, 1 << 15, 64, 2, 8, 8),  # 2^39 bytes: wraps 32 bits
              (2, 1 << 31, 1 << 31, 64, 2, 8, 8),  # 2^70 bytes: wraps 64 bits to 0
              (2, (1 << 32) - 1, (1 << 32) - 1, (1 << 32) - 16, 2, 8, 8)]
    for x in cases:
        pages = {0, 12288, 24576, prod(x[:5]) % (1 << 32), prod(x[:5]) % (1 << 64)}
        for codec, page, (S, stride) in [(c, p, g) for c in MULTIPLE for p in pages for g in (
                (1, 0), (2, 1 << 30), (3, 1 << 30), (4, 1 << 30), (2, 8), (0, 0))]:
            got = _native._dbg_transpose_legal(codec, page, x, S, stride)
            assert got == legal_ref(codec, page, x, S, stride), (codec, page, x, S)


def _build(keys, offsets, block_size=12288, flags=0, **kw):
    return _native._dbg_build_packed_local(3, 1234, 0x7000_0000_0000, 4096, block_size, flags,
                                           17, IPC, offsets, keys, **kw)


def test_framing_and_parser_refusals():
    keys, offs = ["alpha", "b", "gamma-3"], [0, 256, 1 << 33]
    hdr = struct.pack("<iiQQIIII", 3, 1234, 0x7000_0000_0000, 4096, 12288, 3, FLAG_SYNC, 17) + IPC
    tail = struct.pack("<3Q", *offs) + b"alpha\0b\0gamma-3"
    assert _build(keys, offs, flags=FLAG_SYNC, transpose=None) == hdr + tail
    flagged = struct.pack("<iiQQIIII", 3, 1234, 0x7000_0000_0000, 4096, 12288, 3,
                          FLAG_SYNC | FLAG_SEG | FLAG_XPOSE, 17) + IPC
    body = _build(keys, offs, flags=FLAG_SYNC, n_segments=2, segment_stride=8192, transpose=GOOD)
    assert body == (flagged + struct.pack("<IIQ", 2, 0, 8192) + struct.pack("<8I", *GOOD, 0) + tail)
    # the extension comes after all the others: hand-built next to a permutation
    both = _build(["k"], [0], permute=(2, 16, 3, 128), transpose=GOOD)
    assert both[HDR:HDR + 56] == struct.pack("<IIIIQ8I", 2, 16, 3, 0, 128, *GOOD, 0)
    good = _build(["k"], [0], transpose=GOOD)
    zero = bytearray(good)
    struct.pack_into("<I", zero, HDR + 4, 0)  # flag set, tokens == 0
    bad = [good[:cut] for cut in (HDR, HDR + 1, HDR + 31, HDR + 32 + 7)] + [
        bytes(zero), both,
        _build(["k"], [0], transpose=GOOD + (9,)),  # rsvd
        _build(["k"], [0], block_size=24576, transpose=GOOD),  # cut for another page size
        _build(["k"], [0], transpose=(2, 16, 3, 64, 2, 16, 1)),  # a 32-byte run
        # next to the slice or the tensor-set flag
        _build(["k"], [0], block_size=256, slice=(2, 1024, 0, 128, 512),
               transpose=(1, 8, 1, 16, 2, 8, 1)),
        _build(["k"], [0], n_segments=2, tensor_set=(1, 2), transpose=GOOD)]
    for op in ("w", "r"):
        assert _native._dbg_parse_packed_local(op, hdr + tail)["transpose"] is None
        got = _native._dbg_parse_packed_local(op, body)
        assert got["transpose"] == GOOD and got["keys"] == keys and got["offsets"] == offs
        assert (got["n_segments"], got["segment_stride"]) == (2, 8192)
        for b in bad:
            with pytest.raises(ValueError, match="INVALID_REQ"):
                _native._dbg_parse_packed_local(op, b)
    # the request's codec: writes only (rows of half an mxfp4 group)
    b = _build(["k"], [0], flags=FLAG_MXFP4, transpose=(2, 16, 12, 16, 2, 8, 1))
    assert _native._dbg_parse_packed_local("r", b)["transpose"] == (2, 16, 12, 16, 2, 8, 1)
    with pytest.raises(ValueError, match="INVALID_REQ"):
        _native._dbg_parse_packed_local("w", b)


def test_python_refusals():
    cache = torch.zeros(16384, dtype=torch.bfloat16)
    xp, page = PageTranspose(16, 3, 64, 8), 6144
    for call in (_conn(False).write_pages, _conn(False).read_pages, _conn(False).read_pages_async):
        with pytest.raises(ValueError, match="local"):
            call(cache, ["k"], [0], page, page_transpose=xp)
    c = _conn(True)
    ts = TensorSet(c, 1, [torch.zeros(4096, dtype=torch.bfloat16) for _ in range(2)])
    refused = [  # (message, page_size, keyword arguments)
        ("positive", page, dict(page_transpose=xp._replace(tokens=0))),
        ("illegal", page, dict(page_transpose=xp._replace(inner_k=16))),
        ("illegal", page, dict(page_transpose=xp, segments=4, segment_stride=2048)),
        ("aligned", page, dict(page_transpose=xp, offsets=[4])),
        ("page_permute", page, dict(page_transpose=xp, page_permute=PagePermute(2, 16, 3))),
        ("tensor_set", page, dict(page_transpose=xp, tensor_set=ts, cache=None)),
        ("page_slice", 256, dict(page_transpose=PageTranspose(8, 1, 16, 8),
                                 page_slice=PageSlice(1024, 0, 128, 512, 2)))]
    for call in (c.write_pages, c.read_pages, c.read_pages_async):
        for msg, size, kw in refused:
            with pytest.raises(ValueError, match=msg):
                call(**{**dict(cache=cache, keys=["k"], offsets=[0], page_size=size), **kw})
    for quant in ("fp8", "mxfp4"):  # a quant with a non-bf16 cache; rows of half a group
        with pytest.raises(ValueError, match="bf16"):
            c.write_pages(cache.view(torch.int16), ["k"], [0], page, quant=quant, page_transpose=xp)
    with pytest.raises(ValueError, match="transpose"):
        c.write_pages(cache, ["k"], [0], page, quant="mxfp4",
                      page_transpose=PageTranspose(16, 12, 16, 8))
    kv = PagedKVConnector.__new__(PagedKVConnector)
    kv.conn, kv.local, kv.quant, kv._key = _conn(False), False, None, lambda layer, k: k
    for call in (kv.save_layer, kv.load_layer, kv.load_layer_async):
        with pytest.raises(ValueError, match="local"):
            call(0, cache, ["k"], [0], page, page_transpose=xp)
    pa = dict(host="127.0.0.1", port=1, model_tag="m", n_layers=2, block_tokens=16,
              page_elems=page, cache_layout="pa", cache_kv_heads=3)
    for kw in (dict(cache_kv_heads=None), dict(local=False), dict(layer_pages="fused"),
               dict(cache_kv_heads=5), dict(cache_layout="nhd")):
        with pytest.raises(ValueError):
            InfiniStoreKVAdapter(**{**pa, **kw})


@pytest.mark.parametrize("store", [True, False])
@pytest.mark.parametrize("x,S", [((2, 8, 3, 16, 2, 8, 1), 1), ((2, 16, 3, 32, 1, 16, 2), 2),
                                 ((1, 4, 5, 8, 4, 4, 4), 5), ((2, 24, 2, 96, 2, 8, 2), 1)])
def test_cpu_shard_copies_transposed_pages(x, S, store):
    n, page = 3, prod(x[:5])
    seg, stride = page // S, page // S + 5
    at = np.arange(page) // seg * stride + np.arange(page) % seg  # client byte of each page byte
    client = np.full((n, S * stride), 0xA5, dtype=np.uint8)
    pool = np.full((n, page + 8), 0xA5, dtype=np.uint8)
    data = np.random.RandomState(page + S).randint(0, 256, (n, page)).astype(np.uint8)  # canonical
    if store:
        client[:, at] = canonical(data, x, back=True)
    else:
        pool[:, :page] = data
    cp, pp = [client[i].ctypes.data for i in range(n)], [pool[i].ctypes.data for i in range(n)]
    job = (cp if store else pp, pp if store else cp, page, 0, store, S, stride, None, 0)
    res = _native._dbg_shard_run_xpose(-1, 1, 1, 16, [job], [x], 1, 10.0)
    assert res[0]["submitted"] and res[0]["done_calls"] == 1 and res[0]["ok"]
    assert (pool[:, :page] == data).all() and (canonical(client[:, at], x) == data).all()
    assert (np.delete(client, at, axis=1) == 0xA5).all() and (pool[:, page:] == 0xA5).all()
