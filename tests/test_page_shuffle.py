"""Shuffled pages without a GPU: shuffle_legal against its rules written out here, the
framing, the parser's refusals, and every new ValueError."""

import struct
from math import prod

import numpy as np
import pytest
import torch

from infinistore_amd import (PageCast, PagePermute, PageRotate, PageShuffle, PageSlice,
                             PageTranspose, _native)
from infinistore_amd.kv_connector import PagedKVConnector
from infinistore_amd.lib import TensorSet
from infinistore_amd.vllm_adapter import InfiniStoreKVAdapter

from test_page_permute import HDR, IPC, _conn

FLAG_SYNC, FLAG_MXFP4, FLAG_SEG, FLAG_SHUF = 1, 4, 8, 1024
GOOD = (2, 16, 3, 64, 2, 1, 2)  # a 12288-byte bf16 page, K then V
TABLE = np.tile(np.float32([1.0, 0.0]), 32)  # the identity rotation of 32 pairs


def legal_ref(codec, page, x, S, stride):
    outer, T, H, C, eb, *forms = x  # Python integers do not wrap
    if min(outer, T, H, C) < 1 or outer > 2 or eb not in (1, 2, 4) or (codec and eb != 2):
        return False
    X = 16 // eb
    if any(f not in (1, 2) for f in forms) or T % X or C % X or (codec == 2 and C % 32):
        return False
    if outer * T * H * C * eb != page or (T // X) * (C // X) >= 1 << 32 or outer * H >= 1 << 32:
        return False
    return S >= 1 and outer * H % S == 0 and _native._dbg_segments_legal(codec, page, S, stride)


def test_shuffle_legal_matches_its_rules():
    cases = [GOOD[:i] + (v,) + GOOD[i + 1:] for i in range(7) for v in (0, 1, 2, 3, 4, 12, 16, 32)]
    cases += [(2, 8, 1, 8, 2, 1, 2), (1, 16, 2, 48, 1, 2, 1), (2, 4, 1, 4, 4, 2, 2),
              (2, 256, 1, 128, 2, 1, 2),  # a 64 KiB tile: no tile bound
              (2, 16, 12, 16, 2, 1, 2),  # rows of half an mxfp4 group
              (1, 1 << 19, 1, 1 << 19, 2, 1, 2), (1, 1 << 18, 1, 1 << 19, 2, 1, 2),  # 2^32 squares
              (2, 8, 1 << 31, 8, 2, 1, 2), (2, 8, (1 << 31) - 1, 8, 2, 1, 2),  # 2^32 tiles
              (2, 1 << 16, 1 << 15, 64, 2, 1, 2),  # 2^39 bytes: wraps 32 bits
              (2, 1 << 31, 1 << 31, 64, 2, 1, 2),  # 2^70 bytes: wraps 64 bits to 0
              (2, (1 << 32) - 8, (1 << 32) - 1, (1 << 32) - 32, 2, 1, 2)]
    for x in cases:
        pages = {0, 12288, 24576, prod(x[:5]) % (1 << 32), prod(x[:5]) % (1 << 64)}
        for codec, page, (S, stride) in [(c, p, g) for c in (0, 1, 2) for p in pages for g in (
                (1, 0), (2, 1 << 40), (3, 1 << 40), (4, 1 << 40), (2, 8), (0, 0))]:
            got = _native._dbg_shuffle_legal(codec, page, x, S, stride)
            assert got == legal_ref(codec, page, x, S, stride), (codec, page, x, S)


def _build(keys, offsets, block_size=12288, flags=0, **kw):
    return _native._dbg_build_packed_local(3, 1234, 0x7000_0000_0000, 4096, block_size, flags,
                                           17, IPC, offsets, keys, **kw)


def test_framing_and_parser_refusals():
    keys, offs = ["alpha", "b", "gamma-3"], [0, 256, 1 << 33]
    hdr = struct.pack("<iiQQIIII", 3, 1234, 0x7000_0000_0000, 4096, 12288, 3, FLAG_SYNC, 17) + IPC
    tail = struct.pack("<3Q", *offs) + b"alpha\0b\0gamma-3"
    assert _build(keys, offs, flags=FLAG_SYNC, shuffle=None) == hdr + tail
    flagged = struct.pack("<iiQQIIII", 3, 1234, 0x7000_0000_0000, 4096, 12288, 3,
                          FLAG_SYNC | FLAG_SEG | FLAG_SHUF, 17) + IPC
    body = _build(keys, offs, flags=FLAG_SYNC, n_segments=2, segment_stride=8192, shuffle=GOOD)
    assert body == (flagged + struct.pack("<IIQ", 2, 0, 8192) + struct.pack("<8I", *GOOD, 0) + tail)
    # the extension comes after all the others: hand-built behind a rotation and its table
    rot = (1, 2, 3, 64, 64, TABLE)
    behind = _build(["k"], [0], rotate=rot, shuffle=GOOD)
    assert behind[HDR + 24 + 256:HDR + 24 + 256 + 32] == struct.pack("<8I", *GOOD, 0)
    good = _build(["k"], [0], shuffle=GOOD)
    zero = bytearray(good)
    struct.pack_into("<I", zero, HDR + 4, 0)  # flag set, tokens == 0
    bad = [good[:cut] for cut in (HDR, HDR + 1, HDR + 31, HDR + 32 + 7)] + [
        bytes(zero), behind,
        _build(["k"], [0], shuffle=GOOD + (9,)),  # rsvd
        _build(["k"], [0], block_size=24576, shuffle=GOOD),  # cut for another page size
        _build(["k"], [0], shuffle=GOOD[:5] + (1, 3)),  # a form that does not exist
        # next to each other flag
        _build(["k"], [0], block_size=256, slice=(2, 1024, 0, 128, 512),
               shuffle=(1, 8, 1, 16, 2, 1, 2)),
        _build(["k"], [0], n_segments=2, tensor_set=(1, 2), shuffle=GOOD),
        _build(["k"], [0], permute=(2, 16, 3, 128), shuffle=GOOD),
        _build(["k"], [0], transpose=(2, 16, 3, 64, 2, 8, 1), shuffle=GOOD),
        _build(["k"], [0], cast=(1, 2, 0.5, 0.25), shuffle=GOOD)]
    for op in ("w", "r"):
        assert _native._dbg_parse_packed_local(op, hdr + tail)["shuffle"] is None
        got = _native._dbg_parse_packed_local(op, body)
        assert got["shuffle"] == GOOD and got["keys"] == keys and got["offsets"] == offs
        assert (got["n_segments"], got["segment_stride"]) == (2, 8192)
        for b in bad:
            with pytest.raises(ValueError, match="INVALID_REQ"):
                _native._dbg_parse_packed_local(op, b)
    # the request's codec: writes only (rows of half an mxfp4 group)
    b = _build(["k"], [0], flags=FLAG_MXFP4, shuffle=(2, 16, 12, 16, 2, 1, 2))
    assert _native._dbg_parse_packed_local("r", b)["shuffle"] == (2, 16, 12, 16, 2, 1, 2)
    with pytest.raises(ValueError, match="INVALID_REQ"):
        _native._dbg_parse_packed_local("w", b)


def test_python_refusals():
    cache = torch.zeros(16384, dtype=torch.bfloat16)
    sh, page = PageShuffle(16, 3, 64), 6144
    for call in (_conn(False).write_pages, _conn(False).read_pages, _conn(False).read_pages_async):
        with pytest.raises(ValueError, match="local"):
            call(cache, ["k"], [0], page, page_shuffle=sh)
    c = _conn(True)
    ts = TensorSet(c, 1, [torch.zeros(4096, dtype=torch.bfloat16) for _ in range(2)])
    refused = [  # (message, page_size, keyword arguments)
        ("positive", page, dict(page_shuffle=sh._replace(tokens=0))),
        ("forms", page, dict(page_shuffle=sh._replace(forms=("k", "x")))),
        ("elem_bytes", page, dict(page_shuffle=sh._replace(elem_bytes=1))),  # the wrong dtype
        ("illegal", page, dict(page_shuffle=sh._replace(tokens=12, heads=4))),
        ("illegal", page, dict(page_shuffle=sh, segments=4, segment_stride=2048)),
        ("aligned", page, dict(page_shuffle=sh, offsets=[4])),
        ("outside", page, dict(page_shuffle=sh, offsets=[16384 - 64])),
        ("page_permute", page, dict(page_shuffle=sh, page_permute=PagePermute(2, 16, 3))),
        ("page_transpose", page, dict(page_shuffle=sh, page_transpose=PageTranspose(16, 3, 64, 8))),
        ("page_cast", page, dict(page_shuffle=sh, page_cast=PageCast([0.5, 0.25]))),
        ("tensor_set", page, dict(page_shuffle=sh, tensor_set=ts, cache=None))]
    reads = [("page_slice", 256, dict(page_shuffle=PageShuffle(8, 1, 16),
                                      page_slice=PageSlice(1024, 0, 128, 512, 2))),
             ("page_rotate", page, dict(page_shuffle=sh,
                                        page_rotate=PageRotate(3, 64, TABLE.reshape(32, 2))))]
    for call in (c.write_pages, c.read_pages, c.read_pages_async):
        for msg, size, kw in refused + (reads if call != c.write_pages else []):
            with pytest.raises(ValueError, match=msg):
                call(**{**dict(cache=cache, keys=["k"], offsets=[0], page_size=size), **kw})
    for kw in (r[2] for r in reads):  # read-side arguments next to a shuffled write
        with pytest.raises(ValueError):
            c.write_pages(cache, ["k"], [0], page, **kw)
    for quant in ("fp8", "mxfp4"):  # a quant with a cache that is not bf16
        with pytest.raises(ValueError, match="bf16"):
            c.write_pages(cache.view(torch.int16), ["k"], [0], page, quant=quant, page_shuffle=sh)
    with pytest.raises(ValueError, match="shuffle"):  # rows of half an mxfp4 group
        c.write_pages(cache, ["k"], [0], page, quant="mxfp4", page_shuffle=PageShuffle(16, 12, 16))
    kv = PagedKVConnector.__new__(PagedKVConnector)
    kv.conn, kv.local, kv.quant, kv._key = _conn(False), False, None, lambda layer, k: k
    for call in (kv.save_layer, kv.load_layer, kv.load_layer_async):
        with pytest.raises(ValueError, match="local"):
            call(0, cache, ["k"], [0], page, page_shuffle=sh)
    pa = dict(host="127.0.0.1", port=1, model_tag="m", n_layers=2, block_tokens=16,
              page_elems=page, cache_layout="pa_shuffled", cache_kv_heads=3)
    for kw in (dict(cache_kv_heads=None), dict(local=False), dict(layer_pages="fused"),
               dict(head_range=(0, 1), stored_kv_heads=3, head_dim=64), dict(cache_kv_heads=5),
               dict(cache_dtype="fp8_e4m3", k_scale=0.5, v_scale=0.25)):
        with pytest.raises(ValueError):
            InfiniStoreKVAdapter(**{**pa, **kw})
