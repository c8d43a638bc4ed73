"""Rotated reads without a GPU: rotate_legal against its rules written out here, the
framing, the parser's refusals, every new ValueError, and the pair rule on the host."""

import struct

import numpy as np
import pytest
import torch

from infinistore_amd import (PageCast, PagePermute, PageRotate, PageSlice, PageTranspose,
                             _native)
from infinistore_amd.kv_connector import PagedKVConnector
from infinistore_amd.lib import TensorSet

from _kernel_refs import bf16_bits
from _mxfp4_refs import bits_to_f64
from test_page_permute import HDR, IPC, _conn

FLAG_SYNC, FLAG_SEG, FLAG_ROT = 1, 8, 512
ONES = np.ones(256, dtype=np.float32)


def legal_ref(codec, page, geo, table, S, stride):
    style, halves, heads, hd, rd = geo  # Python integers do not wrap
    P = rd // 2
    if style not in (1, 2) or halves not in (1, 2) or min(heads, hd, rd) < 1 or rd > hd:
        return False
    if rd % 2 or P > 128 or hd % 8 or (P % 8 if style == 1 else rd % 8):
        return False
    if codec == 2 and (hd % 32 or rd % 32 or (style == 1 and P % 32)):
        return False
    if page == 0 or page % (halves * heads * hd * 2) or page % {0: 1, 1: 16, 2: 64}[codec]:
        return False
    if not 1 <= S <= 1024 or page % S:
        return False
    if S > 1:
        seg = page // S
        if stride < seg or stride % 16 or seg % (hd * 2) or (codec and seg % (16, 64)[codec - 1]):
            return False
    return bool(np.isfinite(table[:rd]).all())


def test_rotate_legal_matches_its_rules():
    geos = [(1, 2, 2, 64, 64), (2, 2, 2, 64, 64), (1, 1, 1, 32, 32), (2, 1, 3, 128, 8),
            (1, 2, 2, 128, 64), (0, 2, 2, 64, 64), (3, 2, 2, 64, 64), (1, 0, 2, 64, 64),
            (1, 3, 2, 64, 64), (1, 2, 0, 64, 64), (1, 2, 2, 0, 0), (1, 2, 2, 64, 0),
            (1, 2, 2, 64, 128), (1, 2, 2, 64, 24), (2, 2, 2, 64, 12), (2, 2, 2, 60, 8),
            (2, 2, 2, 64, 17), (2, 1, 1, 512, 256), (2, 1, 1, 512, 264), (2, 2, 2, 64, 16),
            # products that wrap 32 and 64 bits into a divisor of the page
            (2, 2, 1 << 31, 8, 8), (2, 2, (1 << 31) + 1, 8, 8), (2, 2, 1 << 28, 1 << 31, 8)]
    pages = [0, 32, 512, 1024, 1536, 2048, 2048 + 64, 4096, 1 << 33, (1 << 64) - 512, 1 << 63]
    segs = [(1, 0), (2, 1 << 40), (2, 1024), (2, 1032), (2, 512), (3, 4096), (4, 512), (0, 0),
            (1024, 1 << 20), (1025, 1 << 20), (2, (1 << 64) - 16)]
    bad_table = np.where(np.arange(256) == 7, np.float32("inf"), ONES)
    for geo in geos:
        rd = min(geo[4], 600)
        for table in (ONES, bad_table):
            rot = (*geo, np.ascontiguousarray(np.resize(table, rd)))
            for codec in (0, 1, 2):
                for page in pages:
                    for S, stride in segs:
                        got = _native._dbg_rotate_legal(codec, page, rot, S, stride)
                        want = legal_ref(codec, page, geo, np.resize(table, rd), S, stride)
                        assert got == want, (codec, page, geo, S, stride)
    nan_last = (1, 2, 2, 64, 64, np.where(np.arange(64) == 63, np.float32("nan"), ONES[:64]))
    assert not _native._dbg_rotate_legal(0, 2048, nan_last, 1, 0)


def _build(keys, offsets, block_size=1024, flags=0, **kw):
    return _native._dbg_build_packed_local(3, 1234, 0x7000_0000_0000, 4096, block_size, flags,
                                           17, IPC, offsets, keys, **kw)


def test_framing_and_parser_refusals():
    keys, offs = ["alpha", "b", "gamma-3"], [0, 256, 1 << 33]
    table = np.arange(32, dtype=np.float32) / 7
    geo = (1, 2, 2, 32, 32)  # 256 bytes a token: 4 tokens in the 1024-byte page
    rot = (*geo, table)
    hdr = struct.pack("<iiQQIIII", 3, 1234, 0x7000_0000_0000, 4096, 1024, 3, FLAG_SYNC, 17) + IPC
    tail = struct.pack("<3Q", *offs) + b"alpha\0b\0gamma-3"
    assert _build(keys, offs, flags=FLAG_SYNC, rotate=None) == hdr + tail
    flagged = struct.pack("<iiQQIIII", 3, 1234, 0x7000_0000_0000, 4096, 1024, 3,
                          FLAG_SYNC | FLAG_SEG | FLAG_ROT, 17) + IPC
    body = _build(keys, offs, flags=FLAG_SYNC, n_segments=2, segment_stride=528, rotate=rot)
    assert body == (flagged + struct.pack("<IIQ", 2, 0, 528) + struct.pack("<6I", *geo, 0)
                    + table.tobytes() + tail)
    # the extension comes after all the others: hand-built next to a cast
    cast = (1, 2, 0.5, 2.0)
    both = _build(["k"], [0], cast=cast, rotate=rot)
    assert both[HDR:HDR + 40] == struct.pack("<IIff", *cast) + struct.pack("<6I", *geo, 0)
    got = _native._dbg_parse_packed_local("r", body)
    assert got["rotate"] == (*geo, table.tobytes())
    assert got["keys"] == keys and got["offsets"] == offs and got["n_segments"] == 2
    assert _native._dbg_parse_packed_local("r", hdr + tail)["rotate"] is None
    good = _build(["k"], [0], rotate=rot)
    assert _native._dbg_parse_packed_local("r", good)["rotate"][:5] == geo
    zero = bytearray(good)
    struct.pack_into("<I", zero, HDR, 0)  # flag set, style == 0
    bad = [good[:cut] for cut in (HDR, HDR + 23, HDR + 24, HDR + 24 + 127)] + [
        bytes(zero), both,
        _build(["k"], [0], rotate=(*geo, table, 1)),  # rsvd
        _build(["k"], [0], block_size=1024 + 64, rotate=rot),  # not whole tokens
        _build(["k"], [0], rotate=(1, 2, 2, 32, 24, table[:24])),  # 12 pairs: half a unit
        _build(["k"], [0], rotate=(*geo, np.where(np.arange(32) == 9, np.float32("inf"), table))),
        _build(["k"], [0], n_segments=2, segment_stride=520, rotate=rot),  # a stride off 16
        # next to the slice, the tensor-set, the permute and the transpose flag
        _build(["k"], [0], block_size=256, slice=(2, 1024, 0, 128, 512), rotate=rot),
        _build(["k"], [0], n_segments=2, tensor_set=(1, 2), rotate=rot),
        _build(["k"], [0], permute=(2, 4, 2, 64), rotate=rot),
        _build(["k"], [0], transpose=(2, 8, 1, 32, 2, 8, 1), rotate=rot)]
    for b in bad:
        with pytest.raises(ValueError, match="INVALID_REQ"):
            _native._dbg_parse_packed_local("r", b)
    with pytest.raises(ValueError, match="INVALID_REQ"):  # reads only
        _native._dbg_parse_packed_local("w", good)


def test_python_refusals():
    cache = torch.zeros(16384, dtype=torch.bfloat16)
    pr, page = PageRotate.from_delta(5, 2, 64), 2048
    for call in (_conn(False).read_pages, _conn(False).read_pages_async):
        with pytest.raises(ValueError, match="local"):
            call(cache, ["k"], [0], page, page_rotate=pr)
    c = _conn(True)
    ts = TensorSet(c, 1, [torch.zeros(4096, dtype=torch.bfloat16) for _ in range(2)])
    inf = np.where(np.arange(64).reshape(32, 2) == 3, np.inf, 1.0)
    refused = [  # (message, keyword arguments)
        ("bfloat16", dict(cache=cache.view(torch.float16))),
        ("illegal", dict(page_size=2048 + 64)),
        ("illegal", dict(page_rotate=PageRotate(2, 64, np.ones((12, 2)), rot_dim=24))),
        ("illegal", dict(page_rotate=PageRotate(2, 64, inf))),
        ("illegal", dict(segments=2, segment_stride=1028)),
        ("aligned", dict(offsets=[4])),
        ("outside", dict(offsets=[16384 - 2040])),
        ("must be a PageRotate", dict(page_rotate=(1, 2, 2, 64, 64))),
        ("page_slice", dict(page_slice=PageSlice(4096, 0, 128, 512, 16))),
        ("page_permute", dict(page_permute=PagePermute(2, 16, 4))),
        ("page_transpose", dict(page_transpose=PageTranspose(16, 2, 64, 8))),
        ("page_cast", dict(page_cast=PageCast([0.5, 2.0]))),
        ("tensor_set", dict(tensor_set=ts, cache=None))]
    for call in (c.read_pages, c.read_pages_async):
        for msg, kw in refused:
            with pytest.raises(ValueError, match=msg):
                call(**{**dict(cache=cache, keys=["k"], offsets=[0], page_size=page,
                               page_rotate=pr), **kw})
    with pytest.raises(TypeError):  # read-only: write_pages has no such parameter
        c.write_pages(cache, ["k"], [0], page, page_rotate=pr)
    for kw in (dict(style="llama"), dict(rot_dim=32), dict(cos_sin=np.ones(64))):
        with pytest.raises(ValueError):
            PageRotate(**{**dict(heads=2, head_dim=64, cos_sin=np.ones((32, 2))), **kw})
    kv = PagedKVConnector.__new__(PagedKVConnector)
    kv.conn, kv.local, kv.quant, kv._key = _conn(False), False, None, lambda layer, k: k
    for call in (kv.load_layer, kv.load_layer_async):
        with pytest.raises(ValueError, match="local"):
            call(0, cache, ["k"], [0], page, page_rotate=pr)


def test_from_delta_and_the_pair_rule_on_the_host():
    pr = PageRotate.from_delta(37, 2, 64, theta=500000.0, rot_dim=32, style="gptj", halves=1)
    ang = 37 * 500000.0 ** (-2 * np.arange(16) / 32)
    assert pr.cos_sin.dtype == np.float32 and pr.cos_sin.shape == (16, 2)
    assert (pr.cos_sin == np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)).all()
    assert pr.wire()[:5] == (2, 1, 2, 64, 32)
    g = torch.Generator().manual_seed(3)
    a, b = (bf16_bits(torch.randn(4096, generator=g).to(torch.bfloat16)) for _ in range(2))
    for c, s in ((1.0, 0.0), (0.0, 1.0), tuple(pr.cos_sin[5])):
        oa, ob = (np.frombuffer(x, dtype=np.uint16)
                  for x in _native._dbg_rotate_pairs(a, b, float(c), float(s)))
        fa, fb = bits_to_f64(a), bits_to_f64(b)
        for got, ref in ((oa, fa * c - fb * s), (ob, fb * c + fa * s)):
            bound = 2.0 ** -8 * np.abs(ref) + 2.0 ** -21 * (np.abs(fa) + np.abs(fb))
            assert (np.abs(bits_to_f64(got) - ref) <= bound).all(), (c, s)
        if s == 0.0:
            assert (oa == a).all() and (ob == b).all()
        if c == 0.0:
            assert (oa == b ^ 0x8000).all() and (ob == a).all()
