"""Cast pages without a GPU: cast_legal against its rules written out here, the framing,
the parser's refusals, every new ValueError, the scalar rules on the host, and a CPU
Shard's jobs."""

import struct

import numpy as np
import pytest
import torch

from infinistore_amd import PageCast, PagePermute, PageSlice, PageTranspose, _native
from infinistore_amd.kv_connector import PagedKVConnector
from infinistore_amd.lib import TensorSet
from infinistore_amd.vllm_adapter import InfiniStoreKVAdapter

from _kernel_refs import all_bf16_patterns, assert_bf16_bits_equal, assert_codes_equal, bf16_bits
from test_gpu_cast_kernels import load_ref, store_ref
from test_page_permute import HDR, IPC, _conn

FLAG_SYNC, FLAG_MXFP4, FLAG_SEG, FLAG_CAST = 1, 4, 8, 256
GOOD = (1, 2, 0.5, 2.0)
SCALES = [1.0, 0.0123, 3.7, 0.3333333, 2.0 ** -20, 1e4]
BAD_SCALES = [0.0, -1.0, 1e-39, float("inf"), float("nan")]  # zero, negative, subnormal, ...


def legal_ref(codec, page, cast, S, stride):
    et, halves, *scales = cast  # Python integers do not wrap
    unit = 32 if codec == 2 else 8
    if et != 1 or halves not in (1, 2):
        return False
    for s in np.asarray(scales, dtype=np.float32):
        if not (np.isfinite(s) and s >= np.float32(2.0 ** -126)):
            return False
    if page == 0 or page % 2 or page % {0: 1, 1: 16, 2: 64}[codec]:
        return False
    elems = page // 2
    if elems % halves or elems // halves % unit or not 1 <= S <= 1024:
        return False
    return S == 1 or (elems % S == 0 and elems // S % unit == 0 and stride >= elems // S
                      and stride % 16 == 0)


def test_cast_legal_matches_its_rules():
    casts = [GOOD, (1, 1, 0.5, 2.0), (0, 2, 1.0, 1.0), (2, 2, 1.0, 1.0), (1, 0, 1.0, 1.0),
             (1, 3, 1.0, 1.0), (1, 2, 2.0 ** -126, 3e38)]
    casts += [(1, 2, s, 1.0) for s in BAD_SCALES] + [(1, 1, 1.0, s) for s in BAD_SCALES]
    pages = [0, 16, 32, 48, 112, 128, 144, 192, 1024, 1024 + 16, 1024 + 64, 3 * 1024,
             (1 << 64) - 128, (1 << 64) - 64, (1 << 64) - 2, (1 << 63) + 64]
    segs = [(1, 0), (2, 1 << 40), (2, 256), (2, 264), (2, 248), (4, 128), (3, 512), (0, 0),
            (1024, 1 << 20), (1025, 1 << 20), (2, (1 << 64) - 16), (2, 1 << 62)]
    for cast in casts:
        for codec in (0, 1, 2):
            for page in pages:
                for S, stride in segs:
                    got = _native._dbg_cast_legal(codec, page, cast, S, stride)
                    assert got == legal_ref(codec, page, cast, S, stride), (codec, page, cast, S)


def _build(keys, offsets, block_size=1024, flags=0, **kw):
    return _native._dbg_build_packed_local(3, 1234, 0x7000_0000_0000, 4096, block_size, flags,
                                           17, IPC, offsets, keys, **kw)


def test_framing_and_parser_refusals():
    keys, offs = ["alpha", "b", "gamma-3"], [0, 256, 1 << 33]
    hdr = struct.pack("<iiQQIIII", 3, 1234, 0x7000_0000_0000, 4096, 1024, 3, FLAG_SYNC, 17) + IPC
    tail = struct.pack("<3Q", *offs) + b"alpha\0b\0gamma-3"
    assert _build(keys, offs, flags=FLAG_SYNC, cast=None) == hdr + tail
    assert _build(keys, offs, flags=FLAG_SYNC) == hdr + tail
    flagged = struct.pack("<iiQQIIII", 3, 1234, 0x7000_0000_0000, 4096, 1024, 3,
                          FLAG_SYNC | FLAG_SEG | FLAG_CAST, 17) + IPC
    # client segments of 256 BYTES, half the logical 512: only cast_legal accepts the stride
    body = _build(keys, offs, flags=FLAG_SYNC, n_segments=2, segment_stride=272, cast=GOOD)
    assert body == flagged + struct.pack("<IIQ", 2, 0, 272) + struct.pack("<IIff", *GOOD) + tail
    # the extension comes after all the others: hand-built next to a transpose
    xp = (2, 8, 1, 32, 2, 8, 1)
    both = _build(["k"], [0], transpose=xp, cast=GOOD)
    assert both[HDR:HDR + 48] == struct.pack("<8IIIff", *xp, 0, *GOOD)
    good = _build(["k"], [0], cast=GOOD)
    zero = bytearray(good)
    struct.pack_into("<I", zero, HDR, 0)  # flag set, elem_type == 0
    bad = [good[:cut] for cut in (HDR, HDR + 1, HDR + 15, HDR + 16 + 7)] + [
        bytes(zero), both,
        _build(["k"], [0], block_size=1024 + 16, cast=GOOD),  # halves of half a lane unit
        _build(["k"], [0], n_segments=2, segment_stride=240, cast=GOOD),  # overlapping
        _build(["k"], [0], cast=(1, 2, 0.0, 1.0)),
        # next to the slice, the tensor-set and the permute flag
        _build(["k"], [0], block_size=256, slice=(2, 1024, 0, 128, 512), cast=GOOD),
        _build(["k"], [0], n_segments=2, tensor_set=(1, 2), cast=GOOD),
        _build(["k"], [0], permute=(2, 4, 2, 64), cast=GOOD)]
    for op in ("w", "r"):
        assert _native._dbg_parse_packed_local(op, hdr + tail)["cast"] is None
        got = _native._dbg_parse_packed_local(op, body)
        assert got["cast"] == GOOD and got["keys"] == keys and got["offsets"] == offs
        assert (got["n_segments"], got["segment_stride"]) == (2, 272)
        for b in bad:
            with pytest.raises(ValueError, match="INVALID_REQ"):
                _native._dbg_parse_packed_local(op, b)
    # the request's codec: writes only (halves of half an mxfp4 group)
    b = _build(["k"], [0], block_size=64 * 3, flags=FLAG_MXFP4, cast=GOOD)
    assert _native._dbg_parse_packed_local("r", b)["cast"] == GOOD
    with pytest.raises(ValueError, match="INVALID_REQ"):
        _native._dbg_parse_packed_local("w", b)


def test_python_refusals():
    cache = torch.zeros(16384, dtype=torch.uint8)
    pc, page = PageCast([0.5, 2.0]), 4096
    for call in (_conn(False).write_pages, _conn(False).read_pages, _conn(False).read_pages_async):
        with pytest.raises(ValueError, match="local"):
            call(cache, ["k"], [0], page, page_cast=pc)
    c = _conn(True)
    ts = TensorSet(c, 1, [torch.zeros(4096, dtype=torch.uint8) for _ in range(2)])
    refused = [  # (message, keyword arguments)
        ("float8_e4m3fn or uint8", dict(cache=cache.view(torch.bfloat16))),
        ("illegal", dict(page_size=4096 + 8)),
        ("illegal", dict(segments=2, segment_stride=2040)),
        ("illegal", dict(segments=2, segment_stride=2056)),
        ("aligned", dict(offsets=[8])),
        ("outside", dict(offsets=[16384 - 4080])),
        ("outside", dict(offsets=[8192], segments=2, segment_stride=8192)),
        ("page_permute", dict(page_permute=PagePermute(2, 16, 4))),
        ("page_transpose", dict(page_transpose=PageTranspose(16, 2, 64, 16))),
        ("tensor_set", dict(tensor_set=ts, cache=None))]
    refused += [("illegal", dict(page_cast=PageCast([1.0, s]))) for s in BAD_SCALES]
    refused += [("must be a PageCast", dict(page_cast=[0.5, 2.0]))]
    # one _cast_arg serves the three entry points: the geometry rules go through one of
    # them, the rules each entry point has a hand in (the last three) through all
    for call, rules in ((c.write_pages, refused), (c.read_pages, refused[7:10]),
                        (c.read_pages_async, refused[7:10])):
        for msg, kw in rules:
            with pytest.raises(ValueError, match=msg):
                call(**{**dict(cache=cache, keys=["k"], offsets=[0], page_size=page, page_cast=pc),
                        **kw})
    for call in (c.read_pages, c.read_pages_async):
        with pytest.raises(ValueError, match="page_slice"):
            call(cache, ["k"], [0], 256, page_cast=pc, page_slice=PageSlice(1024, 0, 128, 512, 2))
    with pytest.raises(ValueError, match="illegal"):  # halves of half an mxfp4 group
        c.write_pages(cache, ["k"], [0], 96, quant="mxfp4", page_cast=pc)
    with pytest.raises(ValueError, match="quant"):
        c.write_pages(cache, ["k"], [0], page, quant="int3", page_cast=pc)
    for scales, halves in (([], None), ([1.0, 2.0, 3.0], None), ([1.0, 2.0], 1), ([1.0], 3)):
        with pytest.raises(ValueError):
            PageCast(scales, halves)
    assert PageCast([0.5], halves=2).wire() == (1, 2, 0.5, 0.5) and PageCast(3.0).halves == 1
    kv = PagedKVConnector.__new__(PagedKVConnector)
    kv.conn, kv.local, kv.quant, kv._key = _conn(False), False, None, lambda layer, k: k
    for call in (kv.save_layer, kv.load_layer, kv.load_layer_async):
        with pytest.raises(ValueError, match="local"):
            call(0, cache, ["k"], [0], page, page_cast=pc)
    f8 = dict(host="127.0.0.1", port=1, model_tag="m", n_layers=2, block_tokens=16,
              page_elems=page, cache_dtype="fp8_e4m3", k_scale=0.5, v_scale=2.0)
    for kw in (dict(k_scale=None), dict(local=False), dict(layer_pages="fused"),
               dict(cache_layout="hnd", cache_kv_heads=2), dict(cache_layout="pa", cache_kv_heads=2),
               dict(head_range=(0, 1), stored_kv_heads=2, head_dim=64, page_elems=2048),
               dict(cache_dtype="fp8_e5m2"), dict(cache_dtype="auto")):
        with pytest.raises(ValueError):
            InfiniStoreKVAdapter(**{**f8, **kw})


@pytest.mark.parametrize("scale", SCALES)
def test_scalar_rules_on_the_host(scale):
    """All 256 codes through the store rule, every bf16 pattern through the load rule,
    against torch's e4m3 cast (NaN codes by the project's rule: the sign is kept), and the
    round trip of the 254 other codes under one scale."""
    codes = np.arange(256, dtype=np.uint8)
    b = np.frombuffer(_native._dbg_cast_store(codes, scale), dtype=np.uint16)
    assert_bf16_bits_equal(b, bf16_bits(store_ref(codes[None], [scale], 1)), f"store {scale}")
    assert (b[[0x7F, 0xFF]] == [0x7FC0, 0xFFC0]).all()
    bits = bf16_bits(all_bf16_patterns())
    got = np.frombuffer(_native._dbg_cast_load(bits, scale), dtype=np.uint8)
    assert_codes_equal(got, load_ref(bits[None], [scale], 1), f"load {scale}")
    nan = (bits & 0x7FFF) > 0x7F80
    assert (got[nan] == ((bits[nan] >> 8) & 0x80 | 0x7F)).all()
    assert got[0x8000] == 0x80 and got[0x7F80] == 0x7E and got[0xFF80] == 0xFE  # -0, +-inf
    back = np.frombuffer(_native._dbg_cast_load(b, scale), dtype=np.uint8)
    assert (back == codes).all(), f"round trip under {scale}"


@pytest.mark.parametrize("store", [True, False])
@pytest.mark.parametrize("N,halves,S", [(64, 2, 1), (96, 1, 3), (256, 2, 2), (512, 2, 4)])
def test_cpu_shard_casts_plain_pages(N, halves, S, store):
    n, cast = 3, (1, halves, 0.0123, 3.7)
    seg, stride = N // S, N // S + 16
    at = np.arange(N) // seg * stride + np.arange(N) % seg  # client byte of each page element
    client = np.full((n, S * stride), 0xA5, dtype=np.uint8)
    pool = np.full((n, N + 4), 0xA5A5, dtype=np.uint16)
    codes = np.random.RandomState(N + S).randint(0, 256, (n, N)).astype(np.uint8)
    codes[(codes & 0x7F) == 0x7F] ^= 1
    b = bf16_bits(store_ref(codes, cast[2:], halves))
    if store:
        client[:, at] = codes
    else:
        pool[:, :N] = b
    cp, pp = [client[i].ctypes.data for i in range(n)], [pool[i].ctypes.data for i in range(n)]
    job = (cp if store else pp, pp if store else cp, 2 * N, 0, store, S, stride, None, 0)
    res = _native._dbg_shard_run_cast(-1, 1, 1, 16, [job], [cast], 1, 10.0)
    assert res[0]["submitted"] and res[0]["done_calls"] == 1 and res[0]["ok"]
    assert (pool[:, :N] == b).all() and (client[:, at] == codes).all()
    assert (np.delete(client, at, axis=1) == 0xA5).all() and (pool[:, N:] == 0xA5A5).all()
    bad = (cp, pp, 2 * N, 0, True, S, stride, None, 0)
    res = _native._dbg_shard_run_cast(-1, 1, 1, 16, [bad], [(1, 3, 1.0, 1.0)], 1, 10.0)
    assert not res[0]["submitted"]
