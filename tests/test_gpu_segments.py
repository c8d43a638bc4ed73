"""Segmented pages end to end: `write_pages` / `read_pages(segments=...)`
through a running server. A page written from a K/V-split `[2, nb, seg]` cache
is stored exactly as the contiguous page `cat(K[b], V[b])` would be, so every
reader, contiguous or segmented with any segment count, gets it back — bit for
bit for plain pages, the reference round trip for fp8 and mxfp4."""

import json
import os
import socket
import struct
import uuid

import numpy as np
import pytest
import torch

from infinistore_amd import _native
from infinistore_amd.vllm_adapter import InfiniStoreKVAdapter

from _kernel_refs import assert_bf16_bits_equal, bf16_bits, fp8_dequant_ref, fp8_quant_ref
from _mxfp4_refs import roundtrip_ref
from test_gpu import gpu_server, local_conn  # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

NB, SEG = 8, 2048  # blocks; bf16 elements of one K or V half
PAGE = 2 * SEG
INVALID_REQ, FINISH = 400, 200
QUANTS = [None, "fp8", "mxfp4"]


def _keys(tag, n):
    pre = uuid.uuid4().hex
    return [f"seg-{tag}-{pre}-{i}" for i in range(n)]


def _pages(n, elems, seed):
    """n bf16 pages with a different magnitude per 32-element group."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(2.0, torch.randint(-12, 12, (n, elems // 32, 1), generator=g).float())
    x = torch.randn(n, elems // 32, 32, generator=g) * mag
    return x.reshape(n, elems).to(torch.bfloat16)


def _through_codec(pages: torch.Tensor, quant) -> np.ndarray:
    """uint16 bits of what a write + read of these (n, elems) pages returns."""
    if quant is None:
        return bf16_bits(pages)
    if quant == "fp8":
        codes, scales = fp8_quant_ref(pages)
        return bf16_bits(fp8_dequant_ref(codes, scales))
    return roundtrip_ref(pages)


def _table(n, seed):
    return np.random.RandomState(seed).permutation(n)


def _split(pages: torch.Tensor, table, S: int) -> torch.Tensor:
    """Lay logical pages out as a `[S, n, page/S]` cache: page p's segment s
    goes to [s, table[p]]."""
    n, elems = pages.shape
    cache = torch.zeros(S, n, elems // S, dtype=pages.dtype)
    cache[:, torch.as_tensor(table)] = pages.reshape(n, S, elems // S).transpose(0, 1)
    return cache


def _joined(cache: torch.Tensor, table) -> torch.Tensor:
    """The inverse of _split: (n, page) logical pages of a `[S, n, seg]` cache."""
    S, n, seg = cache.shape
    return cache[:, torch.as_tensor(table)].transpose(0, 1).reshape(n, S * seg)


@pytest.mark.parametrize("quant", QUANTS)
def test_segmented_write_contiguous_read(gpu_server, quant):
    pages = _pages(NB, PAGE, 1)
    table = _table(NB, 2)
    kv = _split(pages, table, 2).to("cuda:0")  # [2, NB, SEG]
    assert torch.equal(torch.cat([kv[0, table[3]], kv[1, table[3]]]).cpu(), pages[3])
    flat = torch.zeros(NB, PAGE, dtype=torch.bfloat16, device="cuda:0")
    keys = _keys("w", NB)
    conn = local_conn(gpu_server)
    try:
        conn.write_pages(kv.view(-1), keys, table * SEG, PAGE, sync=True, quant=quant,
                         segments=2, segment_stride=NB * SEG)
        conn.read_pages(flat.view(-1), keys, np.arange(NB) * PAGE, PAGE)
        conn.sync()
        assert_bf16_bits_equal(bf16_bits(flat), _through_codec(pages, quant), f"{quant}")
    finally:
        conn.delete_keys(keys)
        conn.close()


@pytest.mark.parametrize("quant", QUANTS)
def test_contiguous_write_segmented_read(gpu_server, quant):
    pages = _pages(NB, PAGE, 3)
    table = _table(NB, 4)
    flat = pages.to("cuda:0")
    kv = torch.zeros(2, NB, SEG, dtype=torch.bfloat16, device="cuda:0")
    keys = _keys("r", NB)
    conn = local_conn(gpu_server)
    try:
        conn.write_pages(flat.view(-1), keys, np.arange(NB) * PAGE, PAGE, sync=True, quant=quant)
        conn.read_pages(kv.view(-1), keys, table * SEG, PAGE, segments=2,
                        segment_stride=NB * SEG)
        conn.sync()
        assert_bf16_bits_equal(bf16_bits(_joined(kv.cpu(), table)),
                               _through_codec(pages, quant), f"{quant}")
    finally:
        conn.delete_keys(keys)
        conn.close()


@pytest.mark.parametrize("quant", QUANTS)
def test_written_with_two_segments_read_with_four(gpu_server, quant):
    pages = _pages(NB, PAGE, 5)
    wt, rt = _table(NB, 6), _table(NB, 7)
    kv2 = _split(pages, wt, 2).to("cuda:0")
    kv4 = torch.zeros(4, NB, SEG // 2, dtype=torch.bfloat16, device="cuda:0")
    keys = _keys("24", NB)
    conn = local_conn(gpu_server)
    try:
        conn.write_pages(kv2.view(-1), keys, wt * SEG, PAGE, sync=True, quant=quant,
                         segments=2, segment_stride=NB * SEG)
        conn.read_pages(kv4.view(-1), keys, rt * (SEG // 2), PAGE, segments=4,
                        segment_stride=NB * SEG // 2)
        conn.sync()
        assert_bf16_bits_equal(bf16_bits(_joined(kv4.cpu(), rt)),
                               _through_codec(pages, quant), f"{quant}")
    finally:
        conn.delete_keys(keys)
        conn.close()


@pytest.mark.parametrize("n", [16, 17])
def test_inline_path_boundary(gpu_server, n):
    """16 pages is the most the contiguous inline-argument launch takes; a
    segmented request of either size uses the pinned-descriptor kernels, and
    the contiguous read of the same keys sits on each side of the boundary."""
    seg = 256
    pages = _pages(n, 2 * seg, n)
    table = _table(n, n + 1)
    kv = _split(pages, table, 2).to("cuda:0")
    flat = torch.zeros(n, 2 * seg, dtype=torch.bfloat16, device="cuda:0")
    back = torch.zeros_like(kv)
    keys = _keys("in", n)
    conn = local_conn(gpu_server)
    try:
        conn.write_pages(kv.view(-1), keys, table * seg, 2 * seg, sync=True, segments=2,
                         segment_stride=n * seg)
        conn.read_pages(flat.view(-1), keys, np.arange(n) * 2 * seg, 2 * seg)
        conn.read_pages(back.view(-1), keys, table * seg, 2 * seg, segments=2,
                        segment_stride=n * seg)
        conn.sync()
        assert torch.equal(flat.cpu().view(torch.int16), pages.view(torch.int16))
        assert torch.equal(back.view(torch.int16), kv.view(torch.int16))
    finally:
        conn.delete_keys(keys)
        conn.close()


def test_uint8_odd_segments_take_the_byte_kernel(gpu_server):
    """513-byte segments of a uint8 tensor: nothing is a 16-byte multiple."""
    n, seg, S = 5, 513, 3
    g = torch.Generator().manual_seed(8)
    pages = torch.randint(0, 256, (n, S * seg), dtype=torch.uint8, generator=g)
    table = _table(n, 9)
    src = _split(pages, table, S).to("cuda:0")
    flat = torch.full((n, S * seg), 0xA5, dtype=torch.uint8, device="cuda:0")
    back = torch.full_like(src, 0xA5)
    keys = _keys("u8", n)
    conn = local_conn(gpu_server)
    try:
        conn.write_pages(src.view(-1), keys, table * seg, S * seg, sync=True, segments=S,
                         segment_stride=n * seg)
        conn.read_pages(flat.view(-1), keys, np.arange(n) * S * seg, S * seg)
        conn.read_pages(back.view(-1), keys, table * seg, S * seg, segments=S,
                        segment_stride=n * seg)
        conn.sync()
        assert torch.equal(flat.cpu(), pages)
        assert torch.equal(back, src)
    finally:
        conn.delete_keys(keys)
        conn.close()


def test_segmented_mixed_codec_read(gpu_server):
    """One segmented read_pages whose keys interleave plain, fp8 and mxfp4
    pages: one job per codec, each with the request's geometry."""
    n = 9
    pages = _pages(n, PAGE, 10)
    flat = pages.to("cuda:0")
    offs = np.arange(n, dtype=np.uint64) * PAGE
    kind = [QUANTS[i % 3] for i in range(n)]
    want = np.empty((n, PAGE), dtype=np.uint16)
    table = _table(n, 11)
    kv = torch.zeros(2, n, SEG, dtype=torch.bfloat16, device="cuda:0")
    keys = _keys("mix", n)
    conn = local_conn(gpu_server)
    try:
        for quant in QUANTS:
            rows = [i for i in range(n) if kind[i] == quant]
            want[rows] = _through_codec(pages[rows], quant)
            conn.write_pages(flat.view(-1), [keys[i] for i in rows], offs[rows], PAGE, sync=True,
                             quant=quant)
        conn.read_pages(kv.view(-1), keys, table * SEG, PAGE, segments=2, segment_stride=n * SEG)
        conn.sync()
        assert_bf16_bits_equal(bf16_bits(_joined(kv.cpu(), table)), want, "interleaved read")
    finally:
        conn.delete_keys(keys)
        conn.close()


@pytest.mark.parametrize("transport", ["shm", "socket"])
def test_segmented_async_read(gpu_server, transport, monkeypatch):
    """read_pages_async + wait_read, segmented, over the shm ring; with the ring
    disabled the same calls go over the socket."""
    if transport == "socket":
        monkeypatch.setenv("IFS_NO_SHM", "1")
    conn = local_conn(gpu_server)
    pages = _pages(NB, PAGE, 12)
    table = _table(NB, 13)
    kv = _split(pages, table, 2).to("cuda:0")
    outs = [torch.zeros_like(kv) for _ in range(2)]
    keys = _keys(transport, NB)
    try:
        assert conn.conn.shm_active() == (transport == "shm")
        conn.write_pages(kv.view(-1), keys, table * SEG, PAGE, sync=True, segments=2,
                         segment_stride=NB * SEG)
        tickets = [conn.read_pages_async(o.view(-1), keys, table * SEG, PAGE, segments=2,
                                         segment_stride=NB * SEG) for o in outs]
        for t in reversed(tickets):
            conn.wait_read(t)
        for o in outs:
            assert torch.equal(o.view(torch.int16), kv.view(torch.int16))
    finally:
        conn.delete_keys(keys)
        conn.close()


def _raw_request(sock, op, body):
    sock.sendall(struct.pack("<IcI", 0xDEADBEEF, op, len(body)) + body)
    buf = b""
    while len(buf) < 4:
        chunk = sock.recv(4 - len(buf))
        assert chunk, "server closed the connection"
        buf += chunk
    return struct.unpack("<i", buf)[0]


def test_illegal_extension_is_invalid_req_and_the_server_keeps_serving(gpu_server):
    """Hand-built packed requests on a raw socket: every illegal extension is
    answered INVALID_REQ with nothing written, and the next, legal, segmented
    request on the same socket is served."""
    pages = _pages(2, PAGE, 14)
    kv = _split(pages, [0, 1], 2).to("cuda:0")
    dst = torch.full((2, 2, SEG), 7.0, dtype=torch.bfloat16, device="cuda:0")
    handle, base_off = _native._dbg_ipc_export(kv.data_ptr())
    dhandle, dbase_off = _native._dbg_ipc_export(dst.data_ptr())
    keys = _keys("raw", 2)
    stride = 2 * SEG * 2  # bytes from K[b] to V[b]

    def body(h, off, ptr, flags, n_seg=2, seg_stride=stride, rsvd=0, cut=None):
        b = bytearray(_native._dbg_build_packed_local(
            0, os.getpid(), ptr - off, off, PAGE * 2, flags, 0, h, [0, SEG * 2], keys,
            n_segments=2, segment_stride=stride))
        b[104:120] = struct.pack("<IIQ", n_seg, rsvd, seg_stride)
        return bytes(b if cut is None else b[:cut])

    def w(**kw):
        return body(handle, base_off, kv.data_ptr(), 1, **kw)  # sync-response write

    def r(**kw):
        return body(dhandle, dbase_off, dst.data_ptr(), 1, **kw)

    conn = local_conn(gpu_server)
    s = socket.create_connection(("127.0.0.1", gpu_server), timeout=30)
    try:
        for bad in (dict(n_seg=0), dict(n_seg=1025), dict(rsvd=1), dict(n_seg=3),
                    dict(seg_stride=SEG * 2 - 16), dict(cut=104 + 8)):
            assert _raw_request(s, b"w", w(**bad)) == INVALID_REQ, bad
        # fp8 write: a stride that is not a 16-byte multiple
        assert _raw_request(s, b"w", body(handle, base_off, kv.data_ptr(), 1 | 2,
                                          seg_stride=stride + 8)) == INVALID_REQ
        assert not any(conn.check_exist(k) for k in keys)

        assert _raw_request(s, b"w", w()) == FINISH  # the same socket still serves
        assert all(conn.check_exist(k) for k in keys)
        for bad in (dict(n_seg=0), dict(n_seg=1025), dict(rsvd=1), dict(n_seg=3),
                    dict(seg_stride=SEG * 2 - 16)):
            assert _raw_request(s, b"r", r(**bad)) == INVALID_REQ, bad
        assert bool((dst == 7.0).all()), "a refused read must leave the destination untouched"
        assert _raw_request(s, b"r", r()) == FINISH
        torch.cuda.synchronize()
        assert torch.equal(dst.view(torch.int16), kv.view(torch.int16))
    finally:
        s.close()
        conn.delete_keys(keys)
        conn.close()


def test_compressed_entry_read_with_a_misaligned_stride_is_refused(gpu_server):
    """The read path checks the geometry against each ENTRY's codec: a stride
    of 8 bytes past a 16-byte multiple is fine for a plain page and
    INVALID_REQ for an fp8 one, whose destination stays untouched."""
    pages = _pages(1, PAGE, 15)
    flat = pages.to("cuda:0")
    dst = torch.zeros(2 * SEG + 64, dtype=torch.bfloat16, device="cuda:0")
    kp, kq = _keys("mis", 2)
    conn = local_conn(gpu_server)
    try:
        conn.write_pages(flat.view(-1), [kp], [0], PAGE, sync=True)
        conn.write_pages(flat.view(-1), [kq], [0], PAGE, sync=True, quant="fp8")
        with pytest.raises(Exception, match=f"-{INVALID_REQ}"):
            conn.read_pages(dst, [kq], [0], PAGE, segments=2, segment_stride=SEG + 4)
        assert bool((dst == 0).all())
        conn.read_pages(dst, [kp], [0], PAGE, segments=2, segment_stride=SEG + 4)
        conn.sync()
        got = torch.cat([dst[:SEG], dst[SEG + 4:2 * SEG + 4]]).cpu()
        assert torch.equal(got.view(torch.int16), pages[0].view(torch.int16))
        assert bool((dst[SEG:SEG + 4] == 0).all()) and bool((dst[2 * SEG + 4:] == 0).all())
    finally:
        conn.delete_keys([kp, kq])
        conn.close()


def test_python_refusals_send_nothing(gpu_server):
    """Every geometry write_pages / read_pages refuses is a ValueError before
    anything is sent: no key appears and the destination keeps its contents."""
    conn = local_conn(gpu_server)
    kv = _pages(1, 2 * NB * SEG, 16).to("cuda:0").view(-1)  # a [2, NB, SEG] cache
    assert kv.data_ptr() % 16 == 0
    dst = torch.zeros_like(kv)
    k = _keys("ve", 1)
    plane = NB * SEG
    bad = [
        dict(page_size=PAGE, segments=0, segment_stride=plane),
        dict(page_size=1025 * 8, segments=1025, segment_stride=8),
        dict(page_size=PAGE, segments=3, segment_stride=plane),  # does not divide
        dict(page_size=PAGE, segments=2, segment_stride=SEG - 1),  # overlap
        dict(page_size=PAGE, segments=2, segment_stride=plane + 1),  # one element out
    ]
    bad_quant = [
        ("fp8", dict(page_size=24, segments=2, segment_stride=plane)),  # 12-element segments
        ("mxfp4", dict(page_size=64, segments=4, segment_stride=64)),  # 16-element segments
        ("fp8", dict(page_size=PAGE, segments=2, segment_stride=SEG + 4)),  # stride % 16 bytes
        ("mxfp4", dict(page_size=PAGE, segments=2, segment_stride=SEG + 4)),
    ]
    try:
        last = (NB - 1) * SEG
        for kw in bad:
            with pytest.raises(ValueError):
                conn.write_pages(kv, k, [last], sync=True, **kw)
            with pytest.raises(ValueError):
                conn.read_pages(dst, k, [last], **kw)
            with pytest.raises(ValueError):
                conn.read_pages_async(dst, k, [last], **kw)
        for quant, kw in bad_quant:
            with pytest.raises(ValueError):
                conn.write_pages(kv, k, [0], sync=True, quant=quant, **kw)
        assert not conn.check_exist(k[0])
        assert bool((dst == 0).all())
        # the largest legal page: ends exactly at numel()
        conn.write_pages(kv, k, [last], PAGE, sync=True, segments=2, segment_stride=plane)
        assert conn.check_exist(k[0])
    finally:
        conn.delete_keys(k)
        conn.close()


@pytest.mark.parametrize("prefill,decode", [("kv_major", "block_major"),
                                            ("block_major", "kv_major"),
                                            ("kv_major", "kv_major")])
def test_adapter_layouts_share_pages(gpu_server, prefill, decode):
    """A prefill adapter with one cache layout and a decode adapter with the
    other, different block tables on the two sides: every layer's pages arrive
    equal to the source."""
    n_layers, block_tokens, n_pages, nblk = 2, 4, 6, 8
    tag = f"segtest-{uuid.uuid4().hex[:8]}"
    tokens = list(range(100, 100 + n_pages * block_tokens))
    pt = [int(b) for b in _table(nblk, 17)[:n_pages]]
    dt = [int(b) for b in _table(nblk, 18)[:n_pages]]

    def make(layout, layer_pages=None, table=None):
        """One layer's cache: [nblk, 2, SEG] or [2, nblk, SEG], holding
        layer_pages at `table` when given, zeros otherwise."""
        c = torch.zeros(nblk, 2, SEG, dtype=torch.bfloat16)
        if layer_pages is not None:
            c[torch.as_tensor(table)] = layer_pages.reshape(n_pages, 2, SEG)
        if layout == "kv_major":
            c = c.transpose(0, 1).contiguous()
        return c.to("cuda:0")

    def logical(cache, layout, table):
        c = cache.cpu()
        if layout == "kv_major":
            c = c.transpose(0, 1)
        return c[torch.as_tensor(table)].reshape(n_pages, PAGE)

    pages = [_pages(n_pages, PAGE, 20 + li) for li in range(n_layers)]
    pa = InfiniStoreKVAdapter("127.0.0.1", gpu_server, tag, n_layers, block_tokens, PAGE,
                              kv_layout=prefill)
    da = InfiniStoreKVAdapter("127.0.0.1", gpu_server, tag, n_layers, block_tokens, PAGE,
                              kv_layout=decode)
    try:
        # saves are asynchronous until wait_for_save: the sources stay alive
        sources = [make(prefill, pages[li], pt) for li in range(n_layers)]
        for li in range(n_layers):
            pa.save_kv_layer(li, sources[li], tokens, pt)
        pa.wait_for_save()
        assert da.get_num_new_matched_tokens(tokens) == len(tokens)
        caches = [make(decode) for _ in range(n_layers)]
        assert da.start_load_kv(caches, tokens, dt) == n_pages
        for li in range(n_layers):
            assert da.wait_for_layer_load(li)
            got = logical(caches[li], decode, dt)
            assert torch.equal(got.view(torch.int16), pages[li].view(torch.int16)), li
    finally:
        pa.evict_request(tokens)
        pa.close()
        da.close()


def test_fp8_segmented_and_contiguous_store_the_same(gpu_server):
    """The same data written segmented under one key set and contiguously under
    another takes the same number of pool blocks and reads back identically:
    one scale per page, not per segment."""
    pages = _pages(NB, PAGE, 30)
    pages[:, :SEG] *= 2.0 ** -8  # K halves far smaller than V halves
    table = _table(NB, 31)
    kv = _split(pages, table, 2).to("cuda:0")
    flat = pages.to("cuda:0")
    ks, kc = _keys("fs", NB), _keys("fc", NB)
    a = torch.zeros(NB, PAGE, dtype=torch.bfloat16, device="cuda:0")
    b = torch.zeros_like(a)
    offs = np.arange(NB) * PAGE
    conn = local_conn(gpu_server)
    try:
        used = lambda: json.loads(conn.get_server_stats_remote())["used_blocks"]  # noqa: E731
        u0 = used()
        conn.write_pages(kv.view(-1), ks, table * SEG, PAGE, sync=True, quant="fp8", segments=2,
                         segment_stride=NB * SEG)
        u1 = used()
        conn.write_pages(flat.view(-1), kc, offs, PAGE, sync=True, quant="fp8")
        u2 = used()
        assert u1 - u0 == u2 - u1 > 0, (u0, u1, u2)
        conn.read_pages(a.view(-1), ks, offs, PAGE)
        conn.read_pages(b.view(-1), kc, offs, PAGE)
        conn.sync()
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        assert_bf16_bits_equal(bf16_bits(a), _through_codec(pages, "fp8"), "fp8")
    finally:
        conn.delete_keys(ks + kc)
        conn.close()
