"""Sliced reads end to end: `read_pages(page_slice=...)` through a running
server. Pages of `[2, T, H, hd]` written whole by a "prefill" client are read
head range by head range, into block-major and kv-major caches, and compared
bit for bit with the whole page (the reference round trip of its codec, and the
server's own whole-page read) sliced in torch."""

import json
import os
import socket
import struct
import uuid

import numpy as np
import pytest
import torch

from infinistore_amd import _native, PageSlice
from infinistore_amd.vllm_adapter import InfiniStoreKVAdapter

from _kernel_refs import assert_bf16_bits_equal, bf16_bits, fp8_dequant_ref, fp8_quant_ref
from _mxfp4_refs import roundtrip_ref
from test_gpu import gpu_server, local_conn  # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

T, H, HD = 4, 4, 32
PAGE = 2 * T * H * HD  # bf16 elements of a stored page
INVALID_REQ, KEY_NOT_FOUND, FINISH = 400, 404, 200
QUANTS = [None, "fp8", "mxfp4"]
HEAD_RANGES = [(0, 2), (2, 4), (1, 2)]


def _keys(tag, n):
    pre = uuid.uuid4().hex
    return [f"slice-{tag}-{pre}-{i}" for i in range(n)]


def _pages(n, elems, seed):
    """n bf16 pages with a different magnitude per 32-element group."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(2.0, torch.randint(-12, 12, (n, elems // 32, 1), generator=g).float())
    x = torch.randn(n, elems // 32, 32, generator=g) * mag
    return x.reshape(n, elems).to(torch.bfloat16)


def _through_codec(pages: torch.Tensor, quant) -> torch.Tensor:
    """(n, elems) int16 bits of what a write + whole read of these pages returns."""
    if quant is None:
        bits = bf16_bits(pages)
    elif quant == "fp8":
        codes, scales = fp8_quant_ref(pages)
        bits = bf16_bits(fp8_dequant_ref(codes, scales))
    else:
        bits = roundtrip_ref(pages)
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).reshape(pages.shape))


def _heads(whole: torch.Tensor, h0, h1) -> torch.Tensor:
    """(n, PAGE) -> (n, 2, T, h1-h0, HD): the head slice, in torch."""
    return whole.reshape(-1, 2, T, H, HD)[:, :, :, h0:h1]


def _slice(h0, h1):
    return PageSlice(page_size=PAGE, offset=h0 * HD, piece=(h1 - h0) * HD, stride=H * HD,
                     count=2 * T)


def _table(n, seed):
    return np.random.RandomState(seed).permutation(n)


def _read_heads(conn, keys, table, h0, h1, layout, read=None):
    """Read heads h0..h1 of `keys` into a fresh cache of `layout`, page p into
    block table[p]; returns (n, 2, T, h, HD) int16 bits in page order."""
    n, h = len(keys), h1 - h0
    half = T * h * HD
    read = read or conn.read_pages
    if layout == "block_major":
        cache = torch.zeros(n, 2, T, h, HD, dtype=torch.bfloat16, device="cuda:0")
        read(cache.view(-1), keys, table * (2 * half), 2 * half, page_slice=_slice(h0, h1))
        conn.sync()
        return cache.cpu()[torch.as_tensor(table)].view(torch.int16)
    cache = torch.zeros(2, n, T, h, HD, dtype=torch.bfloat16, device="cuda:0")
    read(cache.view(-1), keys, table * half, 2 * half, segments=2, segment_stride=n * half,
         page_slice=_slice(h0, h1))
    conn.sync()
    return cache.cpu()[:, torch.as_tensor(table)].transpose(0, 1).contiguous().view(torch.int16)


def _eq(got, want, what=""):
    assert_bf16_bits_equal(got.contiguous().numpy().view(np.uint16),
                           want.contiguous().numpy().view(np.uint16), what)


@pytest.fixture(scope="module")
def stored(gpu_server):  # noqa: F811
    """Per codec: keys of N pages written whole, the reference bits of their
    whole read, and the server's own whole read. Written once for the module."""
    n = 6
    conn = local_conn(gpu_server)
    out = {}
    all_keys = []
    for qi, quant in enumerate(QUANTS):
        pages = _pages(n, PAGE, 50 + qi)
        flat = pages.to("cuda:0")
        keys = _keys(str(quant), n)
        conn.write_pages(flat.view(-1), keys, np.arange(n) * PAGE, PAGE, sync=True, quant=quant)
        back = torch.zeros_like(flat)
        conn.read_pages(back.view(-1), keys, np.arange(n) * PAGE, PAGE)
        conn.sync()
        want = _through_codec(pages, quant)
        _eq(back.cpu().view(torch.int16), want, f"whole read {quant}")
        out[quant] = (keys, want)
        all_keys += keys
    yield out
    conn.delete_keys(all_keys)
    conn.close()


@pytest.mark.parametrize("layout", ["block_major", "kv_major"])
@pytest.mark.parametrize("heads", HEAD_RANGES)
@pytest.mark.parametrize("quant", QUANTS)
def test_head_slices(gpu_server, stored, quant, heads, layout):
    keys, want = stored[quant]
    conn = local_conn(gpu_server)
    try:
        got = _read_heads(conn, keys, _table(len(keys), 3), *heads, layout)
        _eq(got, _heads(want, *heads), f"{quant} {heads} {layout}")
    finally:
        conn.close()


@pytest.mark.parametrize("quant", QUANTS)
def test_two_ranks_reassemble_the_page(gpu_server, stored, quant):
    keys, want = stored[quant]
    conn = local_conn(gpu_server)
    try:
        lo = _read_heads(conn, keys, _table(len(keys), 4), 0, 2, "kv_major")
        hi = _read_heads(conn, keys, _table(len(keys), 5), 2, 4, "block_major")
        _eq(torch.cat([lo, hi], dim=3).reshape(len(keys), PAGE), want, f"{quant}")
    finally:
        conn.close()


def test_all_three_codecs_in_one_request(gpu_server, stored):
    # keys interleaved plain, fp8, mxfp4: one job per codec, same geometry
    n = len(stored[None][0])
    keys = [stored[QUANTS[i % 3]][0][i] for i in range(n)]
    want = torch.stack([stored[QUANTS[i % 3]][1][i] for i in range(n)])
    conn = local_conn(gpu_server)
    try:
        stats = lambda: json.loads(conn.get_server_stats_remote())  # noqa: E731
        out0 = stats()["bytes_out"]
        got = _read_heads(conn, keys, _table(n, 6), 1, 3, "kv_major")
        _eq(got, _heads(want, 1, 3), "interleaved codecs")
        # the counter takes delivered bytes: n sliced pages of 2 * T * 2 heads
        assert stats()["bytes_out"] - out0 == n * 2 * T * 2 * HD * 2
    finally:
        conn.close()


@pytest.mark.parametrize("transport", ["shm", "socket"])
@pytest.mark.parametrize("quant", QUANTS)
def test_both_transports_blocking_and_ticketed(gpu_server, stored, quant, transport, monkeypatch):
    if transport == "socket":
        monkeypatch.setenv("IFS_NO_SHM", "1")
    keys, want = stored[quant]
    conn = local_conn(gpu_server)
    try:
        assert conn.conn.shm_active() == (transport == "shm")
        tickets = []

        def ticketed(*a, **kw):
            tickets.append(conn.read_pages_async(*a, **kw))
            conn.wait_read(tickets[-1])

        for layout in ("block_major", "kv_major"):
            got = _read_heads(conn, keys, _table(len(keys), 7), 2, 4, layout)
            _eq(got, _heads(want, 2, 4), f"blocking {transport} {layout}")
            got = _read_heads(conn, keys, _table(len(keys), 8), 2, 4, layout, read=ticketed)
            _eq(got, _heads(want, 2, 4), f"ticketed {transport} {layout}")
        assert len(tickets) == 2 and all(bool(t) == (transport == "shm") for t in tickets)
    finally:
        conn.close()


@pytest.mark.parametrize("n", [5, 16, 17, 40])
def test_around_the_inline_path_boundary(gpu_server, n):
    """The contiguous copy takes up to 16 aligned blocks inline; a sliced
    request of any size must not."""
    pages = _pages(n, PAGE, n)
    flat = pages.to("cuda:0")
    keys = _keys("in", n)
    conn = local_conn(gpu_server)
    try:
        conn.write_pages(flat.view(-1), keys, np.arange(n) * PAGE, PAGE, sync=True)
        for layout in ("block_major", "kv_major"):
            got = _read_heads(conn, keys, _table(n, n + 1), 1, 2, layout)
            _eq(got, _heads(pages.view(torch.int16), 1, 2), f"{n} {layout}")
    finally:
        conn.delete_keys(keys)
        conn.close()


def test_uint8_pages_take_the_byte_kernel(gpu_server):
    """Odd piece, offset and stride of a uint8 tensor: nothing is 16-byte aligned."""
    n, page, off, piece, stride, count = 5, 3001, 7, 13, 331, 9
    g = torch.Generator().manual_seed(9)
    pages = torch.randint(0, 256, (n, page), dtype=torch.uint8, generator=g)
    src = pages.to("cuda:0")
    dst = torch.full((n, count * piece + 3), 0xA5, dtype=torch.uint8, device="cuda:0")
    keys = _keys("u8", n)
    conn = local_conn(gpu_server)
    try:
        conn.write_pages(src.view(-1), keys, np.arange(n) * page, page, sync=True)
        conn.read_pages(dst.view(-1), keys, np.arange(n) * (count * piece + 3), count * piece,
                        page_slice=PageSlice(page, off, piece, stride, count))
        conn.sync()
        idx = (off + torch.arange(count)[:, None] * stride + torch.arange(piece)[None, :])
        assert torch.equal(dst.cpu()[:, :count * piece], pages[:, idx.reshape(-1)])
        assert bool((dst[:, count * piece:] == 0xA5).all())
    finally:
        conn.delete_keys(keys)
        conn.close()


def test_refused_by_the_server(gpu_server, stored):
    """INVALID_REQ for a slice cut for another page size (plain and fp8 keys)
    and for a geometry off the entry's codec multiple; KEY_NOT_FOUND for a
    mixed request with one key missing. The destination stays untouched."""
    conn = local_conn(gpu_server)
    dst = torch.full((8 * PAGE,), 7.0, dtype=torch.bfloat16, device="cuda:0")
    half = _slice(0, 2)
    sliced = half.count * half.piece
    try:
        for quant in QUANTS:
            keys = stored[quant][0]
            offs = np.arange(len(keys)) * sliced
            # the same heads of a page twice the size: legal, but not what was written
            big = half._replace(page_size=2 * PAGE)
            for read in (conn.read_pages, lambda *a, **kw: conn.wait_read(
                    conn.read_pages_async(*a, **kw))):
                with pytest.raises(Exception, match=f"{INVALID_REQ}"):
                    read(dst, keys, offs, sliced, page_slice=big)
            small = PageSlice(PAGE // 2, 0, 2 * HD, H * HD, T)
            with pytest.raises(Exception, match=f"-{INVALID_REQ}"):
                conn.read_pages(dst, keys, offs[:len(keys)] // 2, T * 2 * HD, page_slice=small)
        # 8-element steps: whole lanes for fp8, part of a group for mxfp4
        fine = PageSlice(PAGE, 8, 8, 24, 4)
        conn.read_pages(dst[PAGE:], stored[None][0][:1], [0], 32, page_slice=fine)
        conn.read_pages(dst[PAGE:], stored["fp8"][0][:1], [32], 32, page_slice=fine)
        with pytest.raises(Exception, match=f"-{INVALID_REQ}"):
            conn.read_pages(dst[PAGE:], stored["mxfp4"][0][:1], [64], 32, page_slice=fine)
        odd = PageSlice(PAGE, 4, 8, 24, 4)  # off the lane unit: plain pages only
        conn.read_pages(dst[PAGE:], stored[None][0][:1], [64], 32, page_slice=odd)
        with pytest.raises(Exception, match=f"-{INVALID_REQ}"):
            conn.read_pages(dst[PAGE:], stored["fp8"][0][:1], [96], 32, page_slice=odd)
        # a compressed entry needs a 16-byte-aligned client address
        with pytest.raises(Exception, match=f"-{INVALID_REQ}"):
            conn.read_pages(dst, stored["fp8"][0][:1], [4], sliced, page_slice=half)
        conn.sync()
        assert bool((dst[:PAGE] == 7.0).all()) and bool((dst[PAGE + 96:] == 7.0).all())
        want = stored[None][1][0]
        got = dst[PAGE:PAGE + 96].cpu().view(torch.int16)
        assert torch.equal(got[:32], torch.cat([want[8 + 24 * p:16 + 24 * p] for p in range(4)]))
        assert torch.equal(got[64:], torch.cat([want[4 + 24 * p:12 + 24 * p] for p in range(4)]))
        want8 = stored["fp8"][1][0]
        _eq(got[32:64], torch.cat([want8[8 + 24 * p:16 + 24 * p] for p in range(4)]), "fp8")
        # one key of a mixed request is missing
        dst.fill_(7.0)
        torch.cuda.synchronize()
        keys = [stored[None][0][0], stored["fp8"][0][1], "slice-no-such-key",
                stored["mxfp4"][0][2]]
        with pytest.raises(Exception, match=f"-{KEY_NOT_FOUND}"):
            conn.read_pages(dst, keys, np.arange(4) * sliced, sliced, page_slice=half)
        assert bool((dst == 7.0).all()), "a refused read must leave the destination untouched"
    finally:
        conn.close()


def _raw_request(sock, op, body):
    sock.sendall(struct.pack("<IcI", 0xDEADBEEF, op, len(body)) + body)
    buf = b""
    while len(buf) < 4:
        chunk = sock.recv(4 - len(buf))
        assert chunk, "server closed the connection"
        buf += chunk
    return struct.unpack("<i", buf)[0]


def test_illegal_extension_is_invalid_req_and_the_server_keeps_serving(gpu_server, stored):
    """Hand-built packed requests on a raw socket: every illegal slice
    extension is answered INVALID_REQ with nothing written; the legal one on
    the same socket is then served."""
    keys, want = stored[None]
    keys = keys[:2]
    half = T * 2 * HD * 2  # bytes of the K (or V) half of a two-head sliced page
    dst = torch.full((2, 2, T, 2, HD), 7.0, dtype=torch.bfloat16, device="cuda:0")
    handle, base_off = _native._dbg_ipc_export(dst.data_ptr())
    good = (2 * T, PAGE * 2, 2 * HD * 2, 2 * HD * 2, H * HD * 2)  # heads 2..4, in bytes

    def body(op_flags=1, ext=good, rsvd=0, block_size=2 * half, cut=None, seg=None):
        kw = dict(n_segments=seg[0], segment_stride=seg[1]) if seg else {}
        b = bytearray(_native._dbg_build_packed_local(
            0, os.getpid(), dst.data_ptr() - base_off, base_off, block_size, op_flags, 0, handle,
            [0, 2 * half], keys, slice=good, **kw))
        pos = 104 + (16 if seg else 0)
        b[pos:pos + 40] = struct.pack("<IIQQQQ", ext[0], rsvd, *ext[1:])
        return bytes(b if cut is None else b[:cut])

    def ext(**kw):
        names = ["n", "page", "offset", "piece", "stride"]
        v = dict(zip(names, good))
        v.update(kw)
        return tuple(v[k] for k in names)

    s = socket.create_connection(("127.0.0.1", gpu_server), timeout=30)
    try:
        bad = [dict(ext=ext(n=0)), dict(ext=ext(n=4097)), dict(rsvd=1),
               dict(ext=ext(n=T)),  # block_size != n * piece
               dict(block_size=half),
               dict(ext=ext(stride=2 * HD * 2 - 2)),  # pieces overlap
               dict(ext=ext(offset=3 * HD * 2)),  # the last piece leaves the page
               dict(ext=ext(page=PAGE * 2 - 2)),
               dict(ext=ext(page=PAGE * 4)),  # legal geometry, not the written page
               dict(cut=104 + 20),
               dict(seg=(3, 1 << 16)),  # 8 pieces into 3 segments
               dict(seg=(2, half - 16))]  # client segments overlap
        for kw in bad:
            assert _raw_request(s, b"r", body(**kw)) == INVALID_REQ, kw
        assert _raw_request(s, b"w", body()) == INVALID_REQ  # no sliced writes
        torch.cuda.synchronize()
        assert bool((dst == 7.0).all()), "a refused read must leave the destination untouched"
        assert _raw_request(s, b"r", body()) == FINISH  # the same socket still serves
        torch.cuda.synchronize()
        _eq(dst.cpu().view(torch.int16), _heads(want[:2], 2, 4), "raw legal read")
    finally:
        s.close()


def test_python_refusals_send_nothing(gpu_server, stored):
    conn = local_conn(gpu_server)
    keys = stored[None][0][:1]
    dst = torch.zeros(2 * PAGE, dtype=torch.bfloat16, device="cuda:0")
    sl = _slice(0, 2)
    sliced = sl.count * sl.piece
    try:
        stats = lambda: json.loads(conn.get_server_stats_remote())  # noqa: E731
        before = stats()["reads"]
        for read in (conn.read_pages, conn.read_pages_async):
            for kw in (dict(page_size=sliced, page_slice=sl._replace(count=0)),
                       dict(page_size=sliced, page_slice=sl._replace(stride=sl.piece - 1)),
                       dict(page_size=sliced, page_slice=sl._replace(offset=3 * HD)),
                       dict(page_size=sliced + 8, page_slice=sl),
                       dict(page_size=sliced, page_slice=sl, segments=3, segment_stride=PAGE)):
                with pytest.raises(ValueError):
                    read(dst, keys, [0], **kw)
            with pytest.raises(ValueError):
                read(dst, keys, [2 * PAGE - sliced + 1], sliced, page_slice=sl)
        with pytest.raises(ValueError, match="read-only"):
            conn.write_pages(dst, keys, [0], sliced, page_slice=sl)
        assert stats()["reads"] == before, "a refused read was served"
        assert bool((dst == 0).all())
    finally:
        conn.close()


@pytest.mark.parametrize("quant", [None, "mxfp4"])
@pytest.mark.parametrize("layout", ["block_major", "kv_major"])
def test_decode_adapter_with_half_the_heads(gpu_server, layout, quant):
    """A full-head prefill adapter saves; a decode adapter that owns heads 2..4
    of the 4 stored ones, in either layout and with its own block table, loads
    exactly that half of every page."""
    n_layers, n_pages, nblk, h0, h1 = 2, 5, 7, 2, 4
    h = h1 - h0
    tag = f"slicetest-{uuid.uuid4().hex[:8]}"
    tokens = list(range(300, 300 + n_pages * T))
    pt = [int(b) for b in _table(nblk, 21)[:n_pages]]
    dt = [int(b) for b in _table(nblk, 22)[:n_pages]]
    pages = [_pages(n_pages, PAGE, 60 + li) for li in range(n_layers)]
    pa = InfiniStoreKVAdapter("127.0.0.1", gpu_server, tag, n_layers, T, PAGE, quant=quant)
    da = InfiniStoreKVAdapter("127.0.0.1", gpu_server, tag, n_layers, T, 2 * T * h * HD,
                              kv_layout=layout, stored_kv_heads=H, head_range=(h0, h1),
                              head_dim=HD)
    try:
        sources = []
        for li in range(n_layers):
            c = torch.zeros(nblk, PAGE, dtype=torch.bfloat16)
            c[torch.as_tensor(pt)] = pages[li]
            sources.append(c.to("cuda:0"))
            pa.save_kv_layer(li, sources[li], tokens, pt)
        pa.wait_for_save()
        with pytest.raises(ValueError, match="load-only"):
            da.save_kv_layer(0, sources[0], tokens, pt)
        assert da.get_num_new_matched_tokens(tokens) == len(tokens)
        shape = (nblk, 2, T, h, HD) if layout == "block_major" else (2, nblk, T, h, HD)
        caches = [torch.zeros(shape, dtype=torch.bfloat16, device="cuda:0")
                  for _ in range(n_layers)]
        assert da.start_load_kv(caches, tokens, dt) == n_pages
        for li in range(n_layers):
            assert da.wait_for_layer_load(li)
            c = caches[li].cpu()
            if layout == "kv_major":
                c = c.transpose(0, 1)
            got = c[torch.as_tensor(dt)].contiguous().view(torch.int16)
            _eq(got, _heads(_through_codec(pages[li], quant), h0, h1), f"layer {li}")
            rest = torch.ones(nblk, dtype=torch.bool)
            rest[torch.as_tensor(dt)] = False
            assert bool((c[rest] == 0).all()), "blocks outside the table were written"
    finally:
        pa.evict_request(tokens)
        pa.close()
        da.close()
