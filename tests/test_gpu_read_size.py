"""The read-size rule on the local GPU path (docs/protocol.md, "read sizes"):
a plain entry serves a whole-page read of at most its own size and returns
that prefix; a larger page is INVALID_REQ before any launch, the destination
stays untouched and the connection keeps serving. Over every way a read
reaches Server::op_local_read: ring and socket, blocking and ticketed,
contiguous and 2-segment destinations, the inline launch (at most 16 blocks)
and the descriptor launch (17), read_cache and the reference's flatbuffers
'R', and the byte kernel.

The keys under test are the FIRST keys of one write of 24 equal pages, which
the pool places as one run of blocks: a server without the rule would read at
most one stored page too far, inside that run, never out of the arena. At this
server's 64 KiB granule every 1 KiB page has a block of its own, so such an
over-read would end in the block's own padding, not in a neighbour's bytes;
the tests that show a neighbour's bytes returned by a server without the rule
are the CPU ones (tests/test_e2e_cpu.py, 16 KiB granule, keys of one granule
and of one granule plus 16)."""

import json
import socket as socklib
import struct
import uuid

import numpy as np
import pytest
import torch

from infinistore_amd import _native
from _kernel_refs import bf16_bits, bf16_from_bits
from test_gpu import gpu_server, local_conn  # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

INVALID_REQ = "-400"
ELEMS = 512  # bf16 elements of the stored pages
N_KEYS = 24
SLOT = 2 * ELEMS + 16  # destination elements per block: the largest page plus a guard
SENT16 = 0xA5A5
U8_BYTES, U8_KEYS, U8_SLOT = 1000, 8, 1040


def _sentinel(n, dtype=torch.bfloat16):
    t = torch.empty(n, dtype=dtype, device="cuda:0")
    t.view(torch.uint8).fill_(0xA5)
    return t


@pytest.fixture(scope="module")
def stored(gpu_server):
    """(keys, bits (N_KEYS, ELEMS) uint16, compressed keys, u8 keys, u8 bytes)."""
    pre = uuid.uuid4().hex[:10]
    rs = np.random.RandomState(5)
    bits = rs.randint(0, 1 << 16, (N_KEYS, ELEMS)).astype(np.uint16)
    bits[bits == SENT16] = 0x3F80  # never the sentinel: "copied" and "untouched" differ
    keys = [f"rs-{pre}-{i}" for i in range(N_KEYS)]
    qpages = (torch.randn(4, 2 * ELEMS, generator=torch.Generator().manual_seed(6)) * 3
              ).to(torch.bfloat16)
    qkeys = {"fp8": [f"rs-{pre}-f{i}" for i in range(2)],
             "mxfp4": [f"rs-{pre}-m{i}" for i in range(2)]}
    u8 = rs.randint(0, 255, (U8_KEYS, U8_BYTES)).astype(np.uint8)
    u8[u8 == 0xA5] = 255
    u8keys = [f"rs-{pre}-b{i}" for i in range(U8_KEYS)]
    conn = local_conn(gpu_server)
    try:
        src = bf16_from_bits(bits.reshape(-1)).to("cuda:0")
        conn.write_pages(src, keys, [i * ELEMS for i in range(N_KEYS)], ELEMS, sync=True)
        qsrc = qpages.reshape(-1).to("cuda:0")
        conn.write_pages(qsrc, qkeys["fp8"], [0, 2 * ELEMS], 2 * ELEMS, sync=True, quant="fp8")
        conn.write_pages(qsrc, qkeys["mxfp4"], [4 * ELEMS, 6 * ELEMS], 2 * ELEMS, sync=True,
                         quant="mxfp4")
        bsrc = torch.from_numpy(u8.reshape(-1)).to("cuda:0")
        conn.write_pages(bsrc, u8keys, [i * U8_BYTES for i in range(U8_KEYS)], U8_BYTES,
                         sync=True)
        yield keys, bits, qkeys, u8keys, u8
        conn.delete_keys(keys + qkeys["fp8"] + qkeys["mxfp4"] + u8keys)
    finally:
        conn.close()


def _counters(conn):
    s = json.loads(conn.get_server_stats_remote())
    return s["reads"], s["bytes_out"]


def _read(conn, mode, dst, keys, offs, page, segments, stride):
    if mode == "blocking":
        conn.read_pages(dst, keys, offs, page, segments=segments, segment_stride=stride)
        conn.sync()
    elif mode == "ticketed":
        conn.wait_read(conn.read_pages_async(dst, keys, offs, page, segments=segments,
                                             segment_stride=stride))
    else:
        assert mode == "read_cache" and segments == 1
        conn.read_cache(dst, list(zip(keys, offs)), page)
        conn.sync()


CASES = [(t, m, s, n) for t in ("ring", "socket") for m in ("blocking", "ticketed")
         for s in (1, 2) for n in (3, 17)]
CASES += [(t, "read_cache", 1, n) for t in ("ring", "socket") for n in (3, 17)]


@pytest.mark.parametrize("transport,mode,segments,n", CASES)
def test_plain_read_sizes(gpu_server, stored, monkeypatch, transport, mode, segments, n):
    keys, bits = stored[0][:n], stored[1][:n]
    if transport == "socket":
        monkeypatch.setenv("IFS_NO_SHM", "1")
    conn = local_conn(gpu_server)
    try:
        assert conn.conn.shm_active() == (transport == "ring")
        half = n * SLOT  # a 2-segment page has its second half `half` elements on
        offs = [j * SLOT for j in range(n)]

        def expect(page):
            want = np.full(2 * half, SENT16, dtype=np.uint16)
            seg = page // segments
            for j in range(n):
                for s in range(segments):
                    want[offs[j] + s * half:offs[j] + s * half + seg] = \
                        bits[j, s * seg:(s + 1) * seg]
            return want

        for page in (ELEMS + 8, 2 * ELEMS):
            dst = _sentinel(2 * half)
            before = _counters(conn)
            with pytest.raises(Exception, match=INVALID_REQ):
                _read(conn, mode, dst, keys, offs, page, segments, half)
            assert _counters(conn) == before, page
            assert bool((dst.view(torch.uint8) == 0xA5).all()), page
        for page in (ELEMS // 2, ELEMS):  # the prefix, then the whole page: still serving
            dst = _sentinel(2 * half)
            before = _counters(conn)
            _read(conn, mode, dst, keys, offs, page, segments, half)
            assert np.array_equal(bf16_bits(dst), expect(page)), page
            assert _counters(conn) == (before[0] + 1, before[1] + n * page * 2), page
    finally:
        conn.close()


def test_flatbuffers_read_sizes(gpu_server, stored):
    """The reference-framed 'R' (flatbuffers LocalMetaRequest on a raw socket):
    400 for a page larger than the entry, 202 and the prefix for a smaller."""
    keys, bits = stored[0], stored[1]
    dst = _sentinel(SLOT)
    handle, base_off = _native._dbg_ipc_export(dst.data_ptr())
    probe = local_conn(gpu_server)
    s = socklib.create_connection(("127.0.0.1", gpu_server), timeout=30)

    def request(page):
        body = _native._dbg_build_local_meta(0, handle, page * 2, [(keys[0], 0)], base_off)
        s.sendall(struct.pack("<IcI", 0xDEADBEEF, b"R", len(body)) + body)
        return struct.unpack("<i", s.recv(4))[0]

    try:
        for page in (ELEMS + 8, 2 * ELEMS):
            before = _counters(probe)
            assert request(page) == 400, page
            assert _counters(probe) == before
            assert bool((dst.view(torch.uint8) == 0xA5).all()), page
        assert request(ELEMS // 2) == 202
        for _ in range(1000):  # reference-framed sync until nothing is in flight
            s.sendall(struct.pack("<IcI", 0xDEADBEEF, b"S", 0))
            buf = b""
            while len(buf) < 8:
                buf += s.recv(8 - len(buf))
            code, remain = struct.unpack("<ii", buf)
            assert code == 200
            if remain == 0:
                break
        assert remain == 0
        got = bf16_bits(dst)
        assert np.array_equal(got[:ELEMS // 2], bits[0, :ELEMS // 2])
        assert bool((got[ELEMS // 2:] == SENT16).all())
    finally:
        s.close()
        probe.close()


@pytest.mark.parametrize("transport", ["ring", "socket"])
def test_byte_kernel_read_sizes(gpu_server, stored, monkeypatch, transport):
    """uint8 pages of 1000 bytes: 1001 and 2000 are refused, 999 (no multiple
    of 16: the byte kernel) returns the prefix."""
    u8keys, u8 = stored[3], stored[4]
    if transport == "socket":
        monkeypatch.setenv("IFS_NO_SHM", "1")
    conn = local_conn(gpu_server)
    try:
        n = 3
        offs = [j * 2 * U8_SLOT for j in range(n)]
        for page in (U8_BYTES + 1, 2 * U8_BYTES):
            dst = _sentinel(n * 2 * U8_SLOT, torch.uint8)
            before = _counters(conn)
            with pytest.raises(Exception, match=INVALID_REQ):
                conn.read_pages(dst, u8keys[:n], offs, page)
            assert _counters(conn) == before
            assert bool((dst == 0xA5).all()), page
        for page in (U8_BYTES - 1, U8_BYTES // 2, U8_BYTES):
            dst = _sentinel(n * 2 * U8_SLOT, torch.uint8)
            conn.read_pages(dst, u8keys[:n], offs, page)
            conn.sync()
            want = np.full(n * 2 * U8_SLOT, 0xA5, dtype=np.uint8)
            for j in range(n):
                want[offs[j]:offs[j] + page] = u8[j, :page]
            assert np.array_equal(dst.cpu().numpy(), want), page
    finally:
        conn.close()


@pytest.mark.parametrize("transport", ["ring", "socket"])
@pytest.mark.parametrize("mode", ["blocking", "ticketed"])
def test_mixed_request_with_a_short_plain_entry_is_refused_whole(gpu_server, stored,
                                                                 monkeypatch, mode, transport):
    """fp8 and mxfp4 entries of the requested size next to a plain entry of
    half of it: nothing is launched for any of them, for a contiguous and for
    a 2-segment destination."""
    keys, bits, qkeys = stored[0], stored[1], stored[2]
    page = 2 * ELEMS
    if transport == "socket":
        monkeypatch.setenv("IFS_NO_SHM", "1")
    conn = local_conn(gpu_server)
    try:
        assert conn.conn.shm_active() == (transport == "ring")
        good = qkeys["fp8"] + qkeys["mxfp4"]
        orders = ([keys[0]] + good, good + [keys[0]], good[:2] + [keys[0]] + good[2:])
        for order, segments in [(o, sg) for o in orders for sg in (1, 2)]:
            offs = [j * SLOT for j in range(len(order))]
            half = len(order) * SLOT  # second segments start here
            dst = _sentinel(2 * half)
            before = _counters(conn)
            with pytest.raises(Exception, match=INVALID_REQ):
                _read(conn, mode, dst, order, offs, page, segments, half)
            assert _counters(conn) == before
            assert bool((dst.view(torch.uint8) == 0xA5).all())
        # the good ones alone are served, and the short one at its own size
        dst = _sentinel(5 * SLOT)
        _read(conn, mode, dst, good, [j * SLOT for j in range(4)], page, 1, 0)
        _read(conn, mode, dst, keys[:1], [4 * SLOT], ELEMS, 1, 0)
        got = bf16_bits(dst).reshape(5, SLOT)
        assert bool((got[:4, :page] != SENT16).any(axis=1).all())
        assert bool((got[:, page:] == SENT16).all())
        assert np.array_equal(got[4, :ELEMS], bits[0])
        assert bool((got[4, ELEMS:] == SENT16).all())
    finally:
        conn.close()
