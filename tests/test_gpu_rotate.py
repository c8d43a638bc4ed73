"""Rotated reads through a running server. Oracle: the whole read of the same keys, rotated
by the same formula in torch float64, within one bf16 rounding of the result plus the float32
evaluation error: |got - ref| <= 2^-8 |ref| + 2^-21 (|a| + |b|)."""

import os
import socket

import numpy as np
import pytest
import torch

from infinistore_amd import PageRotate, _native

from test_gpu import gpu_server, local_conn  # noqa: F401  (fixture + helper)
from test_gpu_permute import _keys
from test_gpu_slices import _eq, _raw_request, _table

pytestmark = pytest.mark.gpu

T, H, HD = 16, 4, 64
PAGE = 2 * T * H * HD
ROT = PageRotate.from_delta(37, H, HD)
QUANTS, INVALID_REQ, FINISH = [None, "fp8", "mxfp4"], 400, 200


def _read(conn, keys, table, ticketed, **kw):  # page p into block table[p] of a fresh cache
    cache = torch.zeros(len(keys), PAGE, dtype=torch.bfloat16, device="cuda:0")
    if ticketed:
        conn.wait_read(conn.read_pages_async(cache.view(-1), keys, table * PAGE, PAGE, **kw))
    else:
        conn.read_pages(cache.view(-1), keys, table * PAGE, PAGE, **kw)
    conn.sync()
    return cache.cpu()[torch.as_tensor(table)]


def _assert_rotated(got, whole, rot, what):
    g, x = (t.double().reshape(-1, 2, T, H, HD) for t in (got, whole))
    P = rot.rot_dim // 2
    cs = torch.from_numpy(rot.cos_sin).double()
    a, b = x[:, 0, ..., :P], x[:, 0, ..., P:2 * P]
    ref = x.clone()
    ref[:, 0, ..., :P] = a * cs[:, 0] - b * cs[:, 1]
    ref[:, 0, ..., P:2 * P] = b * cs[:, 0] + a * cs[:, 1]
    mag = torch.zeros_like(x)
    mag[:, 0, ..., :P] = mag[:, 0, ..., P:2 * P] = a.abs() + b.abs()
    assert bool(((g - ref).abs() <= 2.0 ** -8 * ref.abs() + 2.0 ** -21 * mag).all()), what
    _eq(got.reshape(-1, 2, T * H * HD)[:, 1].view(torch.int16),
        whole.reshape(-1, 2, T * H * HD)[:, 1].view(torch.int16), "V " + what)


@pytest.mark.parametrize("transport", ["shm", "socket"])
@pytest.mark.parametrize("n", [5, 17])
@pytest.mark.parametrize("quant", QUANTS)
def test_rotated_read_is_the_whole_read_rotated(gpu_server, quant, n, transport, monkeypatch):  # noqa: F811
    if transport == "socket":
        monkeypatch.setenv("IFS_NO_SHM", "1")
    pages = torch.randn(n, PAGE, generator=torch.Generator().manual_seed(n)).to(torch.bfloat16)
    conn = local_conn(gpu_server)
    keys, wt = _keys("rot", n), _table(n, n)
    ident = PageRotate(H, HD, np.stack([np.ones(HD // 2), np.zeros(HD // 2)], 1))
    try:
        assert conn.conn.shm_active() == (transport == "shm")
        src = torch.zeros(n, PAGE, dtype=torch.bfloat16)
        src[torch.as_tensor(wt)] = pages
        conn.write_pages(src.to("cuda:0").view(-1), keys, wt * PAGE, PAGE, sync=True, quant=quant)
        whole = _read(conn, keys, _table(n, n + 1), False)
        for ticketed in (False, True):
            what = f"{quant} n={n} {transport} ticketed={ticketed}"
            got = _read(conn, keys, _table(n, n + 2), ticketed, page_rotate=ROT)
            _assert_rotated(got, whole, ROT, what)
            assert not torch.equal(got, whole), what
            # the identity table gives the plain read (x + 0.0 turns -0 into +0)
            same = _read(conn, keys, _table(n, n + 3), ticketed, page_rotate=ident)
            _eq((same + 0.0).view(torch.int16), (whole + 0.0).view(torch.int16), what)
    finally:
        conn.delete_keys(keys)
        conn.close()


def test_invalid_requests_and_the_server_keeps_serving(gpu_server):  # noqa: F811
    n = 2
    pages = torch.randn(n, PAGE, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    conn = local_conn(gpu_server)
    keys = _keys("rinv", n)
    dst = torch.full((n, PAGE), 7.0, dtype=torch.bfloat16, device="cuda:0")
    handle, base_off = _native._dbg_ipc_export(dst.data_ptr())
    wire = ROT.wire()

    def body(ks=keys, flags=1, block_size=PAGE * 2, rot=wire, **kw):
        raw = bytearray(_native._dbg_build_packed_local(
            0, os.getpid(), dst.data_ptr() - base_off, base_off, block_size, 1, 0, handle,
            [0, 2 * PAGE], ks, rotate=rot, **kw))
        raw[32:36] = (flags | 512).to_bytes(4, "little")  # PackedLocalHdr.flags
        return bytes(raw)

    s = socket.create_connection(("127.0.0.1", gpu_server), timeout=30)
    try:
        conn.write_pages(pages.to("cuda:0").view(-1), keys, np.arange(n) * PAGE, PAGE, sync=True)
        other = PageRotate.from_delta(37, 2 * H, HD)  # cut for a page twice the size
        with pytest.raises(Exception, match=f"-{INVALID_REQ}"):
            conn.read_pages(dst.view(-1)[:PAGE], keys[:1], [0], PAGE // 2, page_rotate=ROT)
        for kw in (dict(rot=other.wire(), block_size=4 * PAGE), dict(flags=1 | 16)):
            assert _raw_request(s, b"r", body(**kw)) == INVALID_REQ, kw
        assert _raw_request(s, b"r", body(ks=["rot-no-such-key", keys[1]])) == 404
        torch.cuda.synchronize()
        assert bool((dst == 7).all()), "a refused read must leave the destination untouched"
        assert _raw_request(s, b"r", body()) == FINISH  # the same socket still serves
        torch.cuda.synchronize()
        _assert_rotated(dst.cpu(), pages, ROT, "raw legal read")
    finally:
        s.close()
        conn.delete_keys(keys)
        conn.close()
