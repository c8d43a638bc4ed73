"""Shuffled pages through a running server: a shuffled-cache and a token-major client
share keys. Oracle: the two index formulas and the codec's reference round trip."""

import os
import socket
import struct
import uuid

import numpy as np
import pytest
import torch

from infinistore_amd import _native, PageShuffle
from infinistore_amd.vllm_adapter import InfiniStoreKVAdapter

from test_gpu import gpu_server, local_conn  # noqa: F401  (fixture + helper)
from test_gpu_permute import _keys
from test_gpu_shuffle_kernels import canonical
from test_gpu_slices import _eq, _pages, _raw_request, _table, _through_codec

pytestmark = pytest.mark.gpu

T, H, HD = 8, 3, 32
PAGE = 2 * T * H * HD  # bf16 elements
SHUF, GEO = PageShuffle(T, H, HD), (2, T, H, HD, 2, 1, 2)
QUANTS, INVALID_REQ, FINISH = [None, "fp8", "mxfp4"], 400, 200


def _shuf(nhd: torch.Tensor) -> torch.Tensor:  # token-major pages as shuffled blocks
    bits = nhd.contiguous().view(torch.int16).numpy().view(np.uint8)
    return torch.from_numpy(canonical(bits, GEO, back=True).view(np.int16)).view(nhd.dtype)


def _read(conn, keys, table, ticketed, **kw):  # pages into blocks table[p] of a fresh cache
    cache = torch.zeros(len(keys), PAGE, dtype=torch.bfloat16, device="cuda:0")
    if ticketed:
        conn.wait_read(conn.read_pages_async(cache.view(-1), keys, table * PAGE, PAGE, **kw))
    else:
        conn.read_pages(cache.view(-1), keys, table * PAGE, PAGE, **kw)
    conn.sync()
    return cache.cpu()[torch.as_tensor(table)].view(torch.int16)


@pytest.mark.parametrize("transport", ["shm", "socket"])
@pytest.mark.parametrize("n", [5, 17])
@pytest.mark.parametrize("quant", QUANTS)
def test_shuffled_and_nhd_clients_share_keys(gpu_server, quant, n, transport, monkeypatch):  # noqa: F811
    if transport == "socket":
        monkeypatch.setenv("IFS_NO_SHM", "1")
    nhd = _pages(n, PAGE, 7 * n)  # the canonical pages
    want = _through_codec(nhd, quant)
    wt = _table(n, n)
    conn = local_conn(gpu_server)
    k_sh, k_nhd = _keys("s", n), _keys("n", n)
    try:
        assert conn.conn.shm_active() == (transport == "shm")
        src = torch.zeros(n, PAGE, dtype=torch.bfloat16)
        src[torch.as_tensor(wt)] = _shuf(nhd)
        conn.write_pages(src.to("cuda:0").view(-1), k_sh, wt * PAGE, PAGE, sync=True, quant=quant,
                         page_shuffle=SHUF)
        src[torch.as_tensor(wt)] = nhd
        conn.write_pages(src.to("cuda:0").view(-1), k_nhd, wt * PAGE, PAGE, sync=True, quant=quant)
        for ticketed in (False, True):
            what = f"{quant} n={n} {transport} ticketed={ticketed}"
            _eq(_read(conn, k_sh, _table(n, n + 1), ticketed), want, "shuffled -> NHD " + what)
            _eq(_read(conn, k_nhd, _table(n, n + 2), ticketed, page_shuffle=SHUF), _shuf(want),
                "NHD -> shuffled " + what)
    finally:
        conn.delete_keys(k_sh + k_nhd)
        conn.close()


def test_invalid_requests_and_the_server_keeps_serving(gpu_server):  # noqa: F811
    n = 2
    nhd = _pages(n, PAGE, 5)
    conn = local_conn(gpu_server)
    stored = _keys("inv", n)
    dst = torch.full((n, PAGE), 7.0, dtype=torch.bfloat16, device="cuda:0")
    handle, base_off = _native._dbg_ipc_export(dst.data_ptr())

    def body(flags=1, ext=GEO + (0,), block_size=PAGE * 2):
        b = bytearray(_native._dbg_build_packed_local(
            0, os.getpid(), dst.data_ptr() - base_off, base_off, block_size, flags, 0, handle,
            [0, PAGE * 2], stored, shuffle=GEO))
        b[104:136] = struct.pack("<8I", *ext)
        return bytes(b)

    s = socket.create_connection(("127.0.0.1", gpu_server), timeout=30)
    try:
        conn.write_pages(nhd.to("cuda:0").view(-1), stored, np.arange(n) * PAGE, PAGE, sync=True)
        with pytest.raises(Exception, match=f"-{INVALID_REQ}"):  # half the written page
            conn.read_pages(dst.view(-1), stored, np.arange(n) * PAGE, PAGE // 2,
                            page_shuffle=SHUF._replace(halves=1))
        bad = [dict(flags=1 | 128),  # next to the transpose flag
               dict(ext=(2, 2 * T, H, HD, 2, 1, 2, 0)),  # cut for another page size
               dict(ext=GEO + (1,))]  # rsvd
        for kw in bad:
            assert _raw_request(s, b"r", body(**kw)) == INVALID_REQ, kw
        torch.cuda.synchronize()
        assert bool((dst == 7.0).all()), "a refused read must leave the destination untouched"
        assert _raw_request(s, b"r", body()) == FINISH  # the same socket still serves
        torch.cuda.synchronize()
        _eq(dst.cpu().view(torch.int16), _shuf(nhd.view(torch.int16)), "raw legal read")
    finally:
        s.close()
        conn.delete_keys(stored)
        conn.close()


@pytest.mark.parametrize("layout,quant", [("block_major", None), ("kv_major", "mxfp4"),
                                          ("kv_major", "fp8")])
def test_shuffled_and_nhd_adapters_share_keys(gpu_server, layout, quant):  # noqa: F811
    n_pages, nblk, tag = 5, 7, f"shuftest-{uuid.uuid4().hex[:8]}"
    tokens = list(range(300, 300 + n_pages * T))
    make = lambda **kw: InfiniStoreKVAdapter("127.0.0.1", gpu_server, tag, 1, T, PAGE,  # noqa: E731
                                             quant=quant, kv_layout=layout, **kw)
    adapters = {"nhd": make(), "shuf": make(cache_layout="pa_shuffled", cache_kv_heads=H)}
    nhd = _pages(n_pages, PAGE, 80)
    want = _through_codec(nhd, quant)
    try:
        for writer, reader in (("shuf", "nhd"), ("nhd", "shuf")):
            wt = [int(b) for b in _table(nblk, 31)[:n_pages]]
            rt = [int(b) for b in _table(nblk, 32)[:n_pages]]
            c = torch.zeros(nblk, 2, PAGE // 2, dtype=torch.bfloat16)  # the engine's cache tensor
            c[torch.as_tensor(wt)] = (_shuf(nhd) if writer == "shuf" else nhd).reshape(n_pages, 2, -1)
            source = (c if layout == "block_major" else c.transpose(0, 1).contiguous()).to("cuda:0")
            adapters[writer].save_kv_layer(0, source, tokens, wt)
            adapters[writer].wait_for_save()
            cache = torch.zeros_like(source)
            assert adapters[reader].start_load_kv([cache], tokens, rt) == n_pages
            assert adapters[reader].wait_for_layer_load(0)
            c = cache.cpu() if layout == "block_major" else cache.cpu().transpose(0, 1)
            got = c[torch.as_tensor(rt)].reshape(n_pages, PAGE).view(torch.int16)
            _eq(got, _shuf(want) if reader == "shuf" else want, f"{writer} -> {reader}")
            assert adapters[writer].evict_request(tokens) == n_pages
    finally:
        for a in adapters.values():
            a.close()
