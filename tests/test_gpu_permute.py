"""Permuted pages end to end: a head-major (HND, `[2, H, T, hd]`) client and a
token-major (NHD, `[2, T, H, hd]`) client share keys through a running server,
every codec, both transports; and permuted jobs through a GPU Shard at small
limits. Oracle: the transpose in torch and the codec's reference round trip."""

import os
import socket
import struct
import uuid

import numpy as np
import pytest
import torch

from infinistore_amd import _native, PagePermute, PageSlice
from infinistore_amd.vllm_adapter import InfiniStoreKVAdapter

from test_gpu import gpu_server, local_conn  # noqa: F401  (fixture + helper)
from test_gpu_slices import _eq, _pages, _raw_request, _table, _through_codec

pytestmark = pytest.mark.gpu

T, H, HD = 5, 3, 32
PAGE = 2 * T * H * HD  # bf16 elements
PERM = PagePermute(2, T, H)
INVALID_REQ, FINISH = 400, 200
QUANTS = [None, "fp8", "mxfp4"]


def _keys(tag, n):
    pre = uuid.uuid4().hex
    return [f"perm-{tag}-{pre}-{i}" for i in range(n)]


def _hnd(nhd: torch.Tensor) -> torch.Tensor:
    """(n, PAGE) token-major pages -> the same pages head-major."""
    return nhd.reshape(-1, 2, T, H, HD).transpose(2, 3).reshape(-1, PAGE)


def _read(conn, keys, table, ticketed, **kw):
    """Pages into blocks table[p] of a fresh cache; (n, PAGE) int16 in page order."""
    cache = torch.zeros(len(keys), PAGE, dtype=torch.bfloat16, device="cuda:0")
    if ticketed:
        conn.wait_read(conn.read_pages_async(cache.view(-1), keys, table * PAGE, PAGE, **kw))
    else:
        conn.read_pages(cache.view(-1), keys, table * PAGE, PAGE, **kw)
    conn.sync()
    return cache.cpu()[torch.as_tensor(table)].view(torch.int16)


@pytest.mark.parametrize("transport", ["shm", "socket"])
@pytest.mark.parametrize("n", [5, 16, 17, 40])  # around the inline path's 16 blocks
@pytest.mark.parametrize("quant", QUANTS)
def test_hnd_and_nhd_clients_share_keys(gpu_server, quant, n, transport, monkeypatch):  # noqa: F811
    if transport == "socket":
        monkeypatch.setenv("IFS_NO_SHM", "1")
    nhd = _pages(n, PAGE, 7 * n)  # the canonical pages
    want = _through_codec(nhd, quant)
    wt = _table(n, n)
    conn = local_conn(gpu_server)
    k_hnd, k_nhd = _keys("h", n), _keys("n", n)
    try:
        assert conn.conn.shm_active() == (transport == "shm")
        src = torch.zeros(n, PAGE, dtype=torch.bfloat16)
        src[torch.as_tensor(wt)] = _hnd(nhd)
        conn.write_pages(src.to("cuda:0").view(-1), k_hnd, wt * PAGE, PAGE, sync=True, quant=quant,
                         page_permute=PERM)
        src[torch.as_tensor(wt)] = nhd
        conn.write_pages(src.to("cuda:0").view(-1), k_nhd, wt * PAGE, PAGE, sync=True, quant=quant)
        for ticketed in (False, True):
            what = f"{quant} n={n} {transport} ticketed={ticketed}"
            _eq(_read(conn, k_hnd, _table(n, n + 1), ticketed), want, "HND -> NHD " + what)
            _eq(_read(conn, k_nhd, _table(n, n + 2), ticketed, page_permute=PERM), _hnd(want),
                "NHD -> HND " + what)
        # heads 1..3 of the HND-written pages, as an NHD reader's head_range slice
        out = torch.zeros(n, 2 * T * 2 * HD, dtype=torch.bfloat16, device="cuda:0")
        conn.read_pages(out.view(-1), k_hnd, np.arange(n) * out.shape[1], out.shape[1],
                        page_slice=PageSlice(PAGE, HD, 2 * HD, H * HD, 2 * T))
        conn.sync()
        _eq(out.cpu().view(torch.int16),
            want.reshape(n, 2, T, H, HD)[:, :, :, 1:3].reshape(n, -1), f"slice {quant}")
    finally:
        conn.delete_keys(k_hnd + k_nhd)
        conn.close()


def test_invalid_requests_and_the_server_keeps_serving(gpu_server):  # noqa: F811
    n = 2
    nhd = _pages(n, PAGE, 5)
    conn = local_conn(gpu_server)
    stored = {q: _keys(str(q), n) for q in QUANTS}
    dst = torch.full((n, PAGE), 7.0, dtype=torch.bfloat16, device="cuda:0")
    handle, base_off = _native._dbg_ipc_export(dst.data_ptr())
    good = (2, T, H, HD * 2)

    def body(flags=1, ext=good, rsvd=0, block_size=PAGE * 2, cut=None):
        b = bytearray(_native._dbg_build_packed_local(
            0, os.getpid(), dst.data_ptr() - base_off, base_off, block_size, flags, 0, handle,
            [0, PAGE * 2], stored[None], permute=good))
        b[104:128] = struct.pack("<IIIIQ", *ext[:3], rsvd, ext[3])
        return bytes(b if cut is None else b[:cut])

    s = socket.create_connection(("127.0.0.1", gpu_server), timeout=30)
    try:
        for q in QUANTS:
            conn.write_pages(nhd.to("cuda:0").view(-1), stored[q], np.arange(n) * PAGE, PAGE,
                             sync=True, quant=q)
            with pytest.raises(Exception, match=f"-{INVALID_REQ}"):  # half the written page
                conn.read_pages(dst.view(-1), stored[q], np.arange(n) * PAGE, PAGE // 2,
                                page_permute=PagePermute(1, T, H))
        bad = [dict(ext=(2, 0, H, HD * 2)), dict(ext=(0, T, H, HD * 2)), dict(rsvd=1),
               dict(ext=(2, T, H, HD)), dict(ext=(2, T + 1, H, HD * 2)), dict(block_size=PAGE),
               dict(ext=(1 << 16, 1 << 16, 1, HD * 2)), dict(cut=104 + 12),
               dict(flags=1 | 16), dict(flags=1 | 32)]  # next to the slice and the set flag
        for kw in bad:
            assert _raw_request(s, b"r", body(**kw)) == INVALID_REQ, kw
        # pieces of half a 32-element group: legal plain, refused for an mxfp4 write
        assert _raw_request(s, b"w", body(flags=1 | 4, ext=(2, T, 2 * H, HD))) == INVALID_REQ
        torch.cuda.synchronize()
        assert bool((dst == 7.0).all()), "a refused read must leave the destination untouched"
        assert _raw_request(s, b"r", body()) == FINISH  # the same socket still serves
        torch.cuda.synchronize()
        _eq(dst.cpu().view(torch.int16), _hnd(nhd.view(torch.int16)), "raw legal read")
    finally:
        s.close()
        conn.delete_keys(sum(stored.values(), []))
        conn.close()


@pytest.mark.parametrize("layout,quant", [("block_major", None), ("kv_major", "mxfp4")])
def test_hnd_and_nhd_adapters_share_keys(gpu_server, layout, quant):  # noqa: F811
    n_layers, n_pages, nblk = 2, 5, 7
    tag = f"permtest-{uuid.uuid4().hex[:8]}"
    tokens = list(range(300, 300 + n_pages * T))
    make = lambda **kw: InfiniStoreKVAdapter("127.0.0.1", gpu_server, tag, n_layers, T, PAGE,  # noqa: E731
                                             quant=quant, kv_layout=layout, **kw)
    adapters = {"nhd": make(), "hnd": make(cache_layout="hnd", cache_kv_heads=H)}
    nhd = [_pages(n_pages, PAGE, 80 + li) for li in range(n_layers)]

    def cache_of(pages, table):  # (n_pages, PAGE) -> the engine's cache tensor
        c = torch.zeros(nblk, 2, PAGE // 2, dtype=torch.bfloat16)
        c[torch.as_tensor(table)] = pages.reshape(n_pages, 2, -1)
        return (c if layout == "block_major" else c.transpose(0, 1).contiguous()).to("cuda:0")

    try:
        for writer, reader in (("hnd", "nhd"), ("nhd", "hnd")):
            wt = [int(b) for b in _table(nblk, 31)[:n_pages]]
            rt = [int(b) for b in _table(nblk, 32)[:n_pages]]
            sources = [cache_of(_hnd(p) if writer == "hnd" else p, wt) for p in nhd]
            for li in range(n_layers):  # the saves are asynchronous: sources stay alive
                adapters[writer].save_kv_layer(li, sources[li], tokens, wt)
            adapters[writer].wait_for_save()
            caches = [torch.zeros_like(sources[0]) for _ in range(n_layers)]
            assert adapters[reader].start_load_kv(caches, tokens, rt) == n_pages
            for li in range(n_layers):
                assert adapters[reader].wait_for_layer_load(li)
                c = caches[li].cpu() if layout == "block_major" else caches[li].cpu().transpose(0, 1)
                got = c[torch.as_tensor(rt)].reshape(n_pages, PAGE).view(torch.int16)
                want = _through_codec(nhd[li], quant)
                _eq(got, _hnd(want) if reader == "hnd" else want, f"{writer} -> {reader} {li}")
            assert adapters[writer].evict_request(tokens) == n_layers * n_pages
    finally:
        for a in adapters.values():
            a.close()


@pytest.mark.parametrize("codec", [0, 1, 2])
@pytest.mark.parametrize("n,descs", [(13, 5), (_native._SHARD_FAN_CHUNK + 1, 1000)])
def test_gpu_shard_chunk_loop_and_fan_out_keep_the_permutation(n, descs, codec):
    """Two streams; 5 descriptors per slot (three chunks), and one block more
    than a fan-out sub-job: store permuted, load permuted, compare with the source."""
    geo, stored = (2, T, H, 2 * HD), {0: 2 * PAGE, 1: PAGE, 2: PAGE // 2 + PAGE // 32}[codec]
    g = torch.Generator().manual_seed(n)
    src = (torch.randn(n, PAGE, generator=g) * 4).to(torch.bfloat16)
    d_src, d_out = src.to("cuda:0"), torch.zeros(n, PAGE, dtype=torch.bfloat16, device="cuda:0")
    pool = torch.zeros(n, (stored + 15) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    ptrs = lambda t: [t.data_ptr() + i * t.stride(0) * t.element_size() for i in range(n)]  # noqa: E731
    scales = [0.0] * n if codec == 1 else None
    run = lambda job: _native._dbg_shard_run_perm(0, 2, 2, descs, [job], [geo], 1, 30.0)[0]  # noqa: E731
    res = run((ptrs(d_src), ptrs(pool), 2 * PAGE, codec, True, 1, 0, scales, 0))
    assert res["submitted"] and res["done_calls"] == 1 and res["ok"]
    res2 = run((ptrs(pool), ptrs(d_out), 2 * PAGE, codec, False, 1, 0, res["scales"] or None, 0))
    assert res2["submitted"] and res2["ok"]
    torch.cuda.synchronize()
    # permuted both ways: the client page comes back as the codec's round trip of
    # ITSELF only if the stored block was the canonical page's
    canon = src.reshape(n, 2, H, T, HD).transpose(2, 3).reshape(n, PAGE)
    want = _through_codec(canon, QUANTS[codec]).reshape(n, 2, T, H, HD).transpose(2, 3)
    _eq(d_out.cpu().view(torch.int16), want.reshape(n, PAGE), f"shard n={n} codec={codec}")
