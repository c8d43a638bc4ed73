"""Cast pages through a running server: an fp8 (e4m3fn) and a bf16 client share keys.
Oracle: torch's e4m3 cast composed with the codec's reference round trip, bit for bit."""

import os
import socket
import struct
import uuid

import numpy as np
import pytest
import torch

from infinistore_amd import _native, PageCast, PageSlice
from infinistore_amd.vllm_adapter import InfiniStoreKVAdapter

from _kernel_refs import assert_codes_equal
from test_gpu import gpu_server, local_conn  # noqa: F401  (fixture + helper)
from test_gpu_cast_kernels import K_SCALE, V_SCALE, load_ref, store_ref
from test_gpu_permute import _keys
from test_gpu_slices import _eq, _raw_request, _table, _through_codec

pytestmark = pytest.mark.gpu

T, H, HD = 8, 3, 32
PAGE = 2 * T * H * HD  # elements: bf16 on one side, one byte each on the other
CAST, WIRE = PageCast([K_SCALE, V_SCALE]), (1, 2, K_SCALE, V_SCALE)
QUANTS, INVALID_REQ, FINISH = [None, "fp8", "mxfp4"], 400, 200


def _codes(n, seed):  # (n, PAGE) uint8: random e4m3fn codes without NaN
    c = torch.randint(0, 256, (n, PAGE), dtype=torch.uint8,
                      generator=torch.Generator().manual_seed(seed)).numpy()
    c[(c & 0x7F) == 0x7F] ^= 1
    return c


def _want_codes(bits_i16):  # what an fp8 reader under CAST gets of these bf16 bits
    return load_ref(bits_i16.contiguous().numpy().view(np.uint16), WIRE[2:], 2)


def _read(conn, keys, table, ticketed, dtype, **kw):  # pages into blocks table[p] of a fresh cache
    cache = torch.zeros(len(keys), PAGE, dtype=dtype, device="cuda:0")
    if ticketed:
        conn.wait_read(conn.read_pages_async(cache.view(-1), keys, table * PAGE, PAGE, **kw))
    else:
        conn.read_pages(cache.view(-1), keys, table * PAGE, PAGE, **kw)
    conn.sync()
    out = cache.cpu()[torch.as_tensor(table)]
    return out.view(torch.int16) if dtype == torch.bfloat16 else out.numpy()


@pytest.mark.parametrize("transport", ["shm", "socket"])
@pytest.mark.parametrize("n", [5, 17])
@pytest.mark.parametrize("quant", QUANTS)
def test_fp8_and_bf16_clients_share_keys(gpu_server, quant, n, transport, monkeypatch):  # noqa: F811
    if transport == "socket":
        monkeypatch.setenv("IFS_NO_SHM", "1")
    codes = _codes(n, 7 * n)
    b = store_ref(codes, WIRE[2:], 2)  # the logical pages the fp8 engine's codes stand for
    want = _through_codec(b, quant)  # what every bf16 reader sees of them
    wt = _table(n, n)
    conn = local_conn(gpu_server)
    k_f8, k_bf = _keys("f", n), _keys("b", n)
    try:
        assert conn.conn.shm_active() == (transport == "shm")
        src = torch.zeros(n, PAGE, dtype=torch.uint8)
        src[torch.as_tensor(wt)] = torch.from_numpy(codes)
        conn.write_pages(src.to("cuda:0").view(torch.float8_e4m3fn).view(-1), k_f8, wt * PAGE,
                         PAGE, sync=True, quant=quant, page_cast=CAST)
        srcb = torch.zeros(n, PAGE, dtype=torch.bfloat16)
        srcb[torch.as_tensor(wt)] = b
        conn.write_pages(srcb.to("cuda:0").view(-1), k_bf, wt * PAGE, PAGE, sync=True, quant=quant)
        for ticketed in (False, True):
            what = f"{quant} n={n} {transport} ticketed={ticketed}"
            _eq(_read(conn, k_f8, _table(n, n + 1), ticketed, torch.bfloat16), want,
                "fp8 -> bf16 " + what)
            for keys in (k_bf, k_f8):
                got = _read(conn, keys, _table(n, n + 2), ticketed, torch.uint8, page_cast=CAST)
                assert_codes_equal(got, _want_codes(want), "-> fp8 " + what)
                if quant is None:  # the same scales, no codec: the written codes come back
                    assert (got == codes).all(), what
        # heads 1..3 of the fp8-written pages, as an NHD reader's head_range slice
        out = torch.zeros(n, 2 * T * 2 * HD, dtype=torch.bfloat16, device="cuda:0")
        conn.read_pages(out.view(-1), k_f8, np.arange(n) * out.shape[1], out.shape[1],
                        page_slice=PageSlice(PAGE, HD, 2 * HD, H * HD, 2 * T))
        conn.sync()
        _eq(out.cpu().view(torch.int16),
            want.reshape(n, 2, T, H, HD)[:, :, :, 1:3].reshape(n, -1), f"slice {quant}")
    finally:
        conn.delete_keys(k_f8 + k_bf)
        conn.close()


def test_invalid_requests_and_the_server_keeps_serving(gpu_server):  # noqa: F811
    n = 2
    b = store_ref(_codes(n, 5), WIRE[2:], 2)
    conn = local_conn(gpu_server)
    stored = _keys("inv", n)
    dst = torch.full((n, PAGE), 7, dtype=torch.uint8, device="cuda:0")
    handle, base_off = _native._dbg_ipc_export(dst.data_ptr())

    def body(flags=1, ext=WIRE, block_size=PAGE * 2, **kw):
        raw = bytearray(_native._dbg_build_packed_local(
            0, os.getpid(), dst.data_ptr() - base_off, base_off, block_size, flags, 0, handle,
            [0, PAGE], stored, cast=WIRE, **kw))
        at = 104 + (16 if "n_segments" in kw else 0)  # header, then the segment extension
        raw[at:at + 16] = struct.pack("<IIff", *ext)
        return bytes(raw)

    s = socket.create_connection(("127.0.0.1", gpu_server), timeout=30)
    try:
        conn.write_pages(b.to("cuda:0").view(-1), stored, np.arange(n) * PAGE, PAGE, sync=True)
        with pytest.raises(Exception, match=f"-{INVALID_REQ}"):  # half the written page
            conn.read_pages(dst.view(-1), stored, np.arange(n) * PAGE, PAGE // 2, page_cast=CAST)
        bad = [dict(flags=1 | 16), dict(flags=1 | 32), dict(flags=1 | 64), dict(flags=1 | 128),
               dict(ext=(2, 2, 1.0, 1.0)), dict(ext=(1, 3, 1.0, 1.0)), dict(ext=(1, 2, 0.0, 1.0)),
               dict(ext=(1, 2, 1.0, float("nan"))), dict(block_size=PAGE * 2 + 16),
               dict(n_segments=2, segment_stride=PAGE // 2 - 16),  # overlapping client segments
               dict(n_segments=2, segment_stride=PAGE // 2 + 8)]  # a stride off 16 bytes
        for kw in bad:
            assert _raw_request(s, b"r", body(**kw)) == INVALID_REQ, kw
        torch.cuda.synchronize()
        assert bool((dst == 7).all()), "a refused read must leave the destination untouched"
        assert _raw_request(s, b"r", body()) == FINISH  # the same socket still serves
        torch.cuda.synchronize()
        assert_codes_equal(dst.cpu().numpy(), _want_codes(b.view(torch.int16)), "raw legal read")
    finally:
        s.close()
        conn.delete_keys(stored)
        conn.close()


@pytest.mark.parametrize("layout,quant", [("block_major", None), ("kv_major", "mxfp4"),
                                          ("kv_major", "fp8")])
def test_fp8_and_bf16_adapters_share_keys(gpu_server, layout, quant):  # noqa: F811
    n_pages, nblk, tag = 5, 7, f"casttest-{uuid.uuid4().hex[:8]}"
    tokens = list(range(300, 300 + n_pages * T))
    make = lambda **kw: InfiniStoreKVAdapter("127.0.0.1", gpu_server, tag, 1, T, PAGE,  # noqa: E731
                                             quant=quant, kv_layout=layout, **kw)
    adapters = {"bf16": make(),
                "fp8": make(cache_dtype="fp8_e4m3", k_scale=K_SCALE, v_scale=V_SCALE)}
    codes = _codes(n_pages, 80)
    b = store_ref(codes, WIRE[2:], 2)
    want = _through_codec(b, quant)
    try:
        for writer, reader in (("fp8", "bf16"), ("bf16", "fp8")):
            wt = [int(x) for x in _table(nblk, 31)[:n_pages]]
            rt = [int(x) for x in _table(nblk, 32)[:n_pages]]
            dt = {"bf16": torch.bfloat16, "fp8": torch.uint8}
            c = torch.zeros(nblk, 2, PAGE // 2, dtype=dt[writer])  # the engine's cache tensor
            c[torch.as_tensor(wt)] = (torch.from_numpy(codes) if writer == "fp8" else b).reshape(
                n_pages, 2, -1)
            source = (c if layout == "block_major" else c.transpose(0, 1).contiguous()).to("cuda:0")
            adapters[writer].save_kv_layer(0, source, tokens, wt)
            adapters[writer].wait_for_save()
            cache = torch.zeros(source.shape, dtype=dt[reader], device="cuda:0")
            assert adapters[reader].start_load_kv([cache], tokens, rt) == n_pages
            assert adapters[reader].wait_for_layer_load(0)
            c = cache.cpu() if layout == "block_major" else cache.cpu().transpose(0, 1)
            got = c[torch.as_tensor(rt)].reshape(n_pages, PAGE)
            if reader == "bf16":
                _eq(got.view(torch.int16), want, f"{writer} -> {reader}")
            else:
                assert_codes_equal(got.numpy(), _want_codes(want), f"{writer} -> {reader}")
            assert adapters[writer].evict_request(tokens) == n_pages
    finally:
        for a in adapters.values():
            a.close()


@pytest.mark.parametrize("codec", [0, 1, 2])
@pytest.mark.parametrize("n,descs", [(13, 5), (_native._SHARD_FAN_CHUNK + 1, 1000)])
def test_gpu_shard_chunk_loop_and_fan_out_keep_the_cast(n, descs, codec):
    """Two streams; 5 descriptors per slot (three chunks), and one block more than a
    fan-out sub-job: store the codes, load them back, compare with the composition."""
    stored = {0: 2 * PAGE, 1: PAGE, 2: PAGE // 2 + PAGE // 32}[codec]
    codes = np.tile(_codes(13, n), (-(-n // 13), 1))[:n]
    d_src = torch.from_numpy(codes).to("cuda:0")
    d_out = torch.zeros(n, PAGE, dtype=torch.uint8, device="cuda:0")
    pool = torch.zeros(n, (stored + 15) // 16 * 16, dtype=torch.uint8, device="cuda:0")
    ptrs = lambda t: [t.data_ptr() + i * t.stride(0) * t.element_size() for i in range(n)]  # noqa: E731
    scales = [0.0] * n if codec == 1 else None
    run = lambda job: _native._dbg_shard_run_cast(0, 2, 2, descs, [job], [WIRE], 1, 30.0)[0]  # noqa: E731
    res = run((ptrs(d_src), ptrs(pool), 2 * PAGE, codec, True, 1, 0, scales, 0))
    assert res["submitted"] and res["done_calls"] == 1 and res["ok"]
    res2 = run((ptrs(pool), ptrs(d_out), 2 * PAGE, codec, False, 1, 0, res["scales"] or None, 0))
    assert res2["submitted"] and res2["ok"]
    torch.cuda.synchronize()
    want = _through_codec(store_ref(codes[:13], WIRE[2:], 2), QUANTS[codec])
    got = d_out.cpu().numpy()
    assert_codes_equal(got[:13], _want_codes(want), f"shard n={n} codec={codec}")
    assert (got == np.tile(got[:13], (-(-n // 13), 1))[:n]).all(), "every repeat of the 13 pages"
