"""mxfp4 page compression end to end: `write_pages(quant="mxfp4")` through a
running server and back, compared bit for bit with the numpy reference
(tests/_mxfp4_refs.py); footprint, mixed reads, refusals, snapshot/restore
and compaction."""

import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest
import torch

from _kernel_refs import assert_bf16_bits_equal, bf16_bits, fp8_dequant_ref, fp8_quant_ref
from _mxfp4_refs import roundtrip_ref
from conftest import make_client
from test_gpu import gpu_server, local_conn  # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_REQ = 400


def _pages(n, elems, seed):
    """n pages of bf16 with a different magnitude per 32-element group."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(2.0, torch.randint(-20, 20, (n, elems // 32, 1), generator=g).float())
    x = torch.randn(n, elems // 32, 32, generator=g) * mag
    return x.reshape(n, elems).to(torch.bfloat16)


def _keys(tag, n):
    pre = uuid.uuid4().hex
    return [f"mx-{tag}-{pre}-{i}" for i in range(n)]


@pytest.mark.parametrize("elems,n", [(32, 5), (4096, 3), (123360, 1)])
def test_mxfp4_roundtrip(gpu_server, elems, n):
    pages = _pages(n, elems, elems)
    want = roundtrip_ref(pages)
    src = pages.to("cuda:0").reshape(-1)
    dst = torch.zeros_like(src)
    offs = [i * elems for i in range(n)]
    keys = _keys("rt", n)
    conn = local_conn(gpu_server)
    try:
        conn.write_pages(src, keys, offs, elems, sync=True, quant="mxfp4")
        conn.read_pages(dst, keys, offs, elems)
        conn.sync()
        assert_bf16_bits_equal(bf16_bits(dst), want, f"{elems}-element pages")
    finally:
        conn.delete_keys(keys)
        conn.close()


def test_mxfp4_footprint(gpu_server):
    """123360-element pages store 61680 + 3855 = 65535 bytes: one block of the
    64 KiB granule each, against four for the plain 246720 bytes."""
    elems, n = 123360, 4
    assert elems // 2 + elems // 32 == 65535
    src = _pages(n, elems, 1).to("cuda:0").reshape(-1)
    offs = [i * elems for i in range(n)]
    qkeys, pkeys = _keys("fq", n), _keys("fp", n)
    conn = local_conn(gpu_server)
    try:
        s0 = json.loads(conn.get_server_stats_remote())["used_blocks"]
        conn.write_pages(src, qkeys, offs, elems, sync=True, quant="mxfp4")
        s1 = json.loads(conn.get_server_stats_remote())["used_blocks"]
        conn.write_pages(src, pkeys, offs, elems, sync=True)
        s2 = json.loads(conn.get_server_stats_remote())["used_blocks"]
        assert s1 - s0 == n, (s0, s1)
        assert s2 - s1 == 4 * n, (s1, s2)
    finally:
        conn.delete_keys(qkeys + pkeys)
        conn.close()


def test_mxfp4_mixed_read(gpu_server):
    """One read_pages call whose keys interleave plain, fp8 and mxfp4 pages
    of the same logical size."""
    elems, n = 4096, 9
    pages = _pages(n, elems, 2)
    src = pages.to("cuda:0").reshape(-1)
    offs = np.arange(n, dtype=np.uint64) * elems
    keys = _keys("mix", n)
    kind = [("plain", "fp8", "mxfp4")[i % 3] for i in range(n)]
    want = bf16_bits(pages).copy()
    fp8_rows = [i for i in range(n) if kind[i] == "fp8"]
    mx_rows = [i for i in range(n) if kind[i] == "mxfp4"]
    codes, scales = fp8_quant_ref(pages[fp8_rows])
    want[fp8_rows] = bf16_bits(fp8_dequant_ref(codes, scales))
    want[mx_rows] = roundtrip_ref(pages[mx_rows])
    conn = local_conn(gpu_server)
    try:
        for k, quant in (("plain", None), ("fp8", "fp8"), ("mxfp4", "mxfp4")):
            rows = [i for i in range(n) if kind[i] == k]
            conn.write_pages(src, [keys[i] for i in rows], offs[rows], elems, sync=True,
                             quant=quant)
        dst = torch.zeros_like(src)
        conn.read_pages(dst, keys, offs, elems)
        conn.sync()
        assert_bf16_bits_equal(bf16_bits(dst), want, "interleaved read")
    finally:
        conn.delete_keys(keys)
        conn.close()


def test_three_codecs_fanout_mixed_read(gpu_server):
    """4100 fp8, 4100 mxfp4 and 20 plain pages of 32 elements (64 bytes, the
    smallest page all three formats take), read back by ONE read_pages call
    that interleaves the kinds, then in reversed order. 4100 blocks make each
    compressed job fan out into two sub-jobs (4096 blocks each), so the second
    fp8 sub-job reads the request's scales at a non-zero offset; every fp8 page
    has its own absmax — a distinct odd factor times a power of two — so a
    scale taken from the wrong place shows. Bit for bit, no tolerance."""
    e, nq, npl = 32, 4100, 20
    g = torch.Generator().manual_seed(12)
    i = torch.arange(nq)
    amax = (2.0 * (i % 128) + 1.0) * torch.pow(2.0, (i // 128 - 16).float())
    assert amax.unique().numel() == nq
    fp8_pages = ((torch.rand(nq, e, generator=g) - 0.5) * amax[:, None]).to(torch.bfloat16)
    fp8_pages[i, i % e] = (amax * torch.where(i % 2 == 0, 1.0, -1.0)).to(torch.bfloat16)
    assert torch.equal(fp8_pages.float().abs().max(dim=1).values, amax)  # exact in bf16
    mx_pages = _pages(nq, e, 13)
    plain_pages = _pages(npl, e, 14)
    pages = torch.cat([fp8_pages, mx_pages, plain_pages])
    n = pages.shape[0]
    assert n == 8220
    codes, scales = fp8_quant_ref(fp8_pages)
    want = np.concatenate([bf16_bits(fp8_dequant_ref(codes, scales)),
                           roundtrip_ref(mx_pages).reshape(nq, e), bf16_bits(plain_pages)])
    # fp8 j, mxfp4 j, and plain j while they last
    order = [r for j in range(nq)
             for r in ([j, nq + j] + ([2 * nq + j] if j < npl else []))]
    assert sorted(order) == list(range(n))

    src = pages.to("cuda:0").reshape(-1)
    offs = np.arange(n, dtype=np.uint64) * e
    keys = _keys("mix3", n)
    conn = local_conn(gpu_server)
    try:
        for lo, hi, quant in ((0, nq, "fp8"), (nq, 2 * nq, "mxfp4"), (2 * nq, n, None)):
            conn.write_pages(src, keys[lo:hi], offs[lo:hi], e, sync=True, quant=quant)
        dst = torch.zeros_like(src)
        # page k of dst holds key order[k]
        conn.read_pages(dst, [keys[r] for r in order], offs, e)
        conn.sync()
        assert_bf16_bits_equal(bf16_bits(dst).reshape(n, e), want[order], "interleaved read")
        dst.zero_()
        conn.read_pages(dst, [keys[r] for r in order[::-1]], offs, e)
        conn.sync()
        assert_bf16_bits_equal(bf16_bits(dst).reshape(n, e), want[order[::-1]],
                               "interleaved read, reversed")
    finally:
        conn.delete_keys(keys)
        conn.close()


@pytest.mark.parametrize("quant", ["fp8", "mxfp4"])
def test_write_pages_refusals_are_value_errors(gpu_server, quant):
    """Every quant argument write_pages refuses raises ValueError (checks that
    survive `python -O`), before anything is sent. This is the client-side
    half of tests/test_page_codec.py: write_pages wants a GPU tensor and a
    local connection, so it cannot run there."""
    conn = local_conn(gpu_server)
    multiple = conn.QUANT_MODES[quant][1]
    src = _pages(1, 4 * multiple, 5).to("cuda:0").reshape(-1)
    assert src.data_ptr() % 16 == 0
    k = _keys("ve", 1)
    try:
        with pytest.raises(ValueError, match="int3"):  # unknown mode
            conn.write_pages(src, k, [0], multiple, sync=True, quant="int3")
        with pytest.raises(ValueError, match=quant):  # not a bf16 cache
            conn.write_pages(src.float(), k, [0], multiple, sync=True, quant=quant)
        for bad in (0, multiple // 2, multiple + multiple // 2):  # page size
            with pytest.raises(ValueError, match=quant):
                conn.write_pages(src, k, [0], bad, sync=True, quant=quant)
        with pytest.raises(ValueError, match=quant):  # page 8 bytes off a 16-byte boundary
            conn.write_pages(src, k, [4], multiple, sync=True, quant=quant)
        with pytest.raises(ValueError, match=quant):  # cache 2 bytes off
            conn.write_pages(src[1:], k, [0], multiple, sync=True, quant=quant)
        assert not conn.check_exist(k[0])
    finally:
        conn.close()


def test_mxfp4_refusals(gpu_server):
    elems = 64
    src = _pages(1, 4 * elems, 3).to("cuda:0").reshape(-1)
    assert src.data_ptr() % 16 == 0
    dst = torch.zeros_like(src)
    k = _keys("ref", 6)
    conn = local_conn(gpu_server)
    try:
        # client side, before anything is sent
        with pytest.raises(ValueError):
            conn.write_pages(src, [k[0]], [0], 16, sync=True, quant="mxfp4")
        with pytest.raises(ValueError):
            conn.write_pages(src, [k[1]], [4], elems, sync=True, quant="mxfp4")
        with pytest.raises(ValueError):
            conn.write_pages(src.float(), [k[1]], [0], elems, sync=True, quant="mxfp4")
        # a client that skips those checks meets the server's
        raw = lambda key, off, page_bytes, flags: conn.conn.rw_local_keys(  # noqa: E731
            conn.OP_W, [key], np.array([off], dtype=np.uint64), 2, page_bytes,
            src.data_ptr(), 0, True, flags)
        both = conn.FLAG_QUANT_FP8 | conn.FLAG_QUANT_MXFP4
        assert raw(k[2], 0, 2 * elems, both) == -INVALID_REQ
        assert raw(k[3], 0, 32, conn.FLAG_QUANT_MXFP4) == -INVALID_REQ  # 16 elements
        assert raw(k[4], 4, 2 * elems, conn.FLAG_QUANT_MXFP4) == -INVALID_REQ
        assert not any(conn.check_exist(key) for key in k[:5])

        conn.write_pages(src, [k[5]], [0], elems, sync=True, quant="mxfp4")
        with pytest.raises(Exception):  # another page size
            conn.read_pages(dst, [k[5]], [0], 2 * elems)
        with pytest.raises(Exception):
            conn.read_pages(dst, [k[5]], [0], elems // 2)
        with pytest.raises(Exception):  # destination 8 bytes off a 16-byte boundary
            conn.read_pages(dst, [k[5]], [4], elems)
        assert bool((dst == 0).all()), "a refused read must leave the destination untouched"

        # the fabric moves raw bytes: an mxfp4 entry is refused, not shipped
        rdma = make_client(gpu_server)
        try:
            host = torch.zeros(elems, dtype=torch.bfloat16)
            rdma.register_mr(host)
            with pytest.raises(Exception):
                rdma.read_cache(host, [(k[5], 0)], elems)
            assert bool((host == 0).all())
        finally:
            rdma.close()

        # and the connection still serves
        conn.read_pages(dst, [k[5]], [elems], elems)
        conn.sync()
        assert_bf16_bits_equal(bf16_bits(dst[elems:2 * elems]),
                               roundtrip_ref(src[:elems].cpu()[None, :]))
    finally:
        conn.delete_keys(k)
        conn.close()


def test_mxfp4_snapshot_restore_and_compaction(tmp_path):
    """Snapshot -> purge -> restore reads back bit-identical to the read
    before the snapshot (the header's codec word carries mxfp4); then delete
    alternate keys, compact, and the survivors still read back bit-identical.
    Runs in a subprocess that hosts the server in-process so the python
    snapshot / compaction API is reachable."""
    code = subprocess.run(
        [sys.executable, "-c", f"""
import torch
import infinistore_amd as ifs
from conftest import free_port
port = free_port()
ifs.register_server(ifs.ServerConfig(service_port=port, manage_port=port+1,
                                     prealloc_size=2, minimal_allocate_size=64))
cfg = ifs.ClientConfig(host_addr="127.0.0.1", service_port=port,
                       connection_type=ifs.TYPE_LOCAL_GPU)
c = ifs.InfinityConnection(cfg); c.connect()
torch.manual_seed(4)
for pe, n in ((32, 8), (4096, 8)):
    src = (torch.randn(n*pe) * torch.logspace(-3, 3, n*pe)).to(torch.bfloat16).to("cuda:0")
    offs = [i*pe for i in range(n)]
    mkeys = [f"m{{pe}}-{{i}}" for i in range(n)]
    pkeys = [f"p{{pe}}-{{i}}" for i in range(n)]
    c.write_pages(src, mkeys, offs, pe, sync=True, quant="mxfp4")
    c.write_pages(src, pkeys, offs, pe, sync=True)
    before = torch.zeros_like(src)
    c.read_pages(before, mkeys, offs, pe); c.sync()
    assert not torch.equal(before, src) and bool((before != 0).any())
    snap = {str(tmp_path / 'mx.snap')!r}
    sn, sb = ifs.snapshot_pool(snap)
    assert sn == 2*n, sn
    assert sb == n*(pe//2 + pe//32) + n*pe*2, sb
    ifs.purge_kv_map()
    rn, rb = ifs.restore_pool(snap)
    assert rn == 2*n, rn
    after = torch.zeros_like(src)
    c.read_pages(after, mkeys, offs, pe); c.sync()
    assert torch.equal(after.view(torch.int16), before.view(torch.int16))
    plain = torch.zeros_like(src)
    c.read_pages(plain, pkeys, offs, pe); c.sync()
    assert torch.equal(plain.view(torch.int16), src.view(torch.int16))
    # Restore spreads entries over the shards, so start over on this GPU's
    # shard: n neighbouring blocks, holes below the survivors, then compact.
    ifs.purge_kv_map()
    c.write_pages(src, mkeys, offs, pe, sync=True, quant="mxfp4")
    assert c.delete_keys(mkeys[0::2]) == n // 2
    moved, moved_bytes = ifs.compact_pool()
    assert moved > 0 and moved_bytes == moved * (pe//2 + pe//32), (moved, moved_bytes)
    kept = torch.zeros_like(src)
    c.read_pages(kept, mkeys[1::2], offs[1::2], pe); c.sync()
    for o in offs[1::2]:
        assert torch.equal(kept[o:o+pe].view(torch.int16), before[o:o+pe].view(torch.int16))
    ifs.purge_kv_map()
c.close(); ifs.unregister_server()
print("MXFP4 SNAP OK")
"""],
        cwd=REPO, env={**os.environ, "PYTHONPATH": REPO + ":" + os.path.join(REPO, "tests")},
        timeout=180,
    ).returncode
    assert code == 0
