"""End-to-end protocol tests against a live in-process server with a CPU
(DRAM) pool — the no-GPU/no-RDMA loopback mode (BASELINE config 1). Covers
the behaviors the reference's integration suite checks
(/root/reference/infinistore/test_infinistore.py): write/read roundtrip,
dedup (first write wins), check_exist, get_match_last_index, KEY_NOT_FOUND,
async API, concurrent clients."""

import asyncio
import multiprocessing
import uuid

import pytest
import torch

import infinistore_amd as ifs

from conftest import make_client


def _keys(n, prefix=None):
    prefix = prefix or uuid.uuid4().hex
    return [f"{prefix}-{i}" for i in range(n)]


def put_get_roundtrip(conn, numel, page_elems, dtype=torch.float32):
    src = torch.randn(numel).to(dtype) if dtype.is_floating_point else torch.randint(
        0, 100, (numel,), dtype=dtype
    )
    dst = torch.zeros(numel, dtype=dtype)
    n_pages = numel // page_elems
    keys = _keys(n_pages)
    es = src.element_size()
    conn.register_mr(src)
    conn.register_mr(dst)
    blocks = conn.allocate_rdma(keys, page_elems * es)
    offsets = [i * page_elems for i in range(n_pages)]
    conn.rdma_write_cache(src, offsets, page_elems, blocks)
    conn.sync()
    conn.read_cache(dst, list(zip(keys, offsets)), page_elems)
    conn.sync()
    assert torch.equal(src, dst)
    return keys


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_roundtrip_dtypes(cpu_server, dtype):
    conn = make_client(cpu_server)
    try:
        put_get_roundtrip(conn, 4096, 1024, dtype)
    finally:
        conn.close()


def test_roundtrip_many_pages(cpu_server):
    conn = make_client(cpu_server)
    try:
        put_get_roundtrip(conn, 64 * 1024, 256)  # 256 pages of 1 KiB
    finally:
        conn.close()


def test_1kb_values(cpu_server):
    """BASELINE config 1: local put/get of 1 KB values over TCP loopback."""
    conn = make_client(cpu_server)
    try:
        put_get_roundtrip(conn, 2560, 256)  # 10 pages x 1 KB fp32
    finally:
        conn.close()


def test_dedup_first_write_wins(cpu_server):
    conn = make_client(cpu_server)
    try:
        key = f"dup-{uuid.uuid4()}"
        a = torch.full((256,), 1.0)
        b = torch.full((256,), 2.0)
        out = torch.zeros(256)
        conn.register_mr(a)
        conn.register_mr(b)
        conn.register_mr(out)
        blocks = conn.allocate_rdma([key], 256 * 4)
        conn.rdma_write_cache(a, [0], 256, blocks)
        conn.sync()
        # second allocate returns the FAKE block; write is silently dropped
        blocks2 = conn.allocate_rdma([key], 256 * 4)
        assert tuple(blocks2[0]) == (0, 0)
        conn.rdma_write_cache(b, [0], 256, blocks2)
        conn.sync()
        conn.read_cache(out, [(key, 0)], 256)
        conn.sync()
        assert torch.equal(out, a)
    finally:
        conn.close()


def test_check_exist(cpu_server):
    conn = make_client(cpu_server)
    try:
        keys = put_get_roundtrip(conn, 1024, 512)
        assert conn.check_exist(keys[0])
        assert not conn.check_exist("no-such-key-" + uuid.uuid4().hex)
    finally:
        conn.close()


def test_get_match_last_index(cpu_server):
    conn = make_client(cpu_server)
    try:
        stored = put_get_roundtrip(conn, 4 * 512, 512)  # 4 keys
        probe = stored[:3] + ["missing-1", stored[3], "missing-2"]
        assert conn.get_match_last_index(probe) == 2
        with pytest.raises(Exception):
            conn.get_match_last_index(["missing-a", "missing-b"])
    finally:
        conn.close()


def test_key_not_found(cpu_server):
    conn = make_client(cpu_server)
    try:
        dst = torch.zeros(256)
        conn.register_mr(dst)
        with pytest.raises(Exception):
            conn.read_cache(dst, [("never-stored-" + uuid.uuid4().hex, 0)], 256)
    finally:
        conn.close()


def test_uncommitted_not_readable(cpu_server):
    """Two-phase commit: allocated-but-unwritten keys must not be readable
    and must not count for check_exist / prefix match."""
    conn = make_client(cpu_server)
    try:
        key = f"pending-{uuid.uuid4()}"
        conn.allocate_rdma([key], 1024)
        assert not conn.check_exist(key)
        dst = torch.zeros(256)
        conn.register_mr(dst)
        with pytest.raises(Exception):
            conn.read_cache(dst, [(key, 0)], 256)
    finally:
        conn.close()


def test_purge_and_len(cpu_server):
    conn = make_client(cpu_server)
    try:
        before = ifs.get_kvmap_len()
        put_get_roundtrip(conn, 2048, 512)
        assert ifs.get_kvmap_len() == before + 4
        ifs.purge_kv_map()
        assert ifs.get_kvmap_len() == 0
    finally:
        conn.close()


def test_async_api(cpu_server):
    async def run():
        cfg = ifs.ClientConfig(
            host_addr="127.0.0.1",
            service_port=cpu_server,
            connection_type=ifs.TYPE_RDMA,
            link_type="TCP",
        )
        conn = ifs.InfinityConnection(cfg)
        await conn.connect_async()
        try:
            src = torch.arange(2048, dtype=torch.float32)
            dst = torch.zeros(2048, dtype=torch.float32)
            conn.register_mr(src)
            conn.register_mr(dst)
            keys = _keys(4)
            blocks = await conn.allocate_rdma_async(keys, 512 * 4)
            await conn.rdma_write_cache_async(src, [0, 512, 1024, 1536], 512, blocks)
            conn.sync()
            await conn.read_cache_async(
                dst, list(zip(keys, [0, 512, 1024, 1536])), 512
            )
            conn.sync()
            assert torch.equal(src, dst)
        finally:
            conn.close()

    asyncio.run(run())


def _client_proc(port, result_q):
    try:
        conn = make_client(port)
        put_get_roundtrip(conn, 8192, 512)
        conn.close()
        result_q.put("ok")
    except Exception as e:  # pragma: no cover
        result_q.put(f"fail: {e}")


def test_concurrent_clients(cpu_server):
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_client_proc, args=(cpu_server, q)) for _ in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=60) for _ in procs]
    for p in procs:
        p.join(timeout=30)
    assert results == ["ok", "ok"]


def test_oom_returns_error(ports):
    service_port, manage_port = ports
    cfg = ifs.ServerConfig(
        service_port=service_port,
        manage_port=manage_port,
        prealloc_size=1,  # GB — but granule large => few blocks? use small pool
        minimal_allocate_size=16,
        cpu_only=True,
    )
    # Shrink the pool by using a dedicated tiny server: 1 GB is the minimum
    # prealloc unit, so instead exhaust with large pages.
    ifs.register_server(cfg)
    try:
        conn = make_client(service_port)
        big = 1 << 20  # 1 MiB pages
        keys = _keys(1100)  # ~1.1 GB > 1 GB pool
        with pytest.raises(Exception):
            conn.allocate_rdma(keys, big)
        conn.close()
    finally:
        ifs.unregister_server()


def test_server_restart(ports):
    service_port, manage_port = ports
    for _ in range(2):
        cfg = ifs.ServerConfig(
            service_port=service_port,
            manage_port=manage_port,
            prealloc_size=1,
            minimal_allocate_size=16,
            cpu_only=True,
        )
        ifs.register_server(cfg)
        conn = make_client(service_port)
        put_get_roundtrip(conn, 1024, 512)
        conn.close()
        ifs.unregister_server()


def test_multi_shard_routing(ports):
    """Two CPU shards: allocation spreads via least-used routing; reads must
    gather correctly across shards (the xGMI cross-shard path, CPU-modeled)."""
    service_port, manage_port = ports
    cfg = ifs.ServerConfig(
        service_port=service_port,
        manage_port=manage_port,
        prealloc_size=1,
        minimal_allocate_size=16,
        cpu_only=True,
        cpu_shards=2,
    )
    ifs.register_server(cfg)
    try:
        conn = make_client(service_port)
        # Interleave many small allocations so both shards receive keys.
        put_get_roundtrip(conn, 32 * 1024, 256)  # 128 pages
        import json

        stats = json.loads(ifs.get_server_stats())
        assert stats["shards"] == 2
        conn.close()
    finally:
        ifs.unregister_server()


def test_delete_keys(cpu_server):
    conn = make_client(cpu_server)
    try:
        keys = put_get_roundtrip(conn, 2048, 512)  # 4 keys
        assert conn.delete_keys(keys[:2]) == 2
        assert not conn.check_exist(keys[0])
        assert conn.check_exist(keys[2])
        assert conn.delete_keys(["never-there"]) == 0
        dst = torch.zeros(512)
        conn.register_mr(dst)
        with pytest.raises(Exception):
            conn.read_cache(dst, [(keys[0], 0)], 512)
    finally:
        conn.close()


def test_compaction_defragments(ports):
    """Fill the pool with small pages, delete every other key, verify a big
    allocation fails, compact, verify it then succeeds."""
    service_port, manage_port = ports
    cfg = ifs.ServerConfig(
        service_port=service_port,
        manage_port=manage_port,
        prealloc_size=1,  # 1 GB
        minimal_allocate_size=1024,  # 1 MB granule -> 1024 blocks
        cpu_only=True,
    )
    ifs.register_server(cfg)
    try:
        conn = make_client(service_port)
        page = 1 << 20  # 1 MB pages
        n = 1024        # fill the entire 1 GB pool
        src = torch.zeros(page // 4, dtype=torch.float32)
        conn.register_mr(src)
        keys = [f"frag-{i}" for i in range(n)]
        blocks = conn.allocate_rdma(keys, page)
        assert len(blocks) == n
        # write+commit them all (1 MB each, chunked internally)
        for i in range(n):
            conn.rdma_write_cache(src, [0], page // 4, [blocks[i]])
        conn.sync()
        # free every other key -> 512 MB free but fragmented into 1 MB holes
        conn.delete_keys(keys[0::2])
        big = 16 << 20  # 16 MB needs 16 contiguous blocks
        with pytest.raises(Exception):
            conn.allocate_rdma(["big-page"], big)
        moved, moved_bytes = ifs.compact_pool()
        assert moved > 0 and moved_bytes == moved * page
        got = conn.allocate_rdma(["big-page"], big)
        assert len(got) == 1 and got[0][1] != 0
        conn.close()
    finally:
        ifs.unregister_server()


def test_read_pages_vectorized_api(cpu_server):
    """read_pages (vectorized extension API) over the fabric path."""
    import numpy as np

    conn = make_client(cpu_server)
    try:
        src = torch.randn(4096)
        dst = torch.zeros(4096)
        conn.register_mr(src)
        conn.register_mr(dst)
        keys = _keys(4)
        offsets = [0, 1024, 2048, 3072]
        blocks = conn.allocate_rdma(keys, 1024 * 4)
        conn.rdma_write_cache(src, offsets, 1024, blocks)
        conn.sync()
        conn.read_pages(dst, keys, np.asarray(offsets, dtype=np.uint64), 1024)
        conn.sync()
        assert torch.equal(src, dst)
    finally:
        conn.close()


def test_auto_evict_lru(ports):
    """With auto_evict on, a full pool evicts least-recently-accessed
    committed keys instead of failing; recently-read keys survive."""
    service_port, manage_port = ports
    cfg = ifs.ServerConfig(
        service_port=service_port,
        manage_port=manage_port,
        prealloc_size=1,  # 1 GB
        minimal_allocate_size=1024,  # 1 MB granule -> 1024 blocks
        cpu_only=True,
        auto_evict=True,
    )
    ifs.register_server(cfg)
    try:
        conn = make_client(service_port)
        page = 1 << 20
        src = torch.zeros(page // 4)
        dst = torch.zeros(page // 4)
        conn.register_mr(src)
        conn.register_mr(dst)

        def put(keys):
            blocks = conn.allocate_rdma(keys, page)
            for b in blocks:
                conn.rdma_write_cache(src, [0], page // 4, [b])
            conn.sync()

        put([f"old-{i}" for i in range(512)])
        put([f"mid-{i}" for i in range(512)])  # pool now full
        # touch the old keys so they become most-recently-used
        conn.read_cache(dst, [("old-0", 0)], page // 4)
        conn.sync()
        for i in range(1, 512, 64):
            conn.read_cache(dst, [(f"old-{i}", 0)], page // 4)
        conn.sync()
        # new writes must succeed by evicting the LRU keys (the untouched
        # old-* ones are oldest; the freshly-read ones must survive)
        put([f"new-{i}" for i in range(128)])
        assert conn.check_exist("new-0") and conn.check_exist("new-127")
        assert conn.check_exist("old-0")  # recently read -> survived
        evicted_old = sum(
            0 if conn.check_exist(f"old-{i}") else 1 for i in range(512)
        )
        evicted_mid = sum(
            0 if conn.check_exist(f"mid-{i}") else 1 for i in range(512)
        )
        assert evicted_old + evicted_mid >= 128
        # untouched old keys are evicted before the (younger) mid keys
        assert evicted_old >= evicted_mid
        conn.close()
    finally:
        ifs.unregister_server()


def test_auto_extend_grows_pool(ports):
    """auto_increase: the pool extends in the background when the last arena
    crosses the usage threshold (role of the reference's add_mempool flow)."""
    import json
    import time

    service_port, manage_port = ports
    cfg = ifs.ServerConfig(
        service_port=service_port,
        manage_port=manage_port,
        prealloc_size=1,           # 1 GB initial
        extend_size=1,             # +1 GB per extension
        minimal_allocate_size=1024,
        cpu_only=True,
        auto_increase=True,
    )
    ifs.register_server(cfg)
    try:
        conn = make_client(service_port)
        page = 1 << 20
        src = torch.zeros(page // 4)
        conn.register_mr(src)
        total0 = json.loads(ifs.get_server_stats())["total_blocks"]
        # push usage past 80% to trigger background extension
        keys = [f"x-{i}" for i in range(850)]
        blocks = conn.allocate_rdma(keys, page)
        assert len(blocks) == 850
        deadline = time.time() + 20
        while time.time() < deadline:
            if json.loads(ifs.get_server_stats())["total_blocks"] > total0:
                break
            time.sleep(0.2)
        assert json.loads(ifs.get_server_stats())["total_blocks"] > total0
        # and the extra capacity is usable
        more = conn.allocate_rdma([f"y-{i}" for i in range(400)], page)
        assert len(more) == 400
        conn.close()
    finally:
        ifs.unregister_server()


def test_fabric_via_container_ip(cpu_server):
    """Connect via the container's non-loopback address (the cross-host
    code path, minus the physical network)."""
    import socket as _socket

    try:
        ip = _socket.gethostbyname(_socket.gethostname())
    except OSError:
        pytest.skip("no resolvable host address")
    if ip.startswith("127."):
        pytest.skip("hostname resolves to loopback")
    cfg = ifs.ClientConfig(
        host_addr=ip, service_port=cpu_server,
        connection_type=ifs.TYPE_RDMA, link_type="TCP",
    )
    conn = ifs.InfinityConnection(cfg)
    conn.connect()
    try:
        src = torch.arange(1024, dtype=torch.float32)
        dst = torch.zeros_like(src)
        conn.register_mr(src)
        conn.register_mr(dst)
        key = f"ip-{uuid.uuid4()}"
        blocks = conn.allocate_rdma([key], 4096)
        conn.rdma_write_cache(src, [0], 1024, blocks)
        conn.sync()
        conn.read_cache(dst, [(key, 0)], 1024)
        conn.sync()
        assert torch.equal(src, dst)
    finally:
        conn.close()


def test_tcp_transport_explicit(cpu_server):
    """Force the TCP transport (127.0.0.2 avoids the UDS fast path) so both
    transports stay covered."""
    cfg = ifs.ClientConfig(
        host_addr="127.0.0.2", service_port=cpu_server,
        connection_type=ifs.TYPE_RDMA, link_type="TCP",
    )
    conn = ifs.InfinityConnection(cfg)
    conn.connect()
    try:
        put_get_roundtrip(conn, 2048, 512)
    finally:
        conn.close()


def test_example_client_async(cpu_server):
    from infinistore_amd.example import client_async

    asyncio.run(client_async.main(cpu_server))


def test_ttl_expiry(ports):
    """TTL (extension): keys expire `ttl_seconds` after insert — lookups
    treat them as absent, an expired key can be overwritten with fresh
    data, and the evictor reclaims expired entries first."""
    import time

    service_port, manage_port = ports
    cfg = ifs.ServerConfig(
        service_port=service_port, manage_port=manage_port,
        prealloc_size=1, minimal_allocate_size=16, cpu_only=True,
        ttl_seconds=2, auto_evict=True,
    )
    ifs.register_server(cfg)
    try:
        conn = make_client(service_port)
        src = torch.arange(4096, dtype=torch.float32)
        dst = torch.zeros_like(src)
        conn.register_mr(src)
        conn.register_mr(dst)
        blocks = conn.allocate_rdma(["ttl-key"], 4096 * 4)
        conn.rdma_write_cache(src, [0], 4096, blocks)
        conn.sync()
        assert conn.check_exist("ttl-key")
        conn.read_cache(dst, [("ttl-key", 0)], 4096)
        conn.sync()
        assert torch.equal(src, dst)

        time.sleep(3)  # past the 2 s TTL
        assert not conn.check_exist("ttl-key")
        with pytest.raises(Exception):
            conn.read_cache(dst, [("ttl-key", 0)], 4096)
        # the background sweeper reclaims the memory proactively (period
        # ttl/4, min 1 s; poll past the second-granularity boundary)
        for _ in range(60):
            if ifs.get_kvmap_len() == 0:
                break
            time.sleep(0.2)
        assert ifs.get_kvmap_len() == 0

        # the expired key is overwritable (allocate returns a REAL block,
        # not the dup-key FAKE) and fresh data round-trips
        src2 = src + 1
        conn.register_mr(src2)
        blocks2 = conn.allocate_rdma(["ttl-key"], 4096 * 4)
        assert blocks2[0] != (0, 0) and tuple(blocks2[0])[1] != 0
        conn.rdma_write_cache(src2, [0], 4096, blocks2)
        conn.sync()
        conn.read_cache(dst, [("ttl-key", 0)], 4096)
        conn.sync()
        assert torch.equal(src2, dst)
        conn.close()
    finally:
        ifs.unregister_server()


def test_large_streamed_read(ports):
    """Single-shard reads >32 MB take the segment-streaming path (the
    response is written to the socket while later segments still copy);
    verify byte-exactness across the segment boundaries."""
    service_port, manage_port = ports
    cfg = ifs.ServerConfig(
        service_port=service_port, manage_port=manage_port,
        prealloc_size=1, minimal_allocate_size=128, cpu_only=True,
    )
    ifs.register_server(cfg)
    try:
        conn = make_client(service_port)
        n, pe = 384, 32768  # 384 x 128 KB = 48 MB > 2 x 16 MB segments
        src = torch.rand(n * pe)
        dst = torch.zeros_like(src)
        conn.register_mr(src)
        conn.register_mr(dst)
        keys = [f"big-{i}" for i in range(n)]
        offs = [i * pe for i in range(n)]
        blocks = conn.allocate_rdma(keys, pe * 4)
        conn.rdma_write_cache(src, offs, pe, blocks)
        conn.sync()
        conn.read_cache(dst, list(zip(keys, offs)), pe)
        conn.sync()
        assert torch.equal(src, dst)
        # and a shuffled-offset read (host offsets still ascend per request
        # order on the wire; destination scatter is the client's readv)
        import random
        order = list(range(n))
        random.Random(3).shuffle(order)
        dst.zero_()
        conn.read_cache(dst, [(keys[i], offs[i]) for i in order], pe)
        conn.sync()
        assert torch.equal(src, dst)
        conn.close()
    finally:
        ifs.unregister_server()


# ---- read sizes (docs/protocol.md, "read sizes") ----------------------------
# A plain entry serves a whole-page read of at most its own size and returns
# that prefix; a larger page is INVALID_REQ before anything is copied. The
# sizes: below the 16 KiB granule, exactly one granule, one granule plus 16.
READ_SIZE_KEYS = [1000, 16384, 16400]
SENTINEL = 0xA5
INVALID_REQ = "ret = -400"


@pytest.fixture(scope="module")
def read_size_server():
    """One CPU-pool server for all read-size cases (their keys are unique, and
    a server start and stop costs about 2 s); yields the service port."""
    from conftest import free_port

    port = free_port()
    ifs.register_server(ifs.ServerConfig(
        service_port=port, manage_port=free_port(), prealloc_size=1,
        minimal_allocate_size=16, cpu_only=True))
    yield port
    ifs.unregister_server()


def _u8_pattern(n, seed):
    g = torch.Generator().manual_seed(seed)
    # never the sentinel, so "untouched" and "copied" cannot be confused
    t = torch.randint(0, 255, (n,), dtype=torch.uint8, generator=g)
    t[t == SENTINEL] = 255
    return t


def _put_u8(conn, keys, size, data):
    conn.register_mr(data)
    blocks = conn.allocate_rdma(keys, size)
    conn.rdma_write_cache(data, [i * size for i in range(len(keys))], size, blocks)
    conn.sync()
    return blocks


def _sentinel_dst(conn, n):
    dst = torch.full((n,), SENTINEL, dtype=torch.uint8)
    conn.register_mr(dst)
    return dst


@pytest.mark.parametrize("size", READ_SIZE_KEYS)
def test_read_size_prefix_and_refusal(read_size_server, size):
    conn = make_client(read_size_server)
    try:
        # the key under test first, then neighbours that an over-read would hit
        keys = _keys(4)
        data = _u8_pattern(4 * size, seed=size)
        _put_u8(conn, keys, size, data)
        want = data[:size]
        for page in (size, size - 1, size // 2):
            dst = _sentinel_dst(conn, 2 * size + 16)
            conn.read_cache(dst, [(keys[0], 0)], page)
            conn.sync()
            assert torch.equal(dst[:page], want[:page]), page
            assert bool((dst[page:] == SENTINEL).all()), page
        for page in (size + 1, 2 * size):
            dst = _sentinel_dst(conn, 2 * size + 16)
            with pytest.raises(Exception, match=INVALID_REQ):
                conn.read_cache(dst, [(keys[0], 0)], page)
            assert bool((dst == SENTINEL).all()), page
            # the same connection keeps serving
            conn.read_cache(dst, [(keys[0], 0)], size)
            conn.sync()
            assert torch.equal(dst[:size], want)
            assert bool((dst[size:] == SENTINEL).all())
    finally:
        conn.close()


@pytest.mark.parametrize("size", READ_SIZE_KEYS)
def test_read_size_mixed_request_is_refused_whole(read_size_server, size):
    conn = make_client(read_size_server)
    try:
        big = 2 * size
        good = _keys(3)
        gdata = _u8_pattern(3 * big, seed=size + 1)
        _put_u8(conn, good, big, gdata)
        short = _keys(1)
        _put_u8(conn, short, size, _u8_pattern(size, seed=size + 2))
        for order in ([good[0], good[1], short[0], good[2]], short + good, good + short):
            dst = _sentinel_dst(conn, 4 * big)
            with pytest.raises(Exception, match=INVALID_REQ):
                conn.read_cache(dst, [(k, i * big) for i, k in enumerate(order)], big)
            assert bool((dst == SENTINEL).all())
        dst = _sentinel_dst(conn, 4 * big)
        conn.read_cache(dst, [(k, i * big) for i, k in enumerate(good)], big)
        conn.sync()
        assert torch.equal(dst[: 3 * big], gdata)
        assert bool((dst[3 * big:] == SENTINEL).all())
    finally:
        conn.close()


@pytest.mark.parametrize("size", READ_SIZE_KEYS)
def test_read_size_after_a_larger_rewrite_of_the_key(read_size_server, size):
    """Dedup is first-write-wins at any size: the second writer of a key, with
    a page twice as large, gets the FAKE block, and its own read at its own
    size is refused; the first writer's bytes stay readable."""
    conn = make_client(read_size_server)
    try:
        keys = _keys(4)
        first = _u8_pattern(4 * size, seed=size + 3)
        _put_u8(conn, keys, size, first)
        second = _u8_pattern(2 * size, seed=size + 4)
        blocks2 = _put_u8(conn, keys[:1], 2 * size, second)
        assert tuple(blocks2[0]) == (0, 0)
        dst = _sentinel_dst(conn, 2 * size)
        with pytest.raises(Exception, match=INVALID_REQ):
            conn.read_cache(dst, [(keys[0], 0)], 2 * size)
        assert bool((dst == SENTINEL).all())
        conn.read_cache(dst, [(keys[0], 0)], size)
        conn.sync()
        assert torch.equal(dst[:size], first[:size])
        assert bool((dst[size:] == SENTINEL).all())
    finally:
        conn.close()


def test_read_size_refused_before_a_streamed_response(read_size_server):
    """A 40 MiB single-shard response streams in 16 MiB segments. A short
    entry in the LAST segment must refuse the read before the first segment
    is on the wire: the client sees INVALID_REQ, not a torn payload, and the
    connection's framing survives."""
    conn = make_client(read_size_server)
    try:
        page, n = 128 << 10, 320  # 40 MiB
        keys = _keys(n)
        data = _u8_pattern(n * page, seed=40)
        _put_u8(conn, keys[:-1], page, data)
        _put_u8(conn, keys[-1:], page // 2, data[(n - 1) * page:])
        offs = [i * page for i in range(n)]
        dst = _sentinel_dst(conn, n * page)
        with pytest.raises(Exception, match=INVALID_REQ):
            conn.read_cache(dst, list(zip(keys, offs)), page)
        assert bool((dst == SENTINEL).all())
        # same connection: the streamed path with the good keys only, and the
        # short key at its own size
        conn.read_cache(dst, list(zip(keys[:-1], offs)), page)
        conn.read_cache(dst, [(keys[-1], offs[-1])], page // 2)
        conn.sync()
        assert torch.equal(dst[: (n - 1) * page + page // 2], data[: (n - 1) * page + page // 2])
        assert bool((dst[(n - 1) * page + page // 2:] == SENTINEL).all())
    finally:
        conn.close()
