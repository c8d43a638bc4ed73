"""GPU (MI355X) tests: local IPC path with the batched HIP gather/scatter
kernel, HBM pool shards, fingerprint kernel numerics, and fabric interop.
All tests here are @pytest.mark.gpu and need ROCm hardware."""

import json
import os
import socket
import subprocess
import sys
import time
import uuid

import pytest
import torch

import infinistore_amd as ifs

from _kernel_refs import (
    assert_bf16_bits_equal,
    bf16_bits,
    fingerprint_ref as _fingerprint_ref,
    fp8_dequant_ref,
    fp8_quant_ref,
)
from conftest import free_port, make_client

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wait_port(port, timeout=60):
    t0 = time.time()
    while time.time() - t0 < timeout:
        try:
            s = socket.create_connection(("127.0.0.1", port), timeout=1)
            s.close()
            return True
        except OSError:
            time.sleep(0.3)
    return False


@pytest.fixture(scope="module")
def gpu_server():
    """Server subprocess with HBM pool shards on all GPUs (the local IPC path
    requires separate client/server processes)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    port = free_port()
    proc = subprocess.Popen(
        [
            sys.executable, "-m", "infinistore_amd.server",
            "--service-port", str(port),
            "--manage-port", str(free_port()),
            "--prealloc-size", "4",
            "--minimal-allocate-size", "64",
            "--no-manage",
            "--log-level", "info",
        ],
        cwd=REPO,
    )
    assert _wait_port(port), "server did not come up"
    yield port
    proc.terminate()
    proc.wait(timeout=20)


def local_conn(port):
    cfg = ifs.ClientConfig(
        host_addr="127.0.0.1", service_port=port, connection_type=ifs.TYPE_LOCAL_GPU
    )
    c = ifs.InfinityConnection(cfg)
    c.connect()
    return c


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_local_roundtrip_dtypes(gpu_server, dtype):
    conn = local_conn(gpu_server)
    try:
        n = 64 * 1024
        page = 16 * 1024
        src = torch.randn(n, device="cuda:0").to(dtype)
        dst = torch.zeros(n, dtype=dtype, device="cuda:0")
        keys = [f"{uuid.uuid4()}-{i}" for i in range(n // page)]
        offs = [i * page for i in range(n // page)]
        conn.local_gpu_write_cache(src, list(zip(keys, offs)), page)
        conn.sync()
        conn.read_cache(dst, list(zip(keys, offs)), page)
        conn.sync()
        assert torch.equal(src, dst)
    finally:
        conn.close()


def test_local_roundtrip_caching_allocator(gpu_server):
    """The base_offset protocol extension: tensors allocated by the torch
    caching allocator (NOT at an allocation base) must round-trip."""
    conn = local_conn(gpu_server)
    try:
        pad = torch.empty(1000, device="cuda:0")  # shifts the next alloc
        src = torch.randn(32768, device="cuda:0")
        dst = torch.zeros_like(src)
        del pad
        key = f"off-{uuid.uuid4()}"
        conn.local_gpu_write_cache(src, [(key, 0)], 32768)
        conn.sync()
        conn.read_cache(dst, [(key, 0)], 32768)
        conn.sync()
        assert torch.equal(src, dst)
    finally:
        conn.close()


def test_local_many_blocks_128kb(gpu_server):
    """The headline shape: many 128 KB blocks in one request -> one kernel."""
    conn = local_conn(gpu_server)
    try:
        page_elems = 65536  # 128 KB bf16
        nb = 512            # 64 MB
        src = torch.randn(nb * page_elems, dtype=torch.bfloat16, device="cuda:0")
        dst = torch.zeros_like(src)
        pre = uuid.uuid4().hex
        keys = [f"{pre}-{i}" for i in range(nb)]
        offs = [i * page_elems for i in range(nb)]
        conn.local_gpu_write_cache(src, list(zip(keys, offs)), page_elems)
        conn.sync()
        conn.read_cache(dst, list(zip(keys, offs)), page_elems)
        conn.sync()
        assert torch.equal(src, dst)
    finally:
        conn.close()


def test_local_dedup_and_queries(gpu_server):
    conn = local_conn(gpu_server)
    try:
        a = torch.full((8192,), 1.0, device="cuda:0")
        b = torch.full((8192,), 2.0, device="cuda:0")
        out = torch.zeros(8192, device="cuda:0")
        key = f"dup-{uuid.uuid4()}"
        conn.local_gpu_write_cache(a, [(key, 0)], 8192)
        conn.sync()
        conn.local_gpu_write_cache(b, [(key, 0)], 8192)  # silently dropped
        conn.sync()
        conn.read_cache(out, [(key, 0)], 8192)
        conn.sync()
        assert torch.equal(out, a)
        assert conn.check_exist(key)
        assert conn.get_match_last_index([key, "missing-x"]) == 0
    finally:
        conn.close()


def test_interop_rdma_write_local_read(gpu_server):
    """Write via the fabric path (CPU tensor), read via the local GPU path —
    the reference's CPU-RDMA -> local-GPU interop case."""
    wconn = make_client(gpu_server)
    rconn = local_conn(gpu_server)
    try:
        src = torch.randn(32768)  # CPU
        dst = torch.zeros(32768, device="cuda:0")
        key = f"interop-{uuid.uuid4()}"
        wconn.register_mr(src)
        blocks = wconn.allocate_rdma([key], 32768 * 4)
        wconn.rdma_write_cache(src, [0], 32768, blocks)
        wconn.sync()
        rconn.read_cache(dst, [(key, 0)], 32768)
        rconn.sync()
        assert torch.equal(src, dst.cpu())
    finally:
        wconn.close()
        rconn.close()


def test_gpu_tensor_fabric_roundtrip(gpu_server):
    """RDMA-semantics path with a GPU tensor on the client side (d2h staging
    on the client, h2d into the HBM pool on the server)."""
    conn = make_client(gpu_server)
    try:
        src = torch.randn(65536, device="cuda:0")
        dst = torch.zeros(65536, device="cuda:0")
        conn.register_mr(src)
        conn.register_mr(dst)
        pre = uuid.uuid4().hex
        keys = [f"{pre}-{i}" for i in range(4)]
        offs = [i * 16384 for i in range(4)]
        blocks = conn.allocate_rdma(keys, 16384 * 4)
        conn.rdma_write_cache(src, offs, 16384, blocks)
        conn.sync()
        conn.read_cache(dst, list(zip(keys, offs)), 16384)
        conn.sync()
        assert torch.equal(src, dst)
    finally:
        conn.close()


def test_fabric_staged_multichunk_roundtrip(gpu_server):
    """TCP fabric with a GPU-shard pool across several 32 MB staging chunks:
    600 x 128 KB = 75 MB exercises the double-buffered pinned-stage pipeline
    (chunk k+1's host memcpy overlapping chunk k's H2D+kernel) in both
    directions, including the chunk-boundary descriptor handoff."""
    conn = make_client(gpu_server)
    try:
        n, elems = 600, 32768  # 128 KB blocks of float32
        src = torch.randn(n * elems)  # CPU tensors: the fabric moves bytes
        dst = torch.zeros_like(src)
        conn.register_mr(src)
        conn.register_mr(dst)
        pre = uuid.uuid4().hex[:8]
        keys = [f"fsm-{pre}-{i}" for i in range(n)]
        offs = [i * elems for i in range(n)]
        blocks = conn.allocate_rdma(keys, elems * 4)
        conn.rdma_write_cache(src, offs, elems, blocks)
        conn.sync()
        # read back in a shuffled order so stage slots differ from put order
        import random

        order = list(range(n))
        random.Random(7).shuffle(order)
        conn.read_cache(dst, [(keys[i], offs[i]) for i in order], elems)
        conn.sync()
        assert torch.equal(src, dst)
    finally:
        conn.close()


def test_fingerprint_kernel_vs_cpu_reference():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.manual_seed(0)
    t = torch.randn(16384, device="cuda:0")  # 64 KB fp32
    bs = 16384  # bytes per block -> 4 blocks
    got = ifs.fingerprint_blocks(t, [0, 4096, 8192, 12288], 4096)
    ref = _fingerprint_ref(t.cpu().numpy().tobytes(), bs)
    assert got == ref
    # determinism + sensitivity
    again = ifs.fingerprint_blocks(t, [0, 4096, 8192, 12288], 4096)
    assert again == got
    t2 = t.clone()
    t2[0] += 1.0
    other = ifs.fingerprint_blocks(t2, [0, 4096, 8192, 12288], 4096)
    assert other[0] != got[0] and other[1:] == got[1:]


def test_native_extension_is_loaded():
    """Guard against a silent eager/PyTorch fallback: the HIP extension must
    actually be the thing serving GPU ops."""
    from infinistore_amd import _native

    assert _native.gpu_available()
    assert _native.__file__.endswith(".so")
    assert "infinistore_amd" in _native.__file__


def test_bench_smoke():
    env = dict(os.environ)
    r = subprocess.run(
        [sys.executable, "bench.py", "--full", "--steps", "3", "--warmup", "1",
         "--blocks", "256", "--latency-ops", "30", "--pool-gb", "2"],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=420,
    )
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["metric"] == "put_get_GBps" and out["value"] > 0
    assert out["config"]["path"] == "local_gpu_ipc"
    # --full: the secondary measurements are present
    assert out["config"]["put_GBps"] > 0 and out["config"]["get_GBps"] > 0
    assert out["config"]["p50_put_us"] > 0 and out["config"]["p99_get_us"] > 0


def test_bench_plain_dump_outputs(tmp_path):
    """A plain run times exactly --steps steps, skips the secondary
    measurements and, with --dump-outputs, writes what the last timed step
    read back: one float32 file per client worker, every page sampled at the
    same positions, element 0 of each page carrying that step's salt."""
    import numpy as np

    steps, blocks, procs, page_elems = 3, 256, 4, 128 * 1024 // 2
    r = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps),
         "--warmup", "1", "--blocks", str(blocks), "--pool-gb", "2",
         "--dump-outputs", str(tmp_path)],
        cwd=REPO, env=dict(os.environ), capture_output=True, text=True,
        timeout=420,
    )
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["metric"] == "put_get_GBps" and out["value"] > 0
    assert out["steps"] == steps and out["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region (ms_per_step is
    # rounded to 1 us, i.e. to within 5% for any step of 10 us or longer)
    gb_per_step = 2 * blocks * 128 * 1024 / 1e9
    assert out["value"] == pytest.approx(
        gb_per_step / (out["ms_per_step"] / 1e3), rel=5e-2)
    for k in ("put_GBps", "get_GBps", "p50_put_us", "p99_get_us"):
        assert out["config"][k] is None
    files = sorted(p.name for p in tmp_path.iterdir())
    assert files == [f"get_r0w{w}.npy" for w in range(procs)]
    total = 0
    for f in files:
        a = np.load(tmp_path / f)
        assert a.dtype == np.float32 and np.isfinite(a).all()
        total += a.nbytes
        pages = a.reshape(blocks // procs, -1)
        assert pages.shape[1] <= page_elems
        # the last timed step (index steps-1) writes salt steps
        assert (pages[:, 0] == float(steps)).all()
        assert pages[:, 1:].std() > 0.5  # randn payload, not zeros
    assert total <= 64 << 20


def test_bench_bounded_store(tmp_path):
    """More timed steps than the pool can hold: the run keeps only the
    newest steps resident (deleting the oldest step's keys as it goes) and
    still verifies and dumps the last step. 11 steps of 1024 x 128 KB
    against a 1 GB pool = 8192 blocks, of which 90% minus the warmup keys
    leave room for 5 steps."""
    import numpy as np

    steps, blocks, procs = 11, 1024, 4
    r = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps),
         "--warmup", "1", "--blocks", str(blocks), "--pool-gb", "1",
         "--pool-cap-gb", "1", "--dump-outputs", str(tmp_path)],
        cwd=REPO, env=dict(os.environ), capture_output=True, text=True,
        timeout=420,
    )
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["steps"] == steps and out["value"] > 0
    assert out["config"]["resident_steps"] == 5
    for w in range(procs):
        a = np.load(tmp_path / f"get_r0w{w}.npy")
        pages = a.reshape(blocks // procs, -1)
        # last step index 10 -> salt (10 % 4) + 1
        assert (pages[:, 0] == 3.0).all() and pages[:, 1:].std() > 0.5


def test_cross_gpu_read(gpu_server):
    """Disaggregated pattern over xGMI: writer on GPU 0, reader on GPU 1 —
    the pool shard's copy kernel pushes into peer memory. Runs on the
    multi-GPU round-end box; skipped on 1-GPU boxes."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    wconn = local_conn(gpu_server)
    rconn = local_conn(gpu_server)
    try:
        n = 256 * 1024
        page = 64 * 1024
        src = torch.randn(n, device="cuda:0")
        dst = torch.zeros(n, device="cuda:1")
        pre = uuid.uuid4().hex
        keys = [f"{pre}-{i}" for i in range(n // page)]
        offs = [i * page for i in range(n // page)]
        wconn.local_gpu_write_cache(src, list(zip(keys, offs)), page)
        wconn.sync()
        rconn.read_cache(dst, list(zip(keys, offs)), page)
        rconn.sync()
        assert torch.equal(src.cpu(), dst.cpu())
    finally:
        wconn.close()
        rconn.close()


def test_cross_gpu_write(gpu_server):
    """Writer tensor on GPU 1, shard affinity routes to shard 1; reader on
    GPU 0 pulls across xGMI."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    wconn = local_conn(gpu_server)
    rconn = local_conn(gpu_server)
    try:
        n = 64 * 1024
        src = torch.randn(n, device="cuda:1")
        dst = torch.zeros(n, device="cuda:0")
        key = f"xw-{uuid.uuid4()}"
        wconn.local_gpu_write_cache(src, [(key, 0)], n)
        wconn.sync()
        rconn.read_cache(dst, [(key, 0)], n)
        rconn.sync()
        assert torch.equal(src.cpu(), dst.cpu())
    finally:
        wconn.close()
        rconn.close()


def test_cross_gpu_read_pull_mode(gpu_server):
    """IFS_CROSS_COPY=reader: the copy kernel runs on the READER's shard,
    remote-reading the owner's HBM over xGMI (docs/design.md 'Cross-shard
    copy side'). Own server subprocess because the mode is read once at
    server start. Skipped on 1-GPU boxes."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    port = free_port()
    env = dict(os.environ, IFS_CROSS_COPY="reader")
    proc = subprocess.Popen(
        [sys.executable, "-m", "infinistore_amd.server",
         "--service-port", str(port), "--manage-port", str(free_port()),
         "--prealloc-size", "2", "--minimal-allocate-size", "64",
         "--no-manage"],
        cwd=REPO, env=env,
    )
    try:
        assert _wait_port(port), "pull-mode server did not come up"
        wconn = local_conn(port)
        rconn = local_conn(port)
        try:
            n = 256 * 1024
            page = 64 * 1024
            src = torch.randn(n, device="cuda:0")  # owner shard: GPU 0
            dst = torch.zeros(n, device="cuda:1")  # reader: GPU 1's shard pulls
            pre = uuid.uuid4().hex
            keys = [f"pull-{pre}-{i}" for i in range(n // page)]
            offs = [i * page for i in range(n // page)]
            wconn.local_gpu_write_cache(src, list(zip(keys, offs)), page)
            wconn.sync()
            rconn.read_cache(dst, list(zip(keys, offs)), page)
            rconn.sync()
            assert torch.equal(src.cpu(), dst.cpu())
        finally:
            wconn.close()
            rconn.close()
    finally:
        proc.terminate()
        proc.wait(timeout=20)


def test_benchmark_harness_gpu(gpu_server):
    """Reference-style harness end-to-end on the GPU local path."""
    r = subprocess.run(
        [sys.executable, "-m", "infinistore_amd.benchmark",
         "--port", str(gpu_server), "--local-gpu", "--size", "64",
         "--block-size", "128", "--iteration", "1", "--latency-ops", "10",
         "--json", "--verify"],
        cwd=REPO, capture_output=True, text=True, timeout=300,
    )
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["path"] == "local_gpu" and out["write_MBps"] > 0


def test_example_client_run(gpu_server):
    """The sync client example's core roundtrip against a live server."""
    cfg = ifs.ClientConfig(host_addr="127.0.0.1", service_port=gpu_server,
                           connection_type=ifs.TYPE_LOCAL_GPU)
    conn = ifs.InfinityConnection(cfg)
    conn.connect()
    from infinistore_amd.example import client as ex

    ex.run(conn, "cuda:0", "cuda:0")
    conn.close()


def test_demo_prefill_example(gpu_server):
    """The layer-overlap prefill pattern example end to end."""
    from infinistore_amd.example import demo_prefill

    demo_prefill.main(gpu_server)


def test_gpu_page_hashes_wrapper():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from infinistore_amd.kv_connector import gpu_page_hashes

    t = torch.randn(4 * 4096, device="cuda:0")
    h1 = gpu_page_hashes(t, [0, 4096, 8192, 12288], 4096)
    h2 = gpu_page_hashes(t, [0, 4096, 8192, 12288], 4096)
    assert h1 == h2 and len(set(h1)) == 4  # deterministic chain, distinct
    t2 = t.clone()
    t2[5000] += 1.0  # page 1 changes -> pages 1..3 chain digests change
    h3 = gpu_page_hashes(t2, [0, 4096, 8192, 12288], 4096)
    assert h3[0] == h1[0] and h3[1] != h1[1] and h3[3] != h1[3]


def test_shm_transport_roundtrip(gpu_server):
    """Same-host packed ops ride the shared-memory ring (csrc/core/shm_ring.h):
    the transport must be active on a local conn, round-trip correctly
    (including requests big enough to wrap the 1 MB ring several times), and
    fall back to the socket when disabled via IFS_NO_SHM."""
    conn = local_conn(gpu_server)
    try:
        assert conn.conn.shm_active(), "shm ring should be active on a local conn"
        n_blocks, page = 600, 4096  # ~20 KB of keys/offsets per request
        src = torch.randn(n_blocks * page // 4, device="cuda:0")
        dst = torch.zeros_like(src)
        offs = [i * page // 4 for i in range(n_blocks)]
        for rep in range(8):  # > 8 MB of request records => ring wraps
            keys = [f"shm-{uuid.uuid4()}-{rep}-{i}" for i in range(n_blocks)]
            if rep % 2:  # pre-serialized key-blob form
                blob = ifs.InfinityConnection.pack_keys(keys)
                conn.write_pages(src, blob, offs, page // 4, sync=True)
                dst.zero_()
                conn.read_pages(dst, blob, offs, page // 4)
            else:
                conn.local_gpu_write_cache(src, list(zip(keys, offs)), page // 4)
                conn.sync()
                dst.zero_()
                conn.read_cache(dst, list(zip(keys, offs)), page // 4)
            conn.sync()
            assert torch.equal(src, dst)
    finally:
        conn.close()


def test_shm_disabled_fallback(gpu_server):
    env = os.environ.copy()
    env["IFS_NO_SHM"] = "1"
    code = subprocess.run(
        [sys.executable, "-c", f"""
import torch, uuid
import infinistore_amd as ifs
cfg = ifs.ClientConfig(host_addr="127.0.0.1", service_port={gpu_server},
                       connection_type=ifs.TYPE_LOCAL_GPU)
c = ifs.InfinityConnection(cfg)
c.connect()
assert not c.conn.shm_active()
src = torch.randn(8192, device="cuda:0")
dst = torch.zeros_like(src)
key = f"nshm-{{uuid.uuid4()}}"
c.local_gpu_write_cache(src, [(key, 0)], 8192)
c.sync()
c.read_cache(dst, [(key, 0)], 8192)
c.sync()
assert torch.equal(src, dst)
c.close()
"""],
        env=env, cwd=REPO, timeout=120,
    ).returncode
    assert code == 0


@pytest.mark.parametrize("transport", ["socket", "shm"])
def test_large_batch_dedup_read_delete(gpu_server, transport, monkeypatch):
    """One-request batches of ~32-40 keys per index stripe (the prefetch
    look-ahead runs): first write wins against a second write of other data,
    new keys in that second write land, everything reads back exactly, and
    delete / read-after-delete / check_exist agree. Over both transports."""
    if transport == "socket":
        monkeypatch.setenv("IFS_NO_SHM", "1")
    conn = local_conn(gpu_server)
    try:
        assert conn.conn.shm_active() == (transport == "shm")
        page = 1024  # fp32 elements: 4 KB pages
        n_old, n_new = 2048, 512
        n_all = n_old + n_new
        pre = uuid.uuid4().hex
        keys = [f"{pre}-{i}" for i in range(n_all)]
        offs = [i * page for i in range(n_all)]
        first = torch.randn(n_all * page, device="cuda:0")
        second = torch.randn(n_all * page, device="cuda:0")
        conn.local_gpu_write_cache(first, list(zip(keys[:n_old], offs[:n_old])), page)
        conn.sync()
        conn.local_gpu_write_cache(second, list(zip(keys, offs)), page)
        conn.sync()
        dst = torch.zeros_like(first)
        conn.read_cache(dst, list(zip(keys, offs)), page)
        conn.sync()
        assert torch.equal(dst[: n_old * page], first[: n_old * page])  # old keys keep first data
        assert torch.equal(dst[n_old * page:], second[n_old * page:])  # new keys hold new data

        gone, kept = keys[::2], keys[1::2]
        assert conn.delete_keys(gone) == len(gone)
        with pytest.raises(Exception, match="-404"):  # KEY_NOT_FOUND
            conn.read_cache(dst, [(gone[0], 0)], page)
        assert not conn.check_exist(gone[0]) and not conn.check_exist(gone[-1])
        assert conn.check_exist(kept[0]) and conn.check_exist(kept[-1])
        assert conn.delete_keys(kept) == len(kept)  # leave the shared pool as found
    finally:
        conn.close()


def test_ticketed_async_reads(gpu_server):
    """read_pages_async/wait_read: multiple reads in flight on one conn,
    responses consumed out of submission order."""
    conn = local_conn(gpu_server)
    try:
        page = 32768
        n = 64
        src = torch.randn(page * n // 4, device="cuda:0")
        dsts = [torch.zeros(page * n // 4, device="cuda:0") for _ in range(3)]
        offs = [i * page // 4 for i in range(n)]
        keysets = []
        for rep in range(3):
            keys = [f"tk-{uuid.uuid4()}-{rep}-{i}" for i in range(n)]
            conn.write_pages(src, keys, offs, page // 4, sync=True)
            keysets.append(keys)
        tickets = [conn.read_pages_async(dsts[r], keysets[r], offs, page // 4)
                   for r in range(3)]
        for t in reversed(tickets):  # wait out of order
            conn.wait_read(t)
        for d in dsts:
            assert torch.equal(src, d)
        # missing key surfaces as an error at wait time (or at push for the
        # blocking fallback)
        import pytest as _pytest
        with _pytest.raises(Exception):
            t = conn.read_pages_async(dsts[0], ["tk-missing-key"], [0], page // 4)
            conn.wait_read(t)
    finally:
        conn.close()


def test_disaggregated_decode_gpu(gpu_server):
    """Prefill→store→decode demo over the local IPC + HIP gather path;
    decode logits rebuilt from cached pages must match the monolithic
    forward (infinistore_amd/example/disaggregated.py)."""
    from infinistore_amd.example.disaggregated import main as disagg_main

    disagg_main(port=gpu_server, device="cuda:0")
    disagg_main(port=gpu_server, device="cuda:0", quant="fp8")


def test_fp8_quantized_pages(gpu_server):
    """fp8 e4m3 ingest compression: pages stored at half size with a per-page
    scale; reads dequantize to bf16. Numerics vs torch.float8_e4m3fn
    roundtrip with the same scaling; capacity vs plain storage."""
    conn = local_conn(gpu_server)
    try:
        page_elems = 65536  # 128 KB bf16 -> 64 KB stored
        n = 16
        torch.manual_seed(3)
        src = (torch.randn(n * page_elems, device="cuda:0") * 3).to(torch.bfloat16)
        dst = torch.zeros_like(src)
        offs = [i * page_elems for i in range(n)]
        keys = [f"fp8-{uuid.uuid4()}-{i}" for i in range(n)]

        stats0 = json.loads(conn.get_server_stats_remote())
        conn.write_pages(src, keys, offs, page_elems, sync=True, quant="fp8")
        stats1 = json.loads(conn.get_server_stats_remote())
        conn.read_pages(dst, keys, offs, page_elems)
        conn.sync()

        # Half the blocks of a plain write (64 KB granule on this server).
        pkeys = [f"plain-{k}" for k in keys]
        conn.write_pages(src, pkeys, offs, page_elems, sync=True)
        stats2 = json.loads(conn.get_server_stats_remote())
        q_blocks = stats1["used_blocks"] - stats0["used_blocks"]
        p_blocks = stats2["used_blocks"] - stats1["used_blocks"]
        assert q_blocks * 2 == p_blocks, (q_blocks, p_blocks)

        # bit-exact against the shared codec reference (tests/_kernel_refs.py)
        ref_codes, ref_scales = fp8_quant_ref(src.cpu().reshape(n, page_elems))
        assert_bf16_bits_equal(bf16_bits(dst),
                               bf16_bits(fp8_dequant_ref(ref_codes, ref_scales)))
        for i in range(n):
            page = src[offs[i] : offs[i] + page_elems].float()
            got = dst[offs[i] : offs[i] + page_elems].float()
            # end-to-end error vs the original bf16 page: fp8 mantissa step
            rel = (got - page).abs().max().item() / page.abs().max().item()
            assert rel <= 0.07, (i, rel)

        # fabric reads of compressed entries are refused, not corrupted
        rdma = make_client(gpu_server)
        host = torch.zeros(page_elems, dtype=torch.bfloat16)
        rdma.register_mr(host)
        import pytest as _pytest
        with _pytest.raises(Exception):
            rdma.read_cache(host, [(keys[0], 0)], page_elems)
        rdma.close()
    finally:
        conn.close()


def test_snapshot_restore_hbm(tmp_path):
    """Snapshot/restore of HBM-resident pages (D2H stream out, H2D back),
    including fp8-compressed entries whose scales must survive — run in a
    subprocess that hosts the server in-process so the python snapshot API
    is reachable."""
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
n, pe = 8, 65536
src = torch.randn(n*pe, dtype=torch.bfloat16, device="cuda:0")
dst = torch.zeros_like(src)
offs = [i*pe for i in range(n)]
keys = [f"s-{{i}}" for i in range(n)]
qkeys = [f"q-{{i}}" for i in range(n)]
c.write_pages(src, keys, offs, pe, sync=True)
c.write_pages(src, qkeys, offs, pe, sync=True, quant="fp8")
snap = {str(tmp_path / 'hbm.snap')!r}
sn, sb = ifs.snapshot_pool(snap)
assert sn == 2*n, sn
ifs.purge_kv_map()
rn, rb = ifs.restore_pool(snap)
assert rn == 2*n, rn
c.read_pages(dst, keys, offs, pe); c.sync()
assert torch.equal(src, dst)
dst.zero_()
c.read_pages(dst, qkeys, offs, pe); c.sync()
err = (dst.float()-src.float()).abs().max() / src.abs().max()
assert err < 0.08, err.item()
c.close(); ifs.unregister_server()
print("SNAP OK")
"""],
        cwd=REPO, env={**os.environ, "PYTHONPATH": REPO + ":" + os.path.join(REPO, "tests")},
        timeout=180,
    ).returncode
    assert code == 0


def test_fast_op_pool_many_conns(gpu_server):
    """>=8 ring connections engage the server's fast-op worker pool
    (requests fan across threads instead of per-conn serial handling).
    Concurrent writers+readers on 10 connections must stay correct."""
    import threading

    conns = [local_conn(gpu_server) for _ in range(10)]
    try:
        import numpy as np

        page_elems = 32768  # 64 KB of bf16
        nb = 64
        offs = np.arange(nb, dtype=np.uint64) * page_elems
        srcs = [torch.randn(nb * page_elems, dtype=torch.bfloat16, device="cuda:0")
                for _ in range(10)]
        dsts = [torch.zeros_like(srcs[0]) for _ in range(10)]
        run = uuid.uuid4().hex[:8]
        errs = []

        def worker(i):
            try:
                c = conns[i]
                for it in range(6):
                    keys = [f"pool-{run}-c{i}-it{it}-{j}" for j in range(nb)]
                    c.write_pages(srcs[i], keys, offs, page_elems, sync=True)
                    c.read_pages(dsts[i], keys, offs, page_elems)
                    c.sync()
                    assert torch.equal(srcs[i], dsts[i]), (i, it)
                    c.delete_keys(keys)
            except Exception as e:  # surfaced after join
                errs.append(f"conn {i}: {e}")

        ts = [threading.Thread(target=worker, args=(i,)) for i in range(10)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=120)
        assert not errs, errs
    finally:
        for c in conns:
            c.close()


def test_big_allocation_refused_cleanly(gpu_server):
    """Allocations >= 2 GiB cannot cross the IPC boundary on this driver
    stack (hipIpcOpenMemHandle hangs; scripts/ipc_size_probe.py). The
    server must refuse with an error — NOT hang a poller — and the
    connection must stay usable."""
    conn = local_conn(gpu_server)
    try:
        big = torch.zeros(1 << 30, dtype=torch.bfloat16, device="cuda:0")  # 2 GiB
        with pytest.raises(Exception):
            conn.local_gpu_write_cache(big, [(f"big-{uuid.uuid4()}", 0)], 32768)
            conn.sync()
        del big
        # the conn (and its poller) survived
        small = torch.randn(32768, dtype=torch.bfloat16, device="cuda:0")
        out = torch.zeros_like(small)
        key = f"big-after-{uuid.uuid4()}"
        conn.local_gpu_write_cache(small, [(key, 0)], 32768)
        conn.sync()
        conn.read_cache(out, [(key, 0)], 32768)
        conn.sync()
        assert torch.equal(small, out)
    finally:
        conn.close()


CLIENT_BURST = r"""
import sys, time, numpy as np, torch
sys.path.insert(0, sys.argv[3])
import infinistore_amd as ifs
port = int(sys.argv[1]); tag = sys.argv[2]
conns = []
for _ in range(9):  # >=8 ring peers engages the fast-op worker pool
    c = ifs.InfinityConnection(ifs.ClientConfig(
        host_addr="127.0.0.1", service_port=port,
        connection_type=ifs.TYPE_LOCAL_GPU))
    c.connect(); conns.append(c)
src = torch.randn(256 * 32768, dtype=torch.bfloat16, device="cuda:0")
offs = np.arange(256, dtype=np.uint64) * 32768
print("READY", flush=True)
i = 0
while True:  # async bursts forever; the parent kill -9s us mid-flight
    i += 1
    gen = i % 4  # bounded key space: keys outlive the client (it's a cache),
    for j, c in enumerate(conns):  # so an unbounded burst would fill the pool
        c.write_pages(src, [f"{tag}-{j}-{gen}-{k}" for k in range(256)], offs,
                      32768, sync=False)
"""


def test_client_killed_mid_burst(gpu_server):
    """kill -9 a client while its async write bursts are queued in the
    fast-op pool: the server must tear the conns down (poller joined, refs
    drained) and keep serving other clients."""
    import signal

    tag = uuid.uuid4().hex[:8]
    proc = subprocess.Popen(
        [sys.executable, "-c", CLIENT_BURST, str(gpu_server), tag, REPO],
        cwd=REPO, stdout=subprocess.PIPE, text=True)
    try:
        line = proc.stdout.readline()
        assert "READY" in line, line
        time.sleep(1.5)  # let bursts queue up
        proc.send_signal(signal.SIGKILL)
        proc.wait(timeout=15)
    finally:
        if proc.poll() is None:
            proc.kill()
    # the server survives and serves a fresh client correctly
    time.sleep(1.0)
    conn = local_conn(gpu_server)
    try:
        src = torch.randn(32768, dtype=torch.bfloat16, device="cuda:0")
        dst = torch.zeros_like(src)
        key = f"after-kill-{uuid.uuid4()}"
        conn.local_gpu_write_cache(src, [(key, 0)], 32768)
        conn.sync()
        conn.read_cache(dst, [(key, 0)], 32768)
        conn.sync()
        assert torch.equal(src, dst)
    finally:
        conn.close()


def test_ref_framed_flatbuffers_local_write(gpu_server):
    """The reference's local-op wire shape: a raw-socket 'W' with a
    flatbuffers LocalMetaRequest body (cuda IPC handle + [Block{key,
    byte-offset}]), answered 202, then 'S' sync (FINISH + remain) — and the
    page read back through the normal client. Covers the flatbuffers local
    path, which this repo's own client never uses (it speaks the packed
    extension ops)."""
    import socket as socklib
    import struct

    from infinistore_amd import _native as n

    src = torch.randn(32768, dtype=torch.float32, device="cuda:0")
    handle, base_off = n._dbg_ipc_export(src.data_ptr())
    key = f"fbw-{uuid.uuid4().hex[:8]}"
    body = n._dbg_build_local_meta(0, handle, 32768 * 4, [(key, 0)], base_off)

    s = socklib.create_connection(("127.0.0.1", gpu_server), timeout=30)
    try:
        s.sendall(struct.pack("<IcI", 0xDEADBEEF, b"W", len(body)) + body)
        code = struct.unpack("<i", s.recv(4))[0]
        assert code == 202, code  # TASK_ACCEPTED
        for _ in range(100):  # reference-framed sync until remain == 0
            s.sendall(struct.pack("<IcI", 0xDEADBEEF, b"S", 0))
            buf = b""
            while len(buf) < 8:
                buf += s.recv(8 - len(buf))
            code, remain = struct.unpack("<ii", buf)
            assert code == 200
            if remain == 0:
                break
            time.sleep(0.01)
        assert remain == 0
    finally:
        s.close()

    conn = local_conn(gpu_server)
    try:
        dst = torch.zeros_like(src)
        conn.read_cache(dst, [(key, 0)], 32768)
        conn.sync()
        assert torch.equal(src, dst)
    finally:
        conn.close()

    # and the reference-framed 'R': async accept + poll-sync, data pushed
    # into the raw client's tensor through its IPC handle
    dst2 = torch.zeros_like(src)
    h2, off2 = n._dbg_ipc_export(dst2.data_ptr())
    rbody = n._dbg_build_local_meta(0, h2, 32768 * 4, [(key, 0)], off2)
    s = socklib.create_connection(("127.0.0.1", gpu_server), timeout=30)
    try:
        s.sendall(struct.pack("<IcI", 0xDEADBEEF, b"R", len(rbody)) + rbody)
        code = struct.unpack("<i", s.recv(4))[0]
        assert code == 202, code
        for _ in range(100):
            s.sendall(struct.pack("<IcI", 0xDEADBEEF, b"S", 0))
            buf = b""
            while len(buf) < 8:
                buf += s.recv(8 - len(buf))
            code, remain = struct.unpack("<ii", buf)
            assert code == 200
            if remain == 0:
                break
            time.sleep(0.01)
        assert remain == 0
        assert torch.equal(src, dst2)
    finally:
        s.close()
