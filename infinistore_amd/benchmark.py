"""infinistore-amd benchmark harness.

Superset of the reference's harness (/root/reference/infinistore/benchmark.py:
same workload shape — `--size` MB written as uuid-keyed pages of `--block-size`
KB in `--steps` layer-batches, then read back, printing write/read MB/s) plus
the measurements BASELINE.md requires that the reference lacks: p50/p99
round-trip latency and a concurrent-client saturation mode.

Examples:
    python -m infinistore_amd.benchmark --server 127.0.0.1 --port 22345 \
        --size 1024 --block-size 128 --local-gpu
    python -m infinistore_amd.benchmark ... --clients 8   # saturation
"""

import argparse
import json
import statistics
import sys
import time
import uuid

import torch

from . import lib


def parse_args():
    p = argparse.ArgumentParser(description="infinistore-amd benchmark")
    p.add_argument("--server", default="127.0.0.1")
    p.add_argument("--port", type=int, default=22345)
    p.add_argument("--size", type=int, default=128, help="total MB per iteration")
    p.add_argument("--block-size", type=int, default=32, help="page size in KB")
    p.add_argument("--steps", type=int, default=32,
                   help="layer-batches per iteration (simulates per-layer writes)")
    p.add_argument("--iteration", type=int, default=3)
    p.add_argument("--local-gpu", action="store_true",
                   help="use the local IPC path (default: fabric path)")
    p.add_argument("--src-gpu", type=int, default=0)
    p.add_argument("--dst-gpu", type=int, default=0)
    p.add_argument("--latency-ops", type=int, default=0,
                   help="additionally measure N single-page round-trips")
    p.add_argument("--clients", type=int, default=1,
                   help="concurrent client processes (saturation mode)")
    p.add_argument("--shape", choices=["llama3-8b", "llama3-70b"],
                   help="preset: per-layer paged-KV shapes (16-token pages, "
                        "8 KV heads x 128 dim, bf16 -> 64 KB pages; 8B=32 "
                        "layers, 70B=80 layers); --steps becomes n_layers and "
                        "--size is derived from --seq-len x --batch")
    p.add_argument("--seq-len", type=int, default=8192)
    p.add_argument("--batch", type=int, default=1)
    p.add_argument("--quant", choices=["fp8", "mxfp4"], default=None,
                   help="store pages fp8- or mxfp4-compressed (local-GPU path, bf16)")
    p.add_argument("--segments", type=int, default=1,
                   help="segmented pages (local-GPU path): lay each client "
                        "tensor out [N, n_pages, page/N] and move every page "
                        "as N segments a plane apart; 1 = contiguous pages")
    p.add_argument("--fused-layers", action="store_true",
                   help="with --shape and --local-gpu: one separately allocated "
                        "tensor per layer, registered as a tensor set; every "
                        "block travels as ONE page under ONE key spanning all "
                        "layers (docs/design.md, \"tensor sets\") instead of one "
                        "key per (layer, block)")
    p.add_argument("--slice", default=None, metavar="H0:H1/H",
                   help="sliced reads (local-GPU path): view every page as "
                        "[--slice-rows, H, head] and read only heads H0..H1 of "
                        "each, into tightly packed sliced pages; the read rate "
                        "then counts DELIVERED bytes")
    p.add_argument("--slice-rows", type=int, default=32,
                   help="rows (2 x block tokens) of the page view for --slice")
    p.add_argument("--slice-baseline", action="store_true",
                   help="with --slice: what a reader does without sliced reads, "
                        "for comparison: read whole pages into a bounce buffer, "
                        "then slice-copy the heads into place with torch")
    p.add_argument("--verify", action="store_true")
    p.add_argument("--json", action="store_true", help="print a JSON summary")
    p.add_argument("--spawn-server", action="store_true",
                   help="start a local server subprocess for the benchmark")
    p.add_argument("--prealloc-size", type=int, default=8,
                   help="pool GB per shard for --spawn-server")
    return p.parse_args()


def slice_geometry(args):
    """(h0, h1, H, rows, head_elems) of --slice, or None. The page is viewed as
    [rows, H, head_elems]."""
    if not args.slice:
        return None
    try:
        heads, total = args.slice.split("/")
        h0, h1 = (int(v) for v in heads.split(":"))
        H = int(total)
    except ValueError:
        raise SystemExit("--slice is H0:H1/H, e.g. 0:4/8")
    es = 2 if args.quant else 4
    page_elems = (args.block_size << 10) // es
    rows = args.slice_rows
    if not 0 <= h0 < h1 <= H or rows < 1 or page_elems % (rows * H):
        raise SystemExit("--slice needs 0 <= H0 < H1 <= H and a page of "
                         "--slice-rows x H whole heads")
    return h0, h1, H, rows, page_elems // (rows * H)


def make_conn(args, local):
    cfg = lib.ClientConfig(
        host_addr=args.server,
        service_port=args.port,
        connection_type=lib.TYPE_LOCAL_GPU if local else lib.TYPE_RDMA,
        link_type="TCP",
    )
    conn = lib.InfinityConnection(cfg)
    conn.connect()
    return conn


def make_buffers(args, conn, local, device):
    """src/dst buffers per worker, reused across iterations (fresh tensors
    every iteration would re-export IPC handles and churn the allocator —
    at 64 clients that dominates the wall). Split into sub-tensors under
    ~1.25 GiB each: the local path cannot IPC-import allocations >= 2 GiB
    (hipIpcOpenMemHandle hangs under dmabuf IPC on this driver stack —
    scripts/ipc_size_probe.py), and engines hold per-layer pools anyway.
    Returns (srcs, dsts, blocks_per_sub)."""
    block_bytes = args.block_size << 10
    total_bytes = args.size << 20
    n_blocks = total_bytes // block_bytes
    per_step = max(1, n_blocks // args.steps)
    dt = torch.bfloat16 if args.quant else torch.float32
    es = 2 if args.quant else 4

    cap = (1 << 30) + (1 << 28)  # 1.25 GiB
    n_sub = max(1, -(-total_bytes // cap))
    blocks_per_sub = -(-n_blocks // n_sub)
    blocks_per_sub = -(-blocks_per_sub // per_step) * per_step  # step-aligned
    n_sub = -(-n_blocks // blocks_per_sub)

    dst_dev = f"cuda:{args.dst_gpu}" if local else device
    srcs, dsts = [], []
    for t in range(n_sub):
        nb = min(blocks_per_sub, n_blocks - t * blocks_per_sub)
        elems = nb * block_bytes // es
        srcs.append(torch.rand(elems, dtype=dt, device=device))
        dsts.append(torch.zeros(elems, dtype=dt, device=dst_dev))
        if not local:
            conn.register_mr(srcs[-1])
            conn.register_mr(dsts[-1])
    if local:
        # The store's kernels run in another process: the fill kernels above
        # must have finished before the first request reads the sources. A
        # contiguous first request only reads the start of a tensor, which
        # the fill reaches first; a segmented one also reads a plane further.
        torch.cuda.synchronize()
    return srcs, dsts, blocks_per_sub


# Requests and keys sent by the timed loops, over all iterations of a process.
COUNTS = {"requests": 0, "keys": 0, "seconds": 0.0}


def _count(n_keys):
    COUNTS["requests"] += 1
    COUNTS["keys"] += n_keys


def make_fused_buffers(args, conn, device):
    """--fused-layers: one src and one dst tensor per layer, each its own
    allocation of pages_per_layer pages, registered as two tensor sets.
    Returns (srcs, dsts, src_set, dst_set)."""
    n_layers = SHAPES[args.shape][0]
    block_bytes = args.block_size << 10
    dt = torch.bfloat16 if args.quant else torch.float32
    es = 2 if args.quant else 4
    pages = (args.size << 20) // block_bytes // n_layers
    elems = pages * block_bytes // es
    srcs = [torch.rand(elems, dtype=dt, device=device) for _ in range(n_layers)]
    dsts = [torch.zeros(elems, dtype=dt, device=f"cuda:{args.dst_gpu}") for _ in range(n_layers)]
    torch.cuda.synchronize()
    return srcs, dsts, conn.register_tensor_set(srcs), conn.register_tensor_set(dsts)


def run_once_fused(args, conn, device, bufs=None):
    """One iteration of --fused-layers: block b of ALL layers is one page of
    n_layers * page_elems elements under one key. Requests carry ~64 MB, as
    the per-layer read chunks do; writes are async until the final sync and
    reads ticketed, as in run_once."""
    import numpy as np

    n_layers = SHAPES[args.shape][0]
    block_bytes = args.block_size << 10
    es = 2 if args.quant else 4
    page_elems = block_bytes // es
    srcs, dsts, src_set, dst_set = (bufs if bufs is not None
                                    else make_fused_buffers(args, conn, device))
    pages = srcs[0].numel() // page_elems
    fused_elems = n_layers * page_elems
    total_bytes = pages * fused_elems * es
    run = uuid.uuid4().hex
    keys = [f"{run}-{i}" for i in range(pages)]
    offs = np.arange(pages, dtype=np.uint64) * np.uint64(page_elems)
    chunk = max(1, (64 << 20) // (fused_elems * es))

    t0 = time.perf_counter()
    for c0 in range(0, pages, chunk):
        c1 = min(c0 + chunk, pages)
        conn.write_pages(None, keys[c0:c1], offs[c0:c1], fused_elems, quant=args.quant,
                         tensor_set=src_set)
        _count(c1 - c0)
    conn.sync()
    w_time = time.perf_counter() - t0

    t0 = time.perf_counter()
    tickets = []
    for c0 in range(0, pages, chunk):
        c1 = min(c0 + chunk, pages)
        tickets.append(conn.read_pages_async(None, keys[c0:c1], offs[c0:c1], fused_elems,
                                             tensor_set=dst_set))
        _count(c1 - c0)
    for tk in tickets:
        conn.wait_read(tk)
    conn.sync()
    r_time = time.perf_counter() - t0
    COUNTS["seconds"] += w_time + r_time

    if args.verify:
        for a, b in zip(srcs, dsts):
            assert _close(a.cpu(), b.cpu(), args.quant), "verification failed (fused)"
    try:
        conn.delete_keys(keys)
    except Exception:
        pass
    return total_bytes / w_time / 1e6, total_bytes / r_time / 1e6


def run_once(args, conn, local, device, bufs=None):
    if getattr(args, "fused_layers", False):
        return run_once_fused(args, conn, device, bufs)
    block_bytes = args.block_size << 10
    total_bytes = args.size << 20
    n_blocks = total_bytes // block_bytes
    es = 2 if args.quant else 4
    page_elems = block_bytes // es

    srcs, dsts, blocks_per_sub = (bufs if bufs is not None
                                  else make_buffers(args, conn, local, device))

    run = uuid.uuid4().hex
    keys = [f"{run}-{i}" for i in range(n_blocks)]
    per_step = max(1, n_blocks // args.steps)

    nseg = args.segments
    seg_elems = page_elems // nseg

    # --slice: the reads deliver heads h0..h1 of every page, packed, into outs.
    sg = slice_geometry(args) if local else None
    read_bytes = total_bytes
    if sg:
        h0, h1, n_heads, rows, head = sg
        sliced_elems = rows * (h1 - h0) * head
        read_bytes = n_blocks * sliced_elems * es
        page_slice = lib.PageSlice(page_size=page_elems, offset=h0 * head,
                                   piece=(h1 - h0) * head, stride=n_heads * head,
                                   count=rows)
        outs = [torch.zeros(d.numel() // page_elems * sliced_elems, dtype=d.dtype,
                            device=d.device) for d in dsts]
        torch.cuda.synchronize()

    def sub_of(i):  # block index -> (tensor index, element offset within it)
        return i // blocks_per_sub, (i % blocks_per_sub) * seg_elems

    def geom(t):  # segment arguments for sub-tensor t: [N, n_pages, page/N]
        if nseg == 1:
            return {}
        return {"segments": nseg, "segment_stride": t.numel() // nseg}

    # ---- write (layer-by-layer batches, like prefill; each step's slice
    # lives in ONE sub-tensor by construction) ----
    t0 = time.perf_counter()
    for s0 in range(0, n_blocks, per_step):
        hi = min(s0 + per_step, n_blocks)
        t_idx, _ = sub_of(s0)
        pairs = [(keys[i], sub_of(i)[1]) for i in range(s0, hi)]
        if local:
            if args.quant or nseg > 1:
                conn.write_pages(srcs[t_idx], [p[0] for p in pairs],
                                 [p[1] for p in pairs], page_elems,
                                 quant=args.quant, **geom(srcs[t_idx]))
            else:
                conn.local_gpu_write_cache(srcs[t_idx], pairs, page_elems)
        else:
            blocks = conn.allocate_rdma([p[0] for p in pairs], block_bytes)
            conn.rdma_write_cache(srcs[t_idx], [p[1] for p in pairs],
                                  page_elems, blocks)
        _count(len(pairs))
    conn.sync()
    w_time = time.perf_counter() - t0

    # ---- read ----
    # Local path: ticketed async reads in ~64 MB chunks keep several
    # collect+kernel pipelines in flight per connection (one monolithic
    # request serializes its key-collect phase in front of everything).
    t0 = time.perf_counter()
    if local:
        import numpy as np

        chunk_blocks = max(1, min(blocks_per_sub, (64 << 20) // block_bytes))
        tickets = []
        for t_idx in range(len(dsts)):
            lo = t_idx * blocks_per_sub
            hi = min(lo + blocks_per_sub, n_blocks)
            for c0 in range(lo, hi, chunk_blocks):
                c1 = min(c0 + chunk_blocks, hi)
                ks = [keys[i] for i in range(c0, c1)]
                offs = np.asarray([sub_of(i)[1] for i in range(c0, c1)],
                                  dtype=np.uint64)
                _count(c1 - c0)
                if sg and not args.slice_baseline:
                    offs = offs // np.uint64(page_elems) * np.uint64(sliced_elems)
                    tickets.append(conn.read_pages_async(outs[t_idx], ks, offs,
                                                         sliced_elems,
                                                         page_slice=page_slice))
                    continue
                tickets.append(conn.read_pages_async(dsts[t_idx], ks, offs,
                                                     page_elems,
                                                     **geom(dsts[t_idx])))
        for tk in tickets:
            conn.wait_read(tk)
        if sg and args.slice_baseline:
            # the second pass a reader needs today: pick the heads out of the
            # bounce buffer (dsts) into place
            for d, o in zip(dsts, outs):
                o.view(-1, rows, (h1 - h0) * head).copy_(
                    d.view(-1, rows, n_heads, head)[:, :, h0:h1].reshape(
                        -1, rows, (h1 - h0) * head))
            torch.cuda.synchronize()
    else:
        for t_idx in range(len(dsts)):
            lo = t_idx * blocks_per_sub
            hi = min(lo + blocks_per_sub, n_blocks)
            conn.read_cache(dsts[t_idx],
                            [(keys[i], sub_of(i)[1]) for i in range(lo, hi)],
                            page_elems)
            _count(hi - lo)
    conn.sync()
    r_time = time.perf_counter() - t0
    COUNTS["seconds"] += w_time + r_time

    if args.verify and sg:
        for a, o in zip(srcs, outs):
            want = a.view(-1, rows, n_heads, head)[:, :, h0:h1].reshape(-1)
            assert _close(want.cpu(), o.cpu(), args.quant), "verification failed (slice)"
    elif args.verify:
        for a, b in zip(srcs, dsts):
            assert _close(a.cpu(), b.cpu(), args.quant), "verification failed"
        if nseg > 1:
            _verify_contiguous_read(args, conn, srcs[0], dsts[0].device, keys, page_elems)

    # Steady-state footprint: drop this iteration's keys (each iteration
    # writes a fresh key set; an engine similarly evicts finished
    # sequences). Runs after the timed windows but inside the wall clock.
    try:
        conn.delete_keys(keys)
    except Exception:
        pass

    return total_bytes / w_time / 1e6, read_bytes / r_time / 1e6


# Largest absolute error of a value in [0, 1) after a round trip through a
# codec: fp8 e4m3 with scale absmax/448 is at most half the top binade's step
# (16/448 < 2^-4 of the page's absmax); mxfp4 is at most the saturation gap
# of its top binade (2/8 of the group's power-of-two range).
_QUANT_TOL = {"fp8": 2.0 ** -4, "mxfp4": 0.25}


def _close(a, b, quant):
    """--verify's comparison: exact for plain pages, within the codec's
    error for compressed ones (the harness data is uniform in [0, 1)).
    Says where the first difference is."""
    if quant is None:
        bad = a != b
    else:
        bad = ~((a.float() - b.float()).abs() <= _QUANT_TOL[quant])
    n_bad = int(bad.sum())
    if n_bad:
        first = int(bad.reshape(-1).nonzero()[0])
        print(f"verify: {n_bad} of {a.numel()} elements differ, first at {first}: "
              f"{a.reshape(-1)[first].item()} vs {b.reshape(-1)[first].item()}",
              file=sys.stderr)
    return n_bad == 0


def _verify_contiguous_read(args, conn, src, device, keys, page_elems):
    """--verify for --segments N > 1, second half: so that a mistake common
    to the segmented write and the segmented read cannot hide, the first
    pages read CONTIGUOUSLY must equal the concatenation of their segments
    in the `[N, n_pages, page/N]` source."""
    nseg = args.segments
    n_sub = src.numel() // page_elems
    k = min(n_sub, 64)
    flat = torch.zeros(k * page_elems, dtype=src.dtype, device=device)
    torch.cuda.synchronize()  # the fill must not land after the store's copy
    conn.read_pages(flat, keys[:k], [i * page_elems for i in range(k)], page_elems)
    conn.sync()
    want = src.view(nseg, n_sub, page_elems // nseg)[:, :k].transpose(0, 1).reshape(-1)
    assert _close(want.cpu(), flat.cpu(), args.quant), \
        "verification failed (contiguous read of segmented pages)"


def run_latency(args, conn, local, device):
    block_bytes = args.block_size << 10
    page_elems = block_bytes // 4
    src = torch.rand(page_elems, dtype=torch.float32, device=device)
    dst = torch.zeros_like(src)
    if not local:
        conn.register_mr(src)
        conn.register_mr(dst)
    put_us, get_us = [], []
    run = uuid.uuid4().hex
    for i in range(args.latency_ops):
        key = f"lat-{run}-{i}"
        t0 = time.perf_counter()
        if local:
            conn.local_gpu_write_cache(src, [(key, 0)], page_elems)
        else:
            blocks = conn.allocate_rdma([key], block_bytes)
            conn.rdma_write_cache(src, [0], page_elems, blocks)
        conn.sync()
        t1 = time.perf_counter()
        conn.read_cache(dst, [(key, 0)], page_elems)
        conn.sync()
        t2 = time.perf_counter()
        put_us.append((t1 - t0) * 1e6)
        get_us.append((t2 - t1) * 1e6)
    return put_us, get_us


def pct(v, q):
    if not v:
        return 0.0
    return statistics.quantiles(v, n=100)[q - 1] if len(v) >= 10 else max(v)


def _worker(args_dict, q, barrier, wid):
    ns = argparse.Namespace(**args_dict)
    local = ns.local_gpu and torch.cuda.is_available()
    n_dev = torch.cuda.device_count() if torch.cuda.is_available() else 1
    device = f"cuda:{(ns.src_gpu + wid) % n_dev}" if local else "cpu"
    conn = None
    try:
        conn = make_conn(ns, local)
        bufs = (make_fused_buffers(ns, conn, device) if getattr(ns, "fused_layers", False)
                else make_buffers(ns, conn, local, device))
        run_once(ns, conn, local, device, bufs)  # warm: IPC opens, allocator
        barrier.wait(timeout=600)  # start all clients together (steady state)
        t0 = time.perf_counter()
        w = r = 0.0
        iters = max(1, ns.iteration)
        for _ in range(iters):
            w, r = run_once(ns, conn, local, device, bufs)
        wall = time.perf_counter() - t0
        q.put((w, r, wall, iters))
    except Exception as e:  # report instead of leaving the parent hanging
        q.put(("error", f"worker {wid}: {e}", 0.0, 0))
    finally:
        if conn is not None:
            conn.close()


def _spawn_server(args):
    import socket
    import subprocess
    import sys
    import time as _t

    proc = subprocess.Popen(
        [sys.executable, "-m", "infinistore_amd.server",
         "--service-port", str(args.port),
         "--manage-port", str(args.port + 1),
         "--prealloc-size", str(args.prealloc_size),
         "--minimal-allocate-size", str(args.block_size),
         "--no-manage"],
    )
    t0 = _t.time()
    while _t.time() - t0 < 60:
        try:
            socket.create_connection(("127.0.0.1", args.port), timeout=1).close()
            return proc
        except OSError:
            _t.sleep(0.3)
    raise RuntimeError("spawned server did not come up")


SHAPES = {
    # (n_layers, kv_page_bytes): 16-token pages, 8 KV heads, head_dim 128,
    # bf16, K+V -> 2*16*8*128*2 = 64 KiB per layer-page (Llama-3 GQA).
    "llama3-8b": (32, 64 << 10),
    "llama3-70b": (80, 64 << 10),
}


def apply_shape(args):
    n_layers, page_bytes = SHAPES[args.shape]
    pages_per_layer = (args.seq_len + 15) // 16 * args.batch
    args.block_size = page_bytes >> 10
    args.steps = n_layers  # one layer-batch of pages per step (prefill order)
    args.size = n_layers * pages_per_layer * page_bytes >> 20
    print(f"shape {args.shape}: {n_layers} layers x {pages_per_layer} pages "
          f"x {page_bytes >> 10} KB = {args.size} MB per iteration")


def main():
    args = parse_args()
    if args.shape:
        apply_shape(args)
    if args.segments != 1:
        es = 2 if args.quant else 4
        if not args.local_gpu:
            raise SystemExit("--segments needs --local-gpu")
        if args.segments < 1 or ((args.block_size << 10) // es) % args.segments:
            raise SystemExit("--segments must divide the page's element count")
    if args.fused_layers:
        if not args.shape or not args.local_gpu:
            raise SystemExit("--fused-layers needs --shape and --local-gpu")
        if args.segments != 1 or args.slice:
            raise SystemExit("--fused-layers moves whole contiguous per-layer parts: "
                             "no --segments, no --slice")
    if args.slice:
        if not args.local_gpu or args.segments != 1:
            raise SystemExit("--slice needs --local-gpu and --segments 1")
        slice_geometry(args)  # refuses a malformed option before anything starts
    if args.spawn_server and args.clients > 1:
        # Keys live until each iteration's trailing delete; size the pool
        # for all clients' live iterations plus slack, capped so the pool +
        # the clients' own src/dst tensors (2x size each) still fit in HBM.
        need = args.clients * args.size * 2 * 1.3 / 1024 + 1
        if torch.cuda.is_available() and args.local_gpu:
            total_gb = torch.cuda.get_device_properties(0).total_memory / (1 << 30)
            client_gb = args.clients * args.size * 2 / 1024
            need = min(need, max(4, total_gb * 0.92 - client_gb))
        args.prealloc_size = max(args.prealloc_size, int(need))
    server_proc = _spawn_server(args) if args.spawn_server else None
    local = args.local_gpu and torch.cuda.is_available()
    device = f"cuda:{args.src_gpu}" if local else "cpu"

    if args.clients > 1:
        import multiprocessing

        ctx = multiprocessing.get_context("spawn")
        q = ctx.Queue()
        barrier = ctx.Barrier(args.clients)
        procs = [
            ctx.Process(target=_worker, args=(vars(args), q, barrier, wid))
            for wid in range(args.clients)
        ]
        for p in procs:
            p.start()
        results = [q.get(timeout=600) for _ in procs]
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
        errors = [r for r in results if r[0] == "error"]
        if errors:
            for e in errors:
                print(e[1], file=sys.stderr)
            if server_proc:
                server_proc.terminate()
            raise SystemExit(1)
        wall = max(r[2] for r in results)  # steady-state window (post-barrier)
        iters = results[0][3]
        agg = args.clients * (args.size << 20) * 2 * iters / wall / 1e6
        print(f"saturation: {args.clients} clients, aggregate {agg:.2f} MB/s "
              f"(per-client write {statistics.mean(r[0] for r in results):.2f} MB/s, "
              f"read {statistics.mean(r[1] for r in results):.2f} MB/s)")
        # Server-side truth (the client-side walls include Python/CPU
        # contention in the worker processes):
        try:
            probe = make_conn(args, False)
            stats = json.loads(probe.conn.get_stats())
            print(f"server counters: bytes_in={stats['bytes_in']/1e9:.1f} GB "
                  f"bytes_out={stats['bytes_out']/1e9:.1f} GB op_us={stats.get('op_us')}")
            probe.close()
        except Exception:
            pass
        if server_proc is not None:
            server_proc.terminate()
            server_proc.wait(timeout=20)
        return

    conn = make_conn(args, local)
    try:
        writes, reads = [], []
        # one set of tensors (and one registration) for all iterations, as an
        # engine holds its layer tensors
        bufs = make_fused_buffers(args, conn, device) if args.fused_layers else None
        for it in range(args.iteration):
            w, r = run_once(args, conn, local, device, bufs)
            writes.append(w)
            reads.append(r)
            print(f"[iter {it}] write cache: {w:.2f} MB/s, read cache: {r:.2f} MB/s")
        rps = COUNTS["requests"] / COUNTS["seconds"] if COUNTS["seconds"] else 0.0
        print(f"requests: {COUNTS['requests']} carrying {COUNTS['keys']} keys in "
              f"{COUNTS['seconds']:.3f} s of timed windows: {rps:.0f} requests/s")
        summary = {
            "write_MBps": round(statistics.mean(writes), 2),
            "read_MBps": round(statistics.mean(reads), 2),
            "requests": COUNTS["requests"],
            "keys": COUNTS["keys"],
            "requests_per_s": round(rps, 1),
            "block_kb": args.block_size,
            "size_mb": args.size,
            "path": "local_gpu" if local else "fabric",
        }
        if args.latency_ops:
            put_us, get_us = run_latency(args, conn, local, device)
            summary.update(
                p50_put_us=round(pct(put_us, 50), 1),
                p99_put_us=round(pct(put_us, 99), 1),
                p50_get_us=round(pct(get_us, 50), 1),
                p99_get_us=round(pct(get_us, 99), 1),
            )
            print(f"latency: put p50 {summary['p50_put_us']} us "
                  f"p99 {summary['p99_put_us']} us; get p50 {summary['p50_get_us']} us "
                  f"p99 {summary['p99_get_us']} us")
        if args.json:
            print(json.dumps(summary))
    finally:
        conn.close()
        if server_proc is not None:
            server_proc.terminate()
            server_proc.wait(timeout=20)


if __name__ == "__main__":
    main()
