#!/usr/bin/env python3
"""infinistore-amd flagship benchmark — the BASELINE.json headline metric:
put/get throughput (GB/s, aggregate over all server GPUs) and round-trip
latency on 128 KB KV-cache blocks.

One *step* = write `--blocks` 128 KB blocks from a GPU tensor into the store
(via the local IPC path + batched HIP gather kernel) + sync, then read them
all back + sync. `value` is the whole-job aggregate GB/s of payload moved
(put + get) across all N GPUs.

Launch (driver contract):
    python bench.py --gpus N --steps K --warmup W
A plain run sets up, warms up, times the K steps and prints the result line.
`--full` additionally measures the sequential commit-to-commit put/get rates
and the single-block p50/p99 latency (null in a plain run's `config`);
`--dump-outputs DIR` writes what the last timed step read back.
For N>1 the driver uses torch.distributed.run with one rank per GPU; rank r
runs a client on GPU r, rank 0 additionally hosts the in-process server
sharded over all N GPUs (weak scaling: per-GPU work is fixed).
"""

import argparse
import json
import os
import statistics
import sys
import time
import uuid

import torch


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10,
                   help="timed steps. Every step stores fresh keys; when all "
                        "of them fit in the pool nothing is freed inside the "
                        "timed region, otherwise each worker deletes its "
                        "oldest step's keys while the next copies run (see "
                        "--pool-cap-gb)")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--block-kb", type=int, default=128)
    p.add_argument("--blocks", type=int, default=2048,
                   help="blocks per rank per step (2048 x 128KB = 256 MB)")
    p.add_argument("--pool-gb", type=int, default=8, help="pool GB per shard")
    p.add_argument("--pool-cap-gb", type=int, default=0,
                   help="upper bound for the pool GB per shard (GPU mode; "
                        "default: the GPU's free memory less room for the "
                        "client buffers). A run whose keys would not fit "
                        "below it keeps only the newest steps in the store")
    p.add_argument("--port", type=int, default=0)
    p.add_argument("--server-addr", default="127.0.0.1",
                   help="connect to an external server instead of hosting one "
                        "(multi-node runs; the remote server must be started "
                        "separately)")
    p.add_argument("--cpu", action="store_true",
                   help="CPU-only mode (TCP fabric, DRAM pool) for dev boxes")
    p.add_argument("--latency-ops", type=int, default=200,
                   help="single-block round-trips for the p50/p99 measurement")
    p.add_argument("--cross", action="store_true",
                   help="each rank reads keys written by the next rank "
                        "(forces xGMI cross-shard traffic)")
    p.add_argument("--no-pipeline", action="store_true",
                   help="disable put/get step pipelining (sequential loop)")
    p.add_argument("--quant", choices=["fp8"], default=None,
                   help="store pages fp8-compressed (half HBM per page); "
                        "reads dequantize to bf16 — verification switches "
                        "to an fp8-tolerance comparison")
    p.add_argument("--conns", type=int, default=3,
                   help="LEGACY threaded mode only (--procs 0): write/read "
                        "connection pairs per rank, each a two-deep "
                        "pipelined loop in its own thread (GIL-bound at "
                        "~1.4 TB/s; the default process mode replaces it)")
    p.add_argument("--procs", type=int, default=4,
                   help="client worker PROCESSES per rank (local path): each "
                        "runs a pipelined conn pair over 1/procs of the "
                        "blocks. Python threads serialize the per-step "
                        "request packing on the GIL (~1.4 TB/s ceiling); "
                        "separate processes reach the server's real "
                        "capacity. 0 = legacy threaded mode (--conns).")
    p.add_argument("--full", action="store_true",
                   help="after the timed steps also run the secondary "
                        "measurements (sequential commit-to-commit put/get "
                        "rates, single-block p50/p99 latency); a plain run "
                        "reports them as null")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write what the last timed step read back from the "
                        "store as DIR/<name>.npy (float32; a fixed seeded "
                        "sample when the payload exceeds the size budget)")
    return p.parse_args()


# --dump-outputs budget for the whole job (all ranks and workers together):
# well under 64 MB, so a dump stays cheap to write, keep and compare.
DUMP_BUDGET_BYTES = 32 << 20


def _dump_sample_index(blocks, elems_per_block, budget_elems, seed):
    """Element indices of a buffer of `blocks` pages to dump, or None for all
    of it. Stratified so every page is represented: the same seeded set of
    within-page positions (always including element 0, which carries the
    per-step salt) is taken from each page. Depends only on its arguments,
    so two runs with the same command line sample the same elements."""
    import numpy as np

    if blocks * elems_per_block <= budget_elems:
        return None
    rng = np.random.default_rng(seed)
    per_block = budget_elems // blocks
    if per_block == 0:  # more pages than budget: a seeded subset of pages
        pages = np.sort(rng.choice(blocks, size=max(budget_elems, 1),
                                   replace=False))
        per_block = 1
    else:
        pages = np.arange(blocks)
    within = rng.choice(elems_per_block, size=per_block, replace=False)
    if 0 not in within:
        within[0] = 0
    within.sort()
    return (pages[:, None].astype(np.int64) * elems_per_block
            + within[None, :].astype(np.int64)).ravel()


def dump_read_buffer(dump_dir, name, buf, blocks, elems_per_block, n_parts,
                     seed):
    """Write `buf` (the destination of the last timed read) to
    dump_dir/name.npy as float32, sampled to this part's share of the job's
    dump budget."""
    import numpy as np

    budget_elems = DUMP_BUDGET_BYTES // 4 // max(n_parts, 1)
    idx = _dump_sample_index(blocks, elems_per_block, budget_elems, seed)
    if idx is not None:
        buf = buf[torch.from_numpy(idx).to(buf.device)]
    os.makedirs(dump_dir, exist_ok=True)
    np.save(os.path.join(dump_dir, name + ".npy"),
            buf.float().cpu().numpy())


def _proc_worker(cfg, barrier, q):
    """One pipelined write/read conn pair over a slice of the step payload,
    in its own process (own GIL). Protocol: warmup -> barrier A -> K timed
    steps -> barrier B -> verify -> report."""
    try:
        import numpy as np
        import torch

        import infinistore_amd as ifs

        torch.cuda.set_device(cfg["local_rank"])
        dev = f"cuda:{cfg['local_rank']}"
        blocks = cfg["blocks"]
        elems_per_block = cfg["elems_per_block"]
        K = cfg["steps"]
        n_salt = 4
        torch.manual_seed(9000 + cfg["wid"])
        base = torch.randn(blocks * elems_per_block, dtype=torch.bfloat16,
                           device=dev)
        srcs = [base.clone() for _ in range(n_salt)]
        for b in range(n_salt):
            srcs[b][0::elems_per_block] = float(b + 1)
        del base
        dsts = [torch.zeros_like(srcs[0]) for _ in range(2)]
        offs = np.arange(blocks, dtype=np.uint64) * elems_per_block

        ccfg = ifs.ClientConfig(host_addr="127.0.0.1",
                                service_port=cfg["port"],
                                connection_type=ifs.TYPE_LOCAL_GPU)
        wc = ifs.InfinityConnection(ccfg)
        wc.connect()
        rc = ifs.InfinityConnection(ccfg)
        rc.connect()

        pk = ifs.InfinityConnection.pack_keys
        tag = f"r{cfg['rank']}w{cfg['wid']}-{cfg['run_id']}"

        def keys(s):
            return [f"{tag}-s{s}-{i}" for i in range(blocks)]

        quant = cfg["quant"]
        # warmup: every salt/dst buffer + the write/read machinery
        for w in range(max(cfg["warmup"], 1)):
            wk = pk([f"warm-{k}" for k in keys(w)])
            wc.write_pages(srcs[w % n_salt], wk, offs, elems_per_block,
                           sync=True, quant=quant)
            rc.read_pages(dsts[w % 2], wk, offs, elems_per_block)
            rc.sync()
        for b in range(n_salt):
            wk1 = pk([f"warmbuf-{tag}-{b}"])
            wc.write_pages(srcs[b], wk1, offs[:1], elems_per_block, sync=True,
                           quant=quant)
            for d in range(2):
                rc.read_pages(dsts[d], wk1, offs[:1], elems_per_block)
                rc.sync()
        blobs = [pk(keys(s)) for s in range(K)]
        # Bounded store (the run's keys do not all fit in the pool): only
        # the newest `ring` steps stay resident. The keys of step s+3-ring
        # are deleted over a third connection right after W(s+2) and R(s+1)
        # have been queued, so the delete overlaps their copies and its
        # blocks are free again before W(s+3) allocates. The step was read
        # back long before (ring >= 4 > pipeline depth).
        ring = cfg["ring"] if 0 < cfg["ring"] < K else 0
        dc, del_keys = None, {}
        if ring:
            dc = ifs.InfinityConnection(ccfg)
            dc.connect()
            del_keys = {j: keys(j) for j in range(K - ring)}
        torch.cuda.synchronize()

        barrier.wait(timeout=600)  # ready: all workers warmed up
        barrier.wait(timeout=600)  # start: parent aligned ranks, clock runs
        # two-deep pipelined loop (same schedule as the threaded run_conn)
        wc.write_pages(srcs[0], blobs[0], offs, elems_per_block, sync=True,
                       quant=quant)
        if K > 1:
            wc.write_pages(srcs[1 % n_salt], blobs[1], offs, elems_per_block,
                           sync=False, quant=quant)
            wc.sync()
        tk = rc.read_pages_async(dsts[0], blobs[0], offs, elems_per_block)
        for s in range(K):
            if s + 2 < K:
                wc.write_pages(srcs[(s + 2) % n_salt], blobs[s + 2], offs,
                               elems_per_block, sync=False, quant=quant)
            tk_next = (rc.read_pages_async(dsts[(s + 1) % 2], blobs[s + 1],
                                           offs, elems_per_block)
                       if s + 1 < K else None)
            if ring and ring <= s + 3 < K:
                dc.delete_keys(del_keys.pop(s + 3 - ring))
            rc.wait_read(tk)
            wc.sync()
            tk = tk_next
        torch.cuda.synchronize()
        barrier.wait(timeout=600)  # end: timed region closes

        ok = True
        for s in (K - 1, K - 2) if K > 1 else (K - 1,):
            sb, db = srcs[s % n_salt], dsts[s % 2]
            if quant:
                ok = ok and torch.allclose(sb.float().cpu(), db.float().cpu(),
                                           atol=float(sb.abs().max()) * 0.07)
            else:
                ok = ok and torch.equal(sb.cpu(), db.cpu())
        if cfg["dump_dir"]:
            dump_read_buffer(cfg["dump_dir"],
                             f"get_r{cfg['rank']}w{cfg['wid']}",
                             dsts[(K - 1) % 2], blocks, elems_per_block,
                             cfg["n_parts"], seed=cfg["wid"])
        wc.close()
        rc.close()
        if dc is not None:
            dc.close()
        q.put((cfg["wid"], ok, ""))
    except Exception as e:  # pragma: no cover - surfaced via parent assert
        try:
            barrier.abort()
        except Exception:
            pass
        q.put((cfg["wid"], False, f"{type(e).__name__}: {e}"))


def run_procs_mode(args, rank, world, local_rank, dist, port, block_bytes,
                   elems_per_block, ring=0):
    """Local-path timed loop with worker PROCESSES instead of threads (each
    conn pair owns a GIL). The parent aligns ranks, brackets the timed
    region with barriers, then runs the latency phase and the sequential
    per-direction phase itself."""
    import multiprocessing

    import infinistore_amd as ifs

    torch.cuda.set_device(local_rank)
    run_id = uuid.uuid4().hex[:8]
    if dist:
        obj = [run_id]
        dist.broadcast_object_list(obj, src=0)
        run_id = obj[0]

    P = max(1, min(args.procs, args.blocks))
    base, rem = divmod(args.blocks, P)
    worker_blocks = [base + (1 if w < rem else 0) for w in range(P)]
    ctx = multiprocessing.get_context("spawn")
    barrier = ctx.Barrier(P + 1)
    q = ctx.Queue()
    workers = []
    for w in range(P):
        cfg = dict(rank=rank, wid=w, local_rank=local_rank, port=port,
                   blocks=worker_blocks[w], elems_per_block=elems_per_block,
                   steps=args.steps, warmup=args.warmup, quant=args.quant,
                   run_id=run_id, dump_dir=args.dump_outputs,
                   n_parts=P * world, ring=ring)
        pr = ctx.Process(target=_proc_worker, args=(cfg, barrier, q))
        pr.start()
        workers.append(pr)

    def sync_all():
        torch.cuda.synchronize()
        if dist:
            dist.barrier()

    try:
        barrier.wait(timeout=900)  # ready
    except Exception:
        msgs = []
        while not q.empty():
            msgs.append(q.get_nowait())
        print(json.dumps({"error": f"worker failed during warmup: {msgs}"}))
        sys.exit(1)
    sync_all()
    t0 = time.perf_counter()
    barrier.wait(timeout=600)   # start
    barrier.wait(timeout=1800)  # end
    sync_all()
    elapsed = time.perf_counter() - t0

    results = [q.get(timeout=300) for _ in range(P)]
    for wid, ok, err in results:
        if not ok:
            print(json.dumps({"error": f"worker {wid} failed: {err}"}))
            sys.exit(1)
    for pr in workers:
        pr.join(timeout=60)
        if pr.is_alive():
            pr.terminate()

    if dist:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t[0])

    seq_steps, seq_put, seq_get, lat_put, lat_get = 0, 0.0, 0.0, [], []
    if args.full:
        seq_steps, seq_put, seq_get, lat_put, lat_get = _procs_full_phases(
            args, rank, local_rank, dist, port, elems_per_block, run_id)

    def pct(v, qq):
        if not v:
            return 0.0 if args.full else None
        return round(statistics.quantiles(v, n=100)[qq - 1]
                     if len(v) >= 10 else max(v), 1)

    bytes_per_step_rank = args.blocks * block_bytes
    gbps = 2.0 * bytes_per_step_rank * args.steps * world / 1e9 / elapsed
    put_gbps = (bytes_per_step_rank * seq_steps * world / 1e9 / seq_put
                if seq_put > 0 else None)
    get_gbps = (bytes_per_step_rank * seq_steps * world / 1e9 / seq_get
                if seq_get > 0 else None)
    if rank == 0:
        result = {
            "metric": "put_get_GBps",
            "value": round(gbps, 3),
            "unit": "GB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1000, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16+fp8kv" if args.quant else "bf16",
            "data": "synthetic",
            "config": {
                "model": "kvcache-store",
                "block_kb": args.block_kb,
                "blocks_per_rank_per_step": args.blocks,
                "global_batch": args.blocks * world,
                "seq_len": 0,
                "parallelism": f"shard{world}",
                "path": "local_gpu_ipc",
                "client_procs": P,
                # steps kept resident in the store (null: all of them)
                "resident_steps": ring if 0 < ring < args.steps else None,
                # the fields below are measured only with --full
                "put_GBps": round(put_gbps, 3) if put_gbps else None,
                "get_GBps": round(get_gbps, 3) if get_gbps else None,
                "p50_put_us": pct(lat_put, 50),
                "p99_put_us": pct(lat_put, 99),
                "p50_get_us": pct(lat_get, 50),
                "p99_get_us": pct(lat_get, 99),
            },
        }
        print(json.dumps(result))
    if dist:
        dist.barrier()
    if rank == 0 and not (args.server_addr != "127.0.0.1"):
        print("server stats:", ifs.get_server_stats(), file=sys.stderr)
        ifs.unregister_server()
    if dist:
        dist.destroy_process_group()


def _procs_full_phases(args, rank, local_rank, dist, port, elems_per_block,
                       run_id):
    """--full only: the parent-side secondary measurements of the process
    mode, run after the timed region (sequential per-direction rates, then
    single-block latency). Returns (seq_steps, seq_put_s, seq_get_s,
    lat_put_us, lat_get_us)."""
    import numpy as np

    import infinistore_amd as ifs

    ccfg = ifs.ClientConfig(host_addr="127.0.0.1", service_port=port,
                            connection_type=ifs.TYPE_LOCAL_GPU)
    conn = ifs.InfinityConnection(ccfg)
    conn.connect()
    if rank == 0:
        ifs.purge_kv_map()
    if dist:
        dist.barrier()

    # sequential commit-to-commit per-direction rates (full-size payload;
    # worker memory has been released by now)
    seq_steps = min(args.steps, 4)
    src = torch.randn(args.blocks * elems_per_block, dtype=torch.bfloat16,
                      device=f"cuda:{local_rank}")
    dst = torch.zeros_like(src)
    offs = np.arange(args.blocks, dtype=np.uint64) * elems_per_block
    conn.write_pages(src, [f"seqwarm-{run_id}"], offs[:1], elems_per_block,
                     sync=True, quant=args.quant)
    conn.read_pages(dst, [f"seqwarm-{run_id}"], offs[:1], elems_per_block)
    conn.sync()
    seq_put = seq_get = 0.0
    for s in range(seq_steps):
        ks = [f"seq-r{rank}-{run_id}-s{s}-{i}" for i in range(args.blocks)]
        t1 = time.perf_counter()
        conn.write_pages(src, ks, offs, elems_per_block, sync=True,
                         quant=args.quant)
        t2 = time.perf_counter()
        conn.read_pages(dst, ks, offs, elems_per_block)
        conn.sync()
        seq_put += t2 - t1
        seq_get += time.perf_counter() - t2
    if args.quant:
        ok = torch.allclose(src.float().cpu(), dst.float().cpu(),
                            atol=float(src.abs().max()) * 0.07)
    else:
        ok = torch.equal(src.cpu(), dst.cpu())
    if not ok:
        print(json.dumps({"error": "data mismatch in sequential phase"}))
        sys.exit(1)
    if dist:
        t = torch.tensor([seq_put, seq_get], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        seq_put, seq_get = t.tolist()
    if rank == 0:
        ifs.purge_kv_map()
    if dist:
        dist.barrier()

    lat_put, lat_get = [], []
    for i in range(args.latency_ops):
        key = f"lat-r{rank}-{run_id}-{i}"
        t1 = time.perf_counter()
        conn.local_gpu_write_cache(src, [(key, 0)], elems_per_block)
        conn.sync()
        t2 = time.perf_counter()
        conn.read_cache(dst, [(key, 0)], elems_per_block)
        conn.sync()
        t3 = time.perf_counter()
        lat_put.append((t2 - t1) * 1e6)
        lat_get.append((t3 - t2) * 1e6)
    conn.close()
    if rank == 0:
        ifs.purge_kv_map()
    if dist:
        dist.barrier()

    return seq_steps, seq_put, seq_get, lat_put, lat_get


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    n_gpus = max(args.gpus, world)

    have_gpu = torch.cuda.is_available() and not args.cpu
    if have_gpu:
        local_rank = local_rank % torch.cuda.device_count()
    dist = None
    if world > 1:
        import torch.distributed as tdist

        dist = tdist
        dist.init_process_group(backend="gloo")  # host-side coordination only

    import infinistore_amd as ifs

    port = args.port or (23000 + (os.getpid() % 1000) if world == 1 else 23999)

    external = args.server_addr != "127.0.0.1"
    ring = 0  # steps kept resident when the keys outgrow the pool (0: all)
    # Rank 0 hosts the server, sharded over all visible GPUs.
    if rank == 0 and not external:
        n_shards = min(n_gpus, torch.cuda.device_count()) if have_gpu else 1
        # Keys accumulate across the timed steps (purged only between
        # phases): size each shard for the whole run, including rank
        # oversubscription (more ranks than GPUs on small test boxes).
        ranks_per_shard = max(1, (world + n_shards - 1) // n_shards)
        need_bytes = (args.steps + args.warmup) * args.blocks * args.block_kb * 1024
        need_gb = (need_bytes * ranks_per_shard * 5) // (4 << 30) + 1  # +25% slack
        pool_gb = max(args.pool_gb, int(need_gb))
        if have_gpu:
            # The pool cannot outgrow the GPU. Leave room for the clients on
            # the same device (4 source + 2 destination buffers per rank, 2
            # more with --full, and a HIP context per process), and when the
            # run's keys do not fit under the cap keep only the newest `ring`
            # steps resident, filling the pool to 90% (pages are all one
            # allocation unit, so there is no fragmentation to allow for).
            step_bytes = args.blocks * args.block_kb * 1024 * ranks_per_shard
            free_b = min(torch.cuda.mem_get_info(d)[0] for d in range(n_shards))
            cap_gb = int((free_b - 8 * step_bytes) >> 30) - 12
            if args.pool_cap_gb:
                cap_gb = min(cap_gb, args.pool_cap_gb)
            if pool_gb > cap_gb:
                pool_gb = max(cap_gb, 1)
                ring = (int((pool_gb << 30) * 0.9) // step_bytes
                        - max(args.warmup, 1) - 1)
                if ring >= args.steps:
                    ring = 0  # everything fits after all
                elif ring < 4:
                    print(json.dumps({"error": "pool of %d GB is too small "
                                      "for a step of %d MB" % (
                                          pool_gb, step_bytes >> 20)}))
                    sys.exit(1)
        scfg = ifs.ServerConfig(
            service_port=port,
            manage_port=port + 1,
            prealloc_size=pool_gb,
            minimal_allocate_size=args.block_kb,
            cpu_only=not have_gpu,
            devices=list(range(n_shards)) if have_gpu else [],
            io_threads=max(3, args.conns + 1),
        )
        ifs.register_server(scfg)
    if dist:
        obj = [ring]
        dist.broadcast_object_list(obj, src=0)
        ring = obj[0]

    block_bytes = args.block_kb * 1024
    elems_per_block = block_bytes // 2  # bf16
    total_elems = args.blocks * elems_per_block
    dev = f"cuda:{local_rank}" if have_gpu else "cpu"

    use_local_path_early = have_gpu and not external
    if (args.procs > 0 and use_local_path_early and not (args.cross and world > 1)
            and not args.no_pipeline and not os.environ.get("IFS_BENCH_DEBUG")):
        return run_procs_mode(args, rank, world, local_rank, dist, port,
                              block_bytes, elems_per_block, ring)
    if ring:
        print(json.dumps({"error": "--steps %d does not fit in the pool; only "
                          "the process mode (--procs > 0) can bound the "
                          "store" % args.steps}))
        sys.exit(1)

    if have_gpu:
        torch.cuda.set_device(local_rank)
    # Same seed on every rank: src contents are identical across ranks, so
    # cross-rank reads (--cross) can still be verified against local src.
    torch.manual_seed(12345)
    src = torch.randn(total_elems, dtype=torch.bfloat16, device=dev)
    # Anti-staleness salting: step s writes srcs[s % 4] whose every block
    # carries a distinct salt in its first element, and step s reads land in
    # dsts[s % 2] (adjacent in-flight reads must not share a destination).
    # Verification then detects a read that returned another step's blocks
    # for any staleness within 3 steps — deeper than the pipeline ever runs.
    # (Round 1 wrote identical payloads every step, so returning step s-1's
    # blocks verified clean.)
    n_salt = 4
    srcs = [src.clone() for _ in range(n_salt)]
    for b in range(n_salt):
        srcs[b][0::elems_per_block] = float(b + 1)
    src = srcs[0]
    dsts = [torch.zeros_like(src) for _ in range(2)]
    dst = dsts[0]

    use_local_path = have_gpu and not external
    ccfg = ifs.ClientConfig(
        host_addr=args.server_addr,
        service_port=port,
        connection_type=ifs.TYPE_LOCAL_GPU if use_local_path else ifs.TYPE_RDMA,
        link_type="TCP" if not external else "Ethernet",
    )
    conn = ifs.InfinityConnection(ccfg)
    conn.connect()
    if not use_local_path:
        for t in srcs:
            conn.register_mr(t)
        for t in dsts:
            conn.register_mr(t)

    # Extra connections for intra-rank parallelism (local path only): the
    # blocking waits release the GIL and the server spreads connections over
    # its IO worker loops / ring pollers and HIP streams, so two half-size
    # pipelined loops overlap each other's host-side request latency.
    # Each loop uses a write-conn + read-conn PAIR so the async write handler
    # is never queued in front of the blocking read on one connection — the
    # natural shape for disaggregated serving (prefill writes, decode reads).
    n_conns = args.conns if (use_local_path and not args.cross) else 1
    conns = [conn]   # read conns (conns[0] also serves the latency phase)
    wconns = []      # write conns (writes + syncs)
    for _ in range(n_conns - 1):
        c = ifs.InfinityConnection(ccfg)
        c.connect()
        conns.append(c)
    for _ in range(n_conns if use_local_path else 0):
        c = ifs.InfinityConnection(ccfg)
        c.connect()
        wconns.append(c)
    if not wconns:
        wconns = conns

    import numpy as np

    run_id = uuid.uuid4().hex[:8]
    if dist:  # one shared run id so ranks can name each other's keys
        obj = [run_id]
        dist.broadcast_object_list(obj, src=0)
        run_id = obj[0]
    offsets = [i * elems_per_block for i in range(args.blocks)]
    offsets_np = np.asarray(offsets, dtype=np.uint64)

    read_rank = (rank + 1) % world if (args.cross and world > 1) else rank

    def step_keys(step, owner=None):
        owner = rank if owner is None else owner
        return [f"r{owner}-s{step}-{run_id}-{i}" for i in range(args.blocks)]

    def do_put(keys, s=0):
        sb = srcs[s % n_salt]
        if use_local_path:
            conn.write_pages(sb, keys, offsets_np[: len(keys)], elems_per_block,
                             sync=True, quant=args.quant)
        else:
            blocks = conn.allocate_rdma(keys, block_bytes)
            conn.rdma_write_cache(sb, offsets[: len(keys)], elems_per_block,
                                  blocks)
            conn.sync()

    def do_get(keys, s=0):
        db = dsts[s % 2]
        if use_local_path:
            conn.read_pages(db, keys, offsets_np[: len(keys)], elems_per_block)
            conn.sync()
        else:
            conn.read_cache(db, list(zip(keys, offsets)), elems_per_block)
            conn.sync()

    def purge_all():
        if dist:
            dist.barrier()
        if rank == 0 and not external:
            ifs.purge_kv_map()
        if dist:
            dist.barrier()

    def sync_all():
        if have_gpu:
            torch.cuda.synchronize()
        if dist:
            dist.barrier()

    cross = args.cross and world > 1

    # Pre-generate the per-step key lists (an engine holds its page hash
    # chain already; Python f-string formatting is not part of the store).
    put_keys = [step_keys(s) for s in range(args.steps)]
    get_keys = [step_keys(s, read_rank) for s in range(args.steps)]

    # Per-connection block slices (contiguous ranges; the absolute element
    # offsets stay valid because both tensors are shared by all conns).
    bounds = [(c * args.blocks) // n_conns for c in range(n_conns + 1)]
    csl = [slice(bounds[c], bounds[c + 1]) for c in range(n_conns)]
    coff = [offsets_np[s] for s in csl]
    # Pre-serialized key blobs (an engine caches the serialized page-key
    # chain; joining 1-2k Python strings costs ~30 µs per request).
    pk = ifs.InfinityConnection.pack_keys
    put_blobs = [[pk(put_keys[s][csl[c]]) for c in range(n_conns)]
                 for s in range(args.steps)]
    get_blobs = [[pk(get_keys[s][csl[c]]) for c in range(n_conns)]
                 for s in range(args.steps)]

    # ---- correctness spot-check + warmup ----
    for w in range(args.warmup):
        if use_local_path and not cross:
            wk = [f"warm-{k}" for k in step_keys(w)]
            for c in range(n_conns):  # warm every conn's IPC export + slab
                wconns[c].write_pages(srcs[w % n_salt], wk[csl[c]], coff[c],
                                      elems_per_block, sync=True,
                                      quant=args.quant)
                conns[c].read_pages(dsts[w % 2], wk[csl[c]], coff[c],
                                    elems_per_block)
                conns[c].sync()
        else:
            do_put([f"warm-{k}" for k in step_keys(w)], w)
            if cross:
                dist.barrier()
            do_get([f"warm-{k}" for k in step_keys(w, read_rank)], w)

    def verify(tag, s):
        """dsts[s%2] must hold exactly step s's salted payload; a stale or
        cross-mixed read from any step within ±3 carries a different salt
        in the block's first element and fails the comparison."""
        sb, db = srcs[s % n_salt], dsts[s % 2]
        if args.quant:  # fp8 roundtrip: ~3 mantissa bits, per-page scale
            ok = torch.allclose(sb.float().cpu(), db.float().cpu(),
                                atol=float(sb.abs().max()) * 0.07)
        else:
            ok = torch.equal(sb.cpu(), db.cpu())
        if not ok:
            print(json.dumps({"error": f"data mismatch in {tag} (step {s})"}))
            sys.exit(1)

    if args.warmup:
        verify("warmup", args.warmup - 1)

    # Touch every salt/dst buffer once on every connection (1 block each):
    # the first use of a tensor exports + server-opens its IPC mapping
    # (~1 ms), which must not land inside the timed region when
    # warmup < n_salt. Overwrites dst block 0, so runs after the warmup
    # verification.
    o1 = offsets_np[:1]
    for b in range(n_salt):
        wk1 = [f"warmbuf-{run_id}-r{rank}-{b}"]
        for c in range(n_conns):
            if use_local_path:
                wconns[c].write_pages(srcs[b], wk1, o1, elems_per_block,
                                      sync=True, quant=args.quant)
                for d in range(2):
                    conns[c].read_pages(dsts[d], wk1, o1, elems_per_block)
                    conns[c].sync()
            else:
                do_put(wk1, b)
                for d in range(2):
                    do_get(wk1, d)
    purge_all()

    # ---- timed region ----
    debug_t = {"keygen": 0.0, "put_req": 0.0, "put_sync": 0.0, "get_req": 0.0,
               "get_sync": 0.0}
    debug = os.environ.get("IFS_BENCH_DEBUG")

    # Pipelined mode (default on the local path): the put of step s+1 is
    # issued as a plain async request (server responds before submitting the
    # copy) right before the blocking get of step s, so the put's gather
    # kernel + index insert run on their own HIP stream underneath the get's
    # scatter kernel; the trailing sync only drains whatever is left of the
    # put commit. Every step still moves the full put+get payload — only the
    # host-side request latency is hidden. Sequential when --cross (needs a
    # barrier between a step's put commit and the peer's get) or debugging.
    pipeline = use_local_path and not cross and not debug and not args.no_pipeline

    sync_all()
    t0 = time.perf_counter()
    put_time = 0.0
    get_time = 0.0
    if pipeline:
        def run_conn(c):
            # Two-deep pipeline per pair: writes lead two steps, reads one.
            # Invariant before pushing R(k): W(k) committed (wc_.sync() at
            # the end of iteration k-1 drains the W(k+1) pushed there, and
            # the prime below covers W(0)/W(1)). While the client waits on
            # R(s)'s ticket, W(s+2) and R(s+1) are already queued server-
            # side, so the GPU always has copy work in flight. W(s) writes
            # srcs[s%4] (distinct per-step salt) and R(s) lands in dsts[s%2]
            # so adjacent in-flight reads never share a destination.
            rc_, wc_, o = conns[c], wconns[c], coff[c]
            K = args.steps
            wc_.write_pages(srcs[0], put_blobs[0][c], o, elems_per_block,
                            sync=True, quant=args.quant)
            if K > 1:
                wc_.write_pages(srcs[1 % n_salt], put_blobs[1][c], o,
                                elems_per_block, sync=False, quant=args.quant)
                wc_.sync()
            tk = rc_.read_pages_async(dsts[0], get_blobs[0][c], o,
                                      elems_per_block)
            for s in range(K):
                if s + 2 < K:
                    wc_.write_pages(srcs[(s + 2) % n_salt], put_blobs[s + 2][c],
                                    o, elems_per_block, sync=False,
                                    quant=args.quant)
                tk_next = (rc_.read_pages_async(dsts[(s + 1) % 2],
                                                get_blobs[s + 1][c], o,
                                                elems_per_block)
                           if s + 1 < K else None)
                rc_.wait_read(tk)
                wc_.sync()  # commits W(s+2) before R(s+2) is pushed next iter
                tk = tk_next

        if n_conns == 1:
            run_conn(0)
        else:
            import concurrent.futures as cf

            with cf.ThreadPoolExecutor(n_conns) as ex:
                list(ex.map(run_conn, range(n_conns)))
    else:
        for s in range(args.steps):
            tp = time.perf_counter()
            if debug and use_local_path:
                conn.write_pages(srcs[s % n_salt], put_keys[s], offsets_np,
                                 elems_per_block, sync=True)
                tb = time.perf_counter()
                conn.sync()
                tc = time.perf_counter()
                debug_t["put_req"] += tb - tp
                debug_t["put_sync"] += tc - tb
            else:
                do_put(put_keys[s], s)
            put_time += time.perf_counter() - tp
            if cross:
                dist.barrier()  # readers wait for the writer of their keys
            tg = time.perf_counter()
            if debug and use_local_path:
                conn.read_pages(dsts[s % 2], get_keys[s], offsets_np,
                                elems_per_block)
                tb = time.perf_counter()
                conn.sync()
                debug_t["get_req"] += tb - tg
                debug_t["get_sync"] += time.perf_counter() - tb
            else:
                do_get(get_keys[s], s)
            get_time += time.perf_counter() - tg
    sync_all()
    elapsed = time.perf_counter() - t0
    # Verify the last TWO steps (they cover both dst buffers and two salt
    # values), pipelined or not.
    verify("timed loop", args.steps - 1)
    if args.steps > 1:
        verify("timed loop", args.steps - 2)
    if args.dump_outputs:
        dump_read_buffer(args.dump_outputs, f"get_r{rank}",
                         dsts[(args.steps - 1) % 2], args.blocks,
                         elems_per_block, world, seed=0)
    if debug:
        per = {k: round(v / args.steps * 1e6, 1) for k, v in debug_t.items()}
        print(f"rank {rank} per-step us: {per}", file=sys.stderr)

    # max over ranks; bytes summed over ranks
    if dist:
        t = torch.tensor([elapsed, put_time, get_time], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, put_time, get_time = t.tolist()

    purge_all()

    # ---- honest per-direction throughput (sequential, commit-to-commit) ----
    # The pipelined loop overlaps puts with gets, so splitting its wall time
    # into put/get components is not meaningful (round 1 reported host-issue
    # time of async writes as put_GBps — 2-3x the sustainable rate). Measure
    # put and get separately: each put timed to commit-ACK (sync), each get
    # to completion.
    seq_steps = min(args.steps, 4) if (pipeline and args.full) else 0
    seq_put = seq_get = 0.0
    for s in range(seq_steps):
        ks = [f"seq-{k}" for k in put_keys[s]]
        t1 = time.perf_counter()
        do_put(ks, s)
        t2 = time.perf_counter()
        do_get(ks, s)
        seq_put += t2 - t1
        seq_get += time.perf_counter() - t2
    if seq_steps:
        verify("sequential phase", seq_steps - 1)
        purge_all()
    if dist and seq_steps:
        t = torch.tensor([seq_put, seq_get], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        seq_put, seq_get = t.tolist()

    # ---- latency phase (single-block round trips; --full only) ----
    lat_put, lat_get = [], []
    latency_ops = args.latency_ops if args.full else 0
    lkeys = [f"lat-r{rank}-{run_id}-{i}" for i in range(latency_ops)]
    for i in range(latency_ops):
        t1 = time.perf_counter()
        if use_local_path:
            conn.local_gpu_write_cache(src, [(lkeys[i], 0)], elems_per_block)
            conn.sync()
        else:
            blk = conn.allocate_rdma([lkeys[i]], block_bytes)
            conn.rdma_write_cache(src, [0], elems_per_block, blk)
            conn.sync()
        t2 = time.perf_counter()
        conn.read_cache(dst, [(lkeys[i], 0)], elems_per_block)
        conn.sync()
        t3 = time.perf_counter()
        lat_put.append((t2 - t1) * 1e6)
        lat_get.append((t3 - t2) * 1e6)
    purge_all()

    def pct(v, q):
        if not v:
            return 0.0 if args.full else None
        return round(statistics.quantiles(v, n=100)[q - 1]
                     if len(v) >= 10 else max(v), 1)

    bytes_per_step_rank = args.blocks * block_bytes
    total_gb = 2.0 * bytes_per_step_rank * args.steps * world / 1e9  # put+get
    gbps = total_gb / elapsed
    # Per-direction rates come from sequential commit-to-commit timing only
    # (the pipelined loop's directions overlap and cannot be split honestly).
    if pipeline:
        put_gbps = (bytes_per_step_rank * seq_steps * world / 1e9 / seq_put
                    if seq_steps and seq_put > 0 else None)
        get_gbps = (bytes_per_step_rank * seq_steps * world / 1e9 / seq_get
                    if seq_steps and seq_get > 0 else None)
    else:
        put_gbps = (bytes_per_step_rank * args.steps * world / 1e9 / put_time
                    if put_time > 0 else None)
        get_gbps = (bytes_per_step_rank * args.steps * world / 1e9 / get_time
                    if get_time > 0 else None)

    if rank == 0:
        result = {
            "metric": "put_get_GBps",
            "value": round(gbps, 3),
            "unit": "GB/s",
            "n_gpus": world if have_gpu else 0,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1000, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16+fp8kv" if args.quant else "bf16",
            "data": "synthetic",
            "config": {
                "model": "kvcache-store",
                "block_kb": args.block_kb,
                "blocks_per_rank_per_step": args.blocks,
                "global_batch": args.blocks * world,
                "seq_len": 0,
                "parallelism": f"shard{world}",
                "path": "local_gpu_ipc" if use_local_path else ("fabric_remote" if external else "tcp_fabric_cpu"),
                # sequential commit-to-commit rates (sustained, unpipelined;
                # in the pipelined mode measured only with --full, like the
                # latency percentiles)
                "put_GBps": round(put_gbps, 3) if put_gbps else None,
                "get_GBps": round(get_gbps, 3) if get_gbps else None,
                "p50_put_us": pct(lat_put, 50),
                "p99_put_us": pct(lat_put, 99),
                "p50_get_us": pct(lat_get, 50),
                "p99_get_us": pct(lat_get, 99),
            },
        }
        print(json.dumps(result))

    for c in conns:
        c.close()
    for c in wconns:
        if c not in conns:
            c.close()
    if dist:
        dist.barrier()
    if rank == 0 and not external:
        print("server stats:", ifs.get_server_stats(), file=sys.stderr)
        ifs.unregister_server()
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
