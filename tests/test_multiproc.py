"""Multi-process (torch.distributed, gloo) coverage of the distributed
bench path — the same launch shape the scaling driver uses, on CPU:
rank 0 hosts the server, every rank runs a client, coordination over gloo.
"""

import json
import os
import subprocess
import sys

from conftest import free_port

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench_2rank(extra):
    env = os.environ.copy()
    env["MASTER_ADDR"] = "127.0.0.1"
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(free_port()), "bench.py", "--cpu", "--full",
         "--steps", "2", "--warmup", "1", "--blocks", "16",
         "--latency-ops", "3", "--port", str(free_port())] + extra,
        cwd=REPO, env=env, capture_output=True, text=True, timeout=300,
    )
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["metric"] == "put_get_GBps"
    assert out["steps"] == 2
    assert out["value"] > 0
    return out


def test_bench_two_ranks_gloo():
    _run_bench_2rank([])


def test_bench_two_ranks_gloo_cross():
    # --cross: each rank reads the other rank's keys (the xGMI cross-shard
    # pattern, exercised here over the CPU fabric).
    _run_bench_2rank(["--cross"])


def _run_bench_plain(dump_dir):
    r = subprocess.run(
        [sys.executable, "bench.py", "--cpu", "--gpus", "1", "--steps", "3",
         "--warmup", "1", "--blocks", "16", "--port", str(free_port()),
         "--dump-outputs", str(dump_dir)],
        cwd=REPO, capture_output=True, text=True, timeout=300,
    )
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def test_bench_plain_run_dumps_reproducible_outputs(tmp_path):
    """A plain run (no --full) reports the headline fields, leaves the
    latency percentiles unmeasured, and --dump-outputs writes the last timed
    step's read-back buffer as float32 — identical between two runs with
    the same arguments."""
    import numpy as np

    out = _run_bench_plain(tmp_path / "a")
    assert out["metric"] == "put_get_GBps" and out["unit"] == "GB/s"
    assert out["steps"] == 3 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["higher_is_better"] is True and out["dtype"] == "bf16"
    for k in ("p50_put_us", "p99_put_us", "p50_get_us", "p99_get_us"):
        assert out["config"][k] is None
    _run_bench_plain(tmp_path / "b")

    assert [p.name for p in (tmp_path / "a").iterdir()] == ["get_r0.npy"]
    a = np.load(tmp_path / "a" / "get_r0.npy")
    b = np.load(tmp_path / "b" / "get_r0.npy")
    page_elems = 128 * 1024 // 2
    assert a.dtype == np.float32 and a.shape == (16 * page_elems,)
    # step index 2 (the last of 3) writes the buffer salted with 3.0
    assert (a[0::page_elems] == 3.0).all()
    assert a.std() > 0.5
    assert np.array_equal(a, b)


def test_bench_dump_sample_is_seeded_and_bounded():
    """Payloads over the budget are dumped as a stratified sample: same
    indices for the same arguments, every page represented, element 0 (the
    salt) of every page included, never more than the budget."""
    import numpy as np

    sys.path.insert(0, REPO)
    try:
        import bench
    finally:
        sys.path.remove(REPO)

    assert bench.DUMP_BUDGET_BYTES <= 64 << 20
    assert bench._dump_sample_index(4, 100, 400, seed=0) is None
    idx = bench._dump_sample_index(512, 65536, 1 << 21, seed=3)
    again = bench._dump_sample_index(512, 65536, 1 << 21, seed=3)
    assert np.array_equal(idx, again)
    assert len(idx) <= 1 << 21 and len(np.unique(idx)) == len(idx)
    assert idx.min() == 0 and idx.max() < 512 * 65536
    assert np.array_equal(np.unique(idx // 65536), np.arange(512))
    assert np.isin(np.arange(512) * 65536, idx).all()
    # more pages than budget: a subset of pages, one element each
    few = bench._dump_sample_index(1000, 8, 100, seed=1)
    assert len(few) == 100 and (few % 8 == 0).all()
