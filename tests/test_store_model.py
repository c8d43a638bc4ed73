"""Model-based test of the store, CPU driver: schedules from
tests/_store_model.py run against an in-process server with a DRAM pool over
the TCP fabric, next to a dict key -> expected bytes. Plain uint8 pages of
seven sizes share one pool through dedup, wrong-size reads, delete,
compaction and snapshot/restore; after every operation the index holds
exactly the model's keys, and every read is compared byte for byte, the
untouched part of the destination included. Also here: the check of the
generator itself, for the seeds of both drivers."""

import json

import numpy as np
import pytest
import torch

import infinistore_amd as ifs

import _store_model as sm
from conftest import make_client

SENTINEL = 0xA5
INVALID_REQ = "ret = -400"
BATCH = 12  # keys per read request at most


@pytest.mark.parametrize("profile,seeds,n_ops", [
    (sm.CPU_PROFILE, sm.CPU_SEEDS, sm.CPU_OPS),
    (sm.GPU_PROFILE, sm.GPU_SEEDS, sm.GPU_OPS),
], ids=["cpu", "gpu"])
def test_committed_schedules_cover_what_they_claim(profile, seeds, n_ops):
    """No server. Every committed schedule holds every kind of operation at
    least five times, a compact right after a delete, a restore into a live
    index, an overwrite attempt of every kind the driver has (a driver with
    one codec has no "other codec"), and at least three stored sizes at the
    final compaction; and every operation applies to the store as it is then."""
    assert len(seeds) >= 2
    for seed in seeds:
        ops = sm.schedule(profile, seed, n_ops)
        assert ops == sm.schedule(profile, seed, n_ops), "the generator is not pure"
        assert n_ops <= len(ops) <= n_ops + 9
        cov = sm.coverage(profile, ops)
        assert cov["applicable"], seed
        for kind in sm.KINDS:
            assert cov["kinds"].get(kind, 0) >= 5, (seed, kind, cov["kinds"])
        assert cov["kinds"]["read_all"] == 3  # before the final delete, after the
        # final compaction, after snapshot / purge / restore
        tail = [op["op"] for op in ops[-7:]]
        assert tail == ["read_all", "delete", "compact", "read_all", "snapshot", "restore",
                        "read_all"], (seed, tail)
        assert cov["compact_after_delete"] >= 2, seed  # the final one and another
        assert cov["restore_into_live"] >= 1, seed
        want = [k for k in sm.OVERWRITE_KINDS if k != "codec" or len(profile.codecs) > 1]
        for kind in want:
            assert cov["overwrite_kinds"].get(kind, 0) >= 1, (seed, kind)
        assert cov["final_stored_sizes"] >= 3, seed
        assert cov["final_live"] >= 8, seed
        if profile is sm.GPU_PROFILE:
            reads = [op for op in ops if op["op"] == "read"]
            writes = [op for op in ops if op["op"] in ("write", "overwrite")]
            assert {(op["mode"], op["parts"]) for op in reads} == set(profile.read_modes), seed
            assert {(op["layout"], op["parts"]) for op in writes} == set(profile.layouts), seed
            assert {op["ticketed"] for op in reads} == {True, False}, seed
            assert {op["codec"] for op in writes} == set(profile.codecs), seed


def test_moved_bytes_possible():
    sizes = [17, 17, 272, 2193]
    assert sm.moved_bytes_possible(sizes, 0, 0)
    assert sm.moved_bytes_possible(sizes, 2, 34)
    assert sm.moved_bytes_possible(sizes, 3, 17 + 272 + 2193)
    assert not sm.moved_bytes_possible(sizes, 2, 544)  # only one block of 272
    assert not sm.moved_bytes_possible(sizes, 1, 34)
    assert not sm.moved_bytes_possible(sizes, 5, 17 + 17 + 272 + 2193)


class CpuDriver:
    def __init__(self, conn, tmp_path):
        self.conn = conn
        self.snap_path = str(tmp_path / "model.snap")
        self.model = {}  # key -> np.uint8 array, the bytes a read must return
        self.snap = None
        biggest = max(sm.CPU_PROFILE.sizes)
        self.src = torch.zeros((sm.CPU_PROFILE.max_keys + 1) * biggest, dtype=torch.uint8)
        self.dst = torch.zeros(BATCH * biggest, dtype=torch.uint8)
        conn.register_mr(self.src)
        conn.register_mr(self.dst)

    def _check_read(self, placed, what):
        """placed: [(offset, expected bytes)]; everything else stays sentinel."""
        want = np.full(self.dst.numel(), SENTINEL, dtype=np.uint8)
        for off, data in placed:
            want[off:off + len(data)] = data
        got = self.dst.numpy()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[0]}: "
                                 f"got {got[bad[0]]}, want {want[bad[0]]}")

    def _read(self, keys, size):
        for lo in range(0, len(keys), BATCH):
            part = keys[lo:lo + BATCH]
            self.dst.fill_(SENTINEL)
            self.conn.read_cache(self.dst, [(k, j * size) for j, k in enumerate(part)], size)
            self.conn.sync()
            self._check_read([(j * size, self.model[k]) for j, k in enumerate(part)],
                             f"read of {len(part)} keys at {size}")

    def step(self, op):
        kind, conn, model = op["op"], self.conn, self.model
        if kind in ("write", "overwrite"):
            keys, size = op["keys"] + op.get("new_keys", []), op["size"]
            data = np.random.RandomState(op["seed"]).randint(
                0, 256, (len(keys), size), dtype=np.uint8)
            self.src[: data.size] = torch.from_numpy(data.reshape(-1))
            blocks = conn.allocate_rdma(keys, size)
            for k, b in zip(keys, blocks):  # a live key gets the FAKE block
                assert (tuple(b) == (0, 0)) == (k in model), (k, tuple(b))
            conn.rdma_write_cache(self.src, [j * size for j in range(len(keys))], size, blocks)
            conn.sync()
            for j, k in enumerate(keys):
                model.setdefault(k, data[j].copy())  # first write wins
        elif kind == "read":
            self._read(op["keys"], op["size"])
        elif kind == "read_wrong":
            key, page = op["key"], op["page"]
            self.dst.fill_(SENTINEL)
            if op["expect"] == "prefix":
                assert page < len(model[key])
                conn.read_cache(self.dst, [(key, 0)], page)
                conn.sync()
                self._check_read([(0, model[key][:page])], f"prefix read at {page}")
            else:
                assert page > len(model[key])
                with pytest.raises(Exception, match=INVALID_REQ):
                    conn.read_cache(self.dst, [(key, 0)], page)
                self._check_read([], f"refused read at {page}")
        elif kind == "delete":
            assert conn.delete_keys(op["keys"]) == len(op["keys"])
            for k in op["keys"]:
                del model[k]
        elif kind == "compact":
            moved, moved_bytes = ifs.compact_pool()
            sizes = [len(v) for v in model.values()]
            assert moved <= len(sizes) and moved_bytes <= sum(sizes), (moved, moved_bytes)
            assert sm.moved_bytes_possible(sizes, moved, moved_bytes), (moved, moved_bytes)
            if op.get("final"):
                assert moved > 0
        elif kind == "snapshot":
            got = ifs.snapshot_pool(self.snap_path)
            assert got == (len(model), sum(len(v) for v in model.values())), got
            self.snap = dict(model)
        elif kind == "restore":
            if op["purge"]:
                ifs.purge_kv_map()
                model.clear()
            absent = [k for k in self.snap if k not in model]
            got = ifs.restore_pool(self.snap_path)
            assert got == (len(absent), sum(len(self.snap[k]) for k in absent)), got
            for k in absent:  # live keys win
                model[k] = self.snap[k]
        elif kind == "read_all":
            by_size = {}
            for k, v in model.items():
                by_size.setdefault(len(v), []).append(k)
            for size, keys in by_size.items():
                self._read(keys, size)
        else:
            raise AssertionError(f"unknown operation {kind}")
        assert ifs.get_kvmap_len() == len(model), (ifs.get_kvmap_len(), len(model))


@pytest.mark.parametrize("seed", sm.CPU_SEEDS)
def test_store_model_cpu(cpu_server, tmp_path, seed):
    ops = sm.schedule(sm.CPU_PROFILE, seed, sm.CPU_OPS)
    conn = make_client(cpu_server)
    try:
        driver = CpuDriver(conn, tmp_path)
        for i, op in enumerate(ops):
            try:
                driver.step(op)
            except BaseException:
                print(sm.describe(seed, ops, i))
                raise
        stats = json.loads(ifs.get_server_stats())
        assert stats["kv_len"] == len(driver.model)
    finally:
        conn.close()
