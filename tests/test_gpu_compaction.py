"""Compaction of stored blocks that span several allocator granules, on HBM.

The pool's granule is 16 KiB; bf16 pages are written plain, as fp8 and as
mxfp4 at sizes whose stored blocks take 1, 2, 3 and 6 granules (for every
codec: exactly one granule and just over it, three, six), a few hundred keys
in rounds so that small and large blocks alternate in the pool. All keys of
the 1- and 3-granule sizes are deleted, which leaves holes of 12 and 18
granules between the survivors; compact_pool() moves 2- and 6-granule blocks into them
with the copy kernel; every survivor is read; new 6-granule keys are written
into the space that compaction freed; everything is read again.

Expected bits are computed when a key is written, by the numpy / torch
references (tests/_kernel_refs.py, tests/_mxfp4_refs.py); every comparison is
bit for bit over the whole destination, guard elements between the pages
included. compact_pool() names no keys, so moved_bytes is checked as the store
model checks it: it is a sum of `moved` live stored sizes.

The test body runs in a child process (this file, started as a script) that
hosts the server in-process, so that compact_pool() is reachable."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _store_model as sm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRANULE = 16 << 10
SENT16 = 0xA5A5
GUARD = 16  # elements between destination pages; keeps every page 16-byte aligned
ROUNDS = 8
# granules -> (elements per codec, keys per round)
SIZES = {
    1: ({"plain": 8192, "fp8": 16384, "mxfp4": 30816}, 4),
    2: ({"plain": 8200, "fp8": 16392, "mxfp4": 30848}, 3),
    3: ({"plain": 24576, "fp8": 49152, "mxfp4": 92512}, 2),
    6: ({"plain": 49152, "fp8": 98304, "mxfp4": 185024}, 1),
}
CODECS = ("plain", "fp8", "mxfp4")
DELETED = (1, 3)


def stored(elems, codec):
    return sm.stored_bytes(elems, codec, 2)


def test_sizes_span_the_granules_they_claim():
    for granules, (by_codec, _) in SIZES.items():
        for codec, elems in by_codec.items():
            assert elems % sm.CODEC_MULTIPLE[codec] == 0
            assert -(-stored(elems, codec) // GRANULE) == granules, (granules, codec)
    # exactly one granule, and at most 16 bytes into the second
    assert stored(SIZES[1][0]["plain"], "plain") == GRANULE == stored(SIZES[1][0]["fp8"], "fp8")
    for codec in CODECS:
        assert 0 < stored(SIZES[2][0][codec], codec) - GRANULE <= 16


@pytest.mark.gpu
def test_compaction_moves_multi_granule_blocks(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r = subprocess.run(
        [sys.executable, os.path.abspath(__file__)],
        cwd=REPO, env={**os.environ, "PYTHONPATH": REPO + ":" + os.path.join(REPO, "tests")},
        timeout=180)
    assert r.returncode == 0, "see the child's output above"


def make_pages(n, elems, seed):
    """n bf16 pages with a different magnitude per 32-element group (finite)."""
    g = torch.Generator().manual_seed(seed)
    groups = -(-elems // 32)
    mag = torch.pow(2.0, torch.randint(-20, 20, (n, groups, 1), generator=g).float())
    x = (torch.randn(n, groups, 32, generator=g) * mag).reshape(n, -1)[:, :elems]
    return x.contiguous().to(torch.bfloat16)


class Store:
    def __init__(self, conn):
        self.conn = conn
        self.model = {}  # key -> (uint16 bits of the page as read, codec, stored bytes)
        self.serial = 0

    def write(self, granules, codec, n):
        from test_gpu_store_model import expected_bits
        elems = SIZES[granules][0][codec]
        keys = [f"cmp-{granules}g-{codec}-{self.serial + i}" for i in range(n)]
        self.serial += n
        pages = make_pages(n, elems, self.serial)
        want = expected_bits(pages, codec)  # before anything is sent
        src = pages.to("cuda:0").reshape(-1)
        self.conn.write_pages(src, keys, [j * elems for j in range(n)], elems, sync=True,
                              quant=None if codec == "plain" else codec)
        for j, k in enumerate(keys):
            self.model[k] = (want[j], codec, stored(elems, codec))
        return keys

    def delete(self, granules):
        keys = [k for k in self.model if k.startswith(f"cmp-{granules}g-")]
        assert keys and self.conn.delete_keys(keys) == len(keys)
        for k in keys:
            del self.model[k]

    def read_all(self, what):
        from _kernel_refs import bf16_bits
        by_size = {}
        for k, (bits, _, _) in self.model.items():
            by_size.setdefault(len(bits), []).append(k)
        for elems, keys in by_size.items():
            slot = elems + GUARD
            dst = torch.empty(len(keys) * slot, dtype=torch.bfloat16, device="cuda:0")
            dst.view(torch.uint8).fill_(0xA5)
            want = np.full(dst.numel(), SENT16, dtype=np.uint16)
            for j, k in enumerate(keys):
                want[j * slot:j * slot + elems] = self.model[k][0]
            self.conn.read_pages(dst, keys, [j * slot for j in range(len(keys))], elems)
            self.conn.sync()
            got = bf16_bits(dst)
            if not np.array_equal(got, want):
                bad = np.flatnonzero(got != want)
                raise AssertionError(
                    f"{what}: {len(keys)} keys of {elems} elements: {bad.size} values differ, "
                    f"first at {bad[0]} (key {keys[bad[0] // slot]}): "
                    f"got {got[bad[0]]:#06x} want {want[bad[0]]:#06x}")


def main():
    import infinistore_amd as ifs
    from conftest import free_port

    def largest_free_run():
        return json.loads(ifs.get_server_stats())["largest_free_run_bytes"]

    port = free_port()
    ifs.register_server(ifs.ServerConfig(service_port=port, manage_port=free_port(),
                                         prealloc_size=1, minimal_allocate_size=16,
                                         devices=[0]))  # one shard: /stats reports the
    # largest free run over all shards, and an untouched shard would hide this one's
    try:
        conn = ifs.InfinityConnection(ifs.ClientConfig(
            host_addr="127.0.0.1", service_port=port, connection_type=ifs.TYPE_LOCAL_GPU))
        conn.connect()
        store = Store(conn)
        for _ in range(ROUNDS):  # small and large interleaved
            for granules, (_, per_round) in SIZES.items():
                for codec in CODECS:
                    store.write(granules, codec, per_round)
        assert ifs.get_kvmap_len() == len(store.model) == ROUNDS * 10 * len(CODECS)
        store.read_all("after the writes")

        for granules in DELETED:
            store.delete(granules)
        assert ifs.get_kvmap_len() == len(store.model)
        before = largest_free_run()
        moved, moved_bytes = ifs.compact_pool()
        after = largest_free_run()
        print(f"compact_pool: moved {moved} blocks, {moved_bytes} bytes; "
              f"largest free run {before} -> {after}", flush=True)
        sizes = [s for _, _, s in store.model.values()]
        assert 0 < moved <= len(sizes), moved
        assert sm.moved_bytes_possible(sizes, moved, moved_bytes), (moved, moved_bytes)
        assert after > before, (before, after)
        assert ifs.get_kvmap_len() == len(store.model)
        store.read_all("survivors after compaction")

        for codec in CODECS:  # the largest size, into the freed space
            store.write(6, codec, ROUNDS)
        assert ifs.get_kvmap_len() == len(store.model)
        store.read_all("everything after the new writes")
        conn.close()
    finally:
        ifs.unregister_server()
    print(f"COMPACTION OK: {len(store.model)} keys live")


if __name__ == "__main__":
    main()
