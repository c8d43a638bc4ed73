"""Jobs through a real CPU `Shard` (`_dbg_shard_run` with device = -1): the
segmented memcpy loop of `submit_copy` in both directions, the refusal of
every transform, and the plain-memcpy fabric path. Memory is numpy: sentinel
filled destinations with gaps, so a byte written anywhere else shows."""

import numpy as np
import pytest
import torch

from infinistore_amd import _native

SENTINEL = 0xA5
NONE, FP8, MXFP4 = 0, 1, 2  # codec ids
T = 30  # timeout_s: a guard against a hang, not a measurement


def run(copy_jobs=(), fabric_jobs=(), n_threads=1):
    return _native._dbg_shard_run(-1, 1, 1, 5, list(copy_jobs), list(fabric_jobs), n_threads, T)


class HostArena:
    """n pages of S segments of `seg` bytes, `stride` apart, pages in shuffled
    slots with 7 spare bytes between them, in one numpy byte array."""

    def __init__(self, n, S, seg, stride, fill, seed):
        assert stride >= seg or S == 1
        self.n, self.S, self.seg, self.stride = n, S, seg, stride
        slot = S * max(stride, seg) + 7
        rs = np.random.RandomState(seed)
        total = 5 + n * slot
        self.a = (rs.randint(0, 256, total).astype(np.uint8) if fill == "pattern"
                  else np.full(total, SENTINEL, dtype=np.uint8))
        self.offs = 5 + rs.permutation(n).astype(np.int64) * slot
        self.ptrs = [self.a.ctypes.data + int(o) for o in self.offs]
        so = self.offs[:, None] + np.arange(S)[None, :] * stride  # (n, S)
        self.idx = (so[:, :, None] + np.arange(seg)[None, None, :]).reshape(n, S * seg)
        assert self.idx.min() >= 0 and self.idx.max() < total
        assert np.unique(self.idx).size == self.idx.size

    def pages(self):
        return self.a[self.idx]

    def outside_is_sentinel(self):
        m = np.ones(self.a.size, dtype=bool)
        m[self.idx.reshape(-1)] = False
        return bool((self.a[m] == SENTINEL).all())


@pytest.mark.parametrize("store", [True, False])
@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("seg", [1, 15, 513])
@pytest.mark.parametrize("S", [1, 2, 3])
def test_cpu_plain_copy(S, seg, n, store):
    """Client side segmented (stride = segment + 3), pool side contiguous; the
    pool block is the concatenation of the page's segments."""
    stride = seg + 3
    fill = ("pattern", "sentinel") if store else ("sentinel", "pattern")
    client = HostArena(n, S, seg, stride, fill[0], seed=S * 100 + seg + n)
    pool = HostArena(n, 1, S * seg, S * seg, fill[1], seed=7 + seg)
    src, dst = (client, pool) if store else (pool, client)
    before = src.a.copy()
    job = (src.ptrs, dst.ptrs, S * seg, NONE, store, S, stride if S > 1 else 0, None, 0)
    (res,), _ = run([job])
    assert (res["submitted"], res["done_calls"], res["ok"]) == (True, 1, True), res
    assert np.array_equal(dst.pages(), src.pages())
    assert dst.outside_is_sentinel(), "bytes outside the destination were written"
    assert np.array_equal(src.a, before), "the source was modified"


def test_cpu_shard_refuses_every_transform():
    """fp8 and mxfp4 are GPU-only: submit_copy returns false, never calls done
    and writes nothing — contiguous or segmented, store or load."""
    n, page = 3, 256  # a legal page for both codecs; 2 segments of 128 bytes
    a = HostArena(n, 2, 128, 144, "pattern", seed=1)
    whole = HostArena(n, 1, page, page, "pattern", seed=2)
    out = HostArena(n, 2, 128, 144, "sentinel", seed=3)
    jobs, dsts = [], []
    for codec in (FP8, MXFP4):
        scales = [1.0] * n if codec == FP8 else None
        for store in (True, False):
            jobs.append((whole.ptrs, out.ptrs, page, codec, store, 1, 0, scales, 0))
            jobs.append((a.ptrs, out.ptrs, page, codec, store, 2, 144, scales, 0))
    results, _ = run(jobs)
    assert len(results) == 8
    for r in results:
        assert (r["submitted"], r["done_calls"]) == (False, 0), r
    assert bool((out.a == SENTINEL).all()), "a refused job wrote"


def test_cpu_shard_refusals_and_the_empty_job():
    src = HostArena(3, 1, 64, 64, "pattern", seed=4)
    dst = HostArena(3, 1, 64, 64, "sentinel", seed=5)
    jobs = [
        (src.ptrs, dst.ptrs[:2], 64, NONE, True, 1, 0, None, 0),  # list lengths
        (src.ptrs, dst.ptrs, 0, NONE, True, 1, 0, None, 0),  # empty blocks
        (src.ptrs, dst.ptrs, 64, NONE, True, 0, 0, None, 0),  # no segments
        (src.ptrs, dst.ptrs, 64, NONE, True, 3, 32, None, 0),  # 64 % 3
        (src.ptrs, dst.ptrs, 64, NONE, True, 2, 31, None, 0),  # segments overlap
        ([], [], 64, NONE, True, 1, 0, None, 0),  # nothing to do: done(true)
    ]
    results, _ = run(jobs, n_threads=2)
    for r in results[:-1]:
        assert (r["submitted"], r["done_calls"]) == (False, 0), r
    r = results[-1]
    assert (r["submitted"], r["done_calls"], r["ok"]) == (True, 1, True), r
    assert bool((dst.a == SENTINEL).all())


@pytest.mark.parametrize("bs", [1, 1000])
def test_cpu_fabric_put_and_get(bs):
    """Host offsets shuffled with gaps between the blocks; put fills the pool
    blocks from the host bytes, get fills the host bytes and leaves the gaps."""
    n = 23
    rs = np.random.RandomState(bs)
    offs = [int(o) for o in 3 + rs.permutation(n) * (bs + 5)]
    host = rs.randint(0, 256, 3 + n * (bs + 5)).astype(np.uint8)
    pool = HostArena(n, 1, bs, bs, "sentinel", seed=6)
    host_before = host.copy()
    _, (res,) = run(fabric_jobs=[(True, host, pool.ptrs, offs, bs)])
    assert res == (1, True)
    want = np.stack([host_before[o:o + bs] for o in offs])
    assert np.array_equal(pool.pages(), want)
    assert pool.outside_is_sentinel()
    assert np.array_equal(host, host_before), "a put must not write the host buffer"

    back = np.full(host.size, SENTINEL, dtype=np.uint8)
    pool_before = pool.a.copy()
    _, (res,) = run(fabric_jobs=[(False, back, pool.ptrs, offs, bs)])
    assert res == (1, True)
    covered = np.zeros(back.size, dtype=bool)
    for i, o in enumerate(offs):
        assert np.array_equal(back[o:o + bs], want[i]), f"block {i}"
        covered[o:o + bs] = True
    assert bool((back[~covered] == SENTINEL).all()), "gap bytes were written"
    assert np.array_equal(pool.a, pool_before)


def test_copy_and_fabric_jobs_from_many_threads():
    """Copy jobs first, then fabric jobs, dealt over 4 threads; every job has
    memory of its own and is checked."""
    copies, fabrics, checks = [], [], []
    for k in range(6):
        src = HostArena(5, 2, 15, 18, "pattern", seed=10 + k)
        dst = HostArena(5, 1, 30, 30, "sentinel", seed=20 + k)
        copies.append((src.ptrs, dst.ptrs, 30, NONE, True, 2, 18, None, 0))
        checks.append((src, dst))
    hosts = []
    for k in range(3):
        host = np.random.RandomState(30 + k).randint(0, 256, 400).astype(np.uint8)
        pool = HostArena(4, 1, 50, 50, "sentinel", seed=40 + k)
        fabrics.append((True, host, pool.ptrs, [300, 0, 100, 200], 50))
        hosts.append((host, pool))
    cres, fres = run(copies, fabrics, n_threads=4)
    for r, (src, dst) in zip(cres, checks):
        assert (r["submitted"], r["done_calls"], r["ok"]) == (True, 1, True), r
        assert np.array_equal(dst.pages(), src.pages()) and dst.outside_is_sentinel()
    for r, (host, pool) in zip(fres, hosts):
        assert r == (1, True)
        assert np.array_equal(pool.pages(), host.reshape(4, 100)[[3, 0, 1, 2], :50])
        assert pool.outside_is_sentinel()


def test_binding_refuses_bad_arguments():
    no_gpu = 1 << 20  # an ordinal no machine has
    with pytest.raises(RuntimeError, match="GPU"):
        _native._dbg_shard_run(no_gpu, 1, 1, 5, [], [], 1, T)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            _native._dbg_shard_run(0, 1, 1, 5, [], [], 1, T)
    ok = dict(device=-1, n_streams=1, slots_per_stream=1, max_descs_per_slot=5, copy_jobs=[],
              fabric_jobs=[], n_threads=1, timeout_s=T)
    assert _native._dbg_shard_run(**ok) == ([], [])
    for bad in (dict(device=-2), dict(n_streams=0), dict(slots_per_stream=0),
                dict(max_descs_per_slot=0), dict(n_threads=0), dict(timeout_s=0)):
        with pytest.raises(ValueError):
            _native._dbg_shard_run(**{**ok, **bad})
    buf = np.zeros(16, dtype=np.uint8)
    a = np.zeros(16, dtype=np.uint8)
    for job in ((a.ctypes.data,), ([a.ctypes.data], [a.ctypes.data], 8, 7, True, 1, 0, None, 0)):
        with pytest.raises((ValueError, RuntimeError)):  # not a job of 9; unknown codec
            _native._dbg_shard_run(**{**ok, "copy_jobs": [job]})
    for job in ((True, buf, [a.ctypes.data], [9], 8),  # 9 + 8 > 16
                (True, buf, [a.ctypes.data], [0, 8], 8),  # one offset per block
                (True, buf[::2], [a.ctypes.data], [0], 8)):  # not contiguous
        with pytest.raises(ValueError):
            _native._dbg_shard_run(**{**ok, "fabric_jobs": [job]})
    assert not a.any()
