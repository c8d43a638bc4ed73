"""Jobs through a real GPU `Shard` at small limits (`_dbg_shard_run`): the
chunk loop of `submit_copy` and its scale bookkeeping, fan-out into sub-jobs,
slot exhaustion with many submitters, every refusal, and the staged fabric
pipeline at its bounds. Limits of a few descriptors per slot and one or two
slots per stream make branches run that the server's defaults (4 streams, 48
slots, 16384 descriptors) keep out of reach of any test of affordable size.

All memory is a guarded, bounds-asserted `Region` / `SegArena`; the oracles
are the references of the kernel tests, compared bit for bit (fp8 scales as
float32 bytes), with guards intact and the source unmodified. Every job must
come back submitted, called back exactly once, and ok. At most two streams
per Shard: with torch's the process stays within four hardware queues.

Segmented transform cases take the listed element counts PER SEGMENT: a page
of 8 (fp8) or 32 (mxfp4) elements cannot be cut into two legal segments."""

import numpy as np
import pytest
import torch

from infinistore_amd import _native

from _kernel_refs import (
    SENTINEL,
    Region,
    assert_bf16_bits_equal,
    assert_codes_equal,
    bf16_bits,
    fp8_dequant_ref,
    fp8_quant_ref,
)
from _mxfp4_refs import dequant_ref, quant_ref, stored_bytes
from _seg_refs import SegArena

pytestmark = pytest.mark.gpu

DEV = 0
NONE, FP8, MXFP4 = 0, 1, 2  # codec ids
T = 30  # timeout_s: a guard against a hang, not a measurement
F = _native._SHARD_FAN_CHUNK
D = _native._FAB_STAGE_DESCS
B = _native._FAB_STAGE_BYTES
POISON = float(np.float32(-12345.678))
GEOMS = ["contig", "gapped", "kv_major"]


def shard_run(opts, copy_jobs=(), fabric_jobs=(), n_threads=1):
    """opts = (streams, slots per stream, descriptors per slot). The Shard's
    streams do not wait for torch's: everything torch wrote is synchronized
    first; the Shard is drained and gone when the call returns."""
    assert opts[0] <= 2
    torch.cuda.synchronize()
    return _native._dbg_shard_run(DEV, opts[0], opts[1], opts[2], list(copy_jobs),
                                  list(fabric_jobs), n_threads, T)


def assert_done_ok(res, what):
    assert (res["submitted"], res["done_calls"], res["ok"]) == (True, 1, True), (what, res)


def _same(a, b, what):
    if not torch.equal(a, b):
        bad = (a != b).nonzero()[0].tolist()
        raise AssertionError(f"{what}: block {bad[0]} byte {bad[1]} differs "
                             f"({int((a != b).sum())} bytes wrong)")


def _client(geom, n, page_bytes, fill, seed, misalign=0):
    """The client side of n pages: a Region when contiguous, else a 2-segment
    SegArena. Returns (arena, n_segments, stride)."""
    if geom == "contig":
        r = Region(n, page_bytes, misalign=misalign, fill=fill, seed=seed)
        return r, 1, 0
    a = SegArena(n, 2, page_bytes // 2, geom, fill=fill, seed=seed)
    return a, 2, a.stride


def _pages(arena):
    return arena.blocks() if isinstance(arena, Region) else arena.pages()


def _set_pages(arena, data):
    (arena.set_blocks if isinstance(arena, Region) else arena.set_pages)(data)


# ---------------------------------------------------------------------------
# cases: each builds its memory, hands out a store job and (unless it is a
# contiguous plain copy, which has no direction) a load job, and checks both
# ---------------------------------------------------------------------------
class PlainCase:
    """kind "vec": 256-byte pages, everything 16-byte aligned. kind "byte":
    1000-byte pages with exactly one odd pointer on each side (on the
    kv-major client side, where pages touch, only the pool side has one)."""

    def __init__(self, kind, geom, n, seed):
        self.what = f"plain {kind} {geom} n={n}"
        self.n = n
        self.nbytes = nbytes = 256 if kind == "vec" else 1000
        odd_src = np.zeros(n, dtype=np.int64)
        odd_dst = np.zeros(n, dtype=np.int64)
        if kind == "byte":
            odd_src[n - 1] = 1
            odd_dst[0] = 1
        self.geom = geom
        if geom == "contig":
            self.src = Region(n, nbytes, misalign=odd_src, fill="pattern", seed=seed)
            self.pool = Region(n, nbytes, misalign=odd_dst, fill="sentinel", seed=seed + 1)
            self.S, self.stride = 1, 0
        else:
            self.src = SegArena(n, 2, nbytes // 2, geom, fill="pattern", seed=seed)
            self.out = SegArena(n, 2, nbytes // 2, geom, fill="sentinel", seed=seed + 2)
            if kind == "byte" and geom == "gapped":
                for a, k in ((self.src, n - 1), (self.out, 0)):
                    a.offs[k] += 1
                    a.ptrs[k] += 1
                    a.assert_in_bounds()
            self.pool = Region(n, nbytes, misalign=odd_dst, fill="sentinel", seed=seed + 1)
            self.S, self.stride = 2, self.src.stride
            assert self.out.stride == self.stride
        self.src_before = self.src.t.clone()

    def store_job(self):
        return (self.src.ptrs, self.pool.ptrs, self.nbytes, NONE, True, self.S, self.stride,
                None, 0)

    def check_store(self, res):
        assert_done_ok(res, self.what)
        _same(self.pool.blocks(), _pages(self.src), self.what)
        assert self.pool.guards_intact(), f"{self.what}: bytes outside the pool blocks written"
        assert torch.equal(self.src.t, self.src_before), f"{self.what}: the source was modified"

    def load_job(self):
        if self.geom == "contig":
            return None
        self.pool_before = self.pool.t.clone()
        return (self.pool.ptrs, self.out.ptrs, self.nbytes, NONE, False, self.S, self.stride,
                None, 0)

    def check_load(self, res):
        assert_done_ok(res, self.what)
        _same(self.out.pages(), self.pool.blocks(), self.what + " load")
        assert self.out.guards_intact(), f"{self.what}: bytes outside the segments written"
        assert torch.equal(self.pool.t, self.pool_before), f"{self.what}: the source was modified"


def fp8_pages(n, elems, seed):
    """Every page with its own absmax: a distinct odd factor times a power of
    two, exact in bf16, so a scale stored against the wrong page or chunk
    changes codes."""
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(n)
    amax = (2.0 * (i % 128) + 1.0) * torch.pow(2.0, (i // 128 - 16).float())
    assert amax.unique().numel() == n
    pages = ((torch.rand(n, elems, generator=g) - 0.5) * amax[:, None]).to(torch.bfloat16)
    pages[i, i % elems] = (amax * torch.where(i % 2 == 0, 1.0, -1.0)).to(torch.bfloat16)
    assert torch.equal(pages.float().abs().max(dim=1).values, amax)  # exact in bf16
    return pages


class Fp8Case:
    """Store with scales_off = 3 into n + 7 poison values, then load with the
    scales the store left, from the same offset."""

    OFF, EXTRA = 3, 7

    def __init__(self, geom, n, elems, seed):
        self.what = f"fp8 {geom} n={n} elems={elems}"
        self.n = n
        self.elems = elems = elems if geom == "contig" else 2 * elems
        pages = fp8_pages(n, elems, seed)
        self.want_codes, self.want_scales = fp8_quant_ref(pages)
        assert np.unique(self.want_scales).size == n
        self.want_back = bf16_bits(fp8_dequant_ref(self.want_codes, self.want_scales))
        self.src, self.S, self.stride = _client(geom, n, 2 * elems, "pattern", seed)
        _set_pages(self.src, pages)
        self.pool = Region(n, elems, fill="sentinel", seed=seed + 1)
        self.out, _, stride = _client(geom, n, 2 * elems, "sentinel", seed + 2)
        assert stride == self.stride
        self.src_before = self.src.t.clone()

    def store_job(self):
        return (self.src.ptrs, self.pool.ptrs, 2 * self.elems, FP8, True, self.S, self.stride,
                [POISON] * (self.n + self.EXTRA), self.OFF)

    def check_store(self, res):
        assert_done_ok(res, self.what)
        got = np.asarray(res["scales"], dtype=np.float32)
        want = np.full(self.n + self.EXTRA, POISON, dtype=np.float32)
        want[self.OFF:self.OFF + self.n] = self.want_scales
        assert got.tobytes() == want.tobytes(), (
            f"{self.what}: scales differ at {np.flatnonzero(got != want)[:8]}", got, want)
        assert_codes_equal(self.pool.blocks().cpu().numpy(), self.want_codes.numpy(), self.what)
        assert self.pool.guards_intact(), f"{self.what}: bytes outside the pool blocks written"
        assert torch.equal(self.src.t, self.src_before), f"{self.what}: the source was modified"
        self.scales = res["scales"]

    def load_job(self):
        self.pool_before = self.pool.t.clone()
        return (self.pool.ptrs, self.out.ptrs, 2 * self.elems, FP8, False, self.S, self.stride,
                self.scales, self.OFF)

    def check_load(self, res):
        assert_done_ok(res, self.what)
        assert np.asarray(res["scales"], dtype=np.float32).tobytes() == np.asarray(
            self.scales, dtype=np.float32).tobytes(), f"{self.what}: a load wrote scales"
        got = _pages(self.out).cpu().numpy().view(np.uint16)
        assert_bf16_bits_equal(got, self.want_back, self.what + " load")
        assert self.out.guards_intact(), f"{self.what}: bytes outside the pages written"
        assert torch.equal(self.pool.t, self.pool_before), f"{self.what}: the source was modified"


def mx_pages(n, elems, seed):
    """bf16 pages with a different magnitude per 32-element group."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(2.0, torch.randint(-20, 20, (n, elems // 32, 1), generator=g).float())
    x = torch.randn(n, elems // 32, 32, generator=g) * mag
    return x.reshape(n, elems).to(torch.bfloat16)


class Mxfp4Case:
    def __init__(self, geom, n, elems, seed):
        self.what = f"mxfp4 {geom} n={n} elems={elems}"
        self.n = n
        self.elems = elems = elems if geom == "contig" else 2 * elems
        pages = mx_pages(n, elems, seed)
        self.want = quant_ref(bf16_bits(pages))
        self.want_back = dequant_ref(self.want, elems)
        self.src, self.S, self.stride = _client(geom, n, 2 * elems, "pattern", seed)
        _set_pages(self.src, pages)
        self.pool = Region(n, stored_bytes(elems), fill="sentinel", seed=seed + 1)
        self.out, _, stride = _client(geom, n, 2 * elems, "sentinel", seed + 2)
        assert stride == self.stride
        self.src_before = self.src.t.clone()

    def store_job(self):
        return (self.src.ptrs, self.pool.ptrs, 2 * self.elems, MXFP4, True, self.S, self.stride,
                None, 0)

    def check_store(self, res):
        assert_done_ok(res, self.what)
        got = self.pool.blocks().cpu().numpy()
        assert (got == self.want).all(), f"{self.what}: {(got != self.want).sum()} bytes differ"
        assert self.pool.guards_intact(), f"{self.what}: bytes outside the pool blocks written"
        assert torch.equal(self.src.t, self.src_before), f"{self.what}: the source was modified"

    def load_job(self):
        self.pool_before = self.pool.t.clone()
        return (self.pool.ptrs, self.out.ptrs, 2 * self.elems, MXFP4, False, self.S, self.stride,
                None, 0)

    def check_load(self, res):
        assert_done_ok(res, self.what)
        got = _pages(self.out).cpu().numpy().view(np.uint16)
        assert_bf16_bits_equal(got, self.want_back, self.what + " load")
        assert self.out.guards_intact(), f"{self.what}: bytes outside the pages written"
        assert torch.equal(self.pool.t, self.pool_before), f"{self.what}: the source was modified"


def run_cases(opts, cases, n_threads=1):
    """All stores through one Shard, checked; then all loads through another."""
    results, _ = shard_run(opts, [c.store_job() for c in cases], n_threads=n_threads)
    assert len(results) == len(cases)
    for c, r in zip(cases, results):
        c.check_store(r)
    loads = [(c, j) for c in cases for j in [c.load_job()] if j is not None]
    results, _ = shard_run(opts, [j for _, j in loads], n_threads=n_threads)
    assert len(results) == len(loads)
    for (c, _), r in zip(loads, results):
        c.check_load(r)


# ---------------------------------------------------------------------------
# 1. the chunk loop, 5 descriptors per slot
# ---------------------------------------------------------------------------
CAP = 5
CHUNK_OPTS = [(1, 1, CAP), (1, 2, CAP), (2, 1, CAP)]


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("opts", CHUNK_OPTS)
def test_chunk_loop_plain_vec(opts, geom):
    """Blocks relative to the cap of 5: 17, 20 (whole chunks), 21. A segmented
    copy never goes inline, so 5 (one full chunk) and 6 count there too."""
    ns = [17, 20, 21] + ([5, 6] if geom != "contig" else [])
    run_cases(opts, [PlainCase("vec", geom, n, 100 + n) for n in ns])


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("opts", CHUNK_OPTS)
def test_chunk_loop_plain_byte(opts, geom):
    run_cases(opts, [PlainCase("byte", geom, n, 200 + n) for n in (4, 5, 6, 11)])


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("elems", [8, 520])
@pytest.mark.parametrize("opts", CHUNK_OPTS)
def test_chunk_loop_fp8(opts, elems, geom):
    run_cases(opts, [Fp8Case(geom, n, elems, 300 + n) for n in (1, 4, 5, 6, 11)])


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("elems", [32, 96])
@pytest.mark.parametrize("opts", CHUNK_OPTS)
def test_chunk_loop_mxfp4(opts, elems, geom):
    run_cases(opts, [Mxfp4Case(geom, n, elems, 400 + n) for n in (4, 5, 6, 11)])


def _chained(n):
    """n 16-byte copies where block 5 reads what block 0 writes. Returns
    (job, sources, destinations)."""
    a = Region(n, 16, fill="pattern", seed=n)
    d = Region(n, 16, fill="sentinel", seed=n + 1)
    src = list(a.ptrs)
    src[5] = d.ptrs[0]
    return (src, d.ptrs, 16, NONE, True, 1, 0, None, 0), a, d


def test_sixteen_aligned_blocks_go_inline_and_bypass_the_chunk_loop():
    """With 5 descriptors per slot, the chunk loop would copy blocks 0-4 in one
    launch and block 5 in the next, so block 5 would read block 0's NEW
    destination bytes. The inline kernel moves all sixteen 16-byte blocks with
    sixteen lanes of one wavefront — every load issues before any store — so
    block 5 gets the OLD bytes (the sentinel). 17 blocks, which must take the
    chunk loop, show the other outcome on the same arrangement."""
    job, a, d = _chained(16)
    (res,), _ = shard_run((1, 1, CAP), [job])
    assert_done_ok(res, "inline")
    got, src = d.blocks().cpu(), a.blocks().cpu()
    assert bool((got[5] == SENTINEL).all()), "16 blocks did not go through the inline kernel"
    keep = [i for i in range(16) if i != 5]
    assert torch.equal(got[keep], src[keep]) and d.guards_intact()

    job, a, d = _chained(17)
    (res,), _ = shard_run((1, 1, CAP), [job])
    assert_done_ok(res, "chunked")
    got, src = d.blocks().cpu(), a.blocks().cpu()
    assert torch.equal(got[5], src[0]), "chunks of one job must run in order on one stream"
    keep = [i for i in range(17) if i != 5]
    assert torch.equal(got[keep], src[keep]) and d.guards_intact()


# ---------------------------------------------------------------------------
# 2. fan-out into sub-jobs of F blocks, each chunked
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("streams", [2, 1])
def test_fanout_plus_chunking_plain(streams):
    """F + 1 blocks of 16 bytes, 1000 descriptors per slot. Two streams: one
    sub-job of F blocks in five chunks and one of a single block, which goes
    inline. One stream: no fan-out, the chunk loop alone."""
    n = F + 1
    assert -(-F // 1000) == 5
    src = Region(n, 16, fill="pattern", seed=1)
    dst = Region(n, 16, fill="sentinel", seed=2)
    before = src.t.clone()
    (res,), _ = shard_run((streams, 1, 1000), [(src.ptrs, dst.ptrs, 16, NONE, True, 1, 0, None, 0)])
    assert_done_ok(res, f"fan-out streams={streams}")
    _same(dst.blocks(), src.blocks(), "fan-out")
    assert dst.guards_intact() and torch.equal(src.t, before)


def test_fanout_plus_chunking_fp8_scales():
    """2F + 8 pages of 8 elements, a distinct scale per page: the scale ranges
    cross both sub-job and chunk boundaries."""
    run_cases((2, 1, 1000), [Fp8Case("contig", 2 * F + 8, 8, 5)])


# ---------------------------------------------------------------------------
# 3. many submitters, few slots
# ---------------------------------------------------------------------------
def test_many_submitters_two_slots():
    """48 jobs of 6..21 blocks from 8 threads onto 2 streams of one slot each:
    submitters block in acquire_slot and skip to the other stream. A slot (and
    its pinned scales) handed on before its kernel and scale copy-out are done
    shows as wrong bytes or wrong scales in some job."""
    makers = [
        lambda n, s: PlainCase("vec", "contig", n, s),
        lambda n, s: Fp8Case("contig", n, 8, s),
        lambda n, s: PlainCase("byte", "gapped", n, s),
        lambda n, s: Mxfp4Case("contig", n, 32, s),
        lambda n, s: Fp8Case("kv_major", n, 520, s),
        lambda n, s: PlainCase("byte", "contig", n, s),
        lambda n, s: Mxfp4Case("gapped", n, 96, s),
        lambda n, s: PlainCase("vec", "kv_major", n, s),
        lambda n, s: Fp8Case("gapped", n, 8, s),
        lambda n, s: Mxfp4Case("kv_major", n, 32, s),
        lambda n, s: Fp8Case("contig", n, 520, s),
        lambda n, s: Mxfp4Case("contig", n, 96, s),
    ]
    cases = [makers[k % len(makers)](6 + (7 * k) % 16, 1000 + 10 * k) for k in range(48)]
    assert {c.n for c in cases} == set(range(6, 22))
    run_cases((2, 1, CAP), cases, n_threads=8)


# ---------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------
def test_refusals():
    """Every job is refused at submit or reported failed, and writes nothing.
    All pointers are real, aligned where it is not the alignment that is
    wrong, and in bounds for the largest geometry asked for."""
    n = 3
    client = SegArena(n, 4, 8192, "gapped", fill="pattern", seed=1)
    pool = Region(n, 32768, fill="sentinel", seed=2)
    src_pool = Region(n, 32768, fill="pattern", seed=3)
    out = SegArena(n, 4, 8192, "gapped", fill="sentinel", seed=4)
    odd = SegArena(n, 4, 8192, "gapped", misalign=8, fill="pattern", seed=5)
    odd_out = SegArena(n, 4, 8192, "gapped", misalign=8, fill="sentinel", seed=6)
    scales = [1.0] * n
    jobs = []

    def both(nbytes, codec, S, stride, sc=None, off=0, cl=None, pl=None, cl_out=None):
        """The store (client -> pool) and the load (pool -> out) of one
        refused request."""
        cl, pl = cl or client.ptrs, pl or pool.ptrs
        jobs.append((cl, pl, nbytes, codec, True, S, stride, sc, off))
        jobs.append((src_pool.ptrs[:len(pl)], (cl_out or out.ptrs)[:len(cl)], nbytes, codec,
                     False, S, stride, sc, off))

    both(256, NONE, 1, 0, cl=client.ptrs[:2])  # list lengths
    both(0, NONE, 1, 0)  # empty blocks
    for codec, group, sc in ((NONE, 16, None), (FP8, 16, scales), (MXFP4, 64, None)):
        seg = 4 * group  # bytes per segment, legal for the codec
        both(2 * seg, codec, 0, 1024, sc)  # no segments
        both(1025 * group, codec, 1025, group, sc)  # more than _MAX_PAGE_SEGMENTS
        both(3 * seg + group, codec, 3, 1024, sc)  # page % segments
        both(2 * seg, codec, 2, seg - 16, sc)  # segments overlap
    for codec, group, sc in ((FP8, 16, scales), (MXFP4, 64, None)):
        both(2 * (4 * group + group // 2), codec, 2, 1024, sc)  # half a group per segment
        both(2 * 4 * group, codec, 2, 8 * group + 8, sc)  # stride % 16
        both(256, codec, 1, 0, sc, cl=odd.ptrs, cl_out=odd_out.ptrs)  # misaligned pointers
        both(256, codec, 2, 1024, sc, cl=odd.ptrs, cl_out=odd_out.ptrs)
    both(256, FP8, 1, 0, None)  # fp8 without a scales vector
    both(256, FP8, 1, 0, [1.0] * (n - 1))  # one scale short
    both(256, FP8, 1, 0, [1.0] * (n + 1), off=2)  # long enough only without the offset
    both(32, MXFP4, 1, 0)  # 16 elements: passes segments_legal, the launcher turns it down
    jobs.append(([], [], 256, NONE, True, 1, 0, None, 0))  # nothing to do

    results, _ = shard_run((2, 1, CAP), jobs)
    assert len(results) == len(jobs)
    for k, r in enumerate(results[:-1]):
        refused = not r["submitted"] and r["done_calls"] == 0
        failed = r["done_calls"] == 1 and not r["ok"]
        assert refused or failed, (k, jobs[k][2:7], r)
    r = results[-1]
    assert (r["submitted"], r["done_calls"], r["ok"]) == (True, 1, True), r
    # the 16-element mxfp4 page is the launcher's to refuse: reported, not dropped
    for r in results[-3:-1]:
        assert (r["submitted"], r["done_calls"], r["ok"]) == (True, 1, False), r
    assert bool((pool.t == SENTINEL).all()), "a refused store wrote"
    assert out.untouched() and odd_out.untouched(), "a refused load wrote"


# ---------------------------------------------------------------------------
# 5. fabric staging
# ---------------------------------------------------------------------------
BIG = (11 << 20) + 16
FABRIC_SHAPES = (
    [(48, n) for n in (D - 1, D, D + 1, 2 * D + 1)]  # the descriptor bound; three chunks
    + [(1000, 40)]  # not a multiple of 16: the byte kernel
    + [(BIG, n) for n in (2, 3, 5)]  # two blocks per chunk, the stage not divided evenly
    + [(B, 3)]  # one block per chunk
    + [(B + 16, 2)]  # larger than the stage: the per-block copy
)


@pytest.mark.parametrize("bs,n", FABRIC_SHAPES)
def test_fabric_staging(bs, n):
    """PUT: host bytes at shuffled offsets with gaps -> device blocks, guards
    intact. GET: pattern-filled device blocks -> a sentinel-filled host
    buffer, gap bytes untouched."""
    # Pool blocks are 16-byte aligned whenever the block size is a multiple of
    # 16 — the pool's guarantee, which fabric_run_gpu relies on when it picks
    # the vector kernel by the size alone. Other sizes get every misalignment.
    mis = 0 if bs % 16 == 0 else np.arange(n) % 16
    rs = np.random.RandomState(n)
    gap = 5
    offs = [int(o) for o in 3 + rs.permutation(n).astype(np.int64) * (bs + gap)]
    size = 3 + n * (bs + gap)
    host = rs.randint(0, 256, size, dtype=np.uint8)
    host_before = host.copy()
    back = np.full(size, SENTINEL, dtype=np.uint8)
    put_dst = Region(n, bs, misalign=mis, fill="sentinel", seed=1)
    get_src = Region(n, bs, misalign=mis, fill="pattern", seed=2)
    get_before = get_src.t.clone()
    assert all(0 <= o and o + bs <= size for o in offs)

    _, results = shard_run((1, 1, CAP), fabric_jobs=[
        (True, host, put_dst.ptrs, offs, bs),
        (False, back, get_src.ptrs, offs, bs),
    ])
    assert results == [(1, True), (1, True)], results

    want = torch.from_numpy(np.stack([host_before[o:o + bs] for o in offs]))
    _same(put_dst.blocks().cpu(), want, f"put bs={bs} n={n}")
    assert put_dst.guards_intact(), "put wrote outside the blocks"
    assert np.array_equal(host, host_before), "put wrote the host buffer"

    blocks = get_src.blocks().cpu().numpy()
    covered = np.zeros(size, dtype=bool)
    for i, o in enumerate(offs):
        assert np.array_equal(back[o:o + bs], blocks[i]), f"get bs={bs} n={n}: block {i}"
        covered[o:o + bs] = True
    assert bool((back[~covered] == SENTINEL).all()), "get wrote gap bytes"
    assert torch.equal(get_src.t, get_before), "get modified the device blocks"
