"""Tensor-set jobs through a real GPU `Shard` (`_dbg_shard_run_tset`): the
chunk loop at 5 descriptors per slot, fan-out at kFanChunk + 1 blocks over two
streams, all three codecs, that such a job never takes the inline-argument
path, and every refusal of `submit_copy`.

The client side is a `TensorSetArena` (every tensor its own guarded
`SegArena`, the table not in address order), the pool side a `Region`; the
oracle is the concatenated page through the references of the kernel tests,
bit for bit (fp8 scales as float32 bytes), guards intact, source unmodified.
At most two streams per Shard: with torch's the process stays within four
hardware queues."""

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
from _tset_refs import TensorSetArena

pytestmark = pytest.mark.gpu

DEV = 0
NONE, FP8, MXFP4 = 0, 1, 2  # codec ids
T = 30  # timeout_s: a guard against a hang, not a measurement
F = _native._SHARD_FAN_CHUNK
POISON = float(np.float32(-12345.678))
CAP = 5


def shard_run(opts, jobs, tsets, slices=None):
    """opts = (streams, slots per stream, descriptors per slot). Everything
    torch wrote is synchronized first: the Shard's streams do not wait for
    torch's."""
    assert opts[0] <= 2
    torch.cuda.synchronize()
    return _native._dbg_shard_run_tset(DEV, opts[0], opts[1], opts[2], list(jobs), list(tsets),
                                       1, T, slices)


def assert_done_ok(res, what):
    assert (res["submitted"], res["done_calls"], res["ok"]) == (True, 1, True), (what, res)


def _same(a, b, what):
    if not torch.equal(a, b):
        bad = (a != b).nonzero()[0].tolist()
        raise AssertionError(f"{what}: block {bad[0]} byte {bad[1]} differs "
                             f"({int((a != b).sum())} bytes wrong)")


def fp8_pages(n, elems, seed):
    """Every page with its own absmax, exact in bf16, so a scale stored
    against the wrong page, chunk or sub-job changes codes."""
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(n)
    amax = (2.0 * (i % 128) + 1.0) * torch.pow(2.0, (i // 128 - 16).float())
    assert amax.unique().numel() == n
    pages = ((torch.rand(n, elems, generator=g) - 0.5) * amax[:, None]).to(torch.bfloat16)
    # the absmax in the LAST element: the last tensor's part
    pages[i, elems - 1] = (amax * torch.where(i % 2 == 0, 1.0, -1.0)).to(torch.bfloat16)
    assert torch.equal(pages.float().abs().max(dim=1).values, amax)
    return pages


def mx_pages(n, elems, seed):
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(2.0, torch.randint(-20, 20, (n, elems // 32, 1), generator=g).float())
    x = torch.randn(n, elems // 32, 32, generator=g) * mag
    return x.reshape(n, elems).to(torch.bfloat16)


class Case:
    """One store and one load of n pages over G tensors of `per` segments of
    `seg_bytes`, for one codec."""

    OFF, EXTRA = 3, 7  # fp8: scales_off into n + EXTRA poison values

    def __init__(self, codec, G, per, n, seg_bytes, seed):
        self.what = f"codec={codec} G={G} S/G={per} n={n} seg={seg_bytes}"
        self.codec, self.n, self.per = codec, n, per
        self.src = TensorSetArena(G, n, per, seg_bytes, fill="pattern", seed=seed)
        self.out = TensorSetArena(G, n, per, seg_bytes, fill="sentinel", seed=seed + 2)
        self.S, self.stride, self.page = self.src.n_segments, self.src.stride, self.src.nbytes
        assert self.out.stride == self.stride
        elems = self.page // 2
        if codec == NONE:
            g = torch.Generator().manual_seed(seed)
            pages = torch.randint(0, 256, (n, self.page), dtype=torch.uint8, generator=g)
            self.want_stored = pages
            stored = self.page
        elif codec == FP8:
            pages = fp8_pages(n, elems, seed)
            self.want_stored, self.want_scales = fp8_quant_ref(pages)
            assert np.unique(self.want_scales).size == n
            self.want_back = bf16_bits(fp8_dequant_ref(self.want_stored, self.want_scales))
            stored = elems
        else:
            pages = mx_pages(n, elems, seed)
            self.want_stored = torch.from_numpy(quant_ref(bf16_bits(pages)))
            self.want_back = dequant_ref(self.want_stored.numpy(), elems)
            stored = stored_bytes(elems)
        self.src.set_pages(pages)
        self.pool = Region(n, stored, fill="sentinel", seed=seed + 1)
        self.snap = self.src.snapshot()

    def tset(self, arena):
        return (arena.bases, self.per)

    def store_job(self):
        sc = [POISON] * (self.n + self.EXTRA) if self.codec == FP8 else None
        return ((self.src.offsets, self.pool.ptrs, self.page, self.codec, True, self.S,
                 self.stride, sc, self.OFF if sc else 0), self.tset(self.src))

    def check_store(self, res):
        assert_done_ok(res, self.what)
        got = self.pool.blocks().cpu()
        if self.codec == FP8:
            scales = np.asarray(res["scales"], dtype=np.float32)
            want = np.full(self.n + self.EXTRA, POISON, dtype=np.float32)
            want[self.OFF:self.OFF + self.n] = self.want_scales
            assert scales.tobytes() == want.tobytes(), (
                f"{self.what}: scales differ at {np.flatnonzero(scales != want)[:8]}")
            assert_codes_equal(got.numpy(), self.want_stored.numpy(), self.what)
            self.scales = res["scales"]
        else:
            _same(got, self.want_stored, self.what)
        assert self.pool.guards_intact(), f"{self.what}: bytes outside the pool blocks written"
        assert self.src.unchanged_since(self.snap), f"{self.what}: the source was modified"

    def load_job(self):
        self.pool_before = self.pool.t.clone()
        sc = self.scales if self.codec == FP8 else None
        return ((self.pool.ptrs, self.out.offsets, self.page, self.codec, False, self.S,
                 self.stride, sc, self.OFF if sc else 0), self.tset(self.out))

    def check_load(self, res):
        assert_done_ok(res, self.what)
        if self.codec == NONE:
            _same(self.out.pages(), self.pool.blocks(), self.what + " load")
        else:
            got = self.out.pages().cpu().numpy().view(np.uint16)
            assert_bf16_bits_equal(got, self.want_back, self.what + " load")
        assert self.out.guards_intact(), f"{self.what}: bytes outside the segments written"
        assert torch.equal(self.pool.t, self.pool_before), f"{self.what}: the source was modified"


def run_cases(opts, cases):
    """All stores through one Shard, checked; then all loads through another."""
    jobs = [c.store_job() for c in cases]
    results = shard_run(opts, [j for j, _ in jobs], [t for _, t in jobs])
    assert len(results) == len(cases)
    for c, r in zip(cases, results):
        c.check_store(r)
    jobs = [c.load_job() for c in cases]
    results = shard_run(opts, [j for j, _ in jobs], [t for _, t in jobs])
    for c, r in zip(cases, results):
        c.check_load(r)


# the smallest legal segment of each codec, and one that is several lanes' work
SEG = {NONE: (16, 272), FP8: (16, 1040), MXFP4: (64, 192)}
NS = (4, 5, 6, 10, 11)  # below, at and above whole chunks of 5


@pytest.mark.parametrize("G,per", [(2, 1), (3, 2)])
@pytest.mark.parametrize("codec", [NONE, FP8, MXFP4])
@pytest.mark.parametrize("opts", [(1, 1, CAP), (2, 1, CAP)])
def test_chunk_loop(opts, codec, G, per):
    run_cases(opts, [Case(codec, G, per, n, SEG[codec][k % 2], 100 * codec + n)
                     for k, n in enumerate(NS)])


def test_chunk_loop_byte_kernel():
    """One misaligned base: plain pages take the byte kernel, chunk by chunk."""
    n, G, per, seg = 11, 3, 2, 528
    src = TensorSetArena(G, n, per, seg, misalign=[0, 5, 0], fill="pattern", seed=1)
    pool = Region(n, src.nbytes, fill="sentinel", seed=2)
    job = (src.offsets, pool.ptrs, src.nbytes, NONE, True, G * per, src.stride, None, 0)
    (res,) = shard_run((1, 1, CAP), [job], [(src.bases, per)])
    assert_done_ok(res, "byte")
    _same(pool.blocks(), src.pages(), "byte kernel through the chunk loop")
    assert pool.guards_intact()


@pytest.mark.parametrize("codec", [NONE, FP8, MXFP4])
def test_fanout_two_streams(codec):
    """F + 1 blocks over two streams, 1000 descriptors per slot: one sub-job of
    F blocks in five chunks and one of a single block, each with the table.
    fp8's distinct scales cross both sub-job and chunk boundaries."""
    assert -(-F // 1000) == 5
    run_cases((2, 1, 1000), [Case(codec, 2, 1, F + 1, SEG[codec][0], 7 + codec)])


def test_sixteen_aligned_blocks_do_not_go_inline():
    """A load of 16 aligned 32-byte pages over two tensors, 5 descriptors per
    slot, where block 5's pool source is the 32 bytes at block 0's destination
    in tensor 0: the 16 bytes block 0 writes there, then 16 guard bytes. The
    chunk loop moves blocks 0-4 in one launch and block 5 in the next, so
    block 5 reads block 0's NEW bytes. The inline kernel, which a contiguous
    job of this size takes, would issue every load before any store and block 5
    would get the sentinel."""
    n, G = 16, 2
    out = TensorSetArena(G, n, 1, 16, fill="sentinel", seed=3)
    pool = Region(n, 32, fill="pattern", seed=4)
    src = list(pool.ptrs)
    src[5] = out.bases[0] + out.offsets[0]
    assert all(p % 16 == 0 for p in src + out.bases + out.offsets)
    job = (src, out.offsets, 32, NONE, False, 2, 0, None, 0)
    (res,) = shard_run((1, 1, CAP), [job], [(out.bases, 1)])
    assert_done_ok(res, "16 blocks")
    got, blocks = out.pages().cpu(), pool.blocks().cpu()
    assert torch.equal(got[5, :16], blocks[0, :16]), "the job went through the inline kernel"
    assert bool((got[5, 16:] == SENTINEL).all())
    keep = [i for i in range(n) if i != 5]
    assert torch.equal(got[keep], blocks[keep]) and out.guards_intact()


def test_refusals():
    """Every job is refused at submit or reported failed, and writes nothing."""
    n, G, per, seg = 3, 2, 2, 256
    client = TensorSetArena(G, n, per, seg, fill="pattern", seed=1)
    out = TensorSetArena(G, n, per, seg, fill="sentinel", seed=2)
    odd = TensorSetArena(G, n, per, seg, misalign=[0, 8], fill="pattern", seed=3)
    odd_out = TensorSetArena(G, n, per, seg, misalign=[8, 0], fill="sentinel", seed=4)
    shifted = TensorSetArena(G, n, per, seg, off_shift=4104, fill="pattern", seed=5)
    shifted_out = TensorSetArena(G, n, per, seg, off_shift=4104, fill="sentinel", seed=6)
    pool = Region(n, 4 * seg, fill="sentinel", seed=7)
    src_pool = Region(n, 4 * seg, fill="pattern", seed=8)
    stride = client.stride
    scales = [1.0] * n
    jobs, tsets, slices = [], [], []

    def both(nbytes, codec, S, strd, bases_n=2, per_tensor=2, sc=None, cl=client, ou=out,
             sl=None):
        if sl is None:
            jobs.append((cl.offsets, pool.ptrs, nbytes, codec, True, S, strd, sc, 0))
            tsets.append(((cl.bases * 65)[:bases_n], per_tensor))
            slices.append(None)
        jobs.append((src_pool.ptrs, ou.offsets, nbytes, codec, False, S, strd, sc, 0))
        tsets.append(((ou.bases * 65)[:bases_n], per_tensor))
        slices.append(sl)

    for codec, sc in ((NONE, None), (FP8, scales), (MXFP4, None)):
        both(4 * seg, codec, 4, stride, bases_n=0, sc=sc)  # no tensors
        both(129 * 64, codec, 129, stride, bases_n=129, per_tensor=1, sc=sc)  # G = 129
        both(4 * seg, codec, 4, stride, bases_n=3, per_tensor=1, sc=sc)  # S % G
        both(4 * seg, codec, 0, stride, per_tensor=0, sc=sc)  # no segments
        both(4 * seg + 64, codec, 3 * 2, stride, per_tensor=3, sc=sc)  # page % S
        both(4 * seg, codec, 4, seg - 16, sc=sc)  # a tensor's segments overlap
        both(4 * seg, codec, 4, stride, per_tensor=1, sc=sc)  # segs_per_tensor is not S / G
        both(4 * seg, codec, 4, stride, sc=sc, sl=(4, 4096, 0, seg, 1024))  # with a slice
    for codec, group, sc in ((FP8, 16, scales), (MXFP4, 64, None)):
        both(4 * (2 * group + group // 2), codec, 4, stride, sc=sc)  # half a group per segment
        both(4 * seg, codec, 4, stride + 8, sc=sc)  # stride % 16
        both(4 * seg, codec, 4, stride, sc=sc, cl=odd, ou=odd_out)  # one base off by 8
        both(4 * seg, codec, 4, stride, sc=sc, cl=shifted, ou=shifted_out)  # offsets off by 8
    both(4 * seg, FP8, 4, stride)  # fp8 without a scales vector
    both(4 * seg, FP8, 4, stride, sc=[1.0] * (n - 1))  # one scale short

    results = shard_run((2, 1, CAP), jobs, tsets, slices)
    assert len(results) == len(jobs)
    for k, r in enumerate(results):
        refused = not r["submitted"] and r["done_calls"] == 0
        failed = r["done_calls"] == 1 and not r["ok"]
        assert refused or failed, (k, jobs[k][2:7], r)
    assert bool((pool.t == SENTINEL).all()), "a refused store wrote"
    assert out.untouched() and odd_out.untouched() and shifted_out.untouched(), (
        "a refused load wrote")
