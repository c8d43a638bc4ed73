"""Model of the block allocator (csrc/core/mempool.*) and checked drivers.

`PoolModel` is the plain statement of what a pool is: the set of used block
indices, kept as one Python integer (bit i set = block i used), plus the state
of the contiguous-scan guard as mempool.h states it: a scan for more than one
block that finds nothing disarms `allocate_contiguous` for runs of more than
one block, and the 4096th successful `deallocate` after that arms it again. A
request larger than the number of free blocks is refused without a scan and
leaves the guard alone. The model knows nothing of words, summary bits,
cursors or free lists, and it never predicts WHERE a run is placed: first fit
from a cursor is policy, any free run is a correct answer.

`CheckedPool` wraps a `_native._TestPool` and a `PoolModel` and checks every
operation on the way through:

  a successful allocation   pointer block-aligned and inside the arena, all
                            its blocks free in the model (no overlap, nothing
                            at or past total_blocks())
  completeness              allocate / allocate_below return 0 iff the model
                            has no free run (wholly below the limit);
                            allocate_contiguous returns 0 iff there is no run,
                            the request exceeds the free count, or the guard
                            is disarmed
  deallocate                true iff size > 0, the pointer is aligned and in
                            range and every block of the run is used; on false
                            nothing changes
  state                     used_blocks() and bitmap() equal the model, tail
                            bits of the last word set

`CheckedMM` does the same for `_native._TestMM` with one model per pool.
`random_run` drives a CheckedPool with a seeded mix of all entry points and
returns the counts that the coverage check of tests/test_pool_model.py needs.
"""

import random
from collections import Counter

from infinistore_amd import _native as n

M64 = (1 << 64) - 1
REARM_FREES = 4096  # mempool.cpp: frees after a failed scan until the next one


def blocks_of(size, block):
    return -(-size // block)


class PoolModel:
    def __init__(self, n_blocks):
        self.n_blocks = n_blocks
        self.bits = 0  # bit i: block i used
        self.contig_ok = True
        self.frees_since_fail = 0
        self.rearms = 0

    def used(self):
        return bin(self.bits).count("1")

    def free_mask(self, limit=None):
        lim = self.n_blocks if limit is None else max(0, min(limit, self.n_blocks))
        return ~self.bits & ((1 << lim) - 1)

    def has_run(self, nb, limit=None):
        """Is there a free run of nb blocks, wholly below `limit`?"""
        if nb < 1 or nb > self.n_blocks:
            return False
        x, k = self.free_mask(limit), 1
        while k < nb and x:  # x keeps bit i iff blocks i .. i+k-1 are free
            s = min(k, nb - k)
            x &= x >> s
            k += s
        return x != 0

    def largest_free_run(self):
        free = self.free_mask()
        s = bin(free | (1 << self.n_blocks))[3:]  # n_blocks digits, '1' = free
        return max(map(len, s.split("0")))

    def is_free(self, start, nb):
        mask = ((1 << nb) - 1) << start
        return start + nb <= self.n_blocks and not self.bits & mask

    def is_used(self, start, nb):
        mask = ((1 << nb) - 1) << start
        return start + nb <= self.n_blocks and self.bits & mask == mask

    def take(self, start, nb):
        assert nb >= 1 and self.is_free(start, nb), (start, nb)
        self.bits |= ((1 << nb) - 1) << start

    def release(self, start, nb):
        assert nb >= 1 and self.is_used(start, nb), (start, nb)
        self.bits &= ~(((1 << nb) - 1) << start)
        if not self.contig_ok:
            self.frees_since_fail += 1
            if self.frees_since_fail >= REARM_FREES:
                self.contig_ok = True
                self.rearms += 1

    def scan_failed(self, total):
        if total > 1:
            self.contig_ok = False
            self.frees_since_fail = 0

    def words(self):
        """The used-bitmap as 64-bit words, the tail of the last word set."""
        n_words = (self.n_blocks + 63) // 64
        full = self.bits | (((1 << (n_words * 64 - self.n_blocks)) - 1) << self.n_blocks)
        return [(full >> (64 * i)) & M64 for i in range(n_words)]


class CheckedPool:
    """A _TestPool of n_blocks blocks (plus `slack` bytes that fill no block)
    next to its model. Methods return the first block index, or None."""

    def __init__(self, n_blocks, block=16, slack=0):
        assert 0 <= slack < block
        self.block, self.size = block, n_blocks * block + slack
        self.p = n._TestPool(self.size, block)
        self.base = self.p.base()
        self.m = PoolModel(n_blocks)
        assert self.p.total_blocks() == n_blocks
        self.check_state()

    def ptr(self, start):
        return self.base + start * self.block

    def check_state(self):
        assert self.p.used_blocks() == self.m.used(), (self.p.used_blocks(), self.m.used())
        got, want = self.p.bitmap(), self.m.words()
        assert got == want, [(i, hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want))
                             if g != w][:4]

    def _landed(self, ptr, nb, what):
        off = ptr - self.base
        assert 0 <= off < self.size and off % self.block == 0, (what, hex(ptr))
        start = off // self.block
        assert self.p.block_index_of(ptr) == start
        assert self.m.is_free(start, nb), f"{what}: blocks {start}..{start + nb - 1} not all free"
        self.m.take(start, nb)
        return start

    def allocate(self, size):
        nb = blocks_of(size, self.block)
        expect = self.m.has_run(nb)
        ptr = self.p.allocate(size)
        what = f"allocate({size}) = {nb} blocks"
        assert (ptr != 0) == expect, \
            f"{what}: returned {ptr:#x}, the model has {'a' if expect else 'no'} free run"
        start = self._landed(ptr, nb, what) if ptr else None
        self.check_state()
        return start

    def allocate_below(self, size, limit):
        nb = blocks_of(size, self.block)
        expect = self.m.has_run(nb, limit)
        ptr = self.p.allocate_below(size, limit)
        what = f"allocate_below({size}, {limit}) = {nb} blocks"
        assert (ptr != 0) == expect, \
            f"{what}: returned {ptr:#x}, the model has {'a' if expect else 'no'} run below"
        start = None
        if ptr:
            start = self._landed(ptr, nb, what)
            assert start + nb <= limit, (what, start)
        self.check_state()
        return start

    def allocate_contiguous(self, size, count):
        nb = blocks_of(size, self.block)
        total = nb * count
        m = self.m
        scans = total >= 1 and total <= m.n_blocks - m.used() and (total == 1 or m.contig_ok)
        expect = scans and m.has_run(total)
        ptr = self.p.allocate_contiguous(size, count)
        what = f"allocate_contiguous({size}, {count}) = {total} blocks"
        assert (ptr != 0) == expect, \
            f"{what}: returned {ptr:#x}; model: run {m.has_run(total)}, guard armed {m.contig_ok}"
        start = None
        if ptr:
            start = self._landed(ptr, total, what)
        elif scans:
            m.scan_failed(total)
        self.check_state()
        return start

    def deallocate_ptr(self, ptr, size):
        """deallocate at any address; returns what the pool returned."""
        off = ptr - self.base
        nb = blocks_of(size, self.block)
        ok = (size > 0 and 0 <= off < self.size and off % self.block == 0
              and self.m.is_used(off // self.block, nb))
        got = self.p.deallocate(ptr, size)
        assert got == ok, f"deallocate({off}/{self.block}, {size}) returned {got}, model {ok}"
        if ok:
            self.m.release(off // self.block, nb)
        self.check_state()  # on false nothing changed
        return got

    def deallocate(self, start, nb, size=None):
        return self.deallocate_ptr(self.ptr(start), nb * self.block if size is None else size)


class CheckedMM:
    """A _TestMM next to one PoolModel per pool. allocate() checks every page
    it is given; it does not predict success (placement across fragmented
    pools is policy), the directed tests do that where it is decidable."""

    def __init__(self, pools, block=16):
        self.block = block
        self.mm = n._TestMM()
        self.models, self.bases = [], []
        for nb in pools:
            idx = self.mm.add_pool(nb * block, block)
            assert idx == len(self.models)
            self.models.append(PoolModel(nb))
            self.bases.append(self.mm.pool_base(idx))
        assert self.mm.num_pools() == len(pools)
        assert self.mm.total_blocks() == sum(pools)
        self.check_state()

    def check_state(self):
        for i, m in enumerate(self.models):
            assert self.mm.pool_used_blocks(i) == m.used(), (i, m.used())
        assert self.mm.used_blocks() == sum(m.used() for m in self.models)

    def locate(self, ptr, pool):
        off = ptr - self.bases[pool]
        assert 0 <= off < self.models[pool].n_blocks * self.block and off % self.block == 0
        return off // self.block

    def allocate(self, size, count):
        """[(pool, start)] in callback order, or None."""
        nb = blocks_of(size, self.block)
        pages, calls = self.mm.allocate(size, count)
        if pages is None:
            assert calls == 0, f"failed allocation ran the callback {calls} times"
            self.check_state()  # partial pages undone
            return None
        assert calls == count == len(pages)
        out = []
        for ptr, pool in pages:
            start = self.locate(ptr, pool)
            assert self.models[pool].is_free(start, nb), (pool, start, nb)
            self.models[pool].take(start, nb)
            out.append((pool, start))
        self.check_state()
        return out

    def deallocate(self, pool, start, nb):
        ok = self.models[pool].is_used(start, nb)
        got = self.mm.deallocate(self.bases[pool] + start * self.block, nb * self.block, pool)
        assert got == ok
        if ok:
            self.models[pool].release(start, nb)
        self.check_state()
        return got

    def plan_and_apply(self, pages, strangers=()):
        """plan_moves over pages [(pool, start, nb)] (all of them live) and the
        foreign pointers `strangers`; checks every move against the model,
        applies it (free old, keep new) and returns the pages afterwards."""
        before = [self.mm.pool_largest_free_run(i) for i in range(len(self.models))]
        assert before == [m.largest_free_run() for m in self.models]
        by_ptr = {self.bases[p] + s * self.block: (p, s, nb) for p, s, nb in pages}
        arg = [(ptr, nb * self.block) for ptr, (_, _, nb) in by_ptr.items()]
        arg += [(ptr, self.block) for ptr in strangers]
        moves = self.mm.plan_moves(arg)
        result = dict(by_ptr)
        for old, new, size, pool in moves:
            assert old in result and old in by_ptr, "moved twice, or a pointer nobody owns"
            p, s, nb = by_ptr[old]
            assert pool == p and size == nb * self.block
            new_start = self.locate(new, pool)  # inside the same pool
            assert new_start < s, (new_start, s)
            # free in the model, where every live page still sits at its OLD
            # place and earlier moves' new places are taken
            assert self.models[pool].is_free(new_start, nb), (pool, new_start, nb)
            self.models[pool].take(new_start, nb)
            del result[old]
            result[new] = (p, new_start, nb)
        self.check_state()
        for old, new, size, pool in moves:
            _, s, nb = by_ptr[old]
            assert self.deallocate(pool, s, nb)
        after = [self.mm.pool_largest_free_run(i) for i in range(len(self.models))]
        assert after == [m.largest_free_run() for m in self.models]
        return list(result.values()), before, after


# ---- random runs -------------------------------------------------------------
OP_KINDS = ("allocate", "allocate_contiguous", "allocate_below", "free_whole", "free_partial",
            "free_page", "free_bad")

# (pool blocks, seed): committed; tests/test_pool_model.py checks that each
# meets the coverage conditions. A seed that falls short is replaced by
# another seed, the conditions stay.
# (pool blocks, seed, operations): committed; tests/test_pool_model.py checks
# that each meets the coverage conditions. A seed that falls short is replaced
# by another seed, the conditions stay. The long runs free often enough after
# a failed contiguous scan for the guard to arm again.
RANDOM_RUNS = ((100, 11, 4000), (100, 12, 20000), (128, 21, 4000), (128, 22, 20000),
               (1000, 31, 4000), (1000, 32, 20000), (4200, 41, 4000), (4200, 42, 20000))


def random_run(n_blocks, seed, n_ops):
    """Drives a CheckedPool; returns (Counter of performed kinds, Counter of
    other events). Occupancy is steered to stay mostly within 70..100 %."""
    rng = random.Random(f"pool-{n_blocks}-{seed}")
    block = rng.choice((16, 48, 4096)) if n_blocks <= 1000 else 16
    cp = CheckedPool(n_blocks, block, slack=rng.choice((0, block - 1)))
    m = cp.m
    extents = []  # live (start, nb): each may be freed whole or in part
    kinds, events = Counter(), Counter()
    sizes = [1, 1, 1, 2, 2, 2, 3, 3, 4, 5, 8] + ([7, 16, 33, 64, 65, 130] if n_blocks > 128 else [])
    free_kinds = ("free_whole",) * 3 + ("free_partial",) * 2 + ("free_page",) * 2 + ("free_bad",)

    def some_size(nb):
        return (nb - 1) * block + rng.choice((1, block - 1, block, block))

    def landed(start, nb, pages=1):
        if start is None:
            events["alloc_refused"] += 1
            return
        if nb * pages > 1 and occ >= 0.9:
            events["multi_block_at_90"] += 1
        extents.extend((start + i * nb, nb) for i in range(pages))

    for _ in range(n_ops):
        occ = m.used() / n_blocks
        in_band = 0.7 <= occ
        events["in_band"] += in_band
        events["at_90"] += occ >= 0.9
        p_alloc = 0.95 if occ < 0.72 else 0.75 if occ < 0.93 else 0.45 if occ < 0.98 else 0.15
        if rng.random() < p_alloc or not extents:
            kind = rng.choice(OP_KINDS[:3])
            nb = rng.choice(sizes)
            if kind == "allocate":
                landed(cp.allocate(some_size(nb)), nb)
            elif kind == "allocate_contiguous":
                pages = rng.choice((1, 2, 2, 3, 4, 8))
                nb = rng.choice((1, 1, 2, 3))
                landed(cp.allocate_contiguous(some_size(nb), pages), nb, pages)
            else:
                limit = rng.choice((0, 1, 63, 64, 65, n_blocks - 1, n_blocks, n_blocks + 70)
                                   + tuple(rng.randrange(n_blocks // 2, n_blocks + 1)
                                           for _ in range(16)))
                landed(cp.allocate_below(some_size(nb), limit), nb)
        else:
            kind = rng.choice(free_kinds)
            i = rng.randrange(len(extents))
            start, nb = extents[i]
            if kind == "free_partial" and nb < 2:
                multi = [j for j, e in enumerate(extents) if e[1] > 1]
                if not multi:
                    kind = "free_whole"
                else:
                    i = rng.choice(multi)
                    start, nb = extents[i]
            if kind == "free_whole":
                assert cp.deallocate(start, nb, some_size(nb))
                extents.pop(i)
            elif kind == "free_partial":
                a = rng.randrange(nb)
                b = rng.randint(a + 1, nb if a else nb - 1)
                assert cp.deallocate(start + a, b - a)
                extents.pop(i)
                extents.extend(e for e in ((start, a), (start + b, nb - b)) if e[1])
            elif kind == "free_page":  # one block of a run, as a page of a batch is
                a = rng.randrange(nb)
                assert cp.deallocate(start + a, 1)
                extents.pop(i)
                extents.extend(e for e in ((start, a), (start + a + 1, nb - a - 1)) if e[1])
            else:
                bad = rng.randrange(6)
                if bad == 0:
                    got = cp.deallocate_ptr(cp.ptr(start) + rng.randrange(1, block), block)
                elif bad == 1:
                    got = cp.deallocate_ptr(cp.base + cp.size + rng.randrange(4) * block, block)
                elif bad == 2:
                    got = cp.deallocate_ptr(cp.base - block, block)
                elif bad == 3:
                    got = cp.deallocate(start, nb, size=0)
                elif bad == 4:  # runs over the end of the pool
                    got = cp.deallocate(start, n_blocks - start + 1)
                else:  # a run with a free block in it, if there is one
                    free = [s for s in (start - 1, start + nb) if 0 <= s < n_blocks
                            and m.is_free(s, 1)]
                    if free:
                        lo = min(start, free[0])
                        got = cp.deallocate(lo, nb + 1)
                    else:
                        got = cp.deallocate_ptr(cp.ptr(start) + 1, block)
                assert got is False
                events["free_refused"] += 1
        kinds[kind] += 1
    events["rearms"] = m.rearms
    # everything still live is freeable, and then the pool is empty
    for start, nb in extents:
        assert cp.deallocate(start, nb)
    assert m.used() == 0 and cp.p.used_blocks() == 0
    assert cp.p.largest_free_run() == n_blocks
    return kinds, events
