"""The block allocator against its model (tests/_pool_model.py): directed
cases at the places where the two-level bitmap, the cursor, the single-block
free list and the contiguous-scan guard can go wrong, seeded random runs over
all four entry points, the multi-pool manager and compaction planning.

Every CheckedPool / CheckedMM call asserts, after the operation, that the
allocation lies in free blocks of the model, that refusal and success agree
with the model, and that used_blocks() and bitmap() equal it; a test body that
only calls them is therefore a test of those properties."""

import random

import pytest

from _pool_model import (OP_KINDS, RANDOM_RUNS, REARM_FREES, CheckedMM, CheckedPool,
                         random_run)

B = 16  # block size of the directed cases


def fill_singles(cp):
    """Takes every block with single-block allocations; the next one fails."""
    got = [cp.allocate(cp.block) for _ in range(cp.m.n_blocks)]
    assert sorted(got) == list(range(cp.m.n_blocks))
    assert cp.allocate(cp.block) is None
    return got


def full_pool_with_cursor(n_blocks, word):
    """A full pool whose scan cursor is word `word`: the last successful scan
    found the only free run, two blocks inside that word."""
    cp = CheckedPool(n_blocks, B)
    assert cp.allocate(n_blocks * B) == 0
    assert cp.deallocate(word * 64 + 1, 2)
    assert cp.allocate(2 * B) == word * 64 + 1
    return cp


# ---- cursor split --------------------------------------------------------------
def test_run_across_the_cursor_word_is_found():
    """A free run cut by the word boundary at the cursor: the pass from the
    cursor to the end sees its upper part, the pass from 0 to the cursor its
    lower part."""
    cp = CheckedPool(128, B)
    assert cp.allocate(60 * B) == 0
    assert cp.allocate(10 * B) == 60
    assert cp.allocate(58 * B) == 70  # the cursor is word 1 now
    assert cp.deallocate(60, 10)
    assert cp.p.largest_free_run() == 10
    assert cp.allocate(10 * B) == 60
    assert cp.deallocate(60, 10)
    assert cp.allocate_contiguous(B, 10) == 60


def test_run_across_the_cursor_word_through_mm():
    mm = CheckedMM([128], B)
    assert mm.allocate(60 * B, 1) == [(0, 0)]
    assert mm.allocate(10 * B, 1) == [(0, 60)]
    assert mm.allocate(58 * B, 1) == [(0, 70)]
    assert mm.deallocate(0, 60, 10)
    # one run for the batch, pages in order at the block stride
    assert mm.allocate(B, 10) == [(0, 60 + i) for i in range(10)]


@pytest.mark.parametrize("entry", ["allocate", "allocate_contiguous"])
@pytest.mark.parametrize("lo,hi", [(63, 65), (62, 65), (63, 66), (10, 71), (60, 192)])
def test_run_spanning_the_cursor_boundary(entry, lo, hi):
    """Blocks lo..hi-1 free around the boundary of word 1, the cursor on word
    1: a single block on either side, two on one side, and runs longer than a
    word before and after the boundary."""
    cp = full_pool_with_cursor(192, 1)
    assert cp.deallocate(lo, hi - lo)
    nb = hi - lo
    if entry == "allocate":
        assert cp.allocate(nb * B) == lo
    else:
        assert cp.allocate_contiguous(nb * B, 1) == lo


@pytest.mark.parametrize("word", [0, 1, 2])
def test_every_run_is_found_from_every_cursor(word):
    """All runs of 2..70 blocks at every start of a 192-block pool, the cursor
    on each word in turn."""
    cp = full_pool_with_cursor(192, word)
    for nb in (2, 3, 64, 65, 70):
        for start in range(0, 192 - nb + 1, 1 if nb < 4 else 7):
            assert cp.deallocate(start, nb)
            assert cp.allocate(nb * B) == start
            # put the cursor back where the case wants it
            assert cp.deallocate(word * 64 + 1, 2)
            assert cp.allocate(2 * B) == word * 64 + 1


# ---- tail blocks ---------------------------------------------------------------
@pytest.mark.parametrize("slack", [0, B - 1])
@pytest.mark.parametrize("n_blocks", [1, 63, 64, 65, 100, 4097])
def test_tail_blocks_are_never_handed_out(n_blocks, slack):
    cp = CheckedPool(n_blocks, B, slack)
    # a run ending on the last block, by each scanning entry; one more fails
    for k in {1, min(n_blocks, 3), n_blocks}:
        if n_blocks - k:
            assert cp.allocate((n_blocks - k) * B) == 0
        assert cp.allocate(k * B) == n_blocks - k
        assert cp.deallocate(n_blocks - k, k)
        assert cp.allocate_contiguous(B, k) == n_blocks - k
        assert cp.deallocate(n_blocks - k, k)
        assert cp.allocate_below(k * B, n_blocks + 64) == n_blocks - k
        assert cp.deallocate(n_blocks - k, k)
        assert cp.allocate((k + 1) * B) is None
        assert cp.allocate_contiguous(B, k + 1) is None
        assert cp.allocate_below((k + 1) * B, n_blocks + 64) is None
        if n_blocks - k:
            assert cp.deallocate(0, n_blocks - k)
    # scanning path, then the free-list path: every block once, never more
    got = fill_singles(cp)
    for s in got:
        assert cp.deallocate(s, 1)
    assert cp.p.free_hints() == n_blocks
    fill_singles(cp)
    # the first address past the last block is no block
    assert cp.deallocate_ptr(cp.ptr(n_blocks), B) is False
    assert cp.deallocate(n_blocks - 1, 2) is False


# ---- summary-word skip ---------------------------------------------------------
def test_freed_blocks_under_full_summary_words_are_found():
    cp = CheckedPool(8256, B)  # 129 words, three summary words
    assert cp.allocate(8192 * B) == 0
    assert cp.allocate(64 * B) == 8192  # full; the cursor is the last word
    # one block inside the region that a scan from word 0 jumps over
    assert cp.deallocate(5000, 1)
    assert cp.allocate_contiguous(B, 1) == 5000  # by a scan, not from the free list
    assert cp.deallocate(5000, 1)
    assert cp.allocate_below(B, 8256) == 5000
    # two blocks across words 63 | 64, the border of summary words 0 and 1
    assert cp.deallocate(4095, 2)
    assert cp.allocate(2 * B) == 4095
    assert cp.deallocate(4095, 2)
    assert cp.allocate_below(2 * B, 4097) == 4095
    assert cp.allocate_below(2 * B, 8256) is None
    # the same with the cursor in front of the skipped region
    assert cp.deallocate(1, 2)
    assert cp.allocate(2 * B) == 1  # the cursor is word 0
    assert cp.deallocate(8200, 2)   # behind it: words 1..127 are jumped over
    assert cp.allocate(2 * B) == 8200
    assert cp.deallocate(1, 2)
    assert cp.allocate(2 * B) == 1
    assert cp.deallocate(8191, 2)   # words 127 | 128
    assert cp.allocate(2 * B) == 8191
    assert cp.deallocate(1, 2)
    assert cp.allocate(2 * B) == 1
    assert cp.deallocate(4096 + 64 * 17 + 5, 1)
    assert cp.allocate_contiguous(B, 1) == 4096 + 64 * 17 + 5


# ---- stale hints of the single-block free list ---------------------------------
def test_hint_of_a_block_taken_by_a_run_is_dropped():
    cp = CheckedPool(128, B)
    fill_singles(cp)
    i = 70
    assert cp.deallocate(i, 1) and cp.deallocate(i + 1, 1)
    assert cp.allocate(2 * B) == i  # the hints for i and i + 1 are stale now
    assert cp.allocate(B) is None   # full: neither i nor i + 1 may come back
    assert cp.deallocate(3, 1)
    assert cp.allocate(B) == 3


def test_duplicate_hint_is_dropped():
    cp = CheckedPool(100, B)
    fill_singles(cp)
    assert cp.deallocate(41, 1)
    assert cp.allocate_contiguous(B, 1) == 41  # by a scan; the hint stays
    assert cp.deallocate(41, 1)                # a second hint for block 41
    assert cp.p.free_hints() == 2
    assert cp.allocate(B) == 41
    assert cp.allocate(B) is None  # the second pop finds the bit set
    assert cp.p.free_hints() == 0


def test_hints_stay_within_the_block_count():
    cp = CheckedPool(64, B)
    fill_singles(cp)
    for cycle in range(5 * 64):
        i = cycle * 7 % 64
        assert cp.deallocate(i, 1)
        assert cp.allocate_contiguous(B, 1) == i  # steals the block, leaves the hint
        assert cp.p.free_hints() <= 64
    assert cp.p.free_hints() == 64  # all stale
    assert cp.allocate(B) is None
    assert cp.deallocate(9, 1)  # the list is full: no hint, found by a scan
    assert cp.allocate(B) == 9


# ---- allocate_below ------------------------------------------------------------
@pytest.mark.parametrize("n_blocks", [100, 256])
def test_allocate_below_limits(n_blocks):
    for limit in (0, 1, 63, 64, 65, n_blocks):
        for nb in (1, 2, 63, 64, 65):
            cp = CheckedPool(n_blocks, B)  # empty words
            got = cp.allocate_below(nb * B, limit)
            assert got == (0 if nb <= min(limit, n_blocks) else None)
            cp = CheckedPool(n_blocks, B)  # mixed words: block 0 taken
            assert cp.allocate(B) == 0
            got = cp.allocate_below(nb * B, limit)
            assert got == (1 if nb + 1 <= min(limit, n_blocks) else None)


def test_allocate_below_refuses_a_run_that_ends_above_the_limit():
    cp = CheckedPool(256, B)
    assert cp.allocate_below(64 * B, 63) is None  # empty-word branch, one over
    assert cp.allocate_below(128 * B, 127) is None
    assert cp.allocate_below(128 * B, 128) == 0
    assert cp.deallocate(0, 128)
    assert cp.allocate(B) == 0
    assert cp.allocate_below(10 * B, 10) is None  # mixed-word branch, one over
    assert cp.allocate_below(10 * B, 11) == 1
    assert cp.allocate_below(70 * B, 80) is None  # 11..80 ends on block 81
    assert cp.allocate_below(70 * B, 81) == 11


# ---- size bounds, deallocate ---------------------------------------------------
@pytest.mark.parametrize("n_blocks,slack", [(64, 0), (100, 0), (100, 7)])
def test_size_bounds(n_blocks, slack):
    cp = CheckedPool(n_blocks, B, slack)
    whole = n_blocks * B
    for size in (0, whole + slack + 1, whole + B, 1 << 40):
        assert cp.allocate(size) is None
        assert cp.allocate_below(size, n_blocks) is None
        assert cp.allocate_contiguous(size, 1) is None
    assert cp.allocate_contiguous(B, 0) is None
    assert cp.allocate_contiguous(B, n_blocks + 1) is None
    assert cp.allocate(whole) == 0
    assert cp.deallocate(0, n_blocks)
    assert cp.allocate_below(whole, n_blocks) == 0
    assert cp.deallocate(0, n_blocks)
    assert cp.allocate_contiguous(B, n_blocks) == 0
    assert cp.deallocate(0, n_blocks, size=0) is False  # as allocate(0) refuses
    assert cp.deallocate_ptr(cp.ptr(3) + 1, B) is False
    assert cp.deallocate_ptr(cp.base - B, B) is False
    assert cp.deallocate_ptr(cp.base + cp.size, B) is False
    assert cp.deallocate(n_blocks - 1, 2) is False
    # pages of one batch freed singly, a sub-range of a run, then the rest
    assert cp.deallocate(5, 1) and cp.deallocate(7, 1)
    assert cp.deallocate(5, 3) is False  # block 6 used, 5 and 7 free
    assert cp.deallocate(20, 30)
    assert cp.deallocate(19, 2) is False
    assert cp.deallocate(0, 5) and cp.deallocate(6, 1) and cp.deallocate(8, 12)
    assert cp.deallocate(50, n_blocks - 50)
    assert cp.m.used() == 0


# ---- the contiguous-scan guard -------------------------------------------------
def test_guard_disarms_on_a_failed_scan_and_arms_on_the_4096th_free():
    cp = CheckedPool(200, B)
    fill_singles(cp)
    for s in range(0, 200, 2):
        assert cp.deallocate(s, 1)
    assert cp.allocate_contiguous(B, 2) is None  # 100 free, no run of 2: a failed scan
    assert not cp.m.contig_ok
    assert cp.deallocate(1, 1)  # free 1 of 4096; blocks 0..2 are a run now
    assert cp.allocate_contiguous(B, 2) is None  # refused unscanned
    assert cp.allocate(3 * B) == 0 and cp.deallocate(0, 3)  # allocate is not guarded
    assert cp.allocate_contiguous(B, 1) is not None  # nor is a single block
    # a refused or failed deallocate does not count
    assert cp.deallocate_ptr(cp.ptr(5) + 1, B) is False
    assert cp.deallocate(5, 1, size=0) is False
    for i in range(REARM_FREES - 3):
        assert cp.deallocate(cp.allocate(B), 1)
    assert not cp.m.contig_ok
    assert cp.allocate_contiguous(B, 2) is None
    assert cp.deallocate(cp.allocate(B), 1)  # the 4096th
    assert cp.m.contig_ok
    assert cp.allocate_contiguous(B, 2) is not None
    # larger than the free count: refused without a scan, the guard stays armed
    assert cp.allocate_contiguous(B, 150) is None
    assert cp.m.contig_ok


# ---- random runs ---------------------------------------------------------------
@pytest.fixture(scope="module")
def random_results():
    return {}


@pytest.mark.parametrize("n_blocks,seed,n_ops", RANDOM_RUNS)
def test_random_run(random_results, n_blocks, seed, n_ops):
    kinds, events = random_run(n_blocks, seed, n_ops)
    random_results[(n_blocks, seed)] = (kinds, events, n_ops)
    print(dict(kinds), dict(events))
    # the seed is worth its place (chosen by these counts, not by what fails)
    for kind in OP_KINDS:
        assert kinds[kind] >= 20, (kind, kinds)
    assert events["alloc_refused"] >= 20, events
    assert events["free_refused"] >= 20, events
    assert events["multi_block_at_90"] >= 20, events
    assert events["in_band"] >= 0.8 * n_ops, events  # occupancy mostly in 70..100 %
    if n_ops > 3 * REARM_FREES:
        assert events["rearms"] >= 1, events


# ---- MM ------------------------------------------------------------------------
@pytest.mark.parametrize("pools", [[8, 8], [8, 5, 8]])
def test_mm_cascade(pools):
    mm = CheckedMM(pools, B)
    got = [mm.allocate(B, 1)[0] for _ in range(sum(pools))]
    assert got == [(p, s) for p, nb in enumerate(pools) for s in range(nb)]
    assert mm.allocate(B, 1) is None
    # a run that only a later pool holds
    assert mm.deallocate(len(pools) - 1, 2, 3)
    assert mm.deallocate(0, 1, 1) and mm.deallocate(0, 3, 1)
    assert mm.allocate(3 * B, 1) == [(len(pools) - 1, 2)]
    assert mm.allocate(B, 1) in ([(0, 1)], [(0, 3)])


def test_mm_batch_is_one_run_of_separately_freeable_pages():
    mm = CheckedMM([64, 64], B)
    assert mm.allocate(B, 1) == [(0, 0)]
    pages = mm.allocate(B + B // 2, 5)  # two blocks a page
    assert pages == [(0, 1 + 2 * i) for i in range(5)]
    for pool, start in pages[1::2]:
        assert mm.deallocate(pool, start, 2)
    for pool, start in pages[0::2]:
        assert mm.deallocate(pool, start, 1) and mm.deallocate(pool, start + 1, 1)
    # a batch that only the second pool holds in one run
    assert mm.allocate(40 * B, 1) == [(0, 1)]
    assert mm.allocate(3 * B, 10) == [(1, 3 * i) for i in range(10)]


def fragmented_mm():
    """Two pools of 8: free runs of 2 + 2 blocks in pool 0 and 2 in pool 1."""
    mm = CheckedMM([8, 8], B)
    for _ in range(16):
        assert mm.allocate(B, 1)
    assert mm.deallocate(0, 1, 2) and mm.deallocate(0, 5, 2) and mm.deallocate(1, 3, 2)
    return mm


def test_mm_batch_falls_back_to_single_pages_across_pools():
    mm = fragmented_mm()
    pages = mm.allocate(2 * B, 3)  # no run of 6 anywhere
    assert sorted(pages) == [(0, 1), (0, 5), (1, 3)]
    assert mm.mm.used_blocks() == 16


def test_mm_failed_batch_is_undone():
    mm = fragmented_mm()
    used = mm.mm.used_blocks()
    assert mm.allocate(2 * B, 4) is None  # three pages fit, the fourth does not
    assert mm.mm.used_blocks() == used == 10
    assert mm.allocate(3 * B, 1) is None
    assert sorted(mm.allocate(2 * B, 3)) == [(0, 1), (0, 5), (1, 3)]  # still all there


def test_mm_need_extend_counts_the_last_pool_only():
    mm = CheckedMM([10, 10], B)
    assert not mm.mm.need_extend()
    assert mm.allocate(10 * B, 1) == [(0, 0)]  # the first pool full
    assert not mm.mm.need_extend()
    assert mm.allocate(8 * B, 1) == [(1, 0)]
    assert not mm.mm.need_extend()  # 8 of 10 is not above 0.8
    assert mm.allocate(B, 1) == [(1, 8)]
    assert mm.mm.need_extend()      # 9 of 10
    assert mm.deallocate(0, 0, 10)
    assert mm.mm.need_extend()      # an empty first pool changes nothing
    assert mm.deallocate(1, 8, 1)
    assert not mm.mm.need_extend()
    assert not CheckedMM([], B).mm.need_extend()


# ---- compaction planning -------------------------------------------------------
@pytest.mark.parametrize("n_pages", [64, 200])
def test_plan_moves_packs_single_block_pages(n_pages):
    mm = CheckedMM([n_pages], B)
    pages = [(p, s, 1) for _ in range(n_pages) for p, s in mm.allocate(B, 1)]
    for p, s, nb in pages[0::2]:
        assert mm.deallocate(p, s, nb)
    live, before, after = mm.plan_and_apply(pages[1::2])
    assert before == [1] and after == [n_pages // 2]
    assert sorted(s for _, s, _ in live) == list(range(n_pages // 2))


def filled_mm(rng, pools, sizes):
    mm = CheckedMM(pools, B)
    pages = []
    while True:
        nb = rng.choice(sizes)
        got = mm.allocate(nb * B, 1)
        if got is None:
            if nb == min(sizes):
                return mm, pages
            continue
        pages.append((*got[0], nb))


@pytest.mark.parametrize("sizes", [(1,), (3,), tuple(range(1, 8))], ids=["1", "3", "1-7"])
@pytest.mark.parametrize("seed", range(6))
def test_plan_moves_after_random_deletes(sizes, seed):
    rng = random.Random(f"plan-{sizes}-{seed}")
    mm, pages = filled_mm(rng, [130, 64, 100], sizes)
    stranger = max(mm.bases) + (1 << 30)  # owned by no pool
    for round_ in range(3):
        rng.shuffle(pages)
        cut = rng.randrange(len(pages) // 4, 3 * len(pages) // 4)
        for p, s, nb in pages[cut:]:
            assert mm.deallocate(p, s, nb)
        pages, before, after = mm.plan_and_apply(pages[:cut], strangers=[stranger])
        print(sizes, seed, round_, before, after)
        for b, a in zip(before, after):
            assert a >= b, (before, after)
        if len(sizes) == 1:  # one size: each pool ends up packed from block 0
            for pool in range(3):
                mine = sorted(s for p, s, _ in pages if p == pool)
                assert mine == [i * sizes[0] for i in range(len(mine))]
