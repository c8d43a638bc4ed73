"""The completed-prefix search of Shard::completion_loop
(csrc/server/completed_prefix.h), driven as a pure function through
`_dbg_completed_prefix(has_slot, fired_at_query)`.

A stream's pending FIFO holds real tasks (a slot and a recorded event) and
null-slot tasks (submit failures that only carry a done callback). Events fire
in FIFO order. The prefix that may be taken ends at the first real task whose
event has not fired; a null-slot task completes with the real tasks in front
of it, never ahead of them. The search may ask "fired?" at most
ceil(log2(n + 1)) times.

`parent_prefix` is a transcription of the loop this function replaced. It took
a null-slot task at the probe point for proof that everything before it had
completed, and so released slots whose kernels were still running."""

import itertools
import random


from infinistore_amd import _native


def contract(has_slot, fired):
    """Index of the first real task whose event has not fired, or n, with
    `fired` real tasks (in FIFO order) done."""
    real = 0
    for i, h in enumerate(has_slot):
        if h:
            if real >= fired:
                return i
            real += 1
    return len(has_slot)


def budget(n):
    return n.bit_length()  # == ceil(log2(n + 1))


def parent_prefix(has_slot, fired):
    """The search as completion_loop had it before, on a frozen queue.
    Returns (prefix, queried indices)."""
    n = len(has_slot)
    rank, real = [], 0
    for h in has_slot:
        rank.append(real)
        real += h
    asked = []

    def event_query(i):
        asked.append(i)
        return rank[i] < fired

    done_n = 0
    while done_n < n and not has_slot[done_n]:
        done_n += 1
    if done_n < n:
        lo, hi = done_n, n
        while lo < hi:
            mid = (lo + hi) // 2
            if not has_slot[mid] or event_query(mid):
                lo = mid + 1
            else:
                hi = mid
        done_n = lo
    return done_n, asked


def test_budget_is_the_ceiling_of_log2():
    for n in range(0, 70):
        b = budget(n)
        assert 2 ** b >= n + 1 and (b == 0 or 2 ** (b - 1) < n + 1)


def test_exhaustive_small_queues():
    """n = 0..10, every null mask, every frozen fired-count."""
    for n in range(0, 11):
        for mask in itertools.product([True, False], repeat=n):
            has_slot = list(mask)
            for fired in range(0, sum(has_slot) + 1):
                prefix, asked = _native._dbg_completed_prefix(has_slot, [fired])
                assert prefix == contract(has_slot, fired), (has_slot, fired, prefix)
                assert len(asked) <= budget(n), (has_slot, fired, asked)
                assert all(has_slot[i] for i in asked), (has_slot, asked)


def test_failed_task_behind_a_running_one():
    """pending = [A (real, not fired), X (null)]: nothing may be taken. The
    parent took both, freeing A's slot under its running kernel."""
    has_slot = [True, False]
    assert parent_prefix(has_slot, 0)[0] == 2  # what went wrong
    prefix, asked = _native._dbg_completed_prefix(has_slot, [0])
    assert prefix == 0 and asked == [0]
    # once A has fired, X goes with it
    assert _native._dbg_completed_prefix(has_slot, [1])[0] == 2


def test_failed_tasks_between_running_ones():
    """pending = [X, A, Y, B] with neither A nor B fired: only X may be taken.
    The parent took X, A and Y."""
    has_slot = [False, True, False, True]
    assert parent_prefix(has_slot, 0)[0] == 3  # what went wrong
    prefix, asked = _native._dbg_completed_prefix(has_slot, [0])
    assert prefix == 1 and len(asked) <= budget(4)
    assert _native._dbg_completed_prefix(has_slot, [1])[0] == 3  # A fired: X, A, Y
    assert _native._dbg_completed_prefix(has_slot, [2])[0] == 4


def test_same_queries_as_the_parent_without_failures():
    """All-real queues, n = 1..64, every fired-count: the same indices asked in
    the same order, and the same answer."""
    for n in range(1, 65):
        has_slot = [True] * n
        for fired in range(0, n + 1):
            want_prefix, want_asked = parent_prefix(has_slot, fired)
            assert want_prefix == fired
            prefix, asked = _native._dbg_completed_prefix(has_slot, [fired])
            assert (prefix, asked) == (want_prefix, want_asked), (n, fired)


def test_parent_was_right_only_without_failures():
    """The transcription agrees with the contract on every all-real queue and
    with a null task only at the very front; this pins the transcription
    itself."""
    for n in range(0, 11):
        for fired in range(0, n + 1):
            assert parent_prefix([True] * n, fired)[0] == contract([True] * n, fired)
    assert parent_prefix([False, True, True], 1)[0] == 2


def test_events_firing_during_the_search():
    """fired_at_query grows while the search runs: the answer lies between
    the contract's value when the search began and its value when it ended."""
    rng = random.Random(20240611)
    for _ in range(4000):
        n = rng.randint(0, 32)
        has_slot = [rng.random() < 0.7 for _ in range(n)]
        reals = sum(has_slot)
        counts = sorted(rng.randint(0, reals) for _ in range(rng.randint(1, 8)))
        prefix, asked = _native._dbg_completed_prefix(has_slot, counts)
        lo, hi = contract(has_slot, counts[0]), contract(has_slot, counts[-1])
        assert lo <= prefix <= hi, (has_slot, counts, prefix)
        assert len(asked) <= budget(n), (has_slot, counts, asked)
        # a taken prefix never ends in front of a null task: the next task, if
        # any, is the real one that stopped it
        assert prefix == n or has_slot[prefix]


def test_binding_repeats_the_last_count_and_takes_an_empty_list():
    assert _native._dbg_completed_prefix([True] * 8, [8]) == (8, [4, 6, 7])
    # task 4 had not fired when asked; everything asked later had
    assert _native._dbg_completed_prefix([True] * 8, [0, 8]) == (4, [4, 2, 3])
    assert _native._dbg_completed_prefix([True, True], []) == (0, [1, 0])
    assert _native._dbg_completed_prefix([], []) == (0, [])
