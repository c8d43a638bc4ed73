"""KvIndex unit tests: the server's batched stripe sweep (insert / find /
extract), size() and clear(), replayed against a Python dict. The index is
reserved for 64 keys, so growth rehashes and tombstone reuse both run."""

import random
import string

from infinistore_amd import _native as n


def model(steps):
    """What a dict-backed index answers for the same (op, keys) steps."""
    live, out = {}, []
    for op, keys in steps:
        if op == "insert":
            won = []
            for k in keys:  # first occurrence wins, later ones lose
                won.append(k not in live)
                live.setdefault(k, True)
            out.append(won)
        elif op == "find":
            out.append([k in live for k in keys])
        elif op == "extract":
            out.append(sum(live.pop(k, False) for k in keys))
        elif op == "size":
            out.append(len(live))
        elif op == "clear":
            out.append(len(live))
            live.clear()
    return out


def check(steps):
    got = n._dbg_kvindex_ops(steps)
    assert got == model(steps)
    return got


def rand_keys(count, seed):
    rng = random.Random(seed)
    alphabet = string.ascii_lowercase + string.digits
    return ["".join(rng.choices(alphabet, k=40)) for _ in range(count)]


def test_empty_batch():
    got = check([("insert", []), ("find", []), ("extract", []), ("size", []), ("clear", [])])
    assert got == [[], [], 0, 0, 0]


def test_one_key_batch():
    got = check([
        ("insert", ["k"]), ("find", ["k", "other"]), ("size", []),
        ("insert", ["k"]), ("extract", ["k"]), ("find", ["k"]), ("size", []),
    ])
    assert got == [[True], [True, False], 1, [False], 1, [False], 0]


def test_5000_random_keys():
    keys = rand_keys(5000, 1)
    absent = rand_keys(500, 2)
    half = keys[::2]
    got = check([
        ("insert", keys), ("size", []), ("find", keys + absent),
        ("insert", keys[:100] + absent[:100]),  # old keys lose, new keys win
        ("extract", half + absent[100:]), ("size", []), ("find", keys),
    ])
    assert got[1] == 5000 and got[4] == 2500 and got[5] == 2600


def test_same_key_twice_in_one_batch():
    keys = rand_keys(200, 3)
    batch = keys + [keys[7]] + keys[50:60]
    got = check([("insert", batch), ("size", []), ("find", batch)])
    assert got[0][:200] == [True] * 200 and got[0][200:] == [False] * 11
    assert got[1] == 200


def test_reinsert_after_extract():
    keys = rand_keys(3000, 4)
    steps = []
    for rnd in range(4):  # tombstones from each extract are reused by the next insert
        steps += [("insert", keys), ("extract", keys[rnd::2]), ("insert", keys), ("size", [])]
    got = check(steps)
    assert got[-1] == 3000


def test_find_after_clear():
    keys = rand_keys(1000, 5)
    got = check([
        ("insert", keys), ("clear", []), ("size", []), ("find", keys),
        ("insert", keys[:10]), ("find", keys[:20]),
    ])
    assert got[1] == 1000 and got[2] == 0 and not any(got[3])
