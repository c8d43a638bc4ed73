"""Model-based test of the store: the schedule generator.

`schedule(profile, seed, n_ops)` turns a seed into a list of operations (plain
dicts, printable as JSON). It is pure: no server, no torch, no clock. Two
drivers execute the list against a real server next to a Python dict that maps
each key to its expected bytes (tests/test_store_model.py on a CPU pool over
the TCP fabric, tests/test_gpu_store_model.py on HBM over the local path). The
generator keeps its own abstract copy of the store (key -> (size, codec)) only
to emit operations that apply: a delete needs a live key, a restore needs a
snapshot. Nothing is skipped at run time.

Kinds of operation (KINDS):

  write       new keys, one size, codec and client layout per batch
  overwrite   live keys again at another size ("larger", "smaller") or another
              codec ("codec"), sometimes with a new key in the same batch:
              first write wins, the new key lands
  read        a subset of the live keys of one logical page size
  read_wrong  one live key at another page size: a plain entry answers a
              smaller page with that prefix and refuses a larger one; a
              compressed entry refuses both (docs/protocol.md, "read sizes")
  delete      live keys
  compact     compact_pool()
  snapshot    snapshot_pool()
  restore     restore_pool(), after a purge or into the live index (live keys
              win; the count is the number of snapshot keys absent before)

and `read_all`, which only the fixed ending uses. Every schedule ends the same
way: read everything (so every key the random part left live is checked, the
ones the next step deletes included), delete every second live key in write
order, compact, read everything again, snapshot, purge, restore, read
everything a third time.
"""

import math
import random
from collections import Counter

KINDS = ("write", "overwrite", "read", "read_wrong", "delete", "compact", "snapshot", "restore")
OVERWRITE_KINDS = ("larger", "smaller", "codec")

# Elements of a group that a codec's kernels move whole: a page, and every
# segment or tensor part of it, is a multiple (docs/design.md, "page codecs").
CODEC_MULTIPLE = {"plain": 1, "fp8": 8, "mxfp4": 32}


def stored_bytes(size, codec, elem_bytes):
    """Bytes of the stored block of a page of `size` elements."""
    if codec == "plain":
        return size * elem_bytes
    if codec == "fp8":
        return size
    return size // 2 + size // 32


class Profile:
    """What one driver can do. `sizes` are logical page sizes in elements of
    `elem_bytes`; a layout is (name, parts): the page is `parts` equal pieces on
    the client side."""

    def __init__(self, name, sizes, elem_bytes, codecs, layouts, read_modes, ticketed,
                 slice_sizes=(), max_keys=12):
        self.name = name
        self.sizes = list(sizes)
        self.elem_bytes = elem_bytes
        self.codecs = list(codecs)
        self.layouts = list(layouts)
        self.read_modes = list(read_modes)
        self.ticketed = ticketed
        self.slice_sizes = set(slice_sizes)
        self.max_keys = max_keys

    def stored(self, size, codec):
        return stored_bytes(size, codec, self.elem_bytes)

    def layout_legal(self, size, codec, parts):
        return size % parts == 0 and (size // parts) % CODEC_MULTIPLE[codec] == 0


# uint8 pages at a 16 KiB granule: below it, exactly one granule, one granule
# plus 16, several granules, and sizes that are no multiple of anything.
CPU_PROFILE = Profile(
    "cpu", sizes=[1000, 4096, 16384, 16400, 40000, 65536, 100000], elem_bytes=1,
    codecs=["plain"], layouts=[("contig", 1)], read_modes=[("contig", 1)], ticketed=False)

# bf16 pages. Stored sizes: 64/32/17, 1024/512/272, 8192/4096/2176 and
# 8256/4128/2193 bytes (plain/fp8/mxfp4): 17 bytes takes the byte kernel when
# compaction moves it, 2193 is odd, 272 is a multiple of 16.
GPU_PROFILE = Profile(
    "gpu", sizes=[32, 512, 4096, 4128], elem_bytes=2, codecs=["plain", "fp8", "mxfp4"],
    layouts=[("contig", 1), ("seg", 2), ("tset", 2), ("tset", 4)],
    read_modes=[("contig", 1), ("seg", 2), ("tset", 2), ("tset", 4), ("slice", 1)],
    ticketed=True, slice_sizes=[4096])

# The committed schedules. tests/test_store_model.py checks, without a server,
# that each of them meets the coverage conditions; a new seed is chosen by
# running coverage() here, never by what a server answers.
CPU_SEEDS, CPU_OPS = (1, 3, 23), 300
GPU_SEEDS, GPU_OPS = (4, 7), 150

_WEIGHTS = {"write": 20, "overwrite": 10, "read": 22, "read_wrong": 12, "delete": 13,
            "compact": 2, "snapshot": 3, "restore": 4}


def schedule(profile, seed, n_ops):
    """The operation list of `seed`: about n_ops random operations, then the
    fixed ending."""
    rng = random.Random(f"{profile.name}-{seed}")
    live = {}  # key -> (size, codec), insertion order = write order
    snap = None
    ops = []
    serial = [0]

    def new_keys(n):
        out = [f"{profile.name}{seed}-k{serial[0] + i}" for i in range(n)]
        serial[0] += n
        return out

    def pick_layout(size, codec):
        return rng.choice([l for l in profile.layouts if profile.layout_legal(size, codec, l[1])])

    def do_write():
        size, codec = rng.choice(profile.sizes), rng.choice(profile.codecs)
        keys = new_keys(rng.randint(1, profile.max_keys))
        name, parts = pick_layout(size, codec)
        ops.append({"op": "write", "keys": keys, "size": size, "codec": codec,
                    "layout": name, "parts": parts, "seed": rng.randrange(1 << 30)})
        for k in keys:
            live[k] = (size, codec)

    def do_overwrite():
        anchor = rng.choice(list(live))
        size, codec = live[anchor]
        kinds = [k for k in OVERWRITE_KINDS
                 if (k == "larger" and size != max(profile.sizes))
                 or (k == "smaller" and size != min(profile.sizes))
                 or (k == "codec" and len(profile.codecs) > 1)]
        kind = rng.choice(kinds)
        if kind == "codec":
            size2, codec2 = size, rng.choice([c for c in profile.codecs if c != codec])
        else:
            size2 = rng.choice([s for s in profile.sizes
                                if (s > size if kind == "larger" else s < size)])
            codec2 = codec
        same = [k for k, v in live.items() if v == (size, codec) and k != anchor]
        keys = [anchor] + rng.sample(same, min(len(same), rng.randint(0, 3)))
        fresh = new_keys(rng.randint(0, 1))
        name, parts = pick_layout(size2, codec2)
        ops.append({"op": "overwrite", "kind": kind, "keys": keys, "new_keys": fresh,
                    "size": size2, "codec": codec2, "layout": name, "parts": parts,
                    "seed": rng.randrange(1 << 30)})
        for k in fresh:
            live[k] = (size2, codec2)

    def do_read():
        size = live[rng.choice(list(live))][0]
        group = [k for k, v in live.items() if v[0] == size]
        keys = rng.sample(group, rng.randint(1, min(len(group), 2 * profile.max_keys)))
        codecs = {live[k][1] for k in keys}
        modes = [m for m in profile.read_modes
                 if (m[0] != "slice" or size in profile.slice_sizes)
                 and all(profile.layout_legal(size, c, m[1]) for c in codecs)]
        name, parts = rng.choice(modes)
        ops.append({"op": "read", "keys": keys, "size": size, "mode": name, "parts": parts,
                    "ticketed": profile.ticketed and rng.random() < 0.5,
                    "slice_half": rng.randrange(2)})

    def do_read_wrong():
        key = rng.choice(list(live))
        size, codec = live[key]
        m = CODEC_MULTIPLE[codec]
        # one unit below and above, half, double: at most one page over-read
        pages = {size - m, size + m, size // 2 // m * m, 2 * size} - {0, size}
        page = rng.choice(sorted(pages))
        expect = "prefix" if codec == "plain" and page < size else "refuse"
        ops.append({"op": "read_wrong", "key": key, "page": page, "expect": expect})

    def do_delete():
        keys = rng.sample(list(live), rng.randint(1, min(len(live), 2 * profile.max_keys)))
        ops.append({"op": "delete", "keys": keys})
        for k in keys:
            del live[k]
        if rng.random() < 0.12:
            ops.append({"op": "compact"})

    def do_restore():
        purge = rng.random() < 0.5
        ops.append({"op": "restore", "purge": purge})
        if purge:
            live.clear()
        for k, v in snap.items():
            live.setdefault(k, v)

    while len(ops) < n_ops:
        kinds = [k for k in KINDS
                 if k in ("write", "compact", "snapshot")
                 or (k == "restore" and snap is not None)
                 or (k not in ("restore",) and live)]
        kind = rng.choices(kinds, [_WEIGHTS[k] for k in kinds])[0]
        if kind == "write":
            do_write()
        elif kind == "overwrite":
            do_overwrite()
        elif kind == "read":
            do_read()
        elif kind == "read_wrong":
            do_read_wrong()
        elif kind == "delete":
            do_delete()
        elif kind == "restore":
            do_restore()
        else:
            ops.append({"op": kind})
            if kind == "snapshot":
                snap = dict(live)

    # The fixed ending. Python dicts keep insertion order and a restored key is
    # appended when it comes back, so "write order" is the order in which the
    # live keys entered the index. Nothing below draws from rng.
    ops.append({"op": "read_all"})
    ops.append({"op": "delete", "keys": list(live)[::2], "final": True})
    for k in ops[-1]["keys"]:
        del live[k]
    ops.append({"op": "compact", "final": True})
    ops.append({"op": "read_all"})
    ops.append({"op": "snapshot"})
    ops.append({"op": "restore", "purge": True})
    ops.append({"op": "read_all"})
    return ops


def replay(profile, ops):
    """The abstract store after every operation: yields (index, op, live, snap)
    with live and snap as dicts key -> (size, codec), BEFORE the operation is
    applied, then applies it. The drivers do the same with bytes; the coverage
    check and the drivers' bookkeeping both follow these few rules."""
    live, snap = {}, None
    for i, op in enumerate(ops):
        yield i, op, live, snap
        kind = op["op"]
        if kind == "write":
            for k in op["keys"]:
                assert k not in live, (i, k)
                live[k] = (op["size"], op["codec"])
        elif kind == "overwrite":
            for k in op["new_keys"]:
                live[k] = (op["size"], op["codec"])
        elif kind == "delete":
            for k in op["keys"]:
                del live[k]
        elif kind == "snapshot":
            snap = dict(live)
        elif kind == "restore":
            if op["purge"]:
                live.clear()
            for k, v in snap.items():
                live.setdefault(k, v)


def coverage(profile, ops):
    """Counts the conditions a committed seed must meet."""
    kinds = Counter()
    over = Counter()
    out = {"compact_after_delete": 0, "restore_into_live": 0, "final_stored_sizes": 0,
           "applicable": True}
    prev = None
    for i, op, live, snap in replay(profile, ops):
        kind = op["op"]
        kinds[kind] += 1
        if kind == "overwrite":
            for k in op["keys"]:
                size, codec = live[k]
                was, now = profile.stored(size, codec), profile.stored(op["size"], op["codec"])
                ok = {"larger": now > was and codec == op["codec"],
                      "smaller": now < was and codec == op["codec"],
                      "codec": codec != op["codec"] and size == op["size"]}[op["kind"]]
                out["applicable"] &= ok
            over[op["kind"]] += 1
        elif kind in ("read", "delete"):
            out["applicable"] &= bool(op["keys"]) and all(k in live for k in op["keys"])
            if kind == "read":
                out["applicable"] &= all(live[k][0] == op["size"] for k in op["keys"])
        elif kind == "read_wrong":
            out["applicable"] &= op["key"] in live and op["page"] != live[op["key"]][0]
            out["applicable"] &= 0 < op["page"] <= 2 * live[op["key"]][0]
        elif kind == "compact":
            if prev == "delete":
                out["compact_after_delete"] += 1
            if op.get("final"):
                out["final_stored_sizes"] = len({profile.stored(*v) for v in live.values()})
                out["final_live"] = len(live)
        elif kind == "restore":
            out["applicable"] &= snap is not None
            if not op["purge"] and live:
                out["restore_into_live"] += 1
        prev = kind
    out["kinds"] = dict(kinds)
    out["overwrite_kinds"] = dict(over)
    return out


def moved_bytes_possible(stored_sizes, moved, moved_bytes):
    """Can `moved` of the blocks in `stored_sizes` add up to moved_bytes?
    compact_pool() names no keys, so this is how a driver checks that
    moved_bytes is the sum of the moved keys' stored sizes."""
    if not 0 <= moved <= len(stored_sizes) or moved_bytes < 0:
        return False
    if moved == 0:
        return moved_bytes == 0
    unit = math.gcd(*stored_sizes)
    if moved_bytes % unit:
        return False
    target = moved_bytes // unit
    keep = (1 << (target + 1)) - 1
    # reach[t]: bit s set when t blocks can add up to s units. A size that
    # occurs `count` times enters as bundles of 1, 2, 4, ... blocks.
    reach = [1] + [0] * moved
    for size, count in Counter(stored_sizes).items():
        bundle = 1
        while count:
            take = min(bundle, count)
            count -= take
            bundle *= 2
            for t in range(moved, take - 1, -1):
                if reach[t - take]:
                    reach[t] |= (reach[t - take] << (take * size // unit)) & keep
    return bool(reach[moved] >> target & 1)


def describe(seed, ops, upto):
    """The seed and the operations up to the failing step, for a failure report."""
    import json
    lines = [f"seed {seed}: failed at operation {upto} of {len(ops)}"]
    lines += [f"  {i:4d} {json.dumps(op)}" for i, op in enumerate(ops[:upto + 1])]
    return "\n".join(lines)
