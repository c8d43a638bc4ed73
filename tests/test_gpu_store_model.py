"""Model-based test of the store, GPU driver: schedules from
tests/_store_model.py against an HBM pool over the local path, next to a dict
key -> expected bf16 bits. bf16 pages of 32, 512, 4096 and 4128 elements,
plain, fp8 and mxfp4, share one pool (stored blocks of 17 to 8256 bytes);
they are written contiguous, as 2 segments and over tensor sets of 2 and 4,
and read contiguous, segmented, over tensor sets and sliced, blocking and
ticketed, through dedup, wrong-size reads, delete, compaction and
snapshot/restore.

The expected bits of a key are computed when it is written, with the numpy /
torch references (tests/_kernel_refs.py, tests/_mxfp4_refs.py), never from a
read of the server; every comparison is bit for bit and covers the whole
destination, so a byte written outside the request shows as well.

Every stored size here fits one 64 KiB granule of the pool, so the several
sizes exercise the kernels and compaction's one-job-per-size moves, not
allocator fragmentation; the CPU driver, with 1 to 7 granules per key, does
that.

Each seed runs in a child process (this file, started as a script) that hosts
the server in-process, so that compact_pool, snapshot_pool and purge_kv_map
are reachable."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _store_model as sm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = sm.GPU_PROFILE
INVALID_REQ = "-400"
SENT16 = 0xA5A5
GUARD = 16  # elements between destination pages; keeps every page 16-byte aligned
MAX_PAGE = max(PROFILE.sizes)
MAX_READ = 2 * PROFILE.max_keys  # keys per read request at most
# [2, T, H, hd] view of a 4096-element page, for the sliced reads
T, H, HD = 8, 8, 32
assert 2 * T * H * HD == 4096 and set(PROFILE.slice_sizes) == {4096}


@pytest.mark.gpu
@pytest.mark.parametrize("seed", sm.GPU_SEEDS)
def test_store_model_gpu(tmp_path, seed):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r = subprocess.run(
        [sys.executable, os.path.abspath(__file__), str(seed), str(tmp_path)],
        cwd=REPO, env={**os.environ, "PYTHONPATH": REPO + ":" + os.path.join(REPO, "tests")},
        timeout=180)
    assert r.returncode == 0, f"seed {seed}: see the child's output above"


def make_pages(n, elems, seed):
    """n bf16 pages with a different magnitude per 32-element group (finite)."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(2.0, torch.randint(-20, 20, (n, elems // 32, 1), generator=g).float())
    x = torch.randn(n, elems // 32, 32, generator=g) * mag
    return x.reshape(n, elems).to(torch.bfloat16)


def expected_bits(pages, codec):
    """(n, elems) uint16: what a read of these pages returns, by reference."""
    from _kernel_refs import bf16_bits, fp8_dequant_ref, fp8_quant_ref
    from _mxfp4_refs import roundtrip_ref
    if codec == "plain":
        return bf16_bits(pages).copy()
    if codec == "fp8":
        codes, scales = fp8_quant_ref(pages)
        return bf16_bits(fp8_dequant_ref(codes, scales)).copy()
    return roundtrip_ref(pages)


class GpuDriver:
    def __init__(self, conn, ifs, tmp):
        self.conn, self.ifs = conn, ifs
        self.snap_path = os.path.join(tmp, "model.snap")
        self.model = {}  # key -> (uint16 bits of the page as read, stored bytes)
        self.snap = None
        dev = "cuda:0"
        # sources: a contiguous / 2-segment staging tensor and the tensors of
        # the write sets; destinations likewise
        self.src_half = (PROFILE.max_keys + 1) * MAX_PAGE
        self.src = torch.zeros(2 * self.src_half, dtype=torch.bfloat16, device=dev)
        self.dst_half = MAX_READ * (MAX_PAGE + GUARD)
        self.dst = torch.zeros(2 * self.dst_half, dtype=torch.bfloat16, device=dev)
        self.wsets, self.rsets = {}, {}
        for G in (2, 4):
            w = [torch.zeros(self.src_half // G, dtype=torch.bfloat16, device=dev)
                 for _ in range(G)]
            r = [torch.zeros(MAX_READ * (MAX_PAGE // G + GUARD), dtype=torch.bfloat16,
                             device=dev) for _ in range(G)]
            self.wsets[G] = conn.register_tensor_set(w)
            self.rsets[G] = conn.register_tensor_set(r)
        assert self.src.data_ptr() % 16 == 0 and self.dst.data_ptr() % 16 == 0

    # -- writes ------------------------------------------------------------
    def write(self, op):
        conn = self.conn
        keys, size, codec = op["keys"] + op.get("new_keys", []), op["size"], op["codec"]
        n, parts = len(keys), op["parts"]
        pages = make_pages(n, size, op["seed"])
        want = expected_bits(pages, codec)  # before anything is sent
        quant = None if codec == "plain" else codec
        dev_pages = pages.to("cuda:0")
        if op["layout"] == "contig":
            self.src[: n * size] = dev_pages.reshape(-1)
            conn.write_pages(self.src, keys, [j * size for j in range(n)], size, sync=True,
                             quant=quant)
        elif op["layout"] == "seg":
            seg = size // 2
            for s in range(2):
                self.src[s * self.src_half: s * self.src_half + n * seg] = \
                    dev_pages[:, s * seg:(s + 1) * seg].reshape(-1)
            conn.write_pages(self.src, keys, [j * seg for j in range(n)], size, sync=True,
                             quant=quant, segments=2, segment_stride=self.src_half)
        else:
            ts, part = self.wsets[parts], size // parts
            for g, t in enumerate(ts.tensors):
                t[: n * part] = dev_pages[:, g * part:(g + 1) * part].reshape(-1)
            conn.write_pages(None, keys, [j * part for j in range(n)], size, sync=True,
                             quant=quant, tensor_set=ts)
        stored = PROFILE.stored(size, codec)
        for j, k in enumerate(keys):
            self.model.setdefault(k, (want[j], stored))  # first write wins

    # -- reads -------------------------------------------------------------
    def _fill(self, tensors):
        for t in tensors:
            t.view(torch.uint8).fill_(0xA5)

    def _issue(self, ticketed, *args, **kw):
        if ticketed:
            self.conn.wait_read(self.conn.read_pages_async(*args, **kw))
        else:
            self.conn.read_pages(*args, **kw)
            self.conn.sync()

    def _compare(self, tensors, wants, what):
        from _kernel_refs import bf16_bits
        for i, (t, want) in enumerate(zip(tensors, wants)):
            got = bf16_bits(t)
            if not np.array_equal(got, want):
                bad = np.flatnonzero(got != want)
                raise AssertionError(
                    f"{what}: tensor {i}: {bad.size} values differ, first at {bad[0]}: "
                    f"got {got[bad[0]]:#06x} want {want[bad[0]]:#06x}")

    def read(self, keys, size, mode, parts, ticketed, slice_half=0):
        n = len(keys)
        assert n <= MAX_READ
        exp = np.stack([self.model[k][0] for k in keys])
        assert exp.shape == (n, size)
        what = f"{mode}/{parts} read of {n} keys at {size}, ticketed={ticketed}"
        if mode in ("contig", "seg", "slice"):
            self._fill([self.dst])
            want = np.full(self.dst.numel(), SENT16, dtype=np.uint16)
            kw = {}
            if mode == "slice":
                exp = exp.reshape(n, 2, T, H, HD)[:, :, :, slice_half * H // 2:
                                                  (slice_half + 1) * H // 2, :].reshape(n, -1)
                from infinistore_amd import PageSlice
                kw["page_slice"] = PageSlice(size, slice_half * (H // 2) * HD, (H // 2) * HD,
                                             H * HD, 2 * T)
                page = exp.shape[1]
            else:
                page = size
            seg = page // parts
            slot = seg + GUARD
            offs = [j * slot for j in range(n)]
            if parts > 1:
                kw.update(segments=parts, segment_stride=self.dst_half)
            for j in range(n):
                for s in range(parts):
                    o = offs[j] + s * self.dst_half
                    want[o:o + seg] = exp[j, s * seg:(s + 1) * seg]
            self._issue(ticketed, self.dst, keys, offs, page, **kw)
            self._compare([self.dst], [want], what)
        else:
            ts, part = self.rsets[parts], size // parts
            slot = part + GUARD
            offs = [j * slot for j in range(n)]
            self._fill(ts.tensors)
            wants = []
            for g, t in enumerate(ts.tensors):
                w = np.full(t.numel(), SENT16, dtype=np.uint16)
                for j in range(n):
                    w[offs[j]:offs[j] + part] = exp[j, g * part:(g + 1) * part]
                wants.append(w)
            self._issue(ticketed, None, keys, offs, size, tensor_set=ts)
            self._compare(ts.tensors, wants, what)

    def read_wrong(self, op):
        key, page = op["key"], op["page"]
        bits = self.model[key][0]
        self._fill([self.dst])
        want = np.full(self.dst.numel(), SENT16, dtype=np.uint16)
        if op["expect"] == "prefix":
            assert page < len(bits)
            self._issue(False, self.dst, [key], [0], page)
            want[:page] = bits[:page]
        else:
            with pytest.raises(Exception, match=INVALID_REQ):
                self._issue(False, self.dst, [key], [0], page)
        self._compare([self.dst], [want], f"read of {key} at {page} ({op['expect']})")

    def read_all(self):
        by_size = {}
        for k, (bits, _) in self.model.items():
            by_size.setdefault(len(bits), []).append(k)
        for size, keys in by_size.items():
            for lo in range(0, len(keys), MAX_READ):
                self.read(keys[lo:lo + MAX_READ], size, "contig", 1, ticketed=lo % 2 == 1)

    # -- one operation -------------------------------------------------------
    def step(self, op):
        kind, ifs, model = op["op"], self.ifs, self.model
        if kind in ("write", "overwrite"):
            self.write(op)
        elif kind == "read":
            self.read(op["keys"], op["size"], op["mode"], op["parts"], op["ticketed"],
                      op["slice_half"])
        elif kind == "read_wrong":
            self.read_wrong(op)
        elif kind == "delete":
            assert self.conn.delete_keys(op["keys"]) == len(op["keys"])
            for k in op["keys"]:
                del model[k]
        elif kind == "compact":
            moved, moved_bytes = ifs.compact_pool()
            sizes = [s for _, s in model.values()]
            assert moved <= len(sizes) and moved_bytes <= sum(sizes), (moved, moved_bytes)
            assert sm.moved_bytes_possible(sizes, moved, moved_bytes), (moved, moved_bytes)
            if op.get("final"):
                assert moved > 0
        elif kind == "snapshot":
            got = ifs.snapshot_pool(self.snap_path)
            assert got == (len(model), sum(s for _, s in model.values())), got
            self.snap = dict(model)
        elif kind == "restore":
            if op["purge"]:
                ifs.purge_kv_map()
                model.clear()
            absent = [k for k in self.snap if k not in model]
            got = ifs.restore_pool(self.snap_path)
            assert got == (len(absent), sum(self.snap[k][1] for k in absent)), got
            for k in absent:  # live keys win
                model[k] = self.snap[k]
        elif kind == "read_all":
            self.read_all()
        else:
            raise AssertionError(f"unknown operation {kind}")
        assert ifs.get_kvmap_len() == len(model), (ifs.get_kvmap_len(), len(model))


def main(seed, tmp):
    import infinistore_amd as ifs
    from conftest import free_port

    ops = sm.schedule(PROFILE, seed, sm.GPU_OPS)
    port = free_port()
    ifs.register_server(ifs.ServerConfig(service_port=port, manage_port=free_port(),
                                         prealloc_size=1, minimal_allocate_size=64))
    try:
        conn = ifs.InfinityConnection(ifs.ClientConfig(
            host_addr="127.0.0.1", service_port=port, connection_type=ifs.TYPE_LOCAL_GPU))
        conn.connect()
        driver = GpuDriver(conn, ifs, tmp)
        for i, op in enumerate(ops):
            try:
                driver.step(op)
            except BaseException:
                print(sm.describe(seed, ops, i), flush=True)
                raise
        conn.close()
    finally:
        ifs.unregister_server()
    print(f"STORE MODEL OK seed {seed}: {len(ops)} operations, {len(driver.model)} keys live")


if __name__ == "__main__":
    main(int(sys.argv[1]), sys.argv[2])
