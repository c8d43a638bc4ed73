"""Tensor sets through a server (docs/design.md, "tensor sets"): one key per
block for pages that span several separately allocated tensors. Round trips
against the contiguous page for all three codecs, over the ring and the
socket, blocking and ticketed; every refusal the server makes on a request
that the Python layer would never send (INVALID_REQ, with the connection
still serving afterwards); KEY_NOT_FOUND; and the connection's mapping cache
under a set of 70 distinct allocations."""

import uuid

import numpy as np
import pytest
import torch

import infinistore_amd as ifs
from infinistore_amd.lib import _remap_device_id

from _kernel_refs import bf16_bits, fp8_dequant_ref, fp8_quant_ref
from _mxfp4_refs import roundtrip_ref
from test_gpu import gpu_server, local_conn  # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

PART = 512  # bf16 elements of one tensor's part of a page
QUANTS = [None, "fp8", "mxfp4"]
INVALID_REQ, KEY_NOT_FOUND = 400, 404


def _keys(tag, n):
    u = uuid.uuid4().hex[:12]
    return [f"tset-{tag}-{u}-{i}" for i in range(n)]


def _pages(n, elems, seed):
    """bf16 pages whose groups of 32 differ in magnitude, and whose parts
    differ in absmax, so a scale or a part in the wrong place changes bits."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(2.0, torch.randint(-6, 6, (n, elems // 32, 1), generator=g).float())
    x = torch.randn(n, elems // 32, 32, generator=g) * mag
    return x.reshape(n, elems).to(torch.bfloat16)


def _expected(pages, quant):
    """uint16 bits of what a read returns for pages written with `quant`."""
    if quant is None:
        return bf16_bits(pages)
    if quant == "fp8":
        codes, scales = fp8_quant_ref(pages)
        return bf16_bits(fp8_dequant_ref(codes, scales))
    return roundtrip_ref(pages)


def _table(n, seed):
    return np.random.RandomState(seed).permutation(n).astype(np.int64)


def _scatter(pages, table, G, per=1):
    """G separately allocated device tensors of [n * per * seg] elements;
    block i's part of tensor g is `per` segments, segment r at
    (r * n + table[i]) * seg: a K/V-split layer when per == 2."""
    n, elems = pages.shape
    seg = elems // (G * per)
    parts = pages.reshape(n, G, per, seg)
    out = []
    for g in range(G):
        t = torch.zeros(per, n, seg, dtype=pages.dtype)
        t[:, torch.from_numpy(table)] = parts[:, g].transpose(0, 1)
        out.append(t.reshape(-1).to("cuda:0"))
    return out


def _gather(tensors, table, per=1):
    n = len(table)
    parts = []
    for t in tensors:
        v = t.cpu().reshape(per, n, -1)[:, torch.from_numpy(table)]  # (per, n, seg)
        parts.append(v.transpose(0, 1).reshape(n, -1))
    return torch.cat(parts, dim=1)


def _blank(tensors):
    return [torch.full_like(t, 7.0) for t in tensors]


@pytest.mark.parametrize("nb", [5, 16, 17, 40])
@pytest.mark.parametrize("quant", QUANTS)
def test_fused_write_contiguous_read_and_back(gpu_server, quant, nb):
    G = 4
    elems = G * PART
    pages = _pages(nb, elems, 100 + nb)
    want = _expected(pages, quant)
    table = _table(nb, nb)
    conn = local_conn(gpu_server)
    keys, keys2 = _keys("fw", nb), _keys("cw", nb)
    try:
        # fused write -> contiguous read
        tensors = _scatter(pages, table, G)
        ts = conn.register_tensor_set(tensors)
        conn.write_pages(None, keys, table * PART, elems, sync=True, quant=quant, tensor_set=ts)
        flat = torch.zeros(nb * elems, dtype=torch.bfloat16, device="cuda:0")
        conn.read_pages(flat, keys, np.arange(nb) * elems, elems)
        assert np.array_equal(bf16_bits(flat).reshape(nb, elems), want)
        # contiguous write -> fused read
        src = pages.reshape(-1).to("cuda:0")
        conn.write_pages(src, keys2, np.arange(nb) * elems, elems, sync=True, quant=quant)
        outs = _blank(tensors)
        ts2 = conn.register_tensor_set(outs)
        conn.read_pages(None, keys2, table * PART, elems, tensor_set=ts2)
        assert np.array_equal(bf16_bits(_gather(outs, table)), want)
        # the source tensors of the fused write are unchanged
        assert np.array_equal(bf16_bits(_gather(tensors, table)), bf16_bits(pages))
        conn.release_tensor_set(ts)
        conn.release_tensor_set(ts2)
    finally:
        conn.delete_keys(keys + keys2)
        conn.close()


@pytest.mark.parametrize("quant", QUANTS)
def test_write_over_four_tensors_read_over_two(gpu_server, quant):
    """G=4, S=4 on the way in; G=2, S=4 (two segments per tensor) on the way
    out: the stored block knows nothing of either."""
    nb, seg = 17, PART
    elems = 4 * seg
    pages = _pages(nb, elems, 7)
    want = _expected(pages, quant)
    table = _table(nb, 3)
    conn = local_conn(gpu_server)
    keys = _keys("4to2", nb)
    try:
        ts4 = conn.register_tensor_set(_scatter(pages, table, 4))
        conn.write_pages(None, keys, table * seg, elems, sync=True, quant=quant, segments=4,
                         tensor_set=ts4)
        outs = [torch.full((2 * nb * seg,), 7.0, dtype=torch.bfloat16, device="cuda:0")
                for _ in range(2)]
        ts2 = conn.register_tensor_set(outs)
        conn.read_pages(None, keys, table * seg, elems, segments=4, segment_stride=nb * seg,
                        tensor_set=ts2)
        assert np.array_equal(bf16_bits(_gather(outs, table, per=2)), want)
    finally:
        conn.delete_keys(keys)
        conn.close()


@pytest.mark.parametrize("quant", QUANTS)
@pytest.mark.parametrize("ticketed", [False, True])
@pytest.mark.parametrize("transport", ["shm", "socket"])
def test_transports_blocking_and_ticketed(gpu_server, transport, ticketed, quant, monkeypatch):
    if transport == "socket":
        monkeypatch.setenv("IFS_NO_SHM", "1")
    nb, G = 17, 3
    elems = G * PART
    pages = _pages(nb, elems, 21)
    table = _table(nb, 22)
    conn = local_conn(gpu_server)
    keys = _keys(transport, nb)
    try:
        assert conn.conn.shm_active() == (transport == "shm")
        ts = conn.register_tensor_set(_scatter(pages, table, G))
        conn.write_pages(None, keys, table * PART, elems, quant=quant,
                         tensor_set=ts)  # async write
        conn.sync()
        outs = _blank(ts.tensors)
        ts_out = conn.register_tensor_set(outs)
        if ticketed:
            conn.wait_read(conn.read_pages_async(None, keys, table * PART, elems,
                                                 tensor_set=ts_out))
        else:
            conn.read_pages(None, keys, table * PART, elems, tensor_set=ts_out)
        assert np.array_equal(bf16_bits(_gather(outs, table)), _expected(pages, quant))
    finally:
        conn.delete_keys(keys)
        conn.close()


def _raw(conn, op, ts_id, n_tensors, keys, offs, page_bytes, flags=0, segments=None,
         stride=0):
    """A request the Python layer would refuse, sent as it stands."""
    device = _remap_device_id(torch.empty(0, device="cuda:0"))
    segments = n_tensors if segments is None else segments
    ret, _ = conn.conn.rw_tset_blob(op, conn.pack_keys(keys), np.asarray(offs, dtype=np.uint64),
                                    1, page_bytes, ts_id, n_tensors, device, True, flags,
                                    segments, stride, False)
    return ret


def test_invalid_requests_and_the_connection_keeps_serving(gpu_server):
    nb, G = 3, 2
    elems = G * PART
    pages = _pages(nb, elems, 31)
    table = np.arange(nb)
    conn = local_conn(gpu_server)
    keys = _keys("bad", nb)
    FP8 = conn.FLAG_QUANT_FP8
    try:
        tensors = _scatter(pages, table, G)
        outs = _blank(tensors)
        ts = conn.register_tensor_set(tensors)
        ts_out = conn.register_tensor_set(outs)
        offs = table * PART * 2  # bytes
        conn.write_pages(None, keys, table * PART, elems, sync=True, tensor_set=ts)

        def refused(ret):
            assert ret == -INVALID_REQ, ret

        for op in ("W", "R"):
            tid = ts.set_id if op == "W" else ts_out.set_id
            k = _keys("never", nb) if op == "W" else keys
            refused(_raw(conn, op, 9999, G, k, offs, elems * 2))  # unknown id
            refused(_raw(conn, op, tid, G + 2, k, offs, elems * 2, segments=G + 2))  # wrong G
            # the last part ends one element past the tensor
            refused(_raw(conn, op, tid, G, k, offs + 2, elems * 2))
            refused(_raw(conn, op, tid, G, k, offs, elems * 2, segments=3))  # S % G
        # a misaligned base under fp8: tensor 1 starts 8 bytes into its allocation
        big = [torch.zeros(nb * PART + 4, dtype=torch.bfloat16, device="cuda:0") for _ in range(G)]
        odd = conn.register_tensor_set([big[0][:nb * PART], big[1][4:]])
        refused(_raw(conn, "W", odd.set_id, G, _keys("never", nb), offs, elems * 2, flags=FP8))
        refused(_raw(conn, "W", ts.set_id, G, _keys("never", nb), offs + 8, elems * 2 - 32,
                     flags=FP8))  # misaligned offsets under fp8
        # the flag together with a slice: never built by the client, so by hand
        body = bytearray(ifs._native._dbg_build_packed_local(
            0, 1, 0, 0, elems * 2, 1, 0, bytes(64), [0], [keys[0]], G, 0,
            (2, elems * 2, 0, elems, elems), None))
        with pytest.raises(ValueError, match="INVALID_REQ"):
            flagged = bytearray(body)
            flagged[32] |= 32  # kLocalFlagTensorSet, without even its extension
            ifs._native._dbg_parse_packed_local("r", bytes(flagged))
        ret, _ = conn.conn.rw_tset_blob("R", conn.pack_keys(keys), offs.astype(np.uint64), 1,
                                        elems * 2, ts_out.set_id, G,
                                        _remap_device_id(outs[0]), True, 16, G, 0, False)
        refused(ret)  # kLocalFlagSliced without a slice extension, next to the set
        # a released id
        odd_id = odd.set_id
        conn.release_tensor_set(odd)
        refused(_raw(conn, "W", odd_id, G, _keys("never", nb), offs, elems * 2))
        # nothing above wrote anything
        assert all(bool((o == 7.0).all()) for o in outs)
        # the connection still serves: the legal read
        conn.read_pages(None, keys, table * PART, elems, tensor_set=ts_out)
        assert np.array_equal(bf16_bits(_gather(outs, table)), bf16_bits(pages))
    finally:
        conn.delete_keys(keys)
        conn.close()


def test_the_seventeenth_set_is_refused(gpu_server):
    conn = local_conn(gpu_server)
    try:
        t = [torch.zeros(PART, dtype=torch.bfloat16, device="cuda:0") for _ in range(2)]
        sets = [conn.register_tensor_set(t) for _ in range(conn.MAX_TENSOR_SETS)]
        assert conn.conn.register_tensor_set([x.data_ptr() for x in t], [PART * 2] * 2,
                                             _remap_device_id(t[0])) == -INVALID_REQ
        conn.release_tensor_set(sets[0])
        assert isinstance(conn.register_tensor_set(t), ifs.TensorSet)  # room again
    finally:
        conn.close()


@pytest.mark.parametrize("quant", QUANTS)
def test_key_not_found_leaves_every_tensor_untouched(gpu_server, quant):
    nb, G = 5, 3
    elems = G * PART
    pages = _pages(nb, elems, 41)
    table = _table(nb, 42)
    conn = local_conn(gpu_server)
    keys = _keys("nf", nb)
    try:
        ts = conn.register_tensor_set(_scatter(pages, table, G))
        conn.write_pages(None, keys, table * PART, elems, sync=True, quant=quant,
                         tensor_set=ts)
        outs = _blank(ts.tensors)
        ts_out = conn.register_tensor_set(outs)
        missing = keys[:3] + ["tset-no-such-key"] + keys[4:]
        with pytest.raises(Exception, match=str(KEY_NOT_FOUND)):
            conn.read_pages(None, missing, table * PART, elems, tensor_set=ts_out)
        assert all(bool((o == 7.0).all()) for o in outs)
    finally:
        conn.delete_keys(keys)
        conn.close()


def _distinct_allocations(count, numel, seen, spare):
    """`count` bf16 tensors of `numel` elements, each in an allocation (an IPC
    handle) that no tensor collected so far shares. Requests of this size get
    a segment of their own from the caching allocator unless it can split a
    block it has cached, so the cache is emptied first; a tensor that still
    lands in a shared segment is kept alive in `spare` and not used."""
    torch.cuda.empty_cache()
    out = []
    for _ in range(4 * count):
        t = torch.zeros(numel, dtype=torch.bfloat16, device="cuda:0")
        handle = ifs._native._dbg_ipc_export(t.data_ptr())[0]
        if handle in seen:
            spare.append(t)
            continue
        seen.add(handle)
        out.append(t)
        if len(out) == count:
            return out
    raise AssertionError(f"only {len(out)} of {count} distinct allocations")


def test_a_set_of_70_allocations_survives_the_mapping_cache_flush(gpu_server):
    """70 tensors of 12 MiB each, every one its own allocation and so its own
    IPC handle: six more than the connection's mapping cache holds. 70
    single-tensor requests on OTHER allocations then fill the cache and
    trigger its flush; the set's mappings must survive it."""
    G, nb, big = 70, 3, 6 << 20  # elements: 12 MiB of bf16
    elems = G * PART
    pages = _pages(nb, elems, 51)
    table = np.arange(nb)
    conn = local_conn(gpu_server)
    keys, other_keys = _keys("c70", nb), _keys("other", 70)
    seen, spare = set(), []
    try:
        tensors = _distinct_allocations(G, big, seen, spare)
        parts = pages.reshape(nb, G, PART)
        for g, t in enumerate(tensors):
            t[:nb * PART] = parts[:, g].reshape(-1).to("cuda:0")
        ts = conn.register_tensor_set(tensors)
        conn.write_pages(None, keys, table * PART, elems, sync=True, tensor_set=ts)
        del tensors
        others = _distinct_allocations(len(other_keys), big, seen, spare)  # all alive
        for k, o in zip(other_keys, others):
            conn.write_pages(o, [k], [0], PART, sync=True)
        for t in ts.tensors:
            t[:nb * PART] = 7.0
        torch.cuda.synchronize()
        conn.read_pages(None, keys, table * PART, elems, tensor_set=ts)
        got = torch.cat([t[:nb * PART].cpu().reshape(nb, PART) for t in ts.tensors], dim=1)
        assert np.array_equal(bf16_bits(got), bf16_bits(pages))
    finally:
        conn.delete_keys(keys + other_keys)
        conn.close()


@pytest.mark.parametrize("quant", QUANTS)
def test_tensors_of_unequal_size_are_bounded_by_the_smallest(gpu_server, quant):
    """Three tensors of 5, 3 and 9 blocks. Blocks 0..2 fit every tensor and
    round-trip; block 3 fits tensors 0 and 2 only, and a request for it is
    INVALID_REQ in both directions with nothing written."""
    G, sizes = 3, (5, 3, 9)
    elems = G * PART
    pages = _pages(3, elems, 61)
    conn = local_conn(gpu_server)
    keys = _keys("uneq", 3)
    try:
        parts = pages.reshape(3, G, PART)
        tensors = []
        for g, nblk in enumerate(sizes):
            t = torch.zeros(nblk * PART, dtype=torch.bfloat16)
            t[:3 * PART] = parts[:, g].reshape(-1)
            tensors.append(t.to("cuda:0"))
        ts = conn.register_tensor_set(tensors)
        offs = np.arange(3) * PART
        conn.write_pages(None, keys, offs, elems, sync=True, quant=quant, tensor_set=ts)
        outs = _blank(tensors)
        ts_out = conn.register_tensor_set(outs)
        with pytest.raises(ValueError):  # the Python layer refuses block 3
            conn.read_pages(None, keys[:1], [3 * PART], elems, tensor_set=ts_out)
        flags = conn.QUANT_MODES[quant][0] if quant else 0
        assert _raw(conn, "W", ts.set_id, G, _keys("never", 1), [3 * PART * 2], elems * 2,
                    flags=flags) == -INVALID_REQ
        assert _raw(conn, "R", ts_out.set_id, G, keys[:1], [3 * PART * 2],
                    elems * 2) == -INVALID_REQ
        assert all(bool((o == 7.0).all()) for o in outs)
        conn.read_pages(None, keys, offs, elems, tensor_set=ts_out)
        got = torch.cat([o[:3 * PART].cpu().reshape(3, PART) for o in outs], dim=1)
        assert np.array_equal(bf16_bits(got), _expected(pages, quant))
        assert all(bool((o[3 * PART:] == 7.0).all()) for o in outs)
    finally:
        conn.delete_keys(keys)
        conn.close()


def test_a_plain_entry_of_another_size_is_refused(gpu_server):
    """A set read asks for pages of the size the keys were written with: a
    smaller stored block would be read past its end."""
    G = 2
    conn = local_conn(gpu_server)
    keys = _keys("size", 1)
    try:
        src = torch.ones(PART, dtype=torch.bfloat16, device="cuda:0")
        conn.write_pages(src, keys, [0], PART, sync=True)  # half the set's page
        outs = [torch.full((PART,), 7.0, dtype=torch.bfloat16, device="cuda:0") for _ in range(G)]
        ts = conn.register_tensor_set(outs)
        with pytest.raises(Exception, match=str(INVALID_REQ)):
            conn.read_pages(None, keys, [0], G * PART, tensor_set=ts)
        assert all(bool((o == 7.0).all()) for o in outs)
    finally:
        conn.delete_keys(keys)
        conn.close()


# ---------------------------------------------------------------------------
# the adapter: one key, one write and one read per block for ALL layers
# ---------------------------------------------------------------------------
import json  # noqa: E402

from infinistore_amd.vllm_adapter import InfiniStoreKVAdapter  # noqa: E402

SEG = 256  # elements of K (or V) of one block of one layer
PAGE = 2 * SEG


def _stats(adapter):
    return json.loads(adapter._conn.conn.get_server_stats_remote())


@pytest.mark.parametrize("quant", QUANTS)
@pytest.mark.parametrize("layout", ["block_major", "kv_major"])
def test_fused_adapter_against_the_per_layer_adapter(gpu_server, layout, quant):
    """The same engine state saved and loaded by a fused and by a per-layer
    adapter (different block tables on the two sides): the loaded tensors are
    equal for plain and mxfp4 pages, and for fp8 equal to the reference of the
    fused page (one scale over all layers), where the per-layer adapter's
    differ. The fused save adds n_pages keys with ONE write request and its
    load is ONE read request; the per-layer one n_layers times as many."""
    n_layers, block_tokens, n_pages, nblk = 3, 4, 6, 8
    tokens = list(range(500, 500 + n_pages * block_tokens))
    pt = [int(b) for b in _table(nblk, 71)[:n_pages]]
    dt = [int(b) for b in _table(nblk, 72)[:n_pages]]
    pages = [_pages(n_pages, PAGE, 80 + li) * (4.0 ** li) for li in range(n_layers)]

    def make(layer_pages=None, table=None):
        c = torch.zeros(nblk, 2, SEG, dtype=torch.bfloat16)
        if layer_pages is not None:
            c[torch.as_tensor(table)] = layer_pages.reshape(n_pages, 2, SEG)
        if layout == "kv_major":
            c = c.transpose(0, 1).contiguous()
        return c.to("cuda:0")

    def logical(cache, table):
        c = cache.cpu()
        if layout == "kv_major":
            c = c.transpose(0, 1)
        return c[torch.as_tensor(table)].reshape(n_pages, PAGE)

    def roundtrip(layer_pages):
        tag = f"fusedtest-{layer_pages}-{uuid.uuid4().hex[:8]}"
        kw = dict(kv_layout=layout, quant=quant, layer_pages=layer_pages)
        pa = InfiniStoreKVAdapter("127.0.0.1", gpu_server, tag, n_layers, block_tokens, PAGE, **kw)
        da = InfiniStoreKVAdapter("127.0.0.1", gpu_server, tag, n_layers, block_tokens, PAGE, **kw)
        try:
            sources = [make(pages[li], pt) for li in range(n_layers)]
            s0 = _stats(pa)
            for li in range(n_layers):
                pa.save_kv_layer(li, sources[li], tokens, pt)
            if layer_pages == "fused":  # save_kv_layer only records
                assert _stats(pa)["writes"] == s0["writes"]
            pa.wait_for_save()
            s1 = _stats(pa)
            assert da.get_num_new_matched_tokens(tokens) == len(tokens)
            caches = [make() for _ in range(n_layers)]
            assert da.start_load_kv(caches, tokens, dt) == n_pages
            for li in range(n_layers):
                assert da.wait_for_layer_load(li)
            s2 = _stats(pa)
            got = [logical(caches[li], dt) for li in range(n_layers)]
            counts = (s1["kv_len"] - s0["kv_len"], s1["writes"] - s0["writes"],
                      s2["reads"] - s1["reads"])
            assert pa.evict_request(tokens) == counts[0]
            return got, counts
        finally:
            pa.close()
            da.close()

    fused, fused_counts = roundtrip("fused")
    per_layer, per_layer_counts = roundtrip("per_layer")
    assert fused_counts == (n_pages, 1, 1)  # keys == blocks, not n_layers times it
    assert per_layer_counts == (n_layers * n_pages, n_layers, n_layers)
    whole = torch.cat(pages, dim=1)  # the fused page: the layers' parts in order
    want_fused = _expected(whole, quant).reshape(n_pages, n_layers, PAGE)
    for li in range(n_layers):
        assert np.array_equal(bf16_bits(fused[li]), want_fused[:, li]), li
        assert np.array_equal(bf16_bits(per_layer[li]), _expected(pages[li], quant)), li
        if quant != "fp8":  # everything but fp8's page-wide scale is layer-local
            assert torch.equal(fused[li].view(torch.int16), per_layer[li].view(torch.int16)), li


def test_fused_and_per_layer_keys_do_not_collide(gpu_server):
    """One model tag, both adapters: neither sees the other's pages."""
    n_layers, block_tokens, n_pages = 2, 4, 3
    tag = f"fusedtest-both-{uuid.uuid4().hex[:8]}"
    tokens = list(range(900, 900 + n_pages * block_tokens))
    table = list(range(n_pages))
    fa = InfiniStoreKVAdapter("127.0.0.1", gpu_server, tag, n_layers, block_tokens, PAGE,
                              layer_pages="fused")
    la = InfiniStoreKVAdapter("127.0.0.1", gpu_server, tag, n_layers, block_tokens, PAGE)
    try:
        caches = [_pages(n_pages, PAGE, 95 + li).reshape(-1).to("cuda:0") for li in range(n_layers)]
        for li in range(n_layers):
            fa.save_kv_layer(li, caches[li], tokens, table)
        fa.wait_for_save()
        assert fa.get_num_new_matched_tokens(tokens) == len(tokens)
        assert la.get_num_new_matched_tokens(tokens) == 0
        with pytest.raises(ValueError, match="every layer"):
            fa.save_kv_layer(0, caches[0], tokens, table)
            fa.wait_for_save()
    finally:
        fa.evict_request(tokens)
        fa.close()
        la.close()
