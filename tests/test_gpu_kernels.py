"""The six HIP kernels of csrc/gpu/gpu.hip at their edge shapes, launched
directly through the `_dbg_*` entry points (descriptors in pinned host memory,
as the shard does) and through a running server, compared bit for bit with
plain references (tests/_kernel_refs.py). Every address handed to a kernel is
checked on the host against its tensor before the launch, and every refusal
case is rejected on the host before anything is launched."""

import uuid

import numpy as np
import pytest
import torch

import infinistore_amd as ifs
from infinistore_amd import _native

from _kernel_refs import (
    BF16_MAX_BITS,
    SENTINEL,
    Region,
    assert_bf16_bits_equal,
    assert_codes_equal,
    assert_copied,
    bf16_bits,
    bf16_from_bits,
    every_pattern_page,
    fingerprint_ref,
    fp8_dequant_ref,
    fp8_quant_ref,
)
from test_gpu import gpu_server, local_conn  # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

DEV = 0

# ---------------------------------------------------------------------------
# copy kernels, launched directly
# ---------------------------------------------------------------------------
# In 16-byte units: fewer units than the 512 threads, one below / at / one
# above the workgroup, and several sweeps plus one unit.
VEC_SIZES = [16, 48, 511 * 16, 512 * 16, 513 * 16, (3 * 512 + 1) * 16]


def run_copy(path, n_blocks, nbytes, src_mis=0, dst_mis=0):
    """Source and destination blocks sit in differently permuted, guarded
    slots, so descriptors are out of address order and non-contiguous."""
    src = Region(n_blocks, nbytes, misalign=src_mis, fill="pattern", seed=n_blocks + nbytes)
    dst = Region(n_blocks, nbytes, misalign=dst_mis, fill="sentinel", seed=7 * n_blocks + 1)
    _native._dbg_copy_blocks(src.ptrs, dst.ptrs, nbytes, DEV, path)
    assert_copied(src, dst, f"{path} n={n_blocks} bytes={nbytes} mis=({src_mis},{dst_mis})")


# 4097 blocks force chunks_per_block == 1; 17 and 4096 have want > 1 clamped
# by max_chunks. The large counts use small blocks to stay under 1 MB.
VEC_CASES = [(n, s) for n in (1, 17) for s in VEC_SIZES] + [
    (4096, 16), (4096, 48), (4097, 16), (4097, 48)]


@pytest.mark.parametrize("n_blocks,nbytes", VEC_CASES)
def test_copy_vec(n_blocks, nbytes):
    run_copy("vec", n_blocks, nbytes)


@pytest.mark.parametrize("n_blocks", [1, 17, 4097])
@pytest.mark.parametrize("dst_mis", [0, 1, 3, 8])
@pytest.mark.parametrize("src_mis", [0, 1, 3, 8])
@pytest.mark.parametrize("nbytes", [1, 7, 511, 513, 1000, 4099])
def test_copy_byte(nbytes, src_mis, dst_mis, n_blocks):
    run_copy("byte", n_blocks, nbytes, src_mis, dst_mis)


@pytest.mark.parametrize("n_blocks", [1, 15, 16])
@pytest.mark.parametrize("nbytes", VEC_SIZES)
def test_copy_inline(nbytes, n_blocks):
    run_copy("inline", n_blocks, nbytes)


def test_copy_inline_grid_stride_wraps():
    """16 blocks of 1 MiB + 16 bytes: more than 4096 x 256 units, so every
    thread of the capped grid goes round its loop more than once."""
    nbytes = (1 << 20) + 16
    assert 16 * (nbytes // 16) > 4096 * 256
    run_copy("inline", 16, nbytes)


def _assert_refused(exc, src_ptrs, dst, nbytes, path):
    with pytest.raises(exc):
        _native._dbg_copy_blocks(src_ptrs, dst.ptrs, nbytes, DEV, path)
    assert bool((dst.t == SENTINEL).all()), "a refused request must not launch"


def test_copy_refusals():
    """What a kernel cannot do is refused on the host. All pointers are real
    and in bounds anyway."""
    src = Region(17, 64, fill="pattern")
    dst = Region(17, 64, fill="sentinel", seed=3)
    _assert_refused(ValueError, src.ptrs, dst, 64, "inline")  # 17 blocks
    _assert_refused(ValueError, src.ptrs, dst, 40, "inline")  # size % 16
    _assert_refused(ValueError, src.ptrs, dst, 40, "vec")
    _assert_refused(ValueError, src.ptrs, dst, 0, "byte")
    _assert_refused(ValueError, src.ptrs, dst, 64, "warp")
    _assert_refused(ValueError, src.ptrs[:5], dst, 64, "vec")  # length mismatch
    odd = Region(17, 64, misalign=[0] * 16 + [8], fill="pattern")
    _assert_refused(ValueError, odd.ptrs, dst, 64, "vec")  # one pointer % 16
    odd16 = Region(16, 64, misalign=[0] * 15 + [4], fill="pattern")
    dst16 = Region(16, 64, fill="sentinel", seed=3)
    _assert_refused(ValueError, odd16.ptrs, dst16, 64, "inline")


# ---------------------------------------------------------------------------
# copy through the server: Shard::submit_copy picks the kernel
# ---------------------------------------------------------------------------
def _server_roundtrip(port, src, dst, page):
    conn = local_conn(port)
    keys = [f"kc-{uuid.uuid4().hex}-{i}" for i in range(src.n_blocks)]
    try:
        conn.write_pages(src.t, keys, src.offs, page, sync=True)
        conn.read_pages(dst.t, keys, dst.offs, page)
        conn.sync()
        assert_copied(src, dst, f"server n={src.n_blocks} page={page}")
    finally:
        conn.delete_keys(keys)
        conn.close()


@pytest.mark.parametrize("n_blocks", [3, 40])
def test_server_copy_uint8_odd_offsets(gpu_server, n_blocks):
    """uint8 pages of 1000 bytes at odd element offsets: byte kernel in both
    directions (3 blocks: the would-be inline batch; 40: the chunked path);
    reads land at odd offsets with the bytes around them untouched."""
    odd = [1 + 2 * (i % 7) for i in range(n_blocks)]
    src = Region(n_blocks, 1000, misalign=odd, fill="pattern", seed=n_blocks)
    dst = Region(n_blocks, 1000, misalign=odd[::-1], fill="sentinel", seed=n_blocks + 9)
    assert all(p % 2 == 1 for p in src.ptrs + dst.ptrs)
    _server_roundtrip(gpu_server, src, dst, 1000)


def test_server_copy_16_aligned_blocks_inline(gpu_server):
    src = Region(16, 4096, fill="pattern", seed=21)
    dst = Region(16, 4096, fill="sentinel", seed=22)
    assert all(p % 16 == 0 for p in src.ptrs + dst.ptrs)
    _server_roundtrip(gpu_server, src, dst, 4096)


def test_server_copy_one_odd_offset_takes_byte_path(gpu_server):
    """16 blocks, exactly one client offset odd: the whole job must leave the
    vector kernels and still be exact."""
    src = Region(16, 4096, misalign=[0] * 9 + [1] + [0] * 6, fill="pattern", seed=23)
    dst = Region(16, 4096, misalign=[0] * 4 + [3] + [0] * 11, fill="sentinel", seed=24)
    assert sum(p % 16 != 0 for p in src.ptrs) == 1 and sum(p % 16 != 0 for p in dst.ptrs) == 1
    _server_roundtrip(gpu_server, src, dst, 4096)


# ---------------------------------------------------------------------------
# fp8 quantize / dequantize, launched directly
# ---------------------------------------------------------------------------
def run_fp8(pages: torch.Tensor, what=""):
    """(n, elems) CPU bf16 pages through the quantize and dequantize kernels.
    Stored codes and scales, then the dequantized bf16, must equal the
    reference bit for bit; bytes around every block stay untouched.
    Returns the dequantized pages as a CPU bf16 tensor."""
    n, e = pages.shape
    src = Region(n, 2 * e, fill="sentinel", seed=e)
    src.set_blocks(pages)
    mid = Region(n, e, fill="sentinel", seed=e + 1)
    scales = _native._dbg_quant_blocks(src.ptrs, mid.ptrs, e, DEV)
    ref_codes, ref_scales = fp8_quant_ref(pages)
    got_scales = np.asarray(scales, dtype=np.float32)
    assert got_scales.tobytes() == ref_scales.tobytes(), (what, got_scales, ref_scales)
    assert_codes_equal(mid.blocks().cpu().numpy(), ref_codes.numpy(), f"{what} codes")
    assert mid.guards_intact(), f"{what}: quantize wrote outside its blocks"

    out = Region(n, 2 * e, fill="sentinel", seed=e + 2)
    _native._dbg_dequant_blocks(mid.ptrs, out.ptrs, scales, e, DEV)
    got = out.blocks().cpu().numpy().view(np.uint16)
    assert_bf16_bits_equal(got, bf16_bits(fp8_dequant_ref(ref_codes, ref_scales)),
                           f"{what} dequant")
    assert out.guards_intact(), f"{what}: dequantize wrote outside its blocks"
    return bf16_from_bits(got.reshape(-1)).reshape(n, e)


FP8_ELEMS = [8, 16, 511 * 8, 512 * 8, 513 * 8, (2 * 512 + 3) * 8]


@pytest.mark.parametrize("n_blocks", [1, 3, 65])
@pytest.mark.parametrize("elems", FP8_ELEMS)
def test_fp8_shapes(elems, n_blocks):
    g = torch.Generator().manual_seed(elems * 100 + n_blocks)
    mag = torch.logspace(-3, 3, n_blocks)[:, None]  # a different scale per page
    pages = (torch.randn(n_blocks, elems, generator=g) * mag).to(torch.bfloat16)
    run_fp8(pages, f"elems={elems} n={n_blocks}")


ABSMAX_ELEMS = (2 * 512 + 3) * 8
# one uint4 (8 elements) per thread per sweep: thread t first holds 8t..8t+7
ABSMAX_POS = {
    "element0": 0,
    "lane31": 8 * 31 + 3,
    "lane32": 8 * 32,
    "lane63": 8 * 63 + 7,
    "wave1_lane0": 8 * 64,
    "thread511": 8 * 511 + 5,
    "last_element": ABSMAX_ELEMS - 1,
}


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("where", list(ABSMAX_POS))
def test_fp8_absmax_position(where, sign):
    """A single absmax element, everything else at most half of it: a
    reduction that loses that one lane or wave gets the scale wrong."""
    g = torch.Generator().manual_seed(ABSMAX_POS[where])
    amax = torch.tensor([5.25, 3 * 2.0 ** -8, 1664.0])[:, None]  # three pages, exact in bf16
    pages = ((torch.rand(3, ABSMAX_ELEMS, generator=g) - 0.5) * amax).to(torch.bfloat16)
    pages[:, ABSMAX_POS[where]] = (sign * amax[:, 0]).to(torch.bfloat16)
    top = pages.float().abs()
    assert (top.argmax(dim=1) == ABSMAX_POS[where]).all()
    assert (top.sort(dim=1).values[:, -2] * 2 <= top.max(dim=1).values).all()
    run_fp8(pages, f"absmax at {where}")


@pytest.mark.parametrize("variant", ["absmax_448", "absmax_3", "untouched"])
def test_fp8_every_bf16_pattern(variant):
    page = every_pattern_page(variant)
    out = run_fp8(page[None, :], variant)[0]
    x = page.float()
    assert (out.float()[x == 0] == 0).all()
    assert torch.isfinite(out.float()[torch.isfinite(x)]).all()
    assert torch.isnan(out.float()[torch.isnan(x)]).all()


def _special_page(name, elems=513 * 8):
    if name == "all_zero":
        return torch.zeros(elems, dtype=torch.bfloat16)
    if name == "all_negative_zero":
        return bf16_from_bits(np.full(elems, 0x8000))
    rs = np.random.RandomState(5)
    if name == "tiny":  # bf16 subnormals (both signs) and zeros
        bits = rs.randint(0, 0x80, elems) | (rs.randint(0, 2, elems) << 15)
        bits[::3] = 0
        return bf16_from_bits(bits)
    assert name == "largest_finite"
    page = (torch.randn(elems) * 1e37).to(torch.bfloat16)
    page[::5] = 0
    page[elems // 2] = bf16_from_bits([BF16_MAX_BITS | 0x8000])[0]
    return page


@pytest.mark.parametrize("name", ["all_zero", "all_negative_zero", "tiny", "largest_finite"])
def test_fp8_special_pages(name):
    page = _special_page(name)
    out = run_fp8(page[None, :], name)[0].float()
    assert (out[page.float() == 0] == 0).all(), "zeros must read back as zeros"
    assert torch.isfinite(out).all(), "nothing finite may read back non-finite"


def test_fp8_refusals():
    pages = Region(3, 64, fill="pattern")
    codes = Region(3, 32, fill="sentinel", seed=1)
    odd_pages = Region(3, 64, misalign=[0, 2, 0], fill="pattern")
    odd_codes = Region(3, 32, misalign=[0, 0, 8], fill="sentinel", seed=1)
    for src, dst, elems in [(pages, codes, 12), (pages, codes, 0),
                            (odd_pages, codes, 32), (pages, odd_codes, 32)]:
        with pytest.raises(ValueError):
            _native._dbg_quant_blocks(src.ptrs, dst.ptrs, elems, DEV)
        assert bool((dst.t == SENTINEL).all())
    out = Region(3, 64, fill="sentinel", seed=2)
    odd_out = Region(3, 64, misalign=[2, 0, 0], fill="sentinel", seed=2)
    one = [1.0, 1.0, 1.0]
    for src, dst, scales, elems in [(pages, out, one, 12), (pages, odd_out, one, 32),
                                    (odd_pages, out, one, 32), (pages, out, one[:2], 32)]:
        with pytest.raises(ValueError):
            _native._dbg_dequant_blocks(src.ptrs, dst.ptrs, scales, elems, DEV)
        assert bool((dst.t == SENTINEL).all())


# ---------------------------------------------------------------------------
# fp8 through the server: fan-out, scale bookkeeping, refusals
# ---------------------------------------------------------------------------
def test_server_fp8_fanout_scales(gpu_server):
    """4100 pages of 8 elements in one request: more than one fan-out sub-job
    (4096 blocks each), every page with its own scale — a distinct odd factor
    times a power of two — so a scale stored against the wrong page shows."""
    n, e = 4100, 8
    g = torch.Generator().manual_seed(11)
    i = torch.arange(n)
    amax = (2.0 * (i % 128) + 1.0) * torch.pow(2.0, (i // 128 - 16).float())
    assert amax.unique().numel() == n
    pages = ((torch.rand(n, e, generator=g) - 0.5) * amax[:, None]).to(torch.bfloat16)
    pages[i, i % e] = (amax * torch.where(i % 2 == 0, 1.0, -1.0)).to(torch.bfloat16)
    assert torch.equal(pages.float().abs().max(dim=1).values, amax)  # exact in bf16
    ref_codes, ref_scales = fp8_quant_ref(pages)
    want = bf16_bits(fp8_dequant_ref(ref_codes, ref_scales))

    src = pages.to("cuda:0").reshape(-1)
    offs = np.arange(n, dtype=np.uint64) * e
    keys = [f"kq-{uuid.uuid4().hex}-{k}" for k in range(n)]
    conn = local_conn(gpu_server)
    try:
        conn.write_pages(src, keys, offs, e, sync=True, quant="fp8")
        dst = torch.zeros_like(src)
        conn.read_pages(dst, keys, offs, e)
        conn.sync()
        assert_bf16_bits_equal(bf16_bits(dst), want, "read back")
        # reversed key order: page j of dst now holds key n-1-j
        dst.zero_()
        conn.read_pages(dst, keys[::-1], offs, e)
        conn.sync()
        assert_bf16_bits_equal(bf16_bits(dst), want[::-1], "read back reversed")
    finally:
        conn.delete_keys(keys)
        conn.close()


def test_server_fp8_misaligned_refused(gpu_server):
    """A quantizing write from, or a dequantizing read into, an address that
    is not 16-byte aligned is refused — by the client library and, for a
    client that skips that check, by the server — and the connection keeps
    serving."""
    conn = local_conn(gpu_server)
    src = torch.randn(64, device="cuda:0").to(torch.bfloat16)
    dst = torch.zeros_like(src)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    pre = uuid.uuid4().hex
    try:
        with pytest.raises(Exception):
            conn.write_pages(src, [f"{pre}-a"], [4], 8, sync=True, quant="fp8")
        ret = conn.conn.rw_local_keys(
            conn.OP_W, [f"{pre}-b"], np.array([4], dtype=np.uint64), 2, 16, src.data_ptr(),
            0, True, conn.FLAG_QUANT_FP8)
        assert ret < 0, ret
        assert not conn.check_exist(f"{pre}-a") and not conn.check_exist(f"{pre}-b")

        conn.write_pages(src, [f"{pre}-c"], [8], 8, sync=True, quant="fp8")
        with pytest.raises(Exception):
            conn.read_pages(dst, [f"{pre}-c"], [4], 8)
        assert bool((dst == 0).all())
        conn.read_pages(dst, [f"{pre}-c"], [16], 8)
        conn.sync()
        ref_codes, ref_scales = fp8_quant_ref(src[8:16].cpu()[None, :])
        assert_bf16_bits_equal(bf16_bits(dst[16:24]),
                               bf16_bits(fp8_dequant_ref(ref_codes, ref_scales)))

        # a plain round trip on the same connection
        plain = torch.zeros_like(src)
        conn.write_pages(src, [f"{pre}-d"], [0], 64, sync=True)
        conn.read_pages(plain, [f"{pre}-d"], [0], 64)
        conn.sync()
        assert torch.equal(plain, src)
    finally:
        conn.delete_keys([f"{pre}-c", f"{pre}-d"])
        conn.close()


# ---------------------------------------------------------------------------
# fingerprint kernel
# ---------------------------------------------------------------------------
def _fingerprints(region):
    return _native.hash_blocks(region.base, [int(o) for o in region.offs], region.nbytes, DEV)


def _fingerprints_ref(region):
    return [fingerprint_ref(bytes(b), region.nbytes)[0] for b in region.blocks().cpu().numpy()]


@pytest.mark.parametrize("mis", [0, 1, 2, 4])
@pytest.mark.parametrize("n_blocks", [1, 5])
@pytest.mark.parametrize("nbytes", [1, 7, 8, 9, 2047, 2048, 2056, 4099])
def test_fingerprint_shapes(nbytes, n_blocks, mis):
    r = Region(n_blocks, nbytes, misalign=mis, fill="pattern", seed=nbytes + mis)
    assert all(p % 8 == mis for p in r.ptrs)
    assert _fingerprints(r) == _fingerprints_ref(r)


def test_fingerprint_is_over_bytes_not_addresses():
    a = Region(4, 4099, misalign=0, fill="pattern", seed=1)
    fa = _fingerprints(a)
    for mis in (1, 2, 4, 8):
        b = Region(4, 4099, misalign=mis, fill="sentinel", seed=mis)
        b.set_blocks(a.blocks())
        assert _fingerprints(b) == fa, mis


def test_fingerprint_sensitivity():
    r = Region(2, 4099, misalign=[0, 3], fill="pattern", seed=2)
    before = _fingerprints(r)
    data = r.blocks()
    assert not torch.equal(data[:, 8:16], data[:, 80:88])
    swapped = data.clone()
    swapped[:, 8:16], swapped[:, 80:88] = data[:, 80:88], data[:, 8:16]
    r.set_blocks(swapped)
    after_swap = _fingerprints(r)
    assert all(x != y for x, y in zip(before, after_swap)), "swapping two words must show"
    tail = swapped.clone()
    tail[:, 4098] ^= 0x10  # last of the 3 tail bytes
    r.set_blocks(tail)
    after_tail = _fingerprints(r)
    assert all(x != y for x, y in zip(after_swap, after_tail)), "a tail byte must show"
    assert after_tail == _fingerprints_ref(r)


def test_fingerprint_bf16_odd_element_offset():
    t = torch.randn(3 * 1029 + 8, device="cuda:0").to(torch.bfloat16)
    offs = [1, 1 + 1029, 7 + 2 * 1029]  # odd element offsets: 2-byte aligned only
    got = ifs.fingerprint_blocks(t, offs, 1029)
    raw = t.cpu().view(torch.int16).numpy().tobytes()
    assert got == [fingerprint_ref(raw[2 * o : 2 * (o + 1029)], 2 * 1029)[0] for o in offs]
