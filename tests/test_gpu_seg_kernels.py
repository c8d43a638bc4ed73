"""The six segmented kernels of csrc/gpu/gpu.hip, launched directly through
the `_dbg_*_seg` entry points (descriptors in pinned host memory, as the shard
does). The client side is a guarded, bounds-asserted arena (tests/_seg_refs.py)
in two arrangements, the pool side a `Region`; the oracle is always the
CONCATENATED page put through the existing references, compared bit for bit.
Guards must be intact on both sides and the source unmodified. Every refusal
is raised on the host before anything is launched."""

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
from _mxfp4_refs import dequant_ref, group_exponent_ref, quant_ref, stored_bytes
from _seg_refs import SegArena

pytestmark = pytest.mark.gpu

DEV = 0
FP8, MXFP4 = 1, 2  # codec ids
ARRANGEMENTS = ["gapped", "kv_major"]


def _same(a: torch.Tensor, b: torch.Tensor, what):
    if not torch.equal(a, b):
        bad = (a != b).nonzero()[0].tolist()
        raise AssertionError(f"{what}: block {bad[0]} byte {bad[1]} differs "
                             f"({int((a != b).sum())} bytes wrong)")


# ---------------------------------------------------------------------------
# copy kernels
# ---------------------------------------------------------------------------
def run_copy_seg(path, arrangement, n, S, seg_bytes, to_pool, *, gap=48, client_mis=0,
                 pool_mis=0):
    what = f"{path} {arrangement} n={n} S={S} seg={seg_bytes} to_pool={to_pool}"
    fill = ("pattern", "sentinel") if to_pool else ("sentinel", "pattern")
    client = SegArena(n, S, seg_bytes, arrangement, gap=gap, misalign=client_mis, fill=fill[0],
                      seed=n + seg_bytes)
    pool = Region(n, S * seg_bytes, misalign=pool_mis, fill=fill[1], seed=7 * n + S)
    src_before = (client.t if to_pool else pool.t).clone()
    _native._dbg_copy_blocks_seg(client.ptrs, pool.ptrs, S * seg_bytes, S, client.stride,
                                 to_pool, DEV, path)
    _same(pool.blocks(), client.pages(), what)
    if to_pool:
        assert pool.guards_intact(), f"{what}: bytes outside the pool blocks were written"
        assert torch.equal(client.t, src_before), f"{what}: the source was modified"
    else:
        assert client.guards_intact(), f"{what}: bytes outside the segments were written"
        assert torch.equal(pool.t, src_before), f"{what}: the source was modified"


# 16-byte units against the 512-thread workgroup: one, one below / at / one
# above a workgroup, and three sweeps plus one.
VEC_UNITS = [1, 511, 512, 513, 1537]


@pytest.mark.parametrize("to_pool", [True, False])
@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
@pytest.mark.parametrize("units", VEC_UNITS)
@pytest.mark.parametrize("n", [1, 3, 17])
@pytest.mark.parametrize("S", [2, 3])
def test_copy_vec_seg(S, n, units, arrangement, to_pool):
    run_copy_seg("vec", arrangement, n, S, units * 16, to_pool)


@pytest.mark.parametrize("to_pool", [True, False])
def test_copy_vec_seg_more_rows_than_the_workgroup_target(to_pool):
    """2049 blocks x 2 segments x 1 unit: 4098 (block, segment) rows exceed the
    ~4096-workgroup target, so chunks per segment clamps to 1."""
    run_copy_seg("vec", "kv_major", 2049, 2, 16, to_pool)


@pytest.mark.parametrize("S,units", [(2, 513), (3, 1)])
def test_stride_equal_to_segment_is_the_contiguous_copy(S, units):
    """stride == segment: the segmented kernel must write exactly what the
    contiguous `_dbg_copy_blocks` writes."""
    n, seg = 5, units * 16
    client = SegArena(n, S, seg, "gapped", gap=0, fill="pattern", seed=11)
    assert client.stride == seg
    a = Region(n, S * seg, fill="sentinel", seed=1)
    b = Region(n, S * seg, fill="sentinel", seed=2)
    _native._dbg_copy_blocks_seg(client.ptrs, a.ptrs, S * seg, S, seg, True, DEV, "vec")
    _native._dbg_copy_blocks(client.ptrs, b.ptrs, S * seg, DEV, "vec")
    _same(a.blocks(), b.blocks(), "segmented vs contiguous")
    assert a.guards_intact() and b.guards_intact()


@pytest.mark.parametrize("to_pool", [True, False])
@pytest.mark.parametrize("mis", range(1, 16))
@pytest.mark.parametrize("seg_bytes", [1, 15, 17, 513])
def test_copy_byte_seg(seg_bytes, mis, to_pool):
    """Odd segment sizes, page bases 1..15 bytes off a 16-byte boundary on the
    client side (and differently off on the pool side), stride = segment + 3."""
    run_copy_seg("byte", "gapped", 3, 2 + mis % 2, seg_bytes, to_pool, gap=3, client_mis=mis,
                 pool_mis=(7 * mis) % 16)


@pytest.mark.parametrize("to_pool", [True, False])
def test_copy_byte_seg_kv_major(to_pool):
    run_copy_seg("byte", "kv_major", 17, 3, 513, to_pool, gap=5, client_mis=9)


# ---------------------------------------------------------------------------
# fp8: one scale per PAGE, over all segments
# ---------------------------------------------------------------------------
def _fp8_pages(S, seg_elems):
    """Three pages. Page 0: small values, the only large ones in the LAST
    segment. Page 1: first segment all zero. Page 2: plain random. A scale
    taken per segment, or from the first segment, gives other codes for each."""
    g = torch.Generator().manual_seed(S * 100003 + seg_elems)
    x = torch.randn(3, S, seg_elems, generator=g)
    x[0] *= 2.0 ** -6
    x[0, S - 1, seg_elems - 1] = 300.0
    x[0, S - 1, 0] = -417.0
    x[1, 0] = 0.0
    x[1, 1:] *= 37.0
    x[2] *= 2.0 ** 9
    return x.reshape(3, S * seg_elems).to(torch.bfloat16)


@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
@pytest.mark.parametrize("seg_elems", [8, 4088, 4096, 4104])  # 8 per lane x 512 lanes
@pytest.mark.parametrize("S", [2, 3])
def test_fp8_seg(S, seg_elems, arrangement):
    pages = _fp8_pages(S, seg_elems)
    n, elems = pages.shape
    want_codes, want_scales = fp8_quant_ref(pages)
    seg_scales = fp8_quant_ref(pages.reshape(n * S, seg_elems))[1].reshape(n, S)
    # pages 0 and 1 are built so that no segment-0 scale is the page's
    assert (seg_scales[:2, 0] != want_scales[:2]).all(), "first-segment scales must differ"
    assert (seg_scales[0, :-1] != want_scales[0]).all() and seg_scales[1, 0] == 1.0
    what = f"fp8 {arrangement} S={S} seg={seg_elems}"

    # quantize: segmented bf16 -> contiguous stored blocks
    client = SegArena(n, S, 2 * seg_elems, arrangement, fill="pattern", seed=S + seg_elems)
    client.set_pages(pages)
    pool = Region(n, elems, fill="sentinel", seed=5)
    before = client.t.clone()
    scales = _native._dbg_quant_blocks_seg(FP8, client.ptrs, pool.ptrs, elems, S,
                                           client.stride, DEV)
    got_scales = np.asarray(scales, dtype=np.float32)
    assert got_scales.tobytes() == want_scales.astype(np.float32).tobytes(), (
        what, got_scales, want_scales)
    assert_codes_equal(pool.blocks().cpu().numpy(), want_codes.numpy(), what)
    assert pool.guards_intact(), f"{what}: bytes outside the pool blocks were written"
    assert torch.equal(client.t, before), f"{what}: the source was modified"

    # dequantize: contiguous stored blocks -> segmented bf16
    src = Region(n, elems, fill="pattern", seed=6)
    src.set_blocks(want_codes)
    out = SegArena(n, S, 2 * seg_elems, arrangement, fill="sentinel", seed=3 * S + seg_elems)
    before = src.t.clone()
    _native._dbg_dequant_blocks_seg(FP8, src.ptrs, out.ptrs, list(map(float, want_scales)),
                                    elems, S, out.stride, DEV)
    got = out.pages().cpu().numpy().view(np.uint16)
    assert_bf16_bits_equal(got, bf16_bits(fp8_dequant_ref(want_codes, want_scales)), what)
    assert out.guards_intact(), f"{what}: bytes outside the segments were written"
    assert torch.equal(src.t, before), f"{what}: the source was modified"


# ---------------------------------------------------------------------------
# mxfp4: codes and scale bytes at the page-global unit
# ---------------------------------------------------------------------------
G = _native._MXFP4_GROUPS_PER_ITER


def _mx_pages(n, elems, seed):
    """bf16 pages with a different magnitude per 32-element group."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(2.0, torch.randint(-20, 20, (n, elems // 32, 1), generator=g).float())
    x = torch.randn(n, elems // 32, 32, generator=g) * mag
    return x.reshape(n, elems).to(torch.bfloat16)


@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
@pytest.mark.parametrize("seg_groups", [1, G - 1, G, G + 1, 3 * G + 1])
@pytest.mark.parametrize("n", [1, 3, 17])
@pytest.mark.parametrize("S", [2, 3])
def test_mxfp4_seg(S, n, seg_groups, arrangement):
    seg_elems = 32 * seg_groups
    N = S * seg_elems
    pages = _mx_pages(n, N, S * 1000 + n * 10 + seg_groups)
    bits = bf16_bits(pages)
    want = quant_ref(bits)  # (n, N/2 + N/32)
    what = f"mxfp4 {arrangement} S={S} n={n} groups/seg={seg_groups}"

    client = SegArena(n, S, 2 * seg_elems, arrangement, fill="pattern", seed=n + seg_groups)
    client.set_pages(pages)
    pool = Region(n, stored_bytes(N), fill="sentinel", seed=9)
    before = client.t.clone()
    _native._dbg_quant_blocks_seg(MXFP4, client.ptrs, pool.ptrs, N, S, client.stride, DEV)
    got = pool.blocks().cpu().numpy()
    # the scale byte of group g of segment s sits at N/2 + s*seg_groups + g
    E = group_exponent_ref(bits.reshape(n, S, seg_groups, 32))
    for s in range(S):
        at = N // 2 + s * seg_groups
        assert (got[:, at:at + seg_groups] == E[:, s]).all(), f"{what}: scales of segment {s}"
    assert (got == want).all(), f"{what}: {(got != want).sum()} stored bytes differ"
    assert pool.guards_intact(), f"{what}: bytes outside the pool blocks were written"
    assert torch.equal(client.t, before), f"{what}: the source was modified"

    src = Region(n, stored_bytes(N), fill="pattern", seed=10)
    src.set_blocks(torch.from_numpy(want))
    out = SegArena(n, S, 2 * seg_elems, arrangement, fill="sentinel", seed=2 * n + seg_groups)
    before = src.t.clone()
    _native._dbg_dequant_blocks_seg(MXFP4, src.ptrs, out.ptrs, [], N, S, out.stride, DEV)
    assert_bf16_bits_equal(out.pages().cpu().numpy().view(np.uint16), dequant_ref(want, N), what)
    assert out.guards_intact(), f"{what}: bytes outside the segments were written"
    assert torch.equal(src.t, before), f"{what}: the source was modified"


# ---------------------------------------------------------------------------
# refusals: ValueError before any launch, the destination all sentinel
# ---------------------------------------------------------------------------
def test_seg_refusals():
    """All pointers are real, aligned and in bounds: only the geometry is
    wrong. Arenas are sized for the largest page asked for below."""
    n, S, seg = 3, 2, 256
    client = SegArena(n, 4, 1024, "gapped", fill="pattern", seed=1)
    pool = Region(n, 8192, fill="sentinel", seed=2)
    out = SegArena(n, 4, 1024, "gapped", fill="sentinel", seed=3)
    src_pool = Region(n, 8192, fill="pattern", seed=4)

    def copy_refused(nbytes, n_seg, stride, path="vec", cl=client.ptrs, pl=pool.ptrs):
        with pytest.raises(ValueError):
            _native._dbg_copy_blocks_seg(cl, pl, nbytes, n_seg, stride, True, DEV, path)
        assert bool((pool.t == SENTINEL).all()), "a refused request must not launch"
        with pytest.raises(ValueError):
            _native._dbg_copy_blocks_seg(out.ptrs[:len(cl)], src_pool.ptrs[:len(pl)], nbytes,
                                         n_seg, stride, False, DEV, path)
        assert out.untouched(), "a refused request must not launch"

    for path in ("vec", "byte"):
        copy_refused(S * seg, 0, seg + 48, path)  # no segments
        copy_refused(1025 * 16, 1025, 16, path)  # more than kMaxPageSegments
        copy_refused(S * seg + 32, 3, seg + 48, path)  # page % segments: 544 = 3 * 181 + 1
        copy_refused(S * seg, S, seg - 16, path)  # segments overlap
        copy_refused(0, S, seg, path)  # empty pages
    copy_refused(S * seg, S, seg + 8)  # vec path, stride % 16
    copy_refused(S * 248, S, 256)  # vec path, segment % 16
    copy_refused(S * seg, S, seg + 48, "warp")  # unknown path
    copy_refused(S * seg, S, seg + 48, "inline")  # no inline segmented kernel
    copy_refused(S * seg, S, seg + 48, cl=client.ptrs[:2])  # list lengths

    def transform_refused(codec, elems, n_seg, stride, src=client.ptrs, dst=pool.ptrs):
        with pytest.raises(ValueError):
            _native._dbg_quant_blocks_seg(codec, src, dst, elems, n_seg, stride, DEV)
        assert bool((pool.t == SENTINEL).all()), "a refused request must not launch"
        scales = [1.0] * len(dst) if codec == FP8 else []
        with pytest.raises(ValueError):
            _native._dbg_dequant_blocks_seg(codec, src_pool.ptrs[:len(src)], out.ptrs[:len(dst)],
                                            scales, elems, n_seg, stride, DEV)
        assert out.untouched(), "a refused request must not launch"

    for codec, group in ((FP8, 8), (MXFP4, 32)):
        ok = 4 * group  # elements per segment
        transform_refused(codec, S * ok, 0, 1024)
        transform_refused(codec, 1025 * group, 1025, 2 * group)
        transform_refused(codec, 3 * ok + group, 3, 1024)  # page % segments
        transform_refused(codec, S * ok, S, 2 * ok - 16)  # overlap
        transform_refused(codec, S * (ok + group // 2), S, 1024)  # half a group per segment
        transform_refused(codec, S * ok, S, 2 * ok + 8)  # stride % 16
        transform_refused(codec, S * ok, S, 1024, src=client.ptrs[:2])  # list lengths
    transform_refused(0, 256, S, 1024)  # plain pages do not transform
    transform_refused(3, 256, S, 1024)  # unknown codec
    with pytest.raises(ValueError):  # fp8 dequantize: one scale per block
        _native._dbg_dequant_blocks_seg(FP8, src_pool.ptrs, out.ptrs, [1.0], 64, 2, 1024, DEV)
    assert out.untouched()
    # page bases 8 bytes off a 16-byte boundary, on the segmented side
    odd = SegArena(n, 2, 256, "gapped", misalign=8, fill="pattern", seed=5)
    with pytest.raises(ValueError):
        _native._dbg_quant_blocks_seg(FP8, odd.ptrs, pool.ptrs, 256, 2, odd.stride, DEV)
    assert bool((pool.t == SENTINEL).all())
    odd_out = SegArena(n, 2, 256, "gapped", misalign=8, fill="sentinel", seed=6)
    with pytest.raises(ValueError):
        _native._dbg_dequant_blocks_seg(FP8, src_pool.ptrs, odd_out.ptrs, [1.0] * n, 256, 2,
                                        odd_out.stride, DEV)
    assert odd_out.untouched()
