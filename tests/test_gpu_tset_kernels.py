"""The six tensor-set kernels of csrc/gpu/gpu.hip, launched directly through
the `_dbg_*_tset` entry points (descriptors in pinned host memory, the table of
bases in the kernel arguments, as the shard does). The client side is a
`TensorSetArena` (tests/_tset_refs.py): every tensor its own guarded,
bounds-asserted `SegArena`, the table not in address order. The pool side is a
`Region`; the oracle is always the CONCATENATED page put through the existing
references, compared bit for bit. Guards must be intact on both sides and the
source unmodified. A launcher refusal returns False before anything is
launched."""

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
    bf16_from_bits,
    fp8_dequant_ref,
    fp8_quant_ref,
)
from _mxfp4_refs import E_NAN, dequant_ref, group_exponent_ref, quant_ref, stored_bytes
from _tset_refs import TensorSetArena

pytestmark = pytest.mark.gpu

DEV = 0
NONE, FP8, MXFP4 = 0, 1, 2  # codec ids
copy_tset = _native._dbg_copy_blocks_tset
transform_tset = _native._dbg_transform_blocks_tset


def _same(a: torch.Tensor, b: torch.Tensor, what):
    if not torch.equal(a, b):
        bad = (a != b).nonzero()[0].tolist()
        raise AssertionError(f"{what}: block {bad[0]} byte {bad[1]} differs "
                             f"({int((a != b).sum())} bytes wrong)")


# ---------------------------------------------------------------------------
# copy kernels
# ---------------------------------------------------------------------------
def run_copy(G, per, n, seg_bytes, to_pool, *, arrangement="gapped", force_byte=False, **kw):
    what = f"G={G} S/G={per} n={n} seg={seg_bytes} to_pool={to_pool} byte={force_byte} {kw}"
    fill = ("pattern", "sentinel") if to_pool else ("sentinel", "pattern")
    client = TensorSetArena(G, n, per, seg_bytes, arrangement, fill=fill[0],
                            seed=G + n + seg_bytes, **kw)
    pool = Region(n, client.nbytes, fill=fill[1], seed=7 * n + G)
    if to_pool:
        # the same pattern seed fills every tensor alike: make the parts differ
        g = torch.Generator().manual_seed(per * 131 + seg_bytes)
        client.set_pages(torch.randint(0, 256, (n, client.nbytes), dtype=torch.uint8,
                                       generator=g))
    snap = client.snapshot() if to_pool else pool.t.clone()
    ok = copy_tset(client.bases, client.offsets, pool.ptrs, client.nbytes, client.n_segments,
                   client.stride, to_pool, DEV, force_byte)
    assert ok, what
    _same(pool.blocks(), client.pages(), what)
    if to_pool:
        assert pool.guards_intact(), f"{what}: bytes outside the pool blocks were written"
        assert client.unchanged_since(snap), f"{what}: the source was modified"
    else:
        assert client.guards_intact(), f"{what}: bytes outside the segments were written"
        assert torch.equal(pool.t, snap), f"{what}: the source was modified"
    return client, pool


@pytest.mark.parametrize("to_pool", [True, False])
@pytest.mark.parametrize("force_byte", [False, True])
@pytest.mark.parametrize("units", [1, 513])  # 16-byte units: one lane, a sweep plus one
@pytest.mark.parametrize("per", [1, 2])
@pytest.mark.parametrize("G", [1, 2, 3, 128])
def test_copy_tset(G, per, units, force_byte, to_pool):
    run_copy(G, per, 3, units * 16, to_pool, force_byte=force_byte)


@pytest.mark.parametrize("to_pool", [True, False])
@pytest.mark.parametrize("seg_bytes", [8176, 8192, 8208])  # around one 512-lane sweep
def test_copy_tset_around_one_sweep(seg_bytes, to_pool):
    run_copy(3, 2, 5, seg_bytes, to_pool, arrangement="kv_major")


@pytest.mark.parametrize("to_pool", [True, False])
@pytest.mark.parametrize("per", [1, 2])
def test_copy_tset_tensors_of_different_sizes(per, to_pool):
    client, _ = run_copy(3, per, 4, 272, to_pool, arrangement="kv_major", extra=[0, 3, 1])
    assert len({p.t.numel() for p in client.parts}) == 3


@pytest.mark.parametrize("to_pool", [True, False])
@pytest.mark.parametrize("G,per", [(128, 1), (64, 2)])
def test_copy_tset_more_rows_than_the_workgroup_target(G, per, to_pool):
    """40 blocks x 128 segments of 64 B: 5120 (block, segment) rows exceed the
    ~4096-workgroup target, so chunks per segment clamps to 1."""
    run_copy(G, per, 40, 64, to_pool, arrangement="kv_major")


@pytest.mark.parametrize("per", [1, 2])
@pytest.mark.parametrize("units", [1, 513])
def test_one_tensor_equals_the_segmented_copy(per, units):
    """G = 1 is a segmented page (or, with one segment, a contiguous one) whose
    descriptor is split into base + offset: the result must be the segmented
    kernel's."""
    n, seg = 5, units * 16
    client, a = run_copy(1, per, n, seg, True)
    b = Region(n, client.nbytes, fill="sentinel", seed=2)
    ptrs = [client.bases[0] + o for o in client.offsets]
    _native._dbg_copy_blocks_seg(ptrs, b.ptrs, client.nbytes, per, client.stride, True, DEV,
                                 "vec")
    _same(a.blocks(), b.blocks(), "tensor set of one vs segmented")
    assert b.guards_intact()


@pytest.mark.parametrize("to_pool", [True, False])
@pytest.mark.parametrize("mis", range(1, 16))
def test_byte_kernel_one_misaligned_base(mis, to_pool):
    """Exactly one tensor's base is `mis` bytes off a 16-byte boundary, the
    others, every offset, segment and stride aligned: the launcher must take
    the byte kernel on its own."""
    misalign = [0, 0, 0]
    misalign[mis % 3] = mis
    run_copy(3, 1 + mis % 2, 3, 528, to_pool, misalign=misalign)


@pytest.mark.parametrize("to_pool", [True, False])
@pytest.mark.parametrize("seg_bytes,gap,shift", [(513, 3, 4096), (17, 3, 4097), (512, 48, 4099),
                                                 (512, 8, 4096)])
def test_byte_kernel_odd_segment_stride_or_offset(seg_bytes, gap, shift, to_pool):
    """Aligned bases; the segment, the stride or the offsets are not."""
    run_copy(3, 2, 3, seg_bytes, to_pool, gap=gap, off_shift=shift)


# ---------------------------------------------------------------------------
# fp8: one scale per PAGE, over all tensors
# ---------------------------------------------------------------------------
def _fp8_pages(G, per, seg_elems):
    """Three pages of G tensors x per segments. Page 0: small values, the only
    large ones in the LAST segment of the last tensor. Page 1: the first tensor
    all zero (with one tensor: its first segment, if it has two). Page 2: plain
    random."""
    S = G * per
    g = torch.Generator().manual_seed(S * 100003 + seg_elems)
    x = torch.randn(3, S, seg_elems, generator=g)
    x[0] *= 2.0 ** -6
    x[0, S - 1, seg_elems - 1] = 300.0
    x[0, S - 1, 0] = -417.0
    zero = per if G > 1 else S - 1
    x[1, :zero] = 0.0
    x[1, zero:] *= 37.0
    x[2] *= 2.0 ** 9
    return x.reshape(3, S * seg_elems).to(torch.bfloat16)


@pytest.mark.parametrize("seg_elems", [8, 4088, 4096, 4104])  # 8 per lane x 512 lanes
@pytest.mark.parametrize("G,per", [(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2)])
def test_fp8_tset(G, per, seg_elems):
    S = G * per
    pages = _fp8_pages(G, per, seg_elems)
    n, elems = pages.shape
    want_codes, want_scales = fp8_quant_ref(pages)
    if G > 1:
        # a scale taken per tensor, or from the first tensor, is not the page's
        part_scales = fp8_quant_ref(pages.reshape(n * G, elems // G))[1].reshape(n, G)
        assert (part_scales[:2, 0] != want_scales[:2]).all()
        assert (part_scales[0, :-1] != want_scales[0]).all() and part_scales[1, 0] == 1.0
    what = f"fp8 G={G} S/G={per} seg={seg_elems}"
    arrangement = "kv_major" if seg_elems > 8 else "gapped"

    client = TensorSetArena(G, n, per, 2 * seg_elems, arrangement, fill="pattern",
                            seed=S + seg_elems)
    client.set_pages(pages)
    pool = Region(n, elems, fill="sentinel", seed=5)
    snap = client.snapshot()
    ok, scales = transform_tset(FP8, True, client.bases, client.offsets, pool.ptrs, [], elems, S,
                                client.stride, DEV)
    assert ok, what
    got_scales = np.asarray(scales, dtype=np.float32)
    assert got_scales.tobytes() == want_scales.astype(np.float32).tobytes(), (
        what, got_scales, want_scales)
    assert_codes_equal(pool.blocks().cpu().numpy(), want_codes.numpy(), what)
    assert pool.guards_intact(), f"{what}: bytes outside the pool blocks were written"
    assert client.unchanged_since(snap), f"{what}: the source was modified"

    src = Region(n, elems, fill="pattern", seed=6)
    src.set_blocks(want_codes)
    out = TensorSetArena(G, n, per, 2 * seg_elems, arrangement, fill="sentinel",
                         seed=3 * S + seg_elems)
    before = src.t.clone()
    ok, _ = transform_tset(FP8, False, out.bases, out.offsets, src.ptrs,
                           list(map(float, want_scales)), elems, S, out.stride, DEV)
    assert ok, what
    got = out.pages().cpu().numpy().view(np.uint16)
    assert_bf16_bits_equal(got, bf16_bits(fp8_dequant_ref(want_codes, want_scales)), what)
    assert out.guards_intact(), f"{what}: bytes outside the segments were written"
    assert torch.equal(src.t, before), f"{what}: the source was modified"


def test_fp8_tset_128_tensors_absmax_in_the_last():
    """128 tensors of 8 elements each: the page's absmax sits in tensor 127,
    tensor 0 is all zero."""
    G, seg_elems, n = 128, 8, 3
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, G, seg_elems, generator=g) * 2.0 ** -5
    x[:, 0] = 0.0
    x[:, G - 1, 3] = torch.tensor([300.0, -417.0, 11.0])
    pages = x.reshape(n, G * seg_elems).to(torch.bfloat16)
    want_codes, want_scales = fp8_quant_ref(pages)
    client = TensorSetArena(G, n, 1, 2 * seg_elems, fill="pattern", seed=4)
    client.set_pages(pages)
    pool = Region(n, G * seg_elems, fill="sentinel", seed=5)
    ok, scales = transform_tset(FP8, True, client.bases, client.offsets, pool.ptrs, [],
                                G * seg_elems, G, 0, DEV)
    assert ok
    assert np.asarray(scales, dtype=np.float32).tobytes() == want_scales.tobytes()
    assert_codes_equal(pool.blocks().cpu().numpy(), want_codes.numpy(), "fp8 G=128")
    assert pool.guards_intact()
    out = TensorSetArena(G, n, 1, 2 * seg_elems, fill="sentinel", seed=6)
    ok, _ = transform_tset(FP8, False, out.bases, out.offsets, pool.ptrs,
                           list(map(float, want_scales)), G * seg_elems, G, 0, DEV)
    assert ok
    assert_bf16_bits_equal(out.pages().cpu().numpy().view(np.uint16),
                           bf16_bits(fp8_dequant_ref(want_codes, want_scales)), "fp8 G=128")
    assert out.guards_intact()


# ---------------------------------------------------------------------------
# mxfp4: codes and scale bytes at the page-global unit
# ---------------------------------------------------------------------------
GR = _native._MXFP4_GROUPS_PER_ITER


def _mx_pages(n, elems, seed):
    """bf16 pages with a different magnitude per 32-element group."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.pow(2.0, torch.randint(-20, 20, (n, elems // 32, 1), generator=g).float())
    x = torch.randn(n, elems // 32, 32, generator=g) * mag
    return x.reshape(n, elems).to(torch.bfloat16)


MX_CASES = [(G, per, sg) for G, per in [(1, 2), (2, 1), (2, 2), (3, 1), (3, 2)]
            for sg in (1, GR - 1, GR, GR + 1)]
MX_CASES += [(128, 1, 1), (128, 1, GR + 1)]  # the smallest and the largest segment only


@pytest.mark.parametrize("G,per,seg_groups", MX_CASES)
def test_mxfp4_tset(G, per, seg_groups):
    S, n = G * per, 3
    seg_elems = 32 * seg_groups
    N = S * seg_elems
    bits = bf16_bits(_mx_pages(n, N, S * 1000 + seg_groups)).copy()
    # a NaN in the last group of the last tensor: that group's scale byte is 0xFF
    bits[1, N - 5] = 0x7FC1
    pages = bf16_from_bits(bits)
    want = quant_ref(bits)  # (n, N/2 + N/32)
    assert want[1, -1] == E_NAN
    what = f"mxfp4 G={G} S/G={per} groups/seg={seg_groups}"

    client = TensorSetArena(G, n, per, 2 * seg_elems, fill="pattern", seed=G + seg_groups)
    client.set_pages(pages)
    pool = Region(n, stored_bytes(N), fill="sentinel", seed=9)
    snap = client.snapshot()
    ok, _ = transform_tset(MXFP4, True, client.bases, client.offsets, pool.ptrs, [], N, S,
                           client.stride, DEV)
    assert ok, what
    got = pool.blocks().cpu().numpy()
    # the scale bytes of tensor g sit at N/2 + g * per * seg_groups
    E = group_exponent_ref(bits.reshape(n, G, per * seg_groups, 32))
    for g in range(G):
        at = N // 2 + g * per * seg_groups
        assert (got[:, at:at + per * seg_groups] == E[:, g]).all(), f"{what}: scales of tensor {g}"
    assert (got == want).all(), f"{what}: {(got != want).sum()} stored bytes differ"
    assert pool.guards_intact(), f"{what}: bytes outside the pool blocks were written"
    assert client.unchanged_since(snap), f"{what}: the source was modified"

    src = Region(n, stored_bytes(N), fill="pattern", seed=10)
    src.set_blocks(torch.from_numpy(want))
    out = TensorSetArena(G, n, per, 2 * seg_elems, fill="sentinel", seed=2 * G + seg_groups)
    before = src.t.clone()
    ok, _ = transform_tset(MXFP4, False, out.bases, out.offsets, src.ptrs, [], N, S, out.stride,
                           DEV)
    assert ok, what
    assert_bf16_bits_equal(out.pages().cpu().numpy().view(np.uint16), dequant_ref(want, N), what)
    assert out.guards_intact(), f"{what}: bytes outside the segments were written"
    assert torch.equal(src.t, before), f"{what}: the source was modified"


# ---------------------------------------------------------------------------
# refusals: False before any launch, the destination all sentinel
# ---------------------------------------------------------------------------
def test_tset_refusals():
    """All addresses are real and in bounds, the arenas sized for the largest
    page asked for below: only the geometry or the alignment is wrong."""
    n = 3
    client = TensorSetArena(4, n, 4, 1024, fill="pattern", seed=1)
    out = TensorSetArena(4, n, 4, 1024, fill="sentinel", seed=3)
    pool = Region(n, 16384, fill="sentinel", seed=2)
    src_pool = Region(n, 16384, fill="pattern", seed=4)
    stride = client.stride
    assert stride == out.stride and stride % 16 == 0

    def copy_refused(nbytes, S, strd, bases_to=client.bases, bases_from=out.bases, byte=False):
        assert copy_tset(bases_to, client.offsets, pool.ptrs, nbytes, S, strd, True, DEV,
                         byte) is False
        assert bool((pool.t == SENTINEL).all()), "a refused request must not launch"
        assert copy_tset(bases_from, out.offsets, src_pool.ptrs, nbytes, S, strd, False, DEV,
                         byte) is False
        assert out.untouched(), "a refused request must not launch"

    for byte in (False, True):
        copy_refused(4096, 4, stride, [], [], byte)  # no tensors
        copy_refused(129 * 64, 129, stride, (client.bases * 33)[:129], (out.bases * 33)[:129], byte)  # G = 129
        copy_refused(4096, 6, stride, byte=byte)  # S % G: 6 segments over 4 tensors
        copy_refused(4096, 0, stride, byte=byte)  # no segments
        copy_refused(4096 + 4, 8, stride, byte=byte)  # page % S
        copy_refused(8 * 512, 8, 496, byte=byte)  # segments of a tensor overlap
        copy_refused(2048 * 4, 2048, 16, client.bases * 32, out.bases * 32, byte)  # S > 1024
    # legal: with one segment per tensor the stride is not looked at
    assert copy_tset(client.bases, client.offsets, pool.ptrs, 4096, 4, 1, True, DEV, False)
    assert pool.guards_intact()
    pool.t.fill_(SENTINEL)

    def transform_refused(codec, elems, S, strd, cl=client, ou=out, bases_to=None,
                          bases_from=None, offsets=None):
        ok, _ = transform_tset(codec, True, bases_to if bases_to is not None else cl.bases,
                               offsets or cl.offsets, pool.ptrs, [], elems, S, strd, DEV)
        assert ok is False
        assert bool((pool.t == SENTINEL).all()), "a refused request must not launch"
        scales = [1.0] * n if codec == FP8 else []
        ok, _ = transform_tset(codec, False, bases_from if bases_from is not None else ou.bases,
                               offsets or ou.offsets, src_pool.ptrs, scales, elems, S, strd, DEV)
        assert ok is False
        assert all(p.untouched() for p in ou.parts), "a refused request must not launch"

    for codec, group in ((FP8, 8), (MXFP4, 32)):
        ok_elems = 4 * group  # elements per segment
        transform_refused(codec, 8 * ok_elems, 8, stride, bases_to=[], bases_from=[])
        transform_refused(codec, 8 * ok_elems, 6, stride)  # S % G
        transform_refused(codec, {FP8: 320, MXFP4: 160}[codec], 12, stride)  # page % S
        transform_refused(codec, 8 * (ok_elems + group // 2), 8, stride)  # half a group
        transform_refused(codec, 8 * ok_elems, 8, stride + 8)  # stride % 16
        transform_refused(codec, 8 * ok_elems, 8, 2 * ok_elems - 16)  # overlap
        transform_refused(codec, 4 * (ok_elems + group // 2), 4, 0)  # one per tensor, half a group
        # exactly one base 8 bytes off, then every offset 8 bytes off
        odd = TensorSetArena(4, n, 2, 1024, misalign=[0, 0, 8, 0], fill="pattern", seed=5)
        odd_out = TensorSetArena(4, n, 2, 1024, misalign=[0, 8, 0, 0], fill="sentinel", seed=6)
        transform_refused(codec, 8 * ok_elems, 8, odd.stride, cl=odd, ou=odd_out)
        shifted = TensorSetArena(4, n, 2, 1024, off_shift=4104, fill="pattern", seed=7)
        shifted_out = TensorSetArena(4, n, 2, 1024, off_shift=4104, fill="sentinel", seed=8)
        transform_refused(codec, 8 * ok_elems, 8, shifted.stride, cl=shifted, ou=shifted_out)
    transform_refused(NONE, 8 * 64, 8, stride)  # plain pages do not transform
    with pytest.raises(ValueError):
        transform_tset(3, True, client.bases, client.offsets, pool.ptrs, [], 512, 8, stride, DEV)
    with pytest.raises(ValueError):  # fp8 dequantize: one scale per block
        transform_tset(FP8, False, out.bases, out.offsets, src_pool.ptrs, [1.0], 512, 8, stride,
                       DEV)
    with pytest.raises(ValueError):  # list lengths
        copy_tset(client.bases, client.offsets[:2], pool.ptrs, 4096, 4, stride, True, DEV, False)
    assert bool((pool.t == SENTINEL).all()) and out.untouched()


def test_grid_that_does_not_fit_is_refused():
    """2^31 / 1024 blocks of 1024 one-byte segments would need 2^31 workgroups.
    The launcher refuses from the counts alone: the descriptor arrays are
    never read, so a short list repeated stands in for them."""
    n = (1 << 31) // 1024
    client = TensorSetArena(2, 1, 512, 1, gap=0, fill="pattern", seed=1)
    pool = Region(1, 1024, fill="sentinel", seed=2)
    assert copy_tset(client.bases, client.offsets * n, pool.ptrs * n, 1024, 1024, 1, True, DEV,
                     True) is False
    assert bool((pool.t == SENTINEL).all())
    assert copy_tset(client.bases, client.offsets, pool.ptrs, 1024, 1024, 1, True, DEV, True)
    _same(pool.blocks(), client.pages(), "the same request with one block")
