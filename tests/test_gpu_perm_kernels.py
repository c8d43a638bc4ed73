"""The six permute kernels of csrc/gpu/gpu.hip, launched directly through the
`_dbg_*_perm` entry points. Client side: a guarded `SegArena` holding each page
as [outer, cols, rows, piece]; pool side: a guarded `Region`. Oracle: numpy's
transpose into the canonical page, through the existing references, bit for bit."""

import numpy as np
import pytest
import torch

from infinistore_amd import _native

from _kernel_refs import (SENTINEL, Region, assert_bf16_bits_equal, assert_codes_equal,
                          bf16_bits, bf16_from_bits, fp8_dequant_ref, fp8_quant_ref)
from _mxfp4_refs import E_NAN, dequant_ref, quant_ref
from _seg_refs import SegArena

pytestmark = pytest.mark.gpu

DEV = 0
NONE, FP8, MXFP4 = 0, 1, 2  # codec ids
T = _native._PERM_THREADS
copy_perm = _native._dbg_copy_blocks_perm
transform_perm = _native._dbg_transform_blocks_perm
GEOS = [(1, 3, 5), (2, 5, 3), (2, 1, 7), (2, 7, 1)]  # the last two are the identity
GEO_SEGS = [(g, S) for g in GEOS for S in (1, 2) if S <= g[0]]  # S = 2: K/V planes


def canonical(a, geo, back=False):
    """(n, page) rows in client order [o, c, r, piece] -> stored order, or back."""
    o, r, c = geo
    a = np.ascontiguousarray(a)
    shape = (len(a), o, r, c, -1) if back else (len(a), o, c, r, -1)
    return a.reshape(shape).transpose(0, 1, 3, 2, 4).reshape(len(a), -1)


def arena(n, page, S, fill, seed, **kw):
    return SegArena(n, S, page // S, "kv_major" if S == 2 else "gapped", fill=fill, seed=seed,
                    **kw)


def run_copy(geo, piece, to_pool, *, n=3, S=1, force_byte=False, **kw):
    what = f"{geo} piece={piece} n={n} S={S} to_pool={to_pool} byte={force_byte} {kw}"
    page = geo[0] * geo[1] * geo[2] * piece
    fill = ("pattern", "sentinel") if to_pool else ("sentinel", "pattern")
    client = arena(n, page, S, fill[0], n + piece, **kw)
    pool = Region(n, page, fill=fill[1], seed=7 * n + piece)
    dst, src = (pool, client) if to_pool else (client, pool)
    snap = src.t.clone()
    assert copy_perm(client.ptrs, pool.ptrs, page, (*geo, piece), S, client.stride, to_pool, DEV,
                     force_byte), what
    got, want = pool.blocks().cpu().numpy(), canonical(client.pages().cpu().numpy(), geo)
    assert (got == want).all(), f"{what}: {(got != want).sum()} bytes differ"
    assert dst.guards_intact() and torch.equal(src.t, snap), what
    return client, pool


@pytest.mark.parametrize("to_pool", [True, False])
@pytest.mark.parametrize("unit", [16, 1])  # the 16 B/lane kernel, the byte kernel
@pytest.mark.parametrize("geo", GEOS)
def test_copy_perm(geo, unit, to_pool):
    for units in (1, 3, 16, 17, 65):  # L rounding, lanes idle inside a piece
        client, pool = run_copy(geo, units * unit, to_pool, force_byte=unit == 1)
    if 1 in geo[1:]:  # the identity: the contiguous kernel's output, the page itself
        assert torch.equal(client.pages(), pool.blocks())


@pytest.mark.parametrize("to_pool", [True, False])
def test_copy_perm_steps_chunks_and_segments(to_pool):
    for units, geo in [(1, (1, 7, 73)), (1, (1, 16, 32)), (1, (1, 19, 27)),
                       (8, (2, 7, 9)), (8, (2, 8, 8)), (8, (2, 5, 13))]:
        assert geo[1] * geo[2] - T // units in (-1, 0, 1)  # around one workgroup step
        run_copy(geo, units * 16, to_pool, n=2)
    run_copy((2, 3, 5), 16, to_pool, n=2048)  # 4096 planes: chunks == 1
    run_copy((1, 40, 40), 256, to_pool, n=1)  # one block, 50 chunks of one step
    # 600 planes of 20 steps (32 pieces each): 7 chunks, so a workgroup takes
    # 2 or 3 steps, `chunks` steps apart (the walker all six kernels share)
    run_copy((1, 20, 32), 16, to_pool, n=600, force_byte=True)
    for mis in (1, 15):  # the launcher takes the byte kernel on its own
        run_copy((2, 5, 3), 48, to_pool, misalign=mis)  # client pointer
        run_copy((2, 5, 3), 48 + mis, to_pool)  # piece
        run_copy((2, 5, 3), 48, to_pool, S=2, gap=mis)  # client stride (kv-major)
    for force_byte in (False, True):
        run_copy((2, 5, 3), 80, to_pool, n=5, S=2, force_byte=force_byte)
        run_copy((2, 5, 3), 80, to_pool, S=30, force_byte=force_byte)  # a segment per piece


def run_transform(codec, geo, pages, S):
    """pages: (n, N) bf16 in CLIENT order. Quantize, then dequantize the
    reference's stored blocks; both against the references on the canonical page."""
    n, N = pages.shape
    what = f"codec={codec} {geo} N={N} S={S}"
    canon = bf16_from_bits(canonical(bf16_bits(pages), geo))
    if codec == FP8:
        codes, want_scales = fp8_quant_ref(canon)
        want, back = codes.numpy(), bf16_bits(fp8_dequant_ref(codes, want_scales))
        scales_in = list(map(float, want_scales))
    else:
        want, scales_in = quant_ref(bf16_bits(canon)), []
        back = dequant_ref(want, N)
    perm = (*geo, 2 * N // (geo[0] * geo[1] * geo[2]))
    client = arena(n, 2 * N, S, "pattern", N + S)
    client.set_pages(pages)
    pool = Region(n, want.shape[1], fill="sentinel", seed=5)
    snap = client.t.clone()
    ok, scales = transform_perm(codec, True, client.ptrs, pool.ptrs, [], N, perm, S,
                                client.stride, DEV)
    assert ok, what
    if codec == FP8:
        assert np.asarray(scales, dtype=np.float32).tobytes() == want_scales.tobytes(), what
        assert_codes_equal(pool.blocks().cpu().numpy(), want, what)
    else:
        assert (pool.blocks().cpu().numpy() == want).all(), what
    assert pool.guards_intact() and torch.equal(client.t, snap), what

    src = Region(n, want.shape[1], fill="pattern", seed=6)
    src.set_blocks(torch.from_numpy(want))
    out = arena(n, 2 * N, S, "sentinel", 3 * N + S)
    before = src.t.clone()
    ok, _ = transform_perm(codec, False, out.ptrs, src.ptrs, scales_in, N, perm, S, out.stride,
                           DEV)
    assert ok, what
    assert_bf16_bits_equal(out.pages().cpu().numpy().view(np.uint16),
                           canonical(back, geo, back=True), what)
    assert out.guards_intact() and torch.equal(src.t, before), what
    return want


@pytest.mark.parametrize("units", [1, 3, 16, 17, 65])
@pytest.mark.parametrize("geo,S", GEO_SEGS)
def test_fp8_perm(geo, S, units):
    pieces, pe = geo[0] * geo[1] * geo[2], units * 8
    x = torch.randn(3, pieces, pe, generator=torch.Generator().manual_seed(pieces + units))
    x[0] *= 2.0 ** -6
    x[0, pieces - 1, pe - 1] = -417.0  # the absmax in the LAST client piece
    x[1] = 0.0
    run_transform(FP8, geo, x.reshape(3, -1).to(torch.bfloat16), S)


@pytest.mark.parametrize("units", [4, 12, 20])  # whole 32-element groups: L = 4, 16, 32
@pytest.mark.parametrize("geo,S", GEO_SEGS + [((1, 16, 9), 1), ((2, 43, 3), 2)])  # > 1 step
def test_mxfp4_perm(geo, S, units):
    pieces, pe = geo[0] * geo[1] * geo[2], units * 8
    g = torch.Generator().manual_seed(pieces * 31 + units)
    mag = torch.pow(2.0, torch.randint(-20, 20, (3, pieces * pe // 32, 1), generator=g).float())
    x = (torch.randn(3, pieces * pe // 32, 32, generator=g) * mag).reshape(3, -1)
    bits = bf16_bits(x.to(torch.bfloat16)).copy()
    # a NaN in client piece (o=0, r=0, c=cols-1): stored piece cols-1, its first group
    bits[1, (geo[2] - 1) * geo[1] * pe + 5] = 0x7FC1
    want = run_transform(MXFP4, geo, bf16_from_bits(bits), S)
    scales = want[1, pieces * pe // 2:]
    assert scales[(geo[2] - 1) * pe // 32] == E_NAN and (scales == E_NAN).sum() == 1


def test_perm_refusals():
    """Real, in-bounds addresses: only the geometry, the alignment or the grid
    is wrong. False, and nothing launched."""
    n = 2
    client, out = arena(n, 8192, 1, "pattern", 1), arena(n, 8192, 1, "sentinel", 2)
    pool, src_pool = Region(n, 8192, fill="sentinel", seed=3), Region(n, 8192, fill="pattern", seed=4)
    odd = arena(n, 8192, 1, "sentinel", 5, misalign=8)

    def refused(codec, page, perm, S=1, stride=0, cl=client, ou=out, rep=1):
        for to_pool, c, p in ((True, cl, pool), (False, ou, src_pool)):
            if codec == NONE:
                ok = copy_perm(c.ptrs * rep, p.ptrs * rep, page, perm, S, stride, to_pool, DEV,
                               False)
            else:
                scales = [1.0] * n if codec == FP8 and not to_pool else []
                ok, _ = transform_perm(codec, to_pool, c.ptrs, p.ptrs, scales, page // 2, perm,
                                       S, stride, DEV)
            assert ok is False, (codec, page, perm, S, stride, to_pool)
        assert bool((pool.t == SENTINEL).all()) and ou.untouched(), "a refusal must not launch"

    for codec in (NONE, FP8, MXFP4):
        for perm in [(2, 0, 3, 64), (0, 5, 3, 64), (2, 5, 0, 64), (2, 5, 3, 0),  # a zero
                     (2, 5, 3, 192), (2, 5, 4, 64),  # does not tile the page
                     (1 << 16, 1 << 16, 1, 128)]:  # piece count, and its product wraps
            refused(codec, 3840, perm)
        refused(codec, 3840, (2, 5, 3, 128), S=4, stride=2048)  # pieces % S
        refused(codec, 3840, (2, 5, 3, 128), S=2, stride=1024)  # segments overlap
    refused(FP8, 30 * 24, (2, 5, 3, 24))  # half a lane unit
    refused(MXFP4, 30 * 96, (2, 5, 3, 96))  # half a group
    for codec in (FP8, MXFP4):
        refused(codec, 3840, (2, 5, 3, 128), cl=odd, ou=odd)  # no byte fallback
        refused(codec, 3840, (2, 5, 3, 128), S=2, stride=1928)  # stride % 16
    ok, _ = transform_perm(NONE, True, client.ptrs, pool.ptrs, [], 1920, (2, 5, 3, 128), 1, 0, DEV)
    assert ok is False and bool((pool.t == SENTINEL).all())  # plain pages do not transform
    # 2048 blocks x 2^20 planes would be 2^31 workgroups; refused from the
    # counts alone, the descriptors are never read
    refused(NONE, 1 << 20, (1 << 20, 1, 1, 1), rep=1024)
