"""The shuffle kernels of csrc/gpu/shuffle.hip, launched directly. Client side: a guarded
`SegArena`; pool side: a guarded `Region`. Oracle: the two index formulas of
core/page_codec.h as numpy reshapes, then the existing references, bit for bit."""

from math import prod

import numpy as np
import pytest
import torch

from infinistore_amd import _native

from _kernel_refs import (SENTINEL, Region, assert_bf16_bits_equal, assert_codes_equal,
                          bf16_bits, bf16_from_bits, fp8_dequant_ref, fp8_quant_ref)
from _mxfp4_refs import E_NAN, dequant_ref, quant_ref
from _seg_refs import SegArena

pytestmark = pytest.mark.gpu

NONE, FP8, MXFP4 = ALL = 0, 1, 2  # codec ids
K, V = 1, 2  # forms


def geo(thc, eb=2, forms=(K, V), outer=2):  # (outer, T, H, C, elem_bytes, form_k, form_v)
    return (outer, *thc, eb, *forms)


def canonical(a, x, back=False):
    """(n, page) uint8 rows in client order -> stored order [o, T, H, C], or back."""
    outer, T, H, C, eb = x[:5]
    X = 16 // eb
    e = np.ascontiguousarray(a).view(f"u{eb}").reshape(len(a), outer, -1)
    out = []
    for o, form in enumerate(x[5:5 + outer]):
        if form == K:  # client [H, C/X, T, X]
            h = (e[:, o].reshape(-1, T, H, C // X, X).transpose(0, 2, 3, 1, 4) if back else
                 e[:, o].reshape(-1, H, C // X, T, X).transpose(0, 3, 1, 2, 4))
        else:  # client [H, T/X, C, X]
            h = (e[:, o].reshape(-1, T // X, X, H, C).transpose(0, 3, 1, 4, 2) if back else
                 e[:, o].reshape(-1, H, T // X, C, X).transpose(0, 2, 4, 1, 3))
        out.append(h.reshape(len(a), -1))
    return np.ascontiguousarray(np.concatenate(out, axis=1)).view(np.uint8)


def launch(codec, to_pool, client, pool, scales, page, x, S, stride):  # -> (verdict, scales)
    if codec == NONE:
        return _native._dbg_copy_blocks_shuf(client, pool, page, x, S, stride, to_pool, 0), []
    return _native._dbg_transform_blocks_shuf(codec, to_pool, client, pool, scales, page // 2, x,
                                              S, stride, 0)


def pages(codec, x, n):  # (n, page) uint8 in STORED order, with each codec's edge values
    nbytes, C = prod(x[:5]), x[3]
    g = torch.Generator().manual_seed(nbytes * 31 + codec)
    if codec == NONE:
        return torch.randint(0, 256, (n, nbytes), dtype=torch.uint8, generator=g).numpy()
    N = nbytes // 2
    v = torch.randn(n, N, generator=g)
    if codec == MXFP4:
        v = (v.reshape(n, N // 32, 32) *
             torch.pow(2.0, torch.randint(-20, 20, (n, N // 32, 1), generator=g).float())
             ).reshape(n, N)
    else:
        v[0] *= 2.0 ** -6
        v[0, N - 1] = -417.0  # the absmax in the LAST element, client and stored
    bits = bf16_bits(v.to(torch.bfloat16)).copy()
    if codec == MXFP4:
        bits[n // 2, N - C + 5] = 0x7FC1  # a NaN in the first group of the LAST stored row
    return bits.view(np.uint8)


THC = [(16, 3, 64), (24, 2, 96), (256, 1, 128)]  # the last: a 64 KiB tile
CASES = [(c, geo(thc), 1, 3) for c in ALL for thc in [(8, 1, 32 if c == MXFP4 else 8)] + THC]
CASES += [(c, geo(THC[1], forms=f, outer=o), S, 3) for c in ALL
          for o, f in ((1, (K, V)), (1, (V, K)), (2, (K, V)), (2, (V, V))) for S in (1, 2)]
CASES += [(c, geo(thc), 1, n) for c in ALL
          for thc, n in ((THC[0], 1), (THC[0], 600), (THC[2], 1))]  # the last: 1024 squares
CASES += [(NONE, geo(thc, eb, f), S, 3) for eb, shapes in ((1, [(16, 1, 16), (32, 2, 48)]),
                                                           (4, [(4, 1, 4), (8, 2, 12)]))
          for thc in shapes for f in ((K, V), (V, K)) for S in (1, 2)]


@pytest.mark.parametrize("codec,x,S,n", CASES)
def test_shuf(codec, x, S, n):  # store the client pages, then load the reference's blocks
    what = f"codec={codec} {x} S={S} n={n}"
    canon, nbytes = pages(codec, x, n), prod(x[:5])
    N = nbytes // 2
    if codec == NONE:
        want, back, scales_in = canon, canon, []
    elif codec == FP8:
        codes, want_scales = fp8_quant_ref(bf16_from_bits(canon.view(np.uint16)))
        want, back = codes.numpy(), bf16_bits(fp8_dequant_ref(codes, want_scales))
        scales_in = list(map(float, want_scales))
    else:
        want, scales_in = quant_ref(canon.view(np.uint16)), []
        back = dequant_ref(want, N)
        assert want[n // 2, N // 2 + (N - x[3]) // 32] == E_NAN
    for to_pool in (True, False):
        fill = ("pattern", "sentinel") if to_pool else ("sentinel", "pattern")
        client = SegArena(n, S, nbytes // S, "kv_major" if S == 2 else "gapped", fill=fill[0],
                          seed=N + to_pool)
        pool = Region(n, want.shape[1], fill=fill[1], seed=5 + to_pool)
        if to_pool:
            client.set_pages(torch.from_numpy(canonical(canon, x, back=True)))
        else:
            pool.set_blocks(torch.from_numpy(want))
        dst, src = (pool, client) if to_pool else (client, pool)
        snap = src.t.clone()
        ok, scales = launch(codec, to_pool, client.ptrs, pool.ptrs, [] if to_pool else scales_in,
                            nbytes, x, S, client.stride)
        assert ok, what
        got = (pool.blocks() if to_pool else client.pages()).cpu().numpy()
        if not to_pool:
            want_client = canonical(np.ascontiguousarray(back).view(np.uint8), x, back=True)
            if codec == NONE:
                np.testing.assert_array_equal(got, want_client, what)
            else:
                assert_bf16_bits_equal(got.view(np.uint16), want_client.view(np.uint16), what)
        elif codec == FP8:
            assert np.asarray(scales, dtype=np.float32).tobytes() == want_scales.tobytes(), what
            assert_codes_equal(got, want, what)
        else:
            assert (got == want).all(), what
        assert dst.guards_intact() and torch.equal(src.t, snap), what


LEGAL = geo(THC[0])  # a page of 12288 bytes
REFUSED = {  # rule -> (geometry, page bytes, segments, stride bytes, codecs, pointer misalignment)
    "count_zero": ((2, 0, 3, 64, 2, K, V), 12288, 1, 0, ALL, 0),
    "outer_3": ((3, 16, 2, 64, 2, K, V), 12288, 1, 0, ALL, 0),
    "elem_bytes_3": ((2, 16, 3, 64, 3, K, V), 18432, 1, 0, ALL, 0),
    "codec_elem_bytes": (geo((16, 3, 128), eb=1), 12288, 1, 0, (FP8, MXFP4), 0),
    "form_0": (geo(THC[0], forms=(0, V)), 12288, 1, 0, ALL, 0),
    "form_3_in_the_unused_half": (geo(THC[0], forms=(K, 3), outer=1), 6144, 1, 0, ALL, 0),
    "tokens_not_whole_squares": (geo((12, 4, 64)), 12288, 1, 0, ALL, 0),
    "cols_not_whole_squares": (geo((16, 8, 12, )), 6144, 1, 0, ALL, 0),
    "row_half_an_mxfp4_group": (geo((16, 12, 16)), 12288, 1, 0, (MXFP4,), 0),
    "product": (LEGAL, 12288 + 128, 1, 0, ALL, 0),
    "squares_of_a_tile_wrap": (geo((1 << 19, 1, 1 << 19), outer=1), 1 << 39, 1, 0, ALL, 0),
    "tiles_wrap": (geo((8, 1 << 31, 8)), 1 << 39, 1, 0, ALL, 0),
    "page_of_2_31_squares": (geo((1 << 18, 1, 1 << 19), outer=1), 1 << 38, 1, 0, ALL, 0),
    "tiles_per_segment": (LEGAL, 12288, 4, 4096, ALL, 0),
    "segments_overlap": (LEGAL, 12288, 2, 4096, ALL, 0),
    "stride_misaligned": (LEGAL, 12288, 2, 6152, ALL, 0),
    "pointer_misaligned": (LEGAL, 12288, 1, 0, ALL, 8),
}


@pytest.mark.parametrize("rule", REFUSED)
def test_shuf_refusals(rule):
    """In-bounds addresses, a wrong geometry or alignment: False, nothing launched."""
    x, page, S, stride, codecs, mis = REFUSED[rule]
    n, room = 2, 1 << 17
    client = SegArena(n, 1, room, "gapped", fill="pattern", seed=1, misalign=mis)
    out = SegArena(n, 1, room, "gapped", fill="sentinel", seed=2, misalign=mis)
    pool, src_pool = (Region(n, room, fill=f, seed=3) for f in ("sentinel", "pattern"))
    for codec in codecs:
        for to_pool, c, p in ((True, client, pool), (False, out, src_pool)):
            scales = [1.0] * n if codec == FP8 and not to_pool else []
            ok, _ = launch(codec, to_pool, c.ptrs, p.ptrs, scales, page, x, S, stride)
            assert ok is False, (rule, codec, to_pool)
    assert bool((pool.t == SENTINEL).all()) and out.untouched(), "a refusal must not launch"
