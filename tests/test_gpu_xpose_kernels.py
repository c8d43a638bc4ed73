"""The five transpose kernels of csrc/gpu/transpose.hip, launched directly. Client
side: a guarded `SegArena`; pool side: a guarded `Region`. Oracle: the index formula of
core/page_codec.h in numpy, then the existing references, bit for bit."""

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
THC = [(8, 1, 32), (16, 3, 64), (24, 2, 96), (32, 2, 128)]
SEGS = {"one": lambda x: 1, "kv": lambda x: 2, "tile": lambda x: x[0] * x[2]}  # client segments


def geo(thc, eb=2, xv=1, halves=2):  # (outer, T, H, C, elem_bytes, x_k = 16 / eb, x_v)
    return (halves, *thc, eb, 16 // eb, xv)


def canonical(a, x, back=False):
    """(n, page) uint8 rows in client order -> stored order [o, T, H, C], or back."""
    halves, T, H, C, eb = x[:5]
    e = np.ascontiguousarray(a).view(f"u{eb}").reshape(len(a), halves, -1)
    out = []
    for o, xo in enumerate(x[5:5 + halves]):
        h = (e[:, o].reshape(-1, T, H, C // xo, xo).transpose(0, 2, 3, 1, 4) if back else
             e[:, o].reshape(-1, H, C // xo, T, xo).transpose(0, 3, 1, 2, 4))
        out.append(h.reshape(len(a), -1))
    return np.ascontiguousarray(np.concatenate(out, axis=1)).view(np.uint8)


def launch(codec, to_pool, client, pool, scales, page, x, S, stride):  # -> (verdict, scales)
    if codec == NONE:
        return _native._dbg_copy_blocks_xpose(client, pool, page, x, S, stride, to_pool, 0), []
    return _native._dbg_transform_blocks_xpose(codec, to_pool, client, pool, scales, page // 2, x,
                                               S, stride, 0)


def pages(codec, x, n):  # (n, page) uint8 in STORED order, with each codec's edge values
    N, C = prod(x[:5]) // 2, x[3]
    g = torch.Generator().manual_seed(N * 31 + codec)
    if codec == NONE:
        return torch.randint(0, 256, (n, 2 * N), dtype=torch.uint8, generator=g).numpy()
    mag = torch.pow(2.0, torch.randint(-20, 20, (n, N // 32, 1), generator=g).float())
    v = (torch.randn(n, N // 32, 32, generator=g) * (mag if codec == MXFP4 else 1)).reshape(n, -1)
    if codec == FP8:
        v[0] *= 2.0 ** -6
        v[0, N - 1] = -417.0  # the absmax in the LAST element, client and stored
        v[n // 2, :N // 2] = 0.0  # a page whose first half is zero
    bits = bf16_bits(v.to(torch.bfloat16)).copy()
    if codec == MXFP4:
        bits[n // 2, N - C + 5] = 0x7FC1  # a NaN in the first group of the LAST stored row
    return bits.view(np.uint8)


CASES = [(c, geo(thc, xv=xv, halves=h), seg, 3) for c in ALL for thc in THC for xv in (1, 2)
         for h in (1, 2) for seg in SEGS if seg != "kv" or h * thc[1] % 2 == 0]
CASES += [(c, x, "one", n) for c in ALL for x, n in [
    (geo((128, 1, 128)), 2), (geo((512, 1, 32)), 2),  # tiles of exactly 32 KiB
    (geo(THC[1]), 1), (geo(THC[1]), 600)]]
CASES += [(NONE, geo(thc, eb, xv, h), "one", 3) for thc in THC for eb in (1, 4) for xv in (1, 2)
          for h in (1, 2) if thc[0] % (16 // (xv * eb)) == 0]  # T runs fill whole units


@pytest.mark.parametrize("codec,x,seg,n", CASES)
def test_xpose(codec, x, seg, n):  # store the client pages, then load the reference's blocks
    what = f"codec={codec} {x} seg={seg} n={n}"
    canon, S, N = pages(codec, x, n), SEGS[seg](x), prod(x[:5]) // 2
    if codec == NONE:
        want, back, scales_in = canon, canon, []
    elif codec == FP8:
        codes, want_scales = fp8_quant_ref(bf16_from_bits(canon.view(np.uint16)))
        want, back = codes.numpy(), bf16_bits(fp8_dequant_ref(codes, want_scales))
        scales_in = list(map(float, want_scales))
    else:
        want, scales_in = quant_ref(canon.view(np.uint16)), []
        back = dequant_ref(want, N)
        scales = want[n // 2, N // 2:]  # the second half's scale bytes are the last of them
        assert scales[(N - x[3]) // 32] == E_NAN and (scales == E_NAN).sum() == 1
    for to_pool in (True, False):
        fill = ("pattern", "sentinel") if to_pool else ("sentinel", "pattern")
        client = SegArena(n, S, 2 * N // S, "kv_major" if seg == "kv" else "gapped", fill=fill[0],
                          seed=N + to_pool)
        pool = Region(n, want.shape[1], fill=fill[1], seed=5 + to_pool)
        if to_pool:
            client.set_pages(torch.from_numpy(canonical(canon, x, back=True)))
        else:
            pool.set_blocks(torch.from_numpy(want))
        dst, src = (pool, client) if to_pool else (client, pool)
        snap = src.t.clone()
        ok, scales = launch(codec, to_pool, client.ptrs, pool.ptrs, [] if to_pool else scales_in,
                            2 * N, x, S, client.stride)
        assert ok, what
        got = (pool.blocks() if to_pool else client.pages()).cpu().numpy()
        if not to_pool:
            want_client = canonical(np.ascontiguousarray(back).view(np.uint8), x, back=True)
            (np.testing.assert_array_equal if codec == NONE else assert_bf16_bits_equal)(
                got.view(np.uint16), want_client.view(np.uint16), what)
        elif codec == FP8:
            assert np.asarray(scales, dtype=np.float32).tobytes() == want_scales.tobytes(), what
            assert_codes_equal(got, want, what)
        else:
            assert (got == want).all(), what
        assert dst.guards_intact() and torch.equal(src.t, snap), what


LEGAL = geo(THC[1])  # a page of 12288 bytes
REFUSED = {  # rule -> (geometry, page bytes, segments, stride bytes, codecs, pointer misalignment)
    "count_zero": ((2, 0, 3, 64, 2, 8, 1), 12288, 1, 0, ALL, 0),
    "outer_3": ((3, 16, 2, 64, 2, 8, 1), 12288, 1, 0, ALL, 0),
    "elem_bytes_3": ((2, 16, 3, 64, 3, 4, 1), 18432, 1, 0, ALL, 0),
    "codec_elem_bytes": (geo((16, 3, 128), eb=1, xv=2), 12288, 1, 0, (FP8, MXFP4), 0),
    "inner_not_pow2": ((2, 16, 3, 96, 2, 6, 1), 18432, 1, 0, ALL, 0),
    "inner_over_16_bytes": ((2, 16, 3, 64, 2, 16, 1), 12288, 1, 0, ALL, 0),
    "tokens_not_whole_units": ((2, 12, 4, 64, 2, 8, 1), 12288, 1, 0, ALL, 0),
    "row_not_whole_units": ((2, 16, 4, 12, 2, 4, 4), 3072, 1, 0, ALL, 0),
    "row_half_an_mxfp4_group": ((2, 16, 12, 16, 2, 8, 1), 12288, 1, 0, (MXFP4,), 0),
    "product": (LEGAL, 12288 + 128, 1, 0, ALL, 0),
    "tile_one_row_over": ((2, 129, 1, 128, 2, 8, 8), 2 * 129 * 256, 1, 0, ALL, 0),
    "tiles_per_segment": (LEGAL, 12288, 4, 4096, ALL, 0),
    "segments_overlap": (LEGAL, 12288, 2, 4096, ALL, 0),
    "stride_misaligned": (LEGAL, 12288, 2, 6152, ALL, 0),
    "pointer_misaligned": (LEGAL, 12288, 1, 0, ALL, 8),
}


@pytest.mark.parametrize("rule", REFUSED)
def test_xpose_refusals(rule):
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
