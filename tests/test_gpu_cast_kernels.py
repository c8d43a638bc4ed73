"""The six cast kernels of csrc/gpu/cast.hip, launched directly. Client side: a guarded
`SegArena` of e4m3fn codes; pool side: a guarded `Region`. Oracle: torch's e4m3 cast for
the two conversions, composed through the existing codec references, bit for bit."""

import numpy as np
import pytest
import torch

from infinistore_amd import _native

from _kernel_refs import (SENTINEL, Region, assert_bf16_bits_equal, assert_codes_equal,
                          bf16_bits, bf16_from_bits, fp8_dequant_ref, fp8_encode_ref,
                          fp8_quant_ref)
from _mxfp4_refs import E_NAN, dequant_ref, quant_ref
from _seg_refs import SegArena

pytestmark = pytest.mark.gpu

NONE, FP8, MXFP4 = ALL = 0, 1, 2  # codec ids
K_SCALE, V_SCALE = 0.0123, 3.7
LANES = 8 * _native._CAST_THREADS, 8 * _native._CAST_FP8_THREADS  # one sweep of a workgroup


def half_scales(scales, halves, N):  # (N,) float32: the scale of every element of a page
    s = np.asarray(scales, dtype=np.float32)
    return np.repeat(s[:halves] if halves == 2 else s[:1], N // halves)


def store_ref(codes, scales, halves):  # (n, N) uint8 codes -> the bf16 page, as a tensor
    x = torch.from_numpy(codes.copy()).view(torch.float8_e4m3fn).float()
    return (x * torch.from_numpy(half_scales(scales, halves, codes.shape[1]))).to(torch.bfloat16)


def load_ref(bits, scales, halves):  # (n, N) uint16 bf16 bits -> (n, N) uint8 codes
    inv = (np.float32(1.0) / half_scales(scales, halves, bits.shape[1])).astype(np.float32)
    return fp8_encode_ref(bf16_from_bits(bits).float() * torch.from_numpy(inv)).numpy()


def launch(codec, to_pool, client, pool, scales, N, cast, S, stride):  # -> (verdict, scales)
    if codec == NONE:
        return _native._dbg_copy_blocks_cast(client, pool, 2 * N, cast, S, stride, to_pool, 0), []
    return _native._dbg_transform_blocks_cast(codec, to_pool, client, pool, scales, N, cast, S,
                                              stride, 0)


def client_codes(codec, N, n):  # (n, N) uint8: every code, and each codec's edge pages
    g = torch.Generator().manual_seed(N * 31 + codec)
    c = torch.randint(0, 256, (n, N), dtype=torch.uint8, generator=g).numpy()
    c[(c & 0x7F) == 0x7F] ^= 1  # NaN codes only where they are put on purpose
    if codec == FP8:
        c[n - 1] &= 0xB7  # magnitudes below 1 ...
        c[n - 1, N - 1] = 0xFE  # ... and the page's absmax, -448, in the LAST element of V
    if N >= 256:
        c[0, :256] = np.arange(256)  # all 256 codes, the two NaNs included
    if codec == MXFP4:
        c[n // 2, N - 3] = 0x7F  # a NaN in the LAST group
    return c


CASES = [(c, N, h, S, 3) for c in ALL for N in (64, *(L + d for L in LANES for d in (-64, 0, 64)))
         for h in (1, 2) for S in (1, 2)]
CASES += [(c, 1 << 17, 2, S, 1) for c in ALL for S in (1, 2)]  # one block of many chunks
CASES += [(c, 2112, 2, 2, 600) for c in ALL]


@pytest.mark.parametrize("codec,N,halves,S,n", CASES)
def test_cast(codec, N, halves, S, n):  # store the client codes, then load the reference's blocks
    what = f"codec={codec} N={N} halves={halves} S={S} n={n}"
    cast = (1, halves, K_SCALE, V_SCALE)
    codes = client_codes(codec, N, n)
    b = store_ref(codes, cast[2:], halves)
    if N >= 256:
        assert len(set(codes[0].tolist())) == 256
    if codec == NONE:
        want, back, scales_in = bf16_bits(b).view(np.uint8), bf16_bits(b), []
    elif codec == FP8:
        q, want_scales = fp8_quant_ref(b)
        want, back = q.numpy(), bf16_bits(fp8_dequant_ref(q, want_scales))
        scales_in = list(map(float, want_scales))
        mag = b[n - 1].float().abs().nan_to_num(0.0)
        assert mag[N - 1] > mag[:N - 1].max(), "the absmax is the last element's alone"
    else:
        want, scales_in = quant_ref(bf16_bits(b)), []
        back = dequant_ref(want, N)
        assert want[n // 2, N // 2 + N // 32 - 1] == E_NAN, "the last group is NaN-scaled"
    # the load runs under other scales: K saturates (|x| / scale up to 16 * 448), V does not
    load_cast = (1, halves, K_SCALE / 16, V_SCALE * 3)
    want_client = load_ref(back, load_cast[2:], halves)
    assert ((want_client[:, :N // halves] & 0x7F) == 0x7E).any(), "some loads saturate"
    for to_pool in (True, False):
        fill = ("pattern", "sentinel") if to_pool else ("sentinel", "pattern")
        client = SegArena(n, S, N // S, "kv_major" if S == 2 else "gapped", fill=fill[0],
                          seed=N + to_pool)
        pool = Region(n, want.shape[1], fill=fill[1], seed=5 + to_pool)
        if to_pool:
            client.set_pages(torch.from_numpy(codes))
        else:
            pool.set_blocks(torch.from_numpy(want))
        dst, src = (pool, client) if to_pool else (client, pool)
        snap = src.t.clone()
        ok, scales = launch(codec, to_pool, client.ptrs, pool.ptrs, [] if to_pool else scales_in,
                            N, cast if to_pool else load_cast, S, client.stride)
        assert ok, what
        got = (pool.blocks() if to_pool else client.pages()).cpu().numpy()
        if not to_pool:
            assert_codes_equal(got, want_client, what)
            # the project's rule, not torch's: a NaN keeps the sign it has in the pool
            nan = (want_client & 0x7F) == 0x7F
            sign = {NONE: back >> 15, FP8: want >> 7, MXFP4: np.zeros_like(back)}[codec]
            assert (got[nan] >> 7 == sign[nan]).all(), what
        elif codec == NONE:
            got = np.ascontiguousarray(got).view(np.uint16)
            assert_bf16_bits_equal(got, want.view(np.uint16), what)
            nan = (codes & 0x7F) == 0x7F
            assert (got[nan] >> 15 == codes[nan] >> 7).all(), what
        elif codec == FP8:
            assert np.asarray(scales, dtype=np.float32).tobytes() == want_scales.tobytes(), what
            assert_codes_equal(got, want, what)
        else:
            assert (got == want).all(), what
        assert dst.guards_intact() and torch.equal(src.t, snap), what


GOOD = (1, 2, K_SCALE, V_SCALE)
# rule -> (cast, page elements, segments, stride, codecs, pointer misalignment, descriptor repeats);
# a rule of the cast alone is the same code for every codec and runs under one
REFUSED = {
    "elem_type_2": ((2, 2, 1.0, 1.0), 4096, 1, 0, (NONE,), 0, 1),
    "halves_3": ((1, 3, 1.0, 1.0), 3072, 1, 0, (FP8,), 0, 1),
    "scale_zero": ((1, 2, 0.0, 1.0), 4096, 1, 0, (MXFP4,), 0, 1),
    "scale_inf": ((1, 2, 1.0, float("inf")), 4096, 1, 0, (NONE,), 0, 1),
    "half_not_whole_units": (GOOD, 4096 + 8, 1, 0, (NONE, FP8), 0, 1),
    "half_not_whole_groups": (GOOD, 4096 + 32, 1, 0, (MXFP4,), 0, 1),
    "segments_overlap": (GOOD, 4096, 2, 2032, (NONE,), 0, 1),
    "stride_misaligned": (GOOD, 4096, 2, 2056, (FP8,), 0, 1),
    "segment_half_a_group": (GOOD, 4096 + 64, 4, 2048, (MXFP4,), 0, 1),
    "pointer_misaligned": (GOOD, 4096, 1, 0, ALL, 8, 1),
    "plain_to_the_transform_launcher": (GOOD, 4096, 1, 0, (-1,), 0, 1),
    # 2^21 blocks x 1024 segments of one group would be 2^31 workgroups: refused from the
    # counts alone, the descriptors are never read (the fp8 pair has one workgroup a page)
    "grid_does_not_fit": (GOOD, 32768, 1024, 32, (NONE, MXFP4), 0, 1 << 20),
}


@pytest.mark.parametrize("rule", REFUSED)
def test_cast_refusals(rule):
    """In-bounds addresses, a wrong cast, geometry, alignment or grid: False, nothing launched."""
    cast, N, S, stride, codecs, mis, rep = REFUSED[rule]
    n, room = 2, 1 << 16
    client = SegArena(n, 1, room, "gapped", fill="pattern", seed=1, misalign=mis)
    out = SegArena(n, 1, room, "gapped", fill="sentinel", seed=2, misalign=mis)
    pool, src_pool = (Region(n, room, fill=f, seed=3) for f in ("sentinel", "pattern"))
    for codec in codecs:
        for to_pool, c, p in ((True, client, pool), (False, out, src_pool)):
            scales = [1.0] * n * rep if codec == FP8 and not to_pool else []
            if codec < 0:  # codec "none" handed to the transform launcher
                ok, _ = _native._dbg_transform_blocks_cast(NONE, to_pool, c.ptrs, p.ptrs, [], N,
                                                           cast, S, stride, 0)
            else:
                ok, _ = launch(codec, to_pool, c.ptrs * rep, p.ptrs * rep, scales, N, cast, S,
                               stride)
            assert ok is False, (rule, codec, to_pool)
    assert bool((pool.t == SENTINEL).all()) and out.untouched(), "a refusal must not launch"
