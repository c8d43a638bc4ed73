"""The three rotate kernels of csrc/gpu/rotate.hip, launched directly. Pool side: a guarded
`Region` holding the existing references' stored blocks; client side: a guarded `SegArena`.
Oracle: the rotation of the reference decode in float64.

Signed zeros: IEEE addition gives (-0) + (+0) = +0, so under the fixed arithmetic
fma(a, cos, -(b * sin)) an exact zero result may carry either sign (a = -0 under the identity
table comes back as +0 when b < 0). The bit-for-bit comparisons therefore map -0 to +0 on both
sides; every other value, and everything outside the rotary range, is compared by its bits."""

import numpy as np
import pytest
import torch

from infinistore_amd import PageRotate, _native

from _kernel_refs import (Region, assert_bf16_bits_equal, bf16_bits, fp8_dequant_ref,
                          fp8_quant_ref)
from _mxfp4_refs import bits_to_f64, dequant_ref, quant_ref
from _seg_refs import SegArena

pytestmark = pytest.mark.gpu

NONE, FP8, MXFP4 = ALL = 0, 1, 2  # codec ids
NEOX, GPTJ = 1, 2
SHAPES = [(1, 1, 32, 32), (3, 2, 64, 32), (16, 3, 128, 128)]  # T, heads, head_dim, rot_dim


def tables(heads, hd, rd):  # name -> float32 [P, 2]
    P = rd // 2
    one, zero = np.ones(P, np.float32), np.zeros(P, np.float32)
    return {"identity": np.stack([one, zero], 1), "quarter": np.stack([zero, one], 1),
            "delta37": PageRotate.from_delta(37, heads, hd, rot_dim=rd).cos_sin}


def make_blocks(codec, n, N, nan_at=None):
    """-> (stored uint8 (n, bytes), scales, decoded uint16 bits (n, N)); block i is scaled by
    i + 1, so every fp8 page has its own scale."""
    g = torch.Generator().manual_seed(N + codec)
    pages = (torch.randn(n, N, generator=g) * torch.arange(1, n + 1)[:, None]).to(torch.bfloat16)
    if nan_at is not None:
        pages.view(torch.int16)[n // 2, nan_at] = 0x7FC1
    if codec == NONE:
        return bf16_bits(pages).view(np.uint8), [], bf16_bits(pages)
    if codec == FP8:
        q, sc = fp8_quant_ref(pages)
        assert len(set(sc.tolist())) > 1 or n == 1, "the scale differs per block"
        return q.numpy(), list(map(float, sc)), bf16_bits(fp8_dequant_ref(q, sc))
    blk = quant_ref(bf16_bits(pages))
    return blk, [], dequant_ref(blk, N)


def pair_views(x, style, halves, T, heads, hd, rd):
    """Views (a, b) into x (n, N) of the two channels of every rotary pair of K."""
    k = x.reshape(x.shape[0], halves, T, heads, hd)[:, 0, :, :, :rd]
    return (k[..., :rd // 2], k[..., rd // 2:]) if style == NEOX else (k[..., 0::2], k[..., 1::2])


def canon(bits):  # -0 -> +0
    return np.where(bits == 0x8000, 0, bits).astype(np.uint16)


# rotate_legal wants whole mxfp4 groups in each half of a NeoX rotary range: rot_dim % 64 == 0
CASES = [(c, st, *sh, 2, 1, 3) for c in ALL for st in (NEOX, GPTJ) for sh in SHAPES
         if not (c == MXFP4 and st == NEOX and sh[3] % 64)]
CASES += [(c, st, 3, 2, 128, 64, h, S, 3) for c in ALL for st, h, S in
          ((NEOX, 1, 1), (GPTJ, 1, 2), (NEOX, 2, 2))]
CASES += [(c, NEOX, 512, 8, 128, 64, 2, 1, 1) for c in ALL]  # one block of many chunks
CASES += [(c, GPTJ, 3, 2, 128, 64, 2, 2, 600) for c in ALL]


@pytest.mark.parametrize("codec,style,T,heads,hd,rd,halves,S,n", CASES)
def test_rotate(codec, style, T, heads, hd, rd, halves, S, n):
    what = f"codec={codec} style={style} {(T, heads, hd, rd)} halves={halves} S={S} n={n}"
    N = halves * T * heads * hd
    # mxfp4: a NaN in the partner unit (NeoX) of the first row's first pairs
    nan_at = rd // 2 + 3 if codec == MXFP4 and n > 1 else None
    stored, scales, dec = make_blocks(codec, n, N, nan_at)
    pool = Region(n, stored.shape[1], fill="sentinel", seed=7)
    pool.set_blocks(torch.from_numpy(stored))
    snap = pool.t.clone()
    if codec != NONE:  # the existing contiguous load of the same blocks is the decode
        plain = Region(n, 2 * N, fill="sentinel", seed=8)
        _native._dbg_dequant_blocks_seg(codec, pool.ptrs, plain.ptrs, scales, N, 1, 0, 0)
        assert_bf16_bits_equal(plain.blocks().cpu().numpy().view(np.uint16), dec, what)
    x = bits_to_f64(dec)
    xa, xb = pair_views(x, style, halves, T, heads, hd, rd)
    da, db = pair_views(dec, style, halves, T, heads, hd, rd)
    rotated = np.zeros((n, N), bool)
    for v in pair_views(rotated, style, halves, T, heads, hd, rd):
        v[...] = True
    if nan_at is not None:
        assert np.isnan(xb[n // 2, 0, 0, :4] if style == NEOX else xa[n // 2, 0, 0]).any()
    for name, cs in tables(heads, hd, rd).items():
        client = SegArena(n, S, 2 * N // S, "kv_major" if S == 2 else "gapped", fill="sentinel",
                          seed=N + style)
        rot = (style, halves, heads, hd, rd, cs.reshape(-1))
        assert _native._dbg_load_rotated(codec, pool.ptrs, client.ptrs, scales, N, rot, S,
                                         client.stride, 0), (what, name)
        got = np.ascontiguousarray(client.pages().cpu().numpy()).view(np.uint16)
        assert client.guards_intact() and torch.equal(pool.t, snap), (what, name)
        # V and the non-rotary channels: the decode, bit for bit
        assert_bf16_bits_equal(got[~rotated], dec[~rotated], (what, name))
        c, s = cs[:, 0].astype(np.float64), cs[:, 1].astype(np.float64)
        ref, mag = np.zeros((n, N)), np.zeros((n, N))
        ra, rb = pair_views(ref, style, halves, T, heads, hd, rd)
        with np.errstate(invalid="ignore"):
            ra[...], rb[...] = xa * c - xb * s, xb * c + xa * s
        for v in pair_views(mag, style, halves, T, heads, hd, rd):
            v[...] = np.abs(xa) + np.abs(xb)
        ok = rotated & np.isfinite(ref)
        gv = bits_to_f64(got)
        assert (np.isnan(gv[rotated]) == np.isnan(ref[rotated])).all(), (what, name)
        if name == "delta37":
            err, bound = np.abs(gv - ref)[ok], (2.0 ** -8 * np.abs(ref) + 2.0 ** -21 * mag)[ok]
            assert (err <= bound).all(), (what, float((err - bound).max()))
            continue
        want = np.zeros((n, N), np.uint16)
        wa, wb = pair_views(want, style, halves, T, heads, hd, rd)
        wa[...], wb[...] = (da, db) if name == "identity" else (db ^ 0x8000, da)
        assert (canon(got)[ok] == canon(want)[ok]).all(), (what, name)


GOOD = (NEOX, 2, 2, 64, 64)
N_GOOD = 2 * 4 * 2 * 64
FINITE = np.ones(256, np.float32)
# rule -> (style, halves, heads, head_dim, rot_dim), page elements, segments, stride, codecs,
# pointer misalignment, table; a rule of the geometry alone runs under one codec
REFUSED = {
    "style_0": ((0, 2, 2, 64, 64), N_GOOD, 1, 0, (NONE,), 0, FINITE),
    "style_3": ((3, 2, 2, 64, 64), N_GOOD, 1, 0, (FP8,), 0, FINITE),
    "halves_3": ((NEOX, 3, 2, 64, 64), 3 * 4 * 2 * 64, 1, 0, (NONE,), 0, FINITE),
    "heads_0": ((NEOX, 2, 0, 64, 64), N_GOOD, 1, 0, (NONE,), 0, FINITE),
    "rot_dim_above_head_dim": ((NEOX, 2, 2, 64, 128), N_GOOD, 1, 0, (NONE,), 0, FINITE),
    "too_many_pairs": ((GPTJ, 2, 1, 512, 264), 2 * 512, 1, 0, (NONE,), 0, np.ones(264, "f4")),
    "neox_pairs_not_units": ((NEOX, 2, 2, 64, 24), N_GOOD, 1, 0, (NONE,), 0, FINITE),
    "gptj_rot_dim_not_units": ((GPTJ, 2, 2, 64, 12), N_GOOD, 1, 0, (FP8,), 0, FINITE),
    "head_dim_not_units": ((GPTJ, 2, 2, 60, 8), 2 * 4 * 2 * 60, 1, 0, (NONE,), 0, FINITE),
    "mxfp4_rot_dim_not_groups": ((GPTJ, 2, 2, 64, 16), N_GOOD, 1, 0, (MXFP4,), 0, FINITE),
    "mxfp4_neox_pairs_not_groups": ((NEOX, 2, 2, 64, 32), N_GOOD, 1, 0, (MXFP4,), 0, FINITE),
    "page_not_whole_tokens": (GOOD, N_GOOD + 64, 1, 0, ALL, 0, FINITE),
    "segment_cuts_a_row": ((NEOX, 1, 1, 64, 64), 3 * 64, 2, 512, (NONE,), 0, FINITE),
    "stride_misaligned": (GOOD, N_GOOD, 2, N_GOOD + 8, (NONE,), 0, FINITE),
    "table_inf": (GOOD, N_GOOD, 1, 0, (NONE,), 0, np.where(np.arange(256) == 5, np.inf, FINITE)),
    "table_nan": (GOOD, N_GOOD, 1, 0, (FP8,), 0, np.where(np.arange(256) == 63, np.nan, FINITE)),
    "pointer_misaligned": (GOOD, N_GOOD, 1, 0, ALL, 8, FINITE),
    "fp8_page_not_16_bytes": ((GPTJ, 1, 1, 8, 8), 8 + 4, 1, 0, (FP8,), 0, FINITE),
    "mxfp4_page_not_groups": ((GPTJ, 1, 1, 8, 8), 48, 1, 0, (MXFP4,), 0, FINITE),
}


@pytest.mark.parametrize("rule", REFUSED)
def test_rotate_refusals(rule):
    """In-bounds addresses, a wrong geometry, table or alignment: False, nothing launched."""
    geo, N, S, stride, codecs, mis, table = REFUSED[rule]
    n, room = 2, 1 << 16
    out = SegArena(n, 1, room, "gapped", fill="sentinel", seed=2, misalign=mis)
    src = Region(n, room, fill="pattern", seed=3)
    rot = (*geo, np.ascontiguousarray(table[:geo[4]], dtype=np.float32))
    for codec in codecs:
        scales = [1.0] * n if codec == FP8 else []
        assert _native._dbg_load_rotated(codec, src.ptrs, out.ptrs, scales, N, rot, S, stride,
                                         0) is False, (rule, codec)
    assert out.untouched(), "a refusal must not launch"
