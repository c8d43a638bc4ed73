"""The mxfp4 page codec (csrc/gpu/mxfp4_codec.h) on the host, through the
`_dbg_mxfp4_*` host bindings: the same text the quantize / dequantize kernels
compile, compared bit for bit with the independent numpy reference
(tests/_mxfp4_refs.py). Runs anywhere; the GPU side is in
test_gpu_mxfp4_kernels.py.

A group holding a NaN gets the scale byte 0xFF and decodes to NaN as a whole:
e2m1 has no NaN code, so the OCP convention marks the scale."""

import numpy as np
import pytest

from infinistore_amd import _native

from _kernel_refs import assert_bf16_bits_equal
from _mxfp4_refs import (
    E_NAN,
    GROUP,
    bits_to_f64,
    decode_ref,
    encode_ref,
    finite_patterns,
    group_exponent_ref,
    special_groups,
)

ALL_BITS = np.arange(65536, dtype=np.uint32).astype(np.uint16)


def native_encode(bits, E) -> np.ndarray:
    return np.frombuffer(
        _native._dbg_mxfp4_encode(np.ascontiguousarray(bits, dtype=np.uint16), int(E)),
        dtype=np.uint8)


def native_decode(codes, E) -> np.ndarray:
    return np.frombuffer(
        _native._dbg_mxfp4_decode(np.ascontiguousarray(codes, dtype=np.uint8), int(E)),
        dtype=np.uint16)


def native_exponent(group) -> int:
    return _native._dbg_mxfp4_group_exponent(np.ascontiguousarray(group, dtype=np.uint16))


def assert_same_codes(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (
        f"{what}: {bad.size} codes differ, first at {bad[0]}: "
        f"got {got[bad[0]]:#x} want {want[bad[0]]:#x}")


def natural_exponent(bits) -> np.ndarray:
    """Scale byte of a group whose absmax is this (finite, nonzero) value:
    from the exponent field, as the issue states the rule."""
    ef = ((np.asarray(bits, dtype=np.uint16) & 0x7FFF) >> 7).astype(np.int64)
    return np.maximum(ef - 2, 0)


@pytest.mark.parametrize("E", [0, 1, 2, 3, 125, 126, 127, 128, 129, 250, 251, 252])
def test_encode_every_pattern(E):
    assert_same_codes(native_encode(ALL_BITS, E), encode_ref(ALL_BITS, E), f"E={E}")


def test_encode_ties_and_saturation():
    """The rounding rule, spelled out at E = 127 (scale 1)."""
    import torch
    vals = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0, 7.0, 7.96875, 0.0, float("inf")]
    want = [0, 2, 2, 4, 4, 6, 6, 7, 7, 7, 0, 7]
    bits = torch.tensor(vals).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert native_encode(bits, 127).tolist() == want
    assert native_encode(bits | 0x8000, 127).tolist() == [w | 8 for w in want]
    assert encode_ref(bits, 127).tolist() == want


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_encode_under_natural_exponent(delta):
    """Each finite pattern under the scale its own magnitude would give a
    group, and under the neighbouring scales."""
    bits = finite_patterns()
    bits = bits[(bits & 0x7FFF) != 0]
    E = natural_exponent(bits) + delta
    keep = (E >= 0) & (E <= 254)
    bits, E = bits[keep], E[keep]
    want = encode_ref(bits, E)
    got = np.empty_like(want)
    for e in np.unique(E):
        sel = E == e
        got[sel] = native_encode(bits[sel], e)
    assert_same_codes(got, want, f"natural E{delta:+d}")
    if delta == 0:
        # the absmax element itself lands on 4 or 6 (or below, for E clamped at 0)
        mag = want & 7
        assert (mag[E > 0] >= 6).all()


def test_group_exponent_sweeps_every_magnitude():
    """32-element groups whose absmax is each finite magnitude pattern, at a
    varying position and sign, the rest strictly smaller."""
    mags = np.arange(1, 0x7F80, dtype=np.uint32)
    rs = np.random.RandomState(1)
    groups = (rs.randint(0, 1 << 30, (mags.size, GROUP)) % mags[:, None]).astype(np.uint16)
    groups |= (rs.randint(0, 2, groups.shape) << 15).astype(np.uint16)
    pos = np.arange(mags.size) % GROUP
    groups[np.arange(mags.size), pos] = (mags | ((mags & 1) << 15)).astype(np.uint16)
    want = group_exponent_ref(groups)
    assert (want == natural_exponent(mags)).all()
    got = np.array([native_exponent(g) for g in groups], dtype=np.uint8)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("name,want", [
    ("all_zero", 127), ("all_negative_zero", 127), ("only_inf", 127), ("one_nan", 0xFF),
    ("subnormals_only", 0), ("largest_finite", 252)])
def test_group_exponent_special(name, want):
    g = special_groups()[name]
    assert int(group_exponent_ref(g)) == want
    assert native_exponent(g) == want


def test_decode_every_code_every_exponent():
    """All 16 codes under every scale byte. Past E = 252, which the encoder
    never produces, the largest codes exceed the bf16 range and decode to
    +-inf, as the reference's cast does."""
    codes = np.arange(16, dtype=np.uint8)
    for E in list(range(255)) + [E_NAN]:
        assert_bf16_bits_equal(native_decode(codes, E), decode_ref(codes, E), f"E={E}")
    nan = native_decode(codes, E_NAN)
    assert ((nan & 0x7FFF) > 0x7F80).all()
    x = bits_to_f64(native_decode(codes, 252))
    assert np.isfinite(x).all() and x.max() == np.ldexp(6.0, 125)
    assert bits_to_f64(native_decode(codes, 0))[1] == np.ldexp(1.0, -128)


def test_roundtrip_bound():
    """Finite groups without inf: |decode(encode(x)) - x| < 2 * 2^(E-127).
    From the format: after scaling the group's absmax is below 8, grid gaps
    are at most 2 (error at most 1 inside the grid) and saturating (6, 8) to 6
    loses less than 2."""
    rs = np.random.RandomState(2)
    fin = finite_patterns()
    n = 4096
    # groups of mixed magnitude: a random exponent window per group
    groups = fin[rs.randint(0, fin.size, (n, GROUP))]
    narrow = (rs.randint(0, 0x7F80 - 0x400, n)[:, None] + rs.randint(0, 0x400, (n, GROUP)))
    groups[n // 2:] = (narrow[n // 2:] | (rs.randint(0, 2, (n // 2, GROUP)) << 15))
    groups = groups.astype(np.uint16)
    E = group_exponent_ref(groups)
    assert (E != E_NAN).all()
    got = np.empty_like(groups)
    for i in range(n):
        assert native_exponent(groups[i]) == E[i]
        got[i] = native_decode(native_encode(groups[i], E[i]), E[i])
    err = np.abs(bits_to_f64(got) - bits_to_f64(groups))
    bound = np.ldexp(2.0, E.astype(np.int64) - 127)[:, None]
    assert (err < bound).all(), float((err / bound).max())
    assert_bf16_bits_equal(got, decode_ref(encode_ref(groups, E[:, None]), E[:, None]))
