"""The fp8 e4m3fn page codec (csrc/gpu/fp8_codec.h) on the host, through the
`_dbg_fp8_*` bindings: the same text the quantize / dequantize kernels
compile, compared bit for bit with torch's float8_e4m3fn casts. Runs
anywhere; the GPU side is in test_gpu_kernels.py."""

import numpy as np
import pytest
import torch

from infinistore_amd import _native

from _kernel_refs import (
    BF16_MAX_BITS,
    all_bf16_patterns,
    assert_bf16_bits_equal,
    assert_codes_equal,
    bf16_bits,
    bf16_from_bits,
    every_pattern_page,
    fp8_dequant_ref,
    fp8_encode_ref,
    fp8_quant_ref,
    fp8_scales_ref,
)


def native_encode(y: torch.Tensor) -> np.ndarray:
    return np.frombuffer(_native._dbg_fp8_encode(y.contiguous().numpy()), dtype=np.uint8)


def native_decode(codes: np.ndarray, scale) -> np.ndarray:
    return np.frombuffer(
        _native._dbg_fp8_decode(np.ascontiguousarray(codes, dtype=np.uint8), float(scale)),
        dtype=np.uint16)


def native_scale(page: torch.Tensor) -> np.float32:
    return np.float32(_native._dbg_fp8_scale(bf16_bits(page)))


def native_page_roundtrip(page: torch.Tensor):
    """scale -> encode -> decode of one page, as the two kernels compose it."""
    s = native_scale(page)
    inv = np.float32(1.0) / s
    codes = native_encode(page.float() * float(inv))
    return s, codes, native_decode(codes, s)


# Multipliers for the exhaustive encode test: powers of two (every subnormal
# tie of the bf16 grid is hit exactly) and others; large and small ones move
# the far ends of the bf16 range into (and out of) the e4m3 range.
INVS = [1.0, 0.5, 2.0 ** 7, 2.0 ** -9, 2.0 ** 110, 2.0 ** -120,
        float(np.float32(448.0) / np.float32(3.0)), float(np.float32(1.0) / np.float32(0.0123)),
        float(np.float32(1e-30)), float(np.float32(0.7))]


@pytest.mark.parametrize("inv", INVS)
def test_encode_every_bf16_pattern(inv):
    y = all_bf16_patterns().float() * inv  # fp32 multiply, as in the kernel
    assert_codes_equal(native_encode(y), fp8_encode_ref(y).numpy(), f"inv={inv!r}")


def test_encode_subnormal_ties_go_to_even():
    unit = 2.0 ** -9
    y = torch.tensor([k * unit for k in (0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5)])
    got = native_encode(torch.cat([y, -y]))
    assert got[:8].tolist() == [0, 2, 2, 4, 4, 6, 6, 8]
    assert got[8:].tolist() == [0x80 | c for c in (0, 2, 2, 4, 4, 6, 6, 8)]


def test_encode_special_values():
    inf = float("inf")
    y = np.array([0, 0, inf, -inf, 448.0, -448.0, 1e30, 0.0, -0.0, 464.0, 463.9],
                 dtype=np.float32)
    y.view(np.uint32)[:2] = [0x7FC00000, 0xFFC00001]  # +NaN, -NaN
    got = native_encode(torch.from_numpy(y)).tolist()
    assert got == [0x7F, 0xFF, 0x7E, 0xFE, 0x7E, 0xFE, 0x7E, 0x00, 0x80, 0x7E, 0x7E]


SCALES = [1.0, 2.0 ** -126, float(np.float32(3.0) / np.float32(448.0)),
          float(np.float32(3.3895314e38) / np.float32(448.0)), float(np.float32(0.1)), 2.0 ** -9]


@pytest.mark.parametrize("scale", SCALES)
def test_decode_every_code(scale):
    codes = np.arange(256, dtype=np.uint8)
    want = fp8_dequant_ref(torch.from_numpy(codes)[None, :], [scale])
    assert_bf16_bits_equal(native_decode(codes, scale), bf16_bits(want), f"scale={scale!r}")


def test_decode_nan_codes_are_nan():
    got = native_decode(np.array([0x7F, 0xFF, 0x7E, 0xFE], dtype=np.uint8), 1.0)
    assert (got[:2] & 0x7FFF > 0x7F80).all()
    assert bf16_from_bits(got[2:]).tolist() == [448.0, -448.0]


def _page(vals):
    return torch.tensor(vals, dtype=torch.float32).to(torch.bfloat16)


BF16_MAX = float(bf16_from_bits([BF16_MAX_BITS])[0])
SUBNORMALS = bf16_from_bits([0x0001, 0x807F, 0x0000, 0x8000, 0x0040, 0x0000, 0x0003, 0x0000])

SCALE_CASES = {
    "all_zero": (torch.zeros(16, dtype=torch.bfloat16), np.float32(1.0)),
    "only_negative_zero": (bf16_from_bits([0x8000] * 16), np.float32(1.0)),
    "one_inf": (_page([0.5, -2.0, float("inf"), 1.0] * 2), np.float32(2.0) / np.float32(448)),
    "one_nan": (_page([0.5, -2.0, float("nan"), 1.0] * 2), np.float32(2.0) / np.float32(448)),
    "all_non_finite": (_page([float("inf"), float("-inf"), float("nan"), float("inf")] * 2),
                       np.float32(1.0)),
    "largest_finite_bf16": (_page([1.0, -BF16_MAX, 0.0, 3.0] * 2),
                            np.float32(BF16_MAX) / np.float32(448)),
    "subnormals_and_zeros": (SUBNORMALS, np.float32(2.0 ** -126)),
}


@pytest.mark.parametrize("name", list(SCALE_CASES))
def test_scale_rule(name):
    page, want = SCALE_CASES[name]
    got = native_scale(page)
    assert got.tobytes() == np.float32(want).tobytes(), (name, got, want)
    assert fp8_scales_ref(page[None, :])[0].tobytes() == np.float32(want).tobytes()
    assert np.isfinite(np.float32(1.0) / got)
    # the whole page through the codec: as the reference, zeros stay zeros,
    # nothing finite turns non-finite
    s, codes, out = native_page_roundtrip(page)
    ref_codes, ref_s = fp8_quant_ref(page[None, :])
    assert_codes_equal(codes, ref_codes.numpy(), name)
    assert_bf16_bits_equal(out, bf16_bits(fp8_dequant_ref(ref_codes, ref_s)), name)
    back = bf16_from_bits(out).float()
    src = page.float()
    assert (back[src == 0] == 0).all()
    assert torch.isfinite(back[torch.isfinite(src)]).all()


@pytest.mark.parametrize("variant", ["absmax_448", "absmax_3", "untouched"])
def test_every_pattern_page_roundtrip(variant):
    page = every_pattern_page(variant)
    s, codes, out = native_page_roundtrip(page)
    ref_codes, ref_s = fp8_quant_ref(page[None, :])
    assert s.tobytes() == ref_s[0].tobytes()
    assert_codes_equal(codes, ref_codes.numpy(), variant)
    assert_bf16_bits_equal(out, bf16_bits(fp8_dequant_ref(ref_codes, ref_s)), variant)
    if variant == "absmax_448":
        assert s == np.float32(1.0)  # scale 1: the page IS the encoder input
