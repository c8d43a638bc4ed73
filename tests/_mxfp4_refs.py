"""Independent numpy reference of the mxfp4 page codec (docs/design.md,
"mxfp4 page codec"). It shares no code with csrc/gpu/mxfp4_codec.h: values go
through float64, where the bf16 -> float64 conversion and ldexp by 127-E are
both exact, and the nearest grid value is found by brute force over the eight
of them. Plain module, no fixtures."""

import numpy as np
import torch

from _kernel_refs import bf16_bits, bf16_from_bits

GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
GROUP = 32
E_NAN = 0xFF
E_ONE = 127
BF16_MAX = float(np.ldexp(255.0, 120))  # 0x7f7f


def bits_to_f64(bits) -> np.ndarray:
    b = np.asarray(bits, dtype=np.uint16)
    with np.errstate(invalid="ignore"):  # signalling NaN patterns
        return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def group_exponent_ref(groups) -> np.ndarray:
    """(..., 32) uint16 bits -> scale byte E per group: floor(log2 absmax) -
    2 + 127 over the finite elements, clamped at 0; 127 without a nonzero
    finite element; 0xFF with a NaN."""
    x = bits_to_f64(groups)
    has_nan = np.isnan(x).any(axis=-1)
    mag = np.where(np.isfinite(x), np.abs(x), 0.0).max(axis=-1)
    _, e = np.frexp(mag)  # mag = m * 2^e, m in [0.5, 1): floor(log2) = e - 1
    E = np.maximum(e.astype(np.int64) - 1 + 125, 0)
    E = np.where(mag == 0, E_ONE, E)
    return np.where(has_nan, E_NAN, E).astype(np.uint8)


def encode_ref(bits, E) -> np.ndarray:
    """uint16 bits and scale byte(s) E (scalar or same shape) -> one e2m1 code
    per element (uint8, bit 3 sign). Nearest grid value of |x| * 2^(127-E),
    the even code on a tie, 6 for everything above 6 (inf too). Under
    E = 0xFF every code is 0. A NaN element under another E is, by the
    codec's definition, treated like inf."""
    bits = np.asarray(bits, dtype=np.uint16)
    E = np.broadcast_to(np.asarray(E, dtype=np.int64), bits.shape)
    y = np.ldexp(np.abs(bits_to_f64(bits)), 127 - np.where(E == E_NAN, 127, E))
    y = np.where(np.isnan(y), np.inf, y)
    with np.errstate(invalid="ignore"):
        d = np.abs(y[..., None] - GRID)
    d = np.where(np.isinf(y)[..., None], np.where(np.arange(8) == 7, 0.0, 1.0), d)
    cand = d == d.min(axis=-1, keepdims=True)
    assert (cand.sum(axis=-1)[y <= 8.0] <= 2).all()  # beyond, all are equally far: saturates
    # among the nearest, an even code first
    score = np.where(cand, np.arange(8) % 2, 2)
    code = score.argmin(axis=-1).astype(np.uint8)
    code = np.where(y > 6.0, 7, code).astype(np.uint8)
    code |= ((bits >> 12) & 8).astype(np.uint8)
    return np.where(E == E_NAN, 0, code).astype(np.uint8)


def decode_ref(codes, E) -> np.ndarray:
    """codes (one per element) and scale byte(s) E -> uint16 bf16 bits of
    grid[code] * 2^(E-127). The cast to bf16 is asserted exact wherever the
    value fits the bf16 range (always for E <= 252, all the encoder produces);
    beyond it the cast gives +-inf. E = 0xFF decodes to NaN."""
    codes = np.asarray(codes, dtype=np.uint8)
    E = np.broadcast_to(np.asarray(E, dtype=np.int64), codes.shape)
    v = np.ldexp(GRID[codes & 7], np.where(E == E_NAN, 127, E) - 127)
    v = np.where(codes & 8, -v, v)
    t = torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16)
    back = t.double().numpy()
    fits = np.abs(v) <= BF16_MAX
    assert (back[fits] == v[fits]).all(), "decode must be exact in bf16"
    assert np.isinf(back[~fits]).all()
    out = bf16_bits(t).reshape(codes.shape)
    nan_bits = (0x7FC0 | ((codes.astype(np.uint16) & 8) << 12)).astype(np.uint16)
    return np.where(E == E_NAN, nan_bits, out).astype(np.uint16)


def stored_bytes(elems: int) -> int:
    return elems // 2 + elems // GROUP


def quant_ref(pages_bits) -> np.ndarray:
    """(n, N) uint16 bits -> (n, N/2 + N/32) uint8 stored blocks: codes, the
    even element in the low nibble, then the scale bytes in group order."""
    bits = np.asarray(pages_bits, dtype=np.uint16)
    n, N = bits.shape
    assert N % GROUP == 0
    groups = bits.reshape(n, N // GROUP, GROUP)
    E = group_exponent_ref(groups)
    codes = encode_ref(groups, E[..., None]).reshape(n, N)
    packed = (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)
    return np.concatenate([packed, E], axis=1)


def dequant_ref(blocks, elems: int) -> np.ndarray:
    """(n, N/2 + N/32) uint8 stored blocks -> (n, N) uint16 bits."""
    blocks = np.asarray(blocks, dtype=np.uint8)
    n = blocks.shape[0]
    assert blocks.shape[1] == stored_bytes(elems)
    packed, E = blocks[:, : elems // 2], blocks[:, elems // 2 :]
    codes = np.empty((n, elems), dtype=np.uint8)
    codes[:, 0::2] = packed & 0xF
    codes[:, 1::2] = packed >> 4
    return decode_ref(codes, np.repeat(E, GROUP, axis=1))


def roundtrip_ref(pages: torch.Tensor) -> np.ndarray:
    """(n, N) bf16 pages -> uint16 bits of what a write + read returns."""
    return dequant_ref(quant_ref(bf16_bits(pages)), pages.shape[1])


# --- inputs shared by the CPU and GPU tests ----------------------------------
def finite_patterns() -> np.ndarray:
    """Every finite bf16 bit pattern, both signs."""
    b = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    return b[(b & 0x7FFF) < 0x7F80]


def special_groups() -> dict:
    """name -> (32,) uint16 bits."""
    rs = np.random.RandomState(3)
    finite = (rs.randint(0x3000, 0x4800, GROUP) | (rs.randint(0, 2, GROUP) << 15))
    one_nan = finite.copy()
    one_nan[17] = 0x7FC1
    tiny = rs.randint(0, 0x80, GROUP) | (rs.randint(0, 2, GROUP) << 15)
    tiny[5] = 0x007F
    largest = finite.copy()
    largest[9] = 0xFF7F
    only_inf = np.full(GROUP, 0x7F80)
    only_inf[1::2] = 0xFF80
    return {k: np.asarray(v, dtype=np.uint16) for k, v in {
        "all_zero": np.zeros(GROUP),
        "all_negative_zero": np.full(GROUP, 0x8000),
        "only_inf": only_inf,
        "one_nan": one_nan,
        "subnormals_only": tiny,
        "largest_finite": largest,
    }.items()}


def every_finite_pattern_pages() -> np.ndarray:
    """(2, 65536) uint16: each page holds every finite bf16 pattern once,
    zero-padded. Page 0 is shuffled, so a group mixes magnitudes from the
    whole exponent range (most elements vanish under the group's scale).
    Page 1 deals each run of 512 neighbouring magnitudes (four exponents,
    both signs) over 32 groups, so every group spans four exponents and every
    code and tie is reached."""
    p = finite_patterns()
    page0 = np.zeros(65536, dtype=np.uint16)
    page0[: p.size] = p[np.random.RandomState(9).permutation(p.size)]
    by_mag = np.zeros(65536, dtype=np.uint16)
    by_mag[: p.size] = p[np.argsort(p & 0x7FFF, kind="stable")]
    page1 = by_mag.reshape(64, GROUP, 32).transpose(0, 2, 1).reshape(-1)
    assert np.array_equal(np.sort(page0), np.sort(page1))
    return np.stack([page0, page1])
