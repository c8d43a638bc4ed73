// fp8 e4m3fn page codec: the scalar pieces of the quantize / dequantize
// kernels, written so the same text compiles as device code under hipcc and
// as plain host code under g++. The kernels in gpu.hip include this header,
// and the `_dbg_fp8_*` bindings call it on the host, so a CPU test runs the
// very code the GPU runs. The rules are spelled out in docs/design.md
// ("fp8 page codec").
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define IFS_FP8_HD __host__ __device__ __forceinline__
#else
#define IFS_FP8_HD inline
#endif

namespace ifs {
namespace fp8 {

IFS_FP8_HD uint32_t f32_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
IFS_FP8_HD float bits_f32(uint32_t u) { return __builtin_bit_cast(float, u); }

constexpr uint16_t kBf16AbsMask = 0x7fffu;
constexpr uint16_t kBf16Inf = 0x7f80u;  // |bits| >= this: inf or NaN

// Absmax accumulation runs on the bf16 magnitude BITS (monotone in |x|), so
// it needs no float compare and cannot be bent by a denormal mode. Non-finite
// elements do not take part.
IFS_FP8_HD uint32_t absmax_step(uint32_t acc, uint16_t bf16_bits) {
    uint32_t a = bf16_bits & kBf16AbsMask;
    return (a < kBf16Inf && a > acc) ? a : acc;
}

// Page scale from the largest finite bf16 magnitude (as bits; 0 when the page
// is all zeros or has no finite element): absmax/448, at least 2^-126 so that
// 1/scale stays finite, and 1 for an empty absmax.
IFS_FP8_HD float scale_from_absmax_bits(uint32_t absmax_bits) {
    if (absmax_bits == 0) return 1.f;
    float s = bits_f32(absmax_bits << 16) / 448.f;
    const float kMinScale = 1.17549435e-38f;  // 2^-126
    return s >= kMinScale ? s : kMinScale;
}

// f32 -> e4m3fn code, round-to-nearest-even everywhere (normal and subnormal
// range), finite values clamped to +-448. NaN -> 0x7f (sign kept), +-inf ->
// +-448 (0x7e / 0xfe), -0 -> 0x80.
IFS_FP8_HD uint8_t f32_to_e4m3(float f) {
    uint32_t bits = f32_bits(f);
    uint8_t sign = static_cast<uint8_t>((bits >> 24) & 0x80);
    uint32_t u = bits & 0x7fffffffu;
    if (u > 0x7f800000u) return sign | 0x7f;   // NaN
    if (u >= 0x43e00000u) return sign | 0x7e;  // |x| >= 448 (inf too) -> max
    int e = static_cast<int>(u >> 23) - 127;
    if (e < -6) {                   // subnormal range: unit 2^-9
        if (e < -10) return sign;   // below half a unit
        uint32_t full = 0x800000u | (u & 0x7fffffu);  // 1.m (24-bit)
        int shift = 14 - e;                           // 21..24
        uint32_t q = full >> shift;
        uint32_t rem = full & ((1u << shift) - 1u);
        uint32_t half = 1u << (shift - 1);
        if (rem > half || (rem == half && (q & 1u))) q++;  // ties to even
        return sign | static_cast<uint8_t>(q);             // 8 == min normal code
    }
    // RNE at mantissa bit 20.
    uint32_t rounded = u + 0x0007ffffu + ((u >> 20) & 1u);
    if (rounded >= 0x43e00000u) return sign | 0x7e;
    e = static_cast<int>(rounded >> 23) - 127;
    uint32_t m = (rounded >> 20) & 7u;
    return sign | static_cast<uint8_t>(((e + 7) << 3) | m);
}

// e4m3fn code -> f32 value. The NaN codes (0x7f / 0xff) come back as NaN.
IFS_FP8_HD float e4m3_to_f32(uint8_t v) {
    uint32_t sign = static_cast<uint32_t>(v & 0x80) << 24;
    uint32_t e = (v >> 3) & 0xfu;
    uint32_t m = v & 7u;
    if ((v & 0x7f) == 0x7f) return bits_f32(sign | 0x7fc00000u);
    if (e == 0) {
        float mag = static_cast<float>(m) * 0.001953125f;  // m * 2^-9
        return bits_f32(sign | f32_bits(mag));
    }
    return bits_f32(sign | ((e - 7 + 127) << 23) | (m << 20));
}

// f32 -> bf16 bits, round-to-nearest-even; NaN -> quiet NaN (sign kept).
IFS_FP8_HD uint16_t f32_to_bf16(float f) {
    uint32_t fb = f32_bits(f);
    if ((fb & 0x7fffffffu) > 0x7f800000u)
        return static_cast<uint16_t>(((fb >> 16) & 0x8000u) | 0x7fc0u);
    fb += 0x7fffu + ((fb >> 16) & 1u);
    return static_cast<uint16_t>(fb >> 16);
}

// What the dequantize kernel stores for one code.
IFS_FP8_HD uint16_t decode_to_bf16(uint8_t code, float scale) {
    return f32_to_bf16(e4m3_to_f32(code) * scale);
}

}  // namespace fp8
}  // namespace ifs
