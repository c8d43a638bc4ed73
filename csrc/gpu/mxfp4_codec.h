// OCP microscaling FP4 (MXFP4) page codec: the scalar pieces of the mxfp4
// quantize / dequantize kernels, written so the same text compiles as device
// code under hipcc and as plain host code under g++ (like fp8_codec.h). The
// kernels in gpu.hip include this header, and the `_dbg_mxfp4_*` host
// bindings call it, so a CPU test runs the very code the GPU runs. The rules
// are spelled out in docs/design.md ("mxfp4 page codec").
//
// Everything is integer arithmetic on the bf16 bits: 2^-127 and the bf16
// subnormals are f32 subnormals, so float math here would depend on the
// device's denormal mode.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define IFS_MXFP4_HD __host__ __device__ __forceinline__
#else
#define IFS_MXFP4_HD inline
#endif

namespace ifs {
namespace mxfp4 {

constexpr int kGroupElems = 32;         // elements sharing one e8m0 scale
constexpr uint8_t kScaleNan = 0xffu;    // e8m0 NaN: the whole group is NaN
constexpr uint8_t kScaleOne = 127u;     // 2^0, the scale of an empty group
constexpr uint32_t kKeyNan = 0x8000u;   // group key: a NaN was seen

// What one element contributes to its group's key: its magnitude bits when
// finite (monotone in |x|, as fp8::absmax_step), 0 for +-inf, and kKeyNan for
// NaN. The group key is the plain unsigned max of these, so it reduces across
// lanes with max() and a NaN anywhere wins.
IFS_MXFP4_HD uint32_t elem_key(uint16_t bf16_bits) {
    uint32_t a = bf16_bits & 0x7fffu;
    if (a < 0x7f80u) return a;
    return a == 0x7f80u ? 0u : kKeyNan;
}

IFS_MXFP4_HD uint32_t key_step(uint32_t acc, uint16_t bf16_bits) {
    uint32_t k = elem_key(bf16_bits);
    return k > acc ? k : acc;
}

// e8m0 scale byte E (value 2^(E-127)) from a group key: floor(log2 absmax)
// minus emax(e2m1) = 2, clamped at 0 (a bf16-subnormal absmax has exponent
// field 0 and lands there too); 127 for a group without a nonzero finite
// element; 0xFF for a group holding a NaN.
IFS_MXFP4_HD uint8_t group_exponent(uint32_t key) {
    if (key & kKeyNan) return kScaleNan;
    if (key == 0) return kScaleOne;
    uint32_t ef = key >> 7;
    return static_cast<uint8_t>(ef > 2 ? ef - 2 : 0);
}

// One bf16 -> e2m1 code (bit 3 sign, bits 2..0 index into the grid
// {0, .5, 1, 1.5, 2, 3, 4, 6}) of x * 2^(127-E), round to nearest, ties to
// the even code, everything above 6 (and +-inf) saturating to +-6. Under
// E = 0xFF the group decodes to NaN whatever its codes are; they are stored
// as 0. A NaN element under any other E (no kernel produces that) is treated
// by its magnitude bits, like inf.
IFS_MXFP4_HD uint8_t encode(uint16_t bf16_bits, uint8_t E) {
    if (E == kScaleNan) return 0;
    uint8_t sign = static_cast<uint8_t>((bf16_bits >> 12) & 8u);
    uint32_t a = bf16_bits & 0x7fffu;
    if (a >= 0x7f80u) return sign | 7u;
    uint32_t ef = a >> 7;
    // |x| = M * 2^(eff-134): M carries the hidden bit for normals.
    uint32_t M = (a & 0x7fu) | (ef ? 0x80u : 0u);
    int k = static_cast<int>(ef ? ef : 1u) - static_cast<int>(E);
    // |x| * 2^(127-E) = M * 2^(k-7), M <= 255.
    if (k >= 3) return sign | 7u;  // only normals get here: M >= 128, so >= 8
    if (k <= -3) return sign;      // < 255 * 2^-10 < 0.25
    uint32_t F = M << (k + 2);     // the scaled magnitude in units of 2^-9
    // One threshold between each pair of neighbouring grid values, at their
    // midpoint; the midpoint itself goes to the even code.
    uint32_t c = (F > 128u) + (F >= 384u) + (F > 640u) + (F >= 896u) + (F > 1280u) +
                 (F >= 1792u) + (F > 2560u);
    return sign | static_cast<uint8_t>(c);
}

// One e2m1 code -> bf16 bits of grid[code] * 2^(E-127), built from bits: the
// product has at most 2 significant bits, so it is exact in bf16 wherever it
// fits (every E the encoder produces, 0..252). Past the bf16 range (E > 252
// with the largest codes) it is +-inf, as a float cast would give. E = 0xFF
// is NaN for every code.
IFS_MXFP4_HD uint16_t decode(uint8_t code, uint8_t E) {
    uint16_t sign = static_cast<uint16_t>((code & 8u) << 12);
    if (E == kScaleNan) return sign | 0x7fc0u;
    uint32_t c = code & 7u;
    if (c == 0) return sign;
    // grid[c] = (1 + mbit/2) * 2^p; code 1 (0.5) is e2m1's subnormal.
    int p = c == 1 ? -1 : static_cast<int>(c >> 1) - 1;
    uint32_t mbit = c == 1 ? 0u : (c & 1u);
    int be = p + static_cast<int>(E);  // bf16 exponent field, -1..256
    if (be >= 255) return sign | 0x7f80u;
    if (be <= 0) {
        uint32_t full = 0x80u | (mbit << 6);  // 1.m with 7 fraction bits
        return sign | static_cast<uint16_t>(full >> (1 - be));
    }
    return sign | static_cast<uint16_t>((static_cast<uint32_t>(be) << 7) | (mbit << 6));
}

}  // namespace mxfp4
}  // namespace ifs
