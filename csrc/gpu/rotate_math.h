// Rotated reads: the arithmetic of one rotary pair, written so the same text
// compiles as device code under hipcc and as plain host code under g++ (like
// fp8_codec.h). The kernels of rotate.hip, the CPU shard and the `_dbg_rotate_*`
// host binding all call it. The rules are spelled out in docs/design.md
// ("rotated reads").
#pragma once

#include <cstdint>

#include "fp8_codec.h"

namespace ifs {
namespace rotate {

// One product and one fused multiply-add per output, each rounded once to
// nearest even, so the result does not depend on what a compiler contracts:
//     out_a = fma(a, cos, -(b * sin)),  out_b = fma(b, cos, a * sin).
IFS_FP8_HD void pair_f32(float a, float b, float c, float s, float* out_a, float* out_b) {
#if defined(__HIP_DEVICE_COMPILE__)
    *out_a = __fmaf_rn(a, c, -__fmul_rn(b, s));
    *out_b = __fmaf_rn(b, c, __fmul_rn(a, s));
#else
    // The product is the addend of an explicit fma: nothing is left to contract.
    volatile float bs = b * s, as = a * s;
    *out_a = __builtin_fmaf(a, c, -bs);
    *out_b = __builtin_fmaf(b, c, as);
#endif
}

// The same on bf16 bits: the inputs are the DECODED bf16 values, whatever the
// stored codec, and each result takes the codec headers' round-to-nearest-even
// conversion.
IFS_FP8_HD void pair_bf16(uint16_t a, uint16_t b, float c, float s, uint16_t* out_a,
                          uint16_t* out_b) {
    float fa, fb;
    pair_f32(fp8::bits_f32(static_cast<uint32_t>(a) << 16),
             fp8::bits_f32(static_cast<uint32_t>(b) << 16), c, s, &fa, &fb);
    *out_a = fp8::f32_to_bf16(fa);
    *out_b = fp8::f32_to_bf16(fb);
}

}  // namespace rotate
}  // namespace ifs
