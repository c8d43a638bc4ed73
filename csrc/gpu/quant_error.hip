// Quantization-error probe for the lossy page codecs, MI355X (gfx950).
//
// What a page would lose under a lossy codec, measured on the caller's own
// bf16 pages without storing anything (gpu.h, docs/design.md "quantization-
// error probe"). Both kernels form x^ with the codec headers' functions in the
// quantize and dequantize kernels' own expressions, so x^ is the store's x^ bit
// for bit, and reduce five values per (page, part): sum x^2, sum (x - x^)^2,
// max |x - x^|, max |x|, and the count of elements whose x or x^ is not finite
// (those take no part in the first four).
//
// Arithmetic. x and x^ are bf16, so x - x^ is exact (a codec round trip keeps x^
// within a factor of four of x, or makes it 0), and the squares of x and of the
// difference have at most 16 and 48 significant bits: every TERM is exact in
// float64 and only the additions round. The operands are built from the bf16
// bits with integer operations, so no step depends on the fp32 denormal mode.
//
// Order. A lane adds its elements in address order, segment after segment; a
// wave folds its lanes with shuffles (offsets 32, 16, ... 1); lane 0 of the
// workgroup adds the waves' partial results in wave order. No atomics: the
// order is a function of the geometry alone and two runs agree bit for bit.
//
// This file is a translation unit of its own because it is compiled with the
// packed fp32 instructions (v_pk_*_f32) switched off (infinistore_amd/_build.py):
// the one fp32 product per element, x / scale, is then always the scalar
// multiply whose result the codec's host tests pin, and the kernels of gpu.hip
// keep the code they have.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "fp8_codec.h"
#include "gpu.h"
#include "mxfp4_codec.h"

namespace ifs {
namespace gpu {

// The table of a tensor set's bases rides in the kernel arguments (gpu.hip,
// "tensor sets", says why).
struct QuantErrBases {
    uint64_t base[kMaxPageTensors];
};

constexpr int kMxfp4Threads = 4 * kMxfp4GroupsPerIter;  // as the mxfp4 quantizer

struct QuantErrArgs {
    uint32_t n_parts;        // parts per page: tensors of a set, else segments
    uint32_t segs_per_part;  // S/G for a tensor set, else 1
    uint32_t use_bases;      // tensor set: part p starts at tb.base[p] + desc
    uint64_t seg_elems;
    uint64_t stride;         // client bytes from one segment to the next
};

struct ErrAcc {
    double sx = 0, se = 0, dmax = 0;
    uint32_t xmax = 0;  // largest |x| that took part, as bf16 magnitude bits
    uint32_t bad = 0;
};

// A FINITE bf16 as float64, exactly.
__device__ __forceinline__ double bf16_to_f64(uint16_t h) {
    const uint64_t sign = static_cast<uint64_t>(h & 0x8000u) << 48;
    const uint32_t e = (h >> 7) & 0xffu, m = h & 0x7fu;
    if (e == 0) {  // zero or subnormal: m * 2^-133
        double v = static_cast<double>(static_cast<int>(m)) * 0x1p-133;
        return __builtin_bit_cast(double, sign | __builtin_bit_cast(uint64_t, v));
    }
    return __builtin_bit_cast(double, sign | (static_cast<uint64_t>(e + 896u) << 52) |
                                          (static_cast<uint64_t>(m) << 45));
}

__device__ __forceinline__ void err_step(ErrAcc& a, uint16_t x, uint16_t xh) {
    const uint32_t ax = x & fp8::kBf16AbsMask;
    if (ax >= fp8::kBf16Inf || (xh & fp8::kBf16AbsMask) >= fp8::kBf16Inf) {
        a.bad++;
        return;
    }
    const double dx = bf16_to_f64(x);
    const double d = fabs(dx - bf16_to_f64(xh));
    a.sx += dx * dx;
    a.se += d * d;
    a.dmax = d > a.dmax ? d : a.dmax;
    a.xmax = ax > a.xmax ? ax : a.xmax;
}

// Workgroup reduction of one part's accumulators; lane 0 stores the five
// values. Called by every thread of the workgroup, once per part.
__device__ __forceinline__ void err_reduce_store(ErrAcc a, double* __restrict__ out) {
    __shared__ double rd[8][3];  // at most 512 threads / 64-wide wavefronts
    __shared__ uint64_t ru[8][2];
    uint64_t xmax = a.xmax, bad = a.bad;
    for (int off = 32; off; off >>= 1) {
        a.sx += __shfl_down(a.sx, off, 64);
        a.se += __shfl_down(a.se, off, 64);
        double dm = __shfl_down(a.dmax, off, 64);
        a.dmax = dm > a.dmax ? dm : a.dmax;
        uint64_t xm = __shfl_down(xmax, off, 64);
        xmax = xm > xmax ? xm : xmax;
        bad += __shfl_down(bad, off, 64);
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        rd[wave][0] = a.sx;
        rd[wave][1] = a.se;
        rd[wave][2] = a.dmax;
        ru[wave][0] = xmax;
        ru[wave][1] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < blockDim.x / 64; w++) {
            a.sx += rd[w][0];
            a.se += rd[w][1];
            a.dmax = rd[w][2] > a.dmax ? rd[w][2] : a.dmax;
            xmax = ru[w][0] > xmax ? ru[w][0] : xmax;
            bad += ru[w][1];
        }
        out[0] = a.sx;
        out[1] = a.se;
        out[2] = a.dmax;
        out[3] = bf16_to_f64(static_cast<uint16_t>(xmax));
        out[4] = static_cast<double>(bad);
    }
    __syncthreads();  // the next part reuses rd / ru
}

__device__ __forceinline__ uint64_t quant_err_seg(const QuantErrArgs& a, const QuantErrBases& tb,
                                                  uint64_t desc, uint32_t p, uint32_t r) {
    return (a.use_bases ? tb.base[p] : p * a.stride) + desc + r * a.stride;
}

// fp8: one 512-thread workgroup per page, because the scale is the PAGE's.
// Pass 1 is the quantizer's: absmax over every part. Pass 2 walks the parts in
// order, 16 B (8 elements) per lane per step, and reduces after each part.
__global__ void __launch_bounds__(512)
    quant_error_fp8_kernel(const uint64_t* __restrict__ descs, double* __restrict__ out,
                           QuantErrArgs a, QuantErrBases tb) {
    const uint64_t desc = descs[blockIdx.x];
    __shared__ uint32_t red[8];  // 512 threads / 64-wide wavefronts
    __shared__ float scale_sh;
    uint32_t m = 0;  // largest finite bf16 magnitude, as bits
    const uint64_t n8 = a.seg_elems / 8;
    for (uint32_t p = 0; p < a.n_parts; p++) {
        for (uint32_t r = 0; r < a.segs_per_part; r++) {
            const uint4* src4 = reinterpret_cast<const uint4*>(quant_err_seg(a, tb, desc, p, r));
            for (uint64_t u = threadIdx.x; u < n8; u += blockDim.x) {
                uint4 pk = src4[u];
                const uint16_t* h = reinterpret_cast<const uint16_t*>(&pk);
#pragma unroll
                for (int i = 0; i < 8; i++) m = fp8::absmax_step(m, h[i]);
            }
        }
    }
    for (int off = 32; off; off >>= 1) m = max(m, __shfl_down(m, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t mm = red[0];
        for (int w = 1; w < static_cast<int>(blockDim.x) / 64; w++) mm = max(mm, red[w]);
        scale_sh = fp8::scale_from_absmax_bits(mm);
    }
    __syncthreads();
    const float scale = scale_sh;
    const float inv = 1.f / scale;
    for (uint32_t p = 0; p < a.n_parts; p++) {
        ErrAcc acc;
        for (uint32_t r = 0; r < a.segs_per_part; r++) {
            const uint4* src4 = reinterpret_cast<const uint4*>(quant_err_seg(a, tb, desc, p, r));
            for (uint64_t u = threadIdx.x; u < n8; u += blockDim.x) {
                uint4 pk = src4[u];
                const uint16_t* h = reinterpret_cast<const uint16_t*>(&pk);
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    float f = fp8::bits_f32(static_cast<uint32_t>(h[i]) << 16);
                    uint8_t code = fp8::f32_to_e4m3(f * inv);
                    err_step(acc, h[i], fp8::decode_to_bf16(code, scale));
                }
            }
        }
        err_reduce_store(acc, out + (static_cast<uint64_t>(blockIdx.x) * a.n_parts + p) *
                                        kQuantErrFields);
    }
}

// mxfp4: a scale covers 32 neighbouring elements, so nothing is page-wide and
// the workgroup is (page, part). Four lanes share a group and find its key with
// quad shuffles exactly as the quantizer does; seg_elems % 32 == 0 keeps every
// quad whole inside every segment (gpu.hip, above kMxfp4Threads).
__global__ void __launch_bounds__(kMxfp4Threads)
    quant_error_mxfp4_kernel(const uint64_t* __restrict__ descs, double* __restrict__ out,
                             QuantErrArgs a, QuantErrBases tb) {
    const uint32_t b = blockIdx.x / a.n_parts;
    const uint32_t p = blockIdx.x - b * a.n_parts;
    __shared__ uint64_t lds;
    if (threadIdx.x == 0) lds = descs[b];
    __syncthreads();
    const uint64_t desc = lds;
    const uint64_t n8 = a.seg_elems / 8;
    ErrAcc acc;
    for (uint32_t r = 0; r < a.segs_per_part; r++) {
        const uint4* src4 = reinterpret_cast<const uint4*>(quant_err_seg(a, tb, desc, p, r));
        for (uint64_t u = threadIdx.x; u < n8; u += blockDim.x) {
            uint4 pk = src4[u];
            const uint16_t* h = reinterpret_cast<const uint16_t*>(&pk);
            uint32_t key = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) key = mxfp4::key_step(key, h[i]);
            key = max(key, __shfl_xor(key, 1, 64));
            key = max(key, __shfl_xor(key, 2, 64));
            uint8_t E = mxfp4::group_exponent(key);
#pragma unroll
            for (int i = 0; i < 8; i++)
                err_step(acc, h[i], mxfp4::decode(mxfp4::encode(h[i], E), E));
        }
    }
    err_reduce_store(acc, out + static_cast<uint64_t>(blockIdx.x) * kQuantErrFields);
}


static bool refuse(const char* why, const char* codec_name = "") {
    char msg[160];
    snprintf(msg, sizeof(msg), "launch_quant_error: %s%s", why, codec_name);
    set_last_error(msg);
    return false;
}

bool launch_quant_error(int dev, Stream stream, PageCodec codec, const uint64_t* dev_client_descs,
                        int n_blocks, size_t elems_per_block, PageSegments seg,
                        TensorTable tset, double* dev_out) {
    if (!page_codec_known(static_cast<uint32_t>(codec)) || !page_codec_transforms(codec))
        return refuse("not a lossy codec");
    const char* name = page_codec_info(codec).name;
    const size_t page_bytes = elems_per_block * kPageElemBytes;
    if (elems_per_block == 0 || !page_legal(codec, page_bytes))
        return refuse("not a page of ", name);
    QuantErrArgs a;
    QuantErrBases tb = {};
    bool aligned16 = true;
    if (tset.n > 0) {
        if (!tensors_legal(codec, page_bytes, seg.n, seg.stride_bytes, tset.n) || !tset.bases)
            return refuse("illegal tensor set geometry");
        for (uint32_t g = 0; g < tset.n; g++) {
            tb.base[g] = tset.bases[g];
            if (tset.bases[g] % 16 != 0) aligned16 = false;
        }
        a.n_parts = tset.n;
        a.segs_per_part = seg.n / tset.n;
        a.use_bases = 1;
    } else {
        if (!segments_legal(codec, page_bytes, seg.n, seg.stride_bytes))
            return refuse("illegal page segments");
        a.n_parts = seg.n;
        a.segs_per_part = 1;
        a.use_bases = 0;
    }
    a.seg_elems = elems_per_block / seg.n;
    // A stride that is never applied is passed as 0.
    a.stride = (tset.n > 0 ? a.segs_per_part : seg.n) > 1 ? seg.stride_bytes : 0;
    if (n_blocks <= 0) return true;
    if (!dev_client_descs || !dev_out) return refuse("null descriptors or output");
    for (int i = 0; i < n_blocks; i++)
        if (dev_client_descs[i] % 16 != 0) aligned16 = false;
    if (!aligned16) return refuse("16-byte-aligned bases and pages are needed by ", name);
    uint64_t grid = static_cast<uint64_t>(n_blocks);
    if (codec == PageCodec::kMxfp4) grid *= a.n_parts;
    if (grid > 0x7fffffffull) return refuse("grid does not fit");
    if (hipSetDevice(dev) != hipSuccess) return refuse("hipSetDevice failed");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (codec == PageCodec::kFp8)
        hipLaunchKernelGGL(quant_error_fp8_kernel, dim3(static_cast<uint32_t>(grid)), dim3(512),
                           0, s, dev_client_descs, dev_out, a, tb);
    else
        hipLaunchKernelGGL(quant_error_mxfp4_kernel, dim3(static_cast<uint32_t>(grid)),
                           dim3(kMxfp4Threads), 0, s, dev_client_descs, dev_out, a, tb);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return refuse("launch failed: ", hipGetErrorString(e));
    return true;
}

}  // namespace gpu
}  // namespace ifs
