// Cast pages: fp8 (e4m3fn) engine caches <-> bf16 logical pages, MI355X (gfx950).
//
// The CLIENT side of every page (source of kStore, destination of kLoad) holds
// one-byte OCP e4m3fn codes, element value = code value * scale[h] with h the
// half of the page (K or V) the element lies in (core/page_codec.h, PageCast;
// gpu.h; docs/design.md "cast pages"). The stored block is byte for byte the
// one the contiguous kernels make of the bf16 page of dequantized values
//     b = fp8::cast_code_to_bf16(code, scale[h]),
// and a load hands the client
//     code = fp8::cast_bf16_to_code(b, inv[h]),   inv[h] = 1.0f / scale[h]
// of the bf16 bits b that the codec's own dequantize kernel would have stored.
// inv is computed once on the host, so no lane divides, and it is never folded
// into a stored fp8 page's scale: the two roundings (to bf16, then to e4m3)
// are the specification.
//
// Unit of work. A lane unit is 8 elements, as in the codec kernels of gpu.hip:
// one 8-byte access on every one-byte-per-element side (the client always, the
// stored side under fp8), one 16-byte access on a bf16 side, 4 code bytes
// under mxfp4. Units are numbered over the whole page, g = s * seg_units + u
// for unit u of client segment s; the stored side is indexed by g alone, the
// client side by (s, u). The half of a unit is ONE compare, g >= half_units,
// against a kernel argument (half_units is the page's unit count when there is
// one half, so the compare is then never true). cast_legal keeps every unit,
// and under mxfp4 every 32-element group, inside one half and one segment.
//
// Work split. plain and mxfp4: a workgroup is (block, segment, chunk) with the
// chunk count chosen as the segmented copy kernels choose it, so that few
// large pages still fill the device; the descriptor pair is read once through
// LDS; a page of one segment is the same kernel with S = 1. Nothing is reused,
// so nothing else goes through LDS: each byte is loaded once, converted in
// registers and stored once. fp8: one 512-lane workgroup per page in both
// directions, because the scale is the PAGE's. The quantizer reads the client
// page twice (a linear absmax pass over the decoded bf16 bits, then the
// convert pass) and writes the page's scale to scales[b]; the second read of
// at most a few hundred KiB comes out of L2.
//
// The geometry, the scales and their inverses ride in the kernel arguments.
//
// A translation unit of its own, compiled without packed fp32 instructions as
// transpose.hip is (infinistore_amd/_build.py); the device functions of the
// other units keep the code they have.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>

#include "fp8_codec.h"
#include "gpu.h"
#include "mxfp4_codec.h"

namespace ifs {
namespace gpu {

struct CastArgs {
    uint32_t n_segs;          // client segments
    uint32_t chunks_per_seg;  // (block, segment, chunk) kernels only
    uint64_t seg_units;       // lane units (8 elements) per client segment
    uint64_t half_units;      // units of half 0: page units when halves == 1
    uint64_t seg_stride;      // CLIENT bytes from one segment to the next
    uint64_t page_elems;
    float scale[2];
    float inv[2];             // 1.0f / scale, from the host
};

// 8 client codes -> 8 bf16 (bits), and back.
__device__ __forceinline__ uint4 cast_unit_to_bf16(uint2 pk, float scale) {
    const uint8_t* c = reinterpret_cast<const uint8_t*>(&pk);
    uint16_t out[8];
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = fp8::cast_code_to_bf16(c[i], scale);
    return *reinterpret_cast<const uint4*>(out);
}

__device__ __forceinline__ uint2 cast_unit_to_codes(const uint16_t (&b)[8], float inv) {
    uint8_t out[8];
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = fp8::cast_bf16_to_code(b[i], inv);
    return *reinterpret_cast<const uint2*>(out);
}

// The prologue of the (block, segment, chunk) kernels: decodes the triple from
// blockIdx.x and reads block b's descriptor pair once through LDS.
__device__ __forceinline__ uint32_t cast_seg_chunk(const uint64_t* __restrict__ src_ptrs,
                                                   const uint64_t* __restrict__ dst_ptrs,
                                                   const CastArgs& a, uint64_t (&sd)[2],
                                                   uint32_t* seg) {
    const uint32_t per_block = a.n_segs * a.chunks_per_seg;
    const uint32_t b = blockIdx.x / per_block;
    const uint32_t r = blockIdx.x - b * per_block;
    const uint32_t s = r / a.chunks_per_seg;
    __shared__ uint64_t lds[2];
    if (threadIdx.x == 0) {
        lds[0] = src_ptrs[b];
        lds[1] = dst_ptrs[b];
    }
    __syncthreads();
    sd[0] = lds[0];
    sd[1] = lds[1];
    *seg = s;
    return r - s * a.chunks_per_seg;
}

// plain store: 8 codes in (uint2), 8 bf16 out (uint4) at the page-global unit.
__global__ __launch_bounds__(kCastThreads) void cast_store_plain_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs, CastArgs a) {
    uint64_t sd[2];
    uint32_t seg;
    const uint32_t chunk = cast_seg_chunk(src_ptrs, dst_ptrs, a, sd, &seg);
    const uint2* c2 = reinterpret_cast<const uint2*>(sd[0] + seg * a.seg_stride);
    const uint64_t g0 = seg * a.seg_units;
    uint4* p4 = reinterpret_cast<uint4*>(sd[1]) + g0;
    const uint64_t stride = static_cast<uint64_t>(a.chunks_per_seg) * blockDim.x;
    for (uint64_t u = static_cast<uint64_t>(chunk) * blockDim.x + threadIdx.x; u < a.seg_units;
         u += stride)
        p4[u] = cast_unit_to_bf16(c2[u], g0 + u >= a.half_units ? a.scale[1] : a.scale[0]);
}

// plain load: 8 bf16 in, 8 codes out.
__global__ __launch_bounds__(kCastThreads) void cast_load_plain_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs, CastArgs a) {
    uint64_t sd[2];
    uint32_t seg;
    const uint32_t chunk = cast_seg_chunk(src_ptrs, dst_ptrs, a, sd, &seg);
    const uint64_t g0 = seg * a.seg_units;
    const uint4* p4 = reinterpret_cast<const uint4*>(sd[0]) + g0;
    uint2* c2 = reinterpret_cast<uint2*>(sd[1] + seg * a.seg_stride);
    const uint64_t stride = static_cast<uint64_t>(a.chunks_per_seg) * blockDim.x;
    for (uint64_t u = static_cast<uint64_t>(chunk) * blockDim.x + threadIdx.x; u < a.seg_units;
         u += stride) {
        uint4 pk = p4[u];
        c2[u] = cast_unit_to_codes(*reinterpret_cast<const uint16_t(*)[8]>(&pk),
                                   g0 + u >= a.half_units ? a.inv[1] : a.inv[0]);
    }
}

// fp8 store: one workgroup per page and two passes over the client page, the
// absmax and the re-encoding both taken over the decoded bf16 bits exactly as
// quant_blocks_bf16_fp8_kernel takes them over a bf16 page. Stored byte =
// logical element index, so unit g's codes are the uint2 at index g.
__global__ __launch_bounds__(kCastFp8Threads) void cast_store_fp8_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs,
    float* __restrict__ scales, CastArgs a) {
    __shared__ uint64_t desc[2];
    if (threadIdx.x == 0) {
        desc[0] = src_ptrs[blockIdx.x];
        desc[1] = dst_ptrs[blockIdx.x];
    }
    __syncthreads();
    const uint64_t src = desc[0];
    uint2* d2 = reinterpret_cast<uint2*>(desc[1]);
    __shared__ uint32_t red[kCastFp8Threads / 64];
    __shared__ float scale_sh;
    uint32_t m = 0;  // largest finite bf16 magnitude, as bits
    for (uint32_t sg = 0; sg < a.n_segs; sg++) {
        const uint2* c2 = reinterpret_cast<const uint2*>(src + sg * a.seg_stride);
        const uint64_t g0 = sg * a.seg_units;
        for (uint64_t u = threadIdx.x; u < a.seg_units; u += blockDim.x) {
            uint4 pk = cast_unit_to_bf16(c2[u], g0 + u >= a.half_units ? a.scale[1] : a.scale[0]);
            const uint16_t* hw = reinterpret_cast<const uint16_t*>(&pk);
#pragma unroll
            for (int i = 0; i < 8; i++) m = fp8::absmax_step(m, hw[i]);
        }
    }
    for (int off = 32; off; off >>= 1) m = max(m, __shfl_down(m, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t mm = red[0];
        for (int w = 1; w < static_cast<int>(blockDim.x) / 64; w++) mm = max(mm, red[w]);
        scale_sh = fp8::scale_from_absmax_bits(mm);
        scales[blockIdx.x] = scale_sh;
    }
    __syncthreads();
    const float inv = 1.f / scale_sh;
    for (uint32_t sg = 0; sg < a.n_segs; sg++) {
        const uint2* c2 = reinterpret_cast<const uint2*>(src + sg * a.seg_stride);
        const uint64_t g0 = sg * a.seg_units;
        for (uint64_t u = threadIdx.x; u < a.seg_units; u += blockDim.x) {
            uint4 pk = cast_unit_to_bf16(c2[u], g0 + u >= a.half_units ? a.scale[1] : a.scale[0]);
            const uint16_t* hw = reinterpret_cast<const uint16_t*>(&pk);
            uint8_t out[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                float f = fp8::bits_f32(static_cast<uint32_t>(hw[i]) << 16);
                out[i] = fp8::f32_to_e4m3(f * inv);
            }
            d2[g0 + u] = *reinterpret_cast<const uint2*>(out);
        }
    }
}

// fp8 load: stored code -> bf16 bits under the page's scale, as
// dequant_blocks_fp8_bf16_kernel stores them, -> client code under inv[h].
__global__ __launch_bounds__(kCastFp8Threads) void cast_load_fp8_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs,
    const float* __restrict__ scales, CastArgs a) {
    __shared__ uint64_t desc[2];
    if (threadIdx.x == 0) {
        desc[0] = src_ptrs[blockIdx.x];
        desc[1] = dst_ptrs[blockIdx.x];
    }
    __syncthreads();
    const uint2* s2 = reinterpret_cast<const uint2*>(desc[0]);
    const uint64_t dst = desc[1];
    const float scale = scales[blockIdx.x];
    for (uint32_t sg = 0; sg < a.n_segs; sg++) {
        uint2* c2 = reinterpret_cast<uint2*>(dst + sg * a.seg_stride);
        const uint64_t g0 = sg * a.seg_units;
        for (uint64_t u = threadIdx.x; u < a.seg_units; u += blockDim.x) {
            uint2 pk = s2[g0 + u];
            const uint8_t* c = reinterpret_cast<const uint8_t*>(&pk);
            uint16_t b[8];
#pragma unroll
            for (int i = 0; i < 8; i++) b[i] = fp8::decode_to_bf16(c[i], scale);
            c2[u] = cast_unit_to_codes(b, g0 + u >= a.half_units ? a.inv[1] : a.inv[0]);
        }
    }
}

// mxfp4 store: four lanes per 32-element group, as quant_blocks_bf16_mxfp4_kernel.
// cast_legal makes seg_units a multiple of 4, and chunk * blockDim.x and the
// stride are multiples of 4 too: the four lanes 4k..4k+3 hold units 4j..4j+3
// of one segment in every iteration, all four inside it or none, and g agrees
// with u in its low two bits. __shfl_xor by 1 and 2 thus stays inside the
// group, and exactly the lane with (g & 3) == 0 writes the scale byte, which
// sits behind all codes at page_elems / 2 + (g >> 2).
__global__ __launch_bounds__(kCastThreads) void cast_store_mxfp4_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs, CastArgs a) {
    uint64_t sd[2];
    uint32_t seg;
    const uint32_t chunk = cast_seg_chunk(src_ptrs, dst_ptrs, a, sd, &seg);
    const uint2* c2 = reinterpret_cast<const uint2*>(sd[0] + seg * a.seg_stride);
    const uint64_t g0 = seg * a.seg_units;
    uint32_t* codes = reinterpret_cast<uint32_t*>(sd[1]) + g0;
    uint8_t* scales = reinterpret_cast<uint8_t*>(sd[1]) + a.page_elems / 2 + (g0 >> 2);
    const uint64_t stride = static_cast<uint64_t>(a.chunks_per_seg) * blockDim.x;
    for (uint64_t u = static_cast<uint64_t>(chunk) * blockDim.x + threadIdx.x; u < a.seg_units;
         u += stride) {
        uint4 pk = cast_unit_to_bf16(c2[u], g0 + u >= a.half_units ? a.scale[1] : a.scale[0]);
        const uint16_t* hw = reinterpret_cast<const uint16_t*>(&pk);
        uint32_t key = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) key = mxfp4::key_step(key, hw[i]);
        key = max(key, __shfl_xor(key, 1, 64));
        key = max(key, __shfl_xor(key, 2, 64));
        uint8_t E = mxfp4::group_exponent(key);
        uint32_t out = 0;
#pragma unroll
        for (int i = 0; i < 8; i++)
            out |= static_cast<uint32_t>(mxfp4::encode(hw[i], E)) << (4 * i);
        codes[u] = out;
        if ((u & 3u) == 0) scales[u >> 2] = E;
    }
}

// mxfp4 load is lane-local: 4 code bytes plus the group's scale byte in, 8
// client codes out.
__global__ __launch_bounds__(kCastThreads) void cast_load_mxfp4_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs, CastArgs a) {
    uint64_t sd[2];
    uint32_t seg;
    const uint32_t chunk = cast_seg_chunk(src_ptrs, dst_ptrs, a, sd, &seg);
    const uint64_t g0 = seg * a.seg_units;
    const uint32_t* codes = reinterpret_cast<const uint32_t*>(sd[0]) + g0;
    const uint8_t* scales =
        reinterpret_cast<const uint8_t*>(sd[0]) + a.page_elems / 2 + (g0 >> 2);
    uint2* c2 = reinterpret_cast<uint2*>(sd[1] + seg * a.seg_stride);
    const uint64_t stride = static_cast<uint64_t>(a.chunks_per_seg) * blockDim.x;
    for (uint64_t u = static_cast<uint64_t>(chunk) * blockDim.x + threadIdx.x; u < a.seg_units;
         u += stride) {
        uint32_t pk = codes[u];
        uint8_t E = scales[u >> 2];  // the quad's four lanes read the same byte
        uint16_t b[8];
#pragma unroll
        for (int i = 0; i < 8; i++)
            b[i] = mxfp4::decode(static_cast<uint8_t>((pk >> (4 * i)) & 0xfu), E);
        c2[u] = cast_unit_to_codes(b, g0 + u >= a.half_units ? a.inv[1] : a.inv[0]);
    }
}

static bool cast_refuse(const char* what, const char* why) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", what, why);
    set_last_error(msg);
    return false;
}

static bool cast_hip_ok(const char* what, hipError_t e) {
    return e == hipSuccess || cast_refuse(what, hipGetErrorString(e));
}

// What both launchers do after the codec-specific checks: the refusals they
// share, the kernel arguments and the (block, segment, chunk) grid, sized as
// the segmented copy kernels size theirs (about 4096 workgroups, one
// descriptor read each). need_grid is false for the fp8 pair.
static bool cast_args(const char* what, PageCodec codec, size_t page_bytes, PageCast cast,
                      PageSegments seg, bool aligned16, int n_blocks, bool need_grid,
                      CastArgs* a, uint32_t* grid) {
    if (!cast_legal(codec, page_bytes, cast, seg)) return cast_refuse(what, "illegal page cast");
    if (!aligned16) return cast_refuse(what, "needs 16-byte-aligned pointers");
    const uint64_t units = page_bytes / kPageElemBytes / 8;
    a->n_segs = seg.n;
    a->seg_units = units / seg.n;
    a->half_units = units / cast.halves;
    a->seg_stride = seg.n > 1 ? seg.stride_bytes : 0;
    a->page_elems = page_bytes / kPageElemBytes;
    for (int h = 0; h < 2; h++) {
        a->scale[h] = cast.scale[h];
        a->inv[h] = 1.0f / cast.scale[h];
    }
    const uint64_t rows = static_cast<uint64_t>(n_blocks > 0 ? n_blocks : 0) * seg.n;
    const uint64_t max_chunks = (a->seg_units + kCastThreads - 1) / kCastThreads;
    const uint64_t want = rows ? (4096 + rows - 1) / rows : 1;
    a->chunks_per_seg = static_cast<uint32_t>(
        std::max<uint64_t>(std::min<uint64_t>(want, max_chunks), 1));
    const uint64_t g = rows * a->chunks_per_seg;
    if (need_grid && g > 0x7fffffffull) return cast_refuse(what, "grid does not fit");
    *grid = static_cast<uint32_t>(g);
    return true;
}

bool launch_copy_blocks_cast(int dev, Stream stream, const uint64_t* dev_src,
                             const uint64_t* dev_dst, int n_blocks, size_t bytes_per_block,
                             bool aligned16, PageSegments seg, PageDir dir, PageCast cast) {
    const char* what = "launch_copy_blocks_cast";
    CastArgs a;
    uint32_t grid;
    if (!cast_args(what, PageCodec::kNone, bytes_per_block, cast, seg, aligned16, n_blocks, true,
                   &a, &grid))
        return false;
    if (n_blocks <= 0) return true;
    if (!cast_hip_ok(what, hipSetDevice(dev))) return false;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dir == PageDir::kStore)
        hipLaunchKernelGGL(cast_store_plain_kernel, dim3(grid), dim3(kCastThreads), 0, s, dev_src,
                           dev_dst, a);
    else
        hipLaunchKernelGGL(cast_load_plain_kernel, dim3(grid), dim3(kCastThreads), 0, s, dev_src,
                           dev_dst, a);
    return cast_hip_ok(what, hipGetLastError());
}

bool launch_transform_blocks_cast(int dev, Stream stream, PageCodec codec, PageDir dir,
                                  const uint64_t* dev_src, const uint64_t* dev_dst,
                                  float* dev_scales, int n_blocks, size_t elems_per_block,
                                  bool aligned16, PageSegments seg, PageCast cast) {
    const char* what = "launch_transform_blocks_cast";
    if (!page_codec_known(static_cast<uint32_t>(codec)) || !page_codec_transforms(codec) ||
        elems_per_block == 0 || elems_per_block > SIZE_MAX / kPageElemBytes)
        return cast_refuse(what, "not a page of a transforming codec");
    const bool store = dir == PageDir::kStore;
    const bool fp8_page = codec == PageCodec::kFp8;
    CastArgs a;
    uint32_t grid;
    if (!cast_args(what, codec, elems_per_block * kPageElemBytes, cast, seg, aligned16, n_blocks,
                   !fp8_page, &a, &grid))
        return false;
    if (page_codec_info(codec).page_scale && !dev_scales)
        return cast_refuse(what, "needs a scale per page");
    if (n_blocks <= 0) return true;
    if (!cast_hip_ok(what, hipSetDevice(dev))) return false;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (codec) {
        case PageCodec::kFp8:
            if (store)
                hipLaunchKernelGGL(cast_store_fp8_kernel, dim3(n_blocks), dim3(kCastFp8Threads),
                                   0, s, dev_src, dev_dst, dev_scales, a);
            else
                hipLaunchKernelGGL(cast_load_fp8_kernel, dim3(n_blocks), dim3(kCastFp8Threads), 0,
                                   s, dev_src, dev_dst, dev_scales, a);
            break;
        case PageCodec::kMxfp4:
            if (store)
                hipLaunchKernelGGL(cast_store_mxfp4_kernel, dim3(grid), dim3(kCastThreads), 0, s,
                                   dev_src, dev_dst, a);
            else
                hipLaunchKernelGGL(cast_load_mxfp4_kernel, dim3(grid), dim3(kCastThreads), 0, s,
                                   dev_src, dev_dst, a);
            break;
        default:
            return cast_refuse(what, "no cast kernels for this codec");
    }
    return cast_hip_ok(what, hipGetLastError());
}

}  // namespace gpu
}  // namespace ifs
