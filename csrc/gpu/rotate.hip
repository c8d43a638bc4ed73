// Rotated reads: load cached keys at a new RoPE position, MI355X (gfx950).
//
// A stored page is [halves, T, heads, head_dim] bf16 values (plain, fp8 or
// mxfp4 in the pool) whose K half carries rotary position embedding for the
// position it was written at. These load kernels hand the client the same page
// with every rotary pair of K turned by the angle the request's table gives
// (core/page_codec.h, PageRotate; gpu.h; docs/design.md "rotated reads"):
// decode, rotate and store in one pass, where a reader otherwise loads the
// page and then runs a second kernel over its K half.
//
// Unit of work. A lane unit is 8 elements, as in the codec kernels of gpu.hip:
// one 16-byte access on a bf16 side, 8 code bytes under fp8, 4 under mxfp4
// plus the group's scale byte. Units are numbered over the whole page, g =
// s * seg_units + u for unit u of client segment s; the stored side is
// indexed by g alone, the client side by (s, u). rotate_legal makes head_dim a
// multiple of 8 and keeps a unit inside the rotary range or outside it, so a
// lane classifies its unit with one division: row = g / row_units, j = g -
// row * row_units, and the unit is rotated when g < k_units (the K half) and
// j < rot_units.
//   style 2 (GPT-J): the unit holds four whole pairs (2i, 2i + 1); the lane
//     rotates them in registers, pair index 4j + k.
//   style 1 (NeoX): pair i is channels (i, i + P). The lane whose unit lies in
//     the first half of the rotary range (j < P / 8) also loads the partner
//     unit P / 8 units on, rotates the eight pairs 8j + k and stores both
//     units, 16 bytes each; the lane that would own the partner unit does
//     nothing. No shuffle and no cross-lane LDS traffic; the partner unit has
//     its own mxfp4 group and scale byte. It lies in the same (token, head)
//     row, hence in the same segment and inside the page.
//   V and the non-rotary tail: a 16-byte move, or a dequantizing move.
//
// Work split. A workgroup is (block, segment, chunk), the chunk count chosen
// as the segmented copy kernels choose it; a contiguous page is S = 1. The
// descriptor pair is read once through LDS. The table rides in the kernel
// arguments (1 KiB at most, per request, copied at launch) and is staged once
// per workgroup into LDS as float2[P], because a lane's pair index varies
// across the wave: kernel arguments are scalar memory, LDS serves 64 different
// indices in one access.
//
// There is no byte fallback and no scratch. A translation unit of its own,
// compiled without packed fp32 instructions as cast.hip is
// (infinistore_amd/_build.py); the device functions of the other units keep
// the code they have.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>

#include "fp8_codec.h"
#include "gpu.h"
#include "mxfp4_codec.h"
#include "rotate_math.h"

namespace ifs {
namespace gpu {

struct RotateArgs {
    uint32_t n_segs;          // client segments
    uint32_t chunks_per_seg;
    uint32_t seg_units;       // lane units (8 elements) per client segment
    uint32_t k_units;         // units of half 0: the page's when halves == 1
    uint32_t row_units;       // head_dim / 8
    uint32_t rot_units;       // rot_dim / 8
    uint32_t partner_units;   // style 1: P / 8, the way to the partner unit; style 2: 0
    uint32_t pairs;           // P
    uint64_t seg_stride;      // client bytes from one segment to the next
    uint64_t page_elems;
    float table[2 * kMaxRotatePairs];  // (cos, sin) per pair
};

// Unit g of the stored page as 8 bf16 (bits), exactly what the codec's own
// dequantize kernel stores for it.
template <PageCodec kCodec>
__device__ __forceinline__ uint4 rotate_load_unit(uint64_t src, uint32_t g, float scale,
                                                  uint64_t page_elems) {
    if constexpr (kCodec == PageCodec::kNone) {
        return reinterpret_cast<const uint4*>(src)[g];
    } else if constexpr (kCodec == PageCodec::kFp8) {
        uint2 pk = reinterpret_cast<const uint2*>(src)[g];
        const uint8_t* c = reinterpret_cast<const uint8_t*>(&pk);
        uint16_t out[8];
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = fp8::decode_to_bf16(c[i], scale);
        return *reinterpret_cast<const uint4*>(out);
    } else {
        uint32_t pk = reinterpret_cast<const uint32_t*>(src)[g];
        uint8_t E = reinterpret_cast<const uint8_t*>(src)[page_elems / 2 + (g >> 2)];
        uint16_t out[8];
#pragma unroll
        for (int i = 0; i < 8; i++)
            out[i] = mxfp4::decode(static_cast<uint8_t>((pk >> (4 * i)) & 0xfu), E);
        return *reinterpret_cast<const uint4*>(out);
    }
}

template <PageCodec kCodec>
__global__ __launch_bounds__(kRotateThreads) void rotate_load_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs,
    const float* __restrict__ scales, RotateArgs a) {
    const uint32_t per_block = a.n_segs * a.chunks_per_seg;
    const uint32_t b = blockIdx.x / per_block;
    const uint32_t r = blockIdx.x - b * per_block;
    const uint32_t s = r / a.chunks_per_seg;
    const uint32_t chunk = r - s * a.chunks_per_seg;
    __shared__ uint64_t desc[2];
    __shared__ float2 tab[kMaxRotatePairs];
    if (threadIdx.x == 0) {
        desc[0] = src_ptrs[b];
        desc[1] = dst_ptrs[b];
    }
    for (uint32_t t = threadIdx.x; t < a.pairs; t += blockDim.x)
        tab[t] = make_float2(a.table[2 * t], a.table[2 * t + 1]);
    __syncthreads();
    const uint64_t src = desc[0];
    uint4* dst = reinterpret_cast<uint4*>(desc[1] + s * a.seg_stride);
    float scale = 0.f;
    if constexpr (kCodec == PageCodec::kFp8) scale = scales[b];
    const uint32_t g0 = s * a.seg_units;
    const uint32_t stride = a.chunks_per_seg * blockDim.x;
    for (uint32_t u = chunk * blockDim.x + threadIdx.x; u < a.seg_units; u += stride) {
        const uint32_t g = g0 + u;
        const uint32_t row = g / a.row_units;
        const uint32_t j = g - row * a.row_units;
        if (g >= a.k_units || j >= a.rot_units) {  // V, or the non-rotary tail
            dst[u] = rotate_load_unit<kCodec>(src, g, scale, a.page_elems);
            continue;
        }
        if (a.partner_units == 0) {  // style 2: four pairs inside the unit
            uint4 v = rotate_load_unit<kCodec>(src, g, scale, a.page_elems);
            uint16_t* h = reinterpret_cast<uint16_t*>(&v);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float2 cs = tab[4 * j + k];
                rotate::pair_bf16(h[2 * k], h[2 * k + 1], cs.x, cs.y, &h[2 * k], &h[2 * k + 1]);
            }
            dst[u] = v;
        } else if (j < a.partner_units) {  // style 1: this unit and its partner
            uint4 va = rotate_load_unit<kCodec>(src, g, scale, a.page_elems);
            uint4 vb = rotate_load_unit<kCodec>(src, g + a.partner_units, scale, a.page_elems);
            uint16_t* ha = reinterpret_cast<uint16_t*>(&va);
            uint16_t* hb = reinterpret_cast<uint16_t*>(&vb);
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const float2 cs = tab[8 * j + k];
                rotate::pair_bf16(ha[k], hb[k], cs.x, cs.y, &ha[k], &hb[k]);
            }
            dst[u] = va;
            dst[u + a.partner_units] = vb;
        }
        // else: the second half of the rotary range, written by the partner's lane
    }
}

static bool rotate_refuse(const char* why) {
    char msg[256];
    snprintf(msg, sizeof(msg), "launch_load_rotated: %s", why);
    set_last_error(msg);
    return false;
}

static bool rotate_hip_ok(hipError_t e) {
    return e == hipSuccess || rotate_refuse(hipGetErrorString(e));
}

bool launch_load_rotated(int dev, Stream stream, PageCodec codec, const uint64_t* dev_src,
                         const uint64_t* dev_dst, const float* dev_scales, int n_blocks,
                         size_t elems_per_block, bool aligned16, PageSegments seg,
                         const PageRotate& rot) {
    if (!page_codec_known(static_cast<uint32_t>(codec)) || elems_per_block == 0 ||
        elems_per_block > SIZE_MAX / kPageElemBytes)
        return rotate_refuse("not a bf16 page of a known codec");
    const size_t page_bytes = elems_per_block * kPageElemBytes;
    if (!rotate_legal(codec, page_bytes, rot, seg)) return rotate_refuse("illegal page rotation");
    if (!aligned16) return rotate_refuse("needs 16-byte-aligned pointers");
    if (page_codec_info(codec).page_scale && !dev_scales)
        return rotate_refuse("needs a scale per page");
    // Unit indices are 32-bit in the kernels.
    const uint64_t units = elems_per_block / 8;
    if (units > 0x7fffffffull) return rotate_refuse("page too large");
    RotateArgs a;
    a.n_segs = seg.n;
    a.seg_units = static_cast<uint32_t>(units / seg.n);
    a.k_units = static_cast<uint32_t>(units / rot.halves);
    a.row_units = rot.head_dim / 8;
    a.rot_units = rot.rot_dim / 8;
    a.pairs = rot.rot_dim / 2;
    a.partner_units = rot.style == kRotateNeox ? a.pairs / 8 : 0;
    a.seg_stride = seg.n > 1 ? seg.stride_bytes : 0;
    a.page_elems = elems_per_block;
    std::copy(rot.table, rot.table + rot.rot_dim, a.table);
    std::fill(a.table + rot.rot_dim, a.table + 2 * kMaxRotatePairs, 0.f);
    // About 4096 workgroups, as the segmented copy kernels size their grids.
    const uint64_t rows = static_cast<uint64_t>(n_blocks > 0 ? n_blocks : 0) * seg.n;
    const uint64_t max_chunks = (a.seg_units + kRotateThreads - 1) / kRotateThreads;
    const uint64_t want = rows ? (4096 + rows - 1) / rows : 1;
    a.chunks_per_seg =
        static_cast<uint32_t>(std::max<uint64_t>(std::min<uint64_t>(want, max_chunks), 1));
    const uint64_t grid = rows * a.chunks_per_seg;
    if (grid > 0x7fffffffull) return rotate_refuse("grid does not fit");
    if (n_blocks <= 0) return true;
    if (!rotate_hip_ok(hipSetDevice(dev))) return false;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 g(static_cast<uint32_t>(grid)), t(kRotateThreads);
    switch (codec) {
        case PageCodec::kNone:
            hipLaunchKernelGGL(rotate_load_kernel<PageCodec::kNone>, g, t, 0, s, dev_src, dev_dst,
                               dev_scales, a);
            break;
        case PageCodec::kFp8:
            hipLaunchKernelGGL(rotate_load_kernel<PageCodec::kFp8>, g, t, 0, s, dev_src, dev_dst,
                               dev_scales, a);
            break;
        case PageCodec::kMxfp4:
            hipLaunchKernelGGL(rotate_load_kernel<PageCodec::kMxfp4>, g, t, 0, s, dev_src,
                               dev_dst, dev_scales, a);
            break;
    }
    return rotate_hip_ok(hipGetLastError());
}

}  // namespace gpu
}  // namespace ifs
