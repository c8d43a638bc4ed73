// Shuffled pages: shuffled cache blocks <-> canonical pages, MI355X (gfx950).
//
// The CLIENT side of every page (source of kStore, destination of kLoad) is a
// shuffled cache block (core/page_codec.h, PageShuffle; gpu.h; docs/design.md
// "shuffled pages"): per half o and head h one tile of T x C elements, held as
// [C/X, T, X] (form 1, K) or [T/X, C, X] (form 2, V), X = 16 / elem_bytes. The
// stored block is byte-identical to the one the contiguous kernels make of the
// canonical [outer, T, H, C] page.
//
// Unit of work. One SQUARE is X tokens x X channels of one tile. On the stored
// side it is one 16-byte unit in each of X consecutive (token, head) rows,
// H * C * elem_bytes apart. On the client it is X * 16 CONTIGUOUS bytes under
// both forms: form 1 keeps the X units one after the other in token order,
// form 2 holds the square transposed (unit i is channel i's X tokens). So a
// lane owns a square: X 16-byte loads, for form 2 an X x X transpose in its
// own registers, X 16-byte stores. Nothing crosses lanes, so there is no LDS
// tile, no barrier and no bound on the tile's size.
//
// Numbering. The squares of a page are numbered tile by tile, token slab by
// token slab, channel group fastest:
//     q = ((o*H + h) * (T/X) + t/X) * (C/X) + c/X.
// Neighbouring lanes thus hold neighbouring channel groups: on the stored side
// each of the X accesses of a wavefront covers neighbouring units of the same
// rows, on the client side the lanes are X * 16 bytes apart in each access and
// a wavefront covers one contiguous range over its X accesses. A workgroup is
// (block, chunk) over the squares and reads the block's descriptor pair once
// through LDS, as block_chunk_descs does; the geometry rides in the kernel
// arguments. One square costs three 32-bit divisions, none per unit.
//
// Codecs act on the stored side only, row by row of the square, with the codec
// headers' functions in the contiguous kernels' own expressions; the registers
// always hold bf16. The fp8 scale is the PAGE's: its quantizer is one
// workgroup per page, a linear absmax pass over the client bytes, then the
// squares. An mxfp4 group is 32 elements of one row: four neighbouring
// squares, i.e. an aligned quad of lanes, reduced once per row of the square.
//
// LDS: the descriptor pair, and in the fp8 quantizer the absmax reduction.
//
// A translation unit of its own, compiled without packed fp32 instructions as
// transpose.hip is (infinistore_amd/_build.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>

#include "fp8_codec.h"
#include "gpu.h"
#include "mxfp4_codec.h"

namespace ifs {
namespace gpu {

struct ShufArgs {
    uint32_t slabs;          // T / X
    uint32_t cgroups;        // C / X
    uint32_t tokens;         // T
    uint32_t heads;          // H
    uint32_t form0, form1;   // form of half 0 and of half 1
    uint32_t tiles_per_seg;  // outer * heads / client segments
    uint32_t n_segs;         // client segments
    uint32_t chunks;         // workgroups per block
    uint32_t squares;        // squares per page, < 2^31
    uint32_t to_pool;        // 1: client -> stored block, 0: stored block -> client
    uint64_t seg_stride;     // client bytes from one segment to the next
    uint64_t tile_bytes;     // T * C * elem_bytes
    uint64_t page_elems;
};

// The X x X square of elements of EB bytes in X registers quadruples, word k of
// unit i at w[i][k].
template <int EB>
struct Square {
    static constexpr int X = 16 / EB;
    uint32_t w[X][4];
    __device__ __forceinline__ void load_run(const uint4* p) {  // X consecutive units
#pragma unroll
        for (int i = 0; i < X; i++) *reinterpret_cast<uint4*>(w[i]) = p[i];
    }
    __device__ __forceinline__ void store_run(uint4* p) const {
#pragma unroll
        for (int i = 0; i < X; i++) p[i] = *reinterpret_cast<const uint4*>(w[i]);
    }
    // Element (i, j): the j-th element of unit i. Every index is a constant
    // once the loops are unrolled, so the square stays in registers.
    __device__ __forceinline__ uint32_t get(int i, int j) const {
        constexpr int per = 4 / EB;  // elements per word
        if constexpr (EB == 4) return w[i][j];
        return (w[i][j / per] >> (8 * EB * (j % per))) & ((1u << (8 * EB % 32)) - 1u);
    }
    __device__ __forceinline__ void transpose() {
        constexpr int per = 4 / EB;
        uint32_t t[X][4];
#pragma unroll
        for (int i = 0; i < X; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint32_t word = 0;
#pragma unroll
                for (int e = 0; e < per; e++) word |= get(k * per + e, i) << (8 * EB * e % 32);
                t[i][k] = word;
            }
#pragma unroll
        for (int i = 0; i < X; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) w[i][k] = t[i][k];
    }
};

// Where square q of a page lies: its first stored unit g0 (the unit of row j is
// g0 + j * row_step, page-global, ((o*T + t)*H + h) * (C/X) + c/X), the first
// of its X client units, and its form.
struct SquarePlace {
    uint64_t g0, row_step;
    uint4* client;
    uint32_t form;
};

template <int X>
__device__ __forceinline__ SquarePlace shuf_place(const ShufArgs& a, uint64_t client, uint32_t q) {
    const uint32_t rest = q / a.cgroups;
    const uint32_t cg = q - rest * a.cgroups;
    const uint32_t ti = rest / a.slabs;
    const uint32_t slab = rest - ti * a.slabs;
    const uint32_t o = ti >= a.heads ? 1u : 0u;  // outer <= 2
    const uint32_t h = ti - o * a.heads;
    const uint32_t sg = ti / a.tiles_per_seg;
    SquarePlace p;
    p.form = o ? a.form1 : a.form0;
    p.row_step = static_cast<uint64_t>(a.heads) * a.cgroups;
    p.g0 = (static_cast<uint64_t>(o) * a.tokens + static_cast<uint64_t>(slab) * X) * p.row_step +
           static_cast<uint64_t>(h) * a.cgroups + cg;
    // form 1: unit (c/X)*T + t; form 2: unit ((t/X)*(C/X) + c/X)*X + c%X
    const uint64_t unit = p.form == 1
                              ? static_cast<uint64_t>(cg) * a.tokens + static_cast<uint64_t>(slab) * X
                              : (static_cast<uint64_t>(slab) * a.cgroups + cg) * X;
    p.client = reinterpret_cast<uint4*>(client + sg * a.seg_stride +
                                        static_cast<uint64_t>(ti - sg * a.tiles_per_seg) *
                                            a.tile_bytes) +
               unit;
    return p;
}

// The prologue of the four (block, chunk) kernels: reads block b's descriptor
// pair once through LDS as block_chunk_descs does and hands out the pool and
// client base addresses whichever way the copy runs; returns the chunk.
__device__ __forceinline__ uint32_t shuf_block_chunk(const uint64_t* __restrict__ src_ptrs,
                                                     const uint64_t* __restrict__ dst_ptrs,
                                                     const ShufArgs& a, uint32_t* b,
                                                     uint64_t* pool, uint64_t* client) {
    *b = blockIdx.x / a.chunks;
    const uint32_t chunk = blockIdx.x - *b * a.chunks;
    __shared__ uint64_t lds[2];
    if (threadIdx.x == 0) {
        lds[0] = src_ptrs[*b];
        lds[1] = dst_ptrs[*b];
    }
    __syncthreads();
    *pool = a.to_pool ? lds[1] : lds[0];
    *client = a.to_pool ? lds[0] : lds[1];
    return chunk;
}

// plain, both directions: raw elements of EB bytes.
template <int EB>
__global__ __launch_bounds__(kShufThreads) void copy_blocks_shuf_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs, ShufArgs a) {
    constexpr int X = 16 / EB;
    uint32_t b;
    uint64_t pool, client;
    const uint32_t chunk = shuf_block_chunk(src_ptrs, dst_ptrs, a, &b, &pool, &client);
    uint4* p4 = reinterpret_cast<uint4*>(pool);
    const uint32_t stride = a.chunks * kShufThreads;
    for (uint32_t q = chunk * kShufThreads + threadIdx.x; q < a.squares; q += stride) {
        const SquarePlace p = shuf_place<X>(a, client, q);
        Square<EB> sq;
        if (a.to_pool) {
            sq.load_run(p.client);
            if (p.form == 2) sq.transpose();
#pragma unroll
            for (int j = 0; j < X; j++)
                p4[p.g0 + j * p.row_step] = *reinterpret_cast<const uint4*>(sq.w[j]);
        } else {
#pragma unroll
            for (int j = 0; j < X; j++)
                *reinterpret_cast<uint4*>(sq.w[j]) = p4[p.g0 + j * p.row_step];
            if (p.form == 2) sq.transpose();
            sq.store_run(p.client);
        }
    }
}

// fp8 quantize: one workgroup per page and two passes, because the scale is
// the PAGE's. The absmax does not depend on the order of the elements, so pass
// 1 reads the client page linearly, segment by segment. Pass 2 walks the
// page's squares: 8 bf16 of row j -> 8 codes (uint2); stored byte = logical
// element index, so unit g's codes are the uint2 at index g.
__global__ __launch_bounds__(kShufThreads) void quant_blocks_bf16_fp8_shuf_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs,
    float* __restrict__ scales, ShufArgs a) {
    __shared__ uint64_t desc[2];
    if (threadIdx.x == 0) {
        desc[0] = src_ptrs[blockIdx.x];
        desc[1] = dst_ptrs[blockIdx.x];
    }
    __syncthreads();
    const uint64_t src = desc[0];
    uint2* d2 = reinterpret_cast<uint2*>(desc[1]);
    __shared__ uint32_t red[kShufThreads / 64];
    __shared__ float scale_sh;
    uint32_t m = 0;  // largest finite bf16 magnitude, as bits
    const uint64_t seg16 = a.tiles_per_seg * (a.tile_bytes / 16);
    for (uint32_t sg = 0; sg < a.n_segs; sg++) {
        const uint4* src4 = reinterpret_cast<const uint4*>(src + sg * a.seg_stride);
        for (uint64_t u = threadIdx.x; u < seg16; u += kShufThreads) {
            uint4 pk = src4[u];
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
        for (int w = 1; w < kShufThreads / 64; w++) mm = max(mm, red[w]);
        scale_sh = fp8::scale_from_absmax_bits(mm);
        scales[blockIdx.x] = scale_sh;
    }
    __syncthreads();
    const float inv = 1.f / scale_sh;
    for (uint32_t q = threadIdx.x; q < a.squares; q += kShufThreads) {
        const SquarePlace p = shuf_place<8>(a, src, q);
        Square<2> sq;
        sq.load_run(p.client);
        if (p.form == 2) sq.transpose();
#pragma unroll
        for (int j = 0; j < 8; j++) {
            uint32_t out[2] = {0, 0};
#pragma unroll
            for (int i = 0; i < 8; i++) {
                float f = fp8::bits_f32(sq.get(j, i) << 16);
                out[i / 4] |= static_cast<uint32_t>(fp8::f32_to_e4m3(f * inv)) << (8 * (i % 4));
            }
            d2[p.g0 + j * p.row_step] = make_uint2(out[0], out[1]);
        }
    }
}

// Row j of a square from 8 decoded bf16 (bits).
__device__ __forceinline__ void shuf_set_row(Square<2>& sq, int j, const uint16_t (&v)[8]) {
#pragma unroll
    for (int k = 0; k < 4; k++)
        sq.w[j][k] = static_cast<uint32_t>(v[2 * k]) | static_cast<uint32_t>(v[2 * k + 1]) << 16;
}

// fp8 dequantize: nothing needs a page-wide pass, so the workgroup is a
// (block, chunk), with block b's scale in scales[b]. Per row 8 codes in
// (uint2) -> 8 bf16.
__global__ __launch_bounds__(kShufThreads) void dequant_blocks_fp8_bf16_shuf_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs,
    const float* __restrict__ scales, ShufArgs a) {
    uint32_t b;
    uint64_t pool, client;
    const uint32_t chunk = shuf_block_chunk(src_ptrs, dst_ptrs, a, &b, &pool, &client);
    const float scale = scales[b];
    const uint2* s2 = reinterpret_cast<const uint2*>(pool);
    const uint32_t stride = a.chunks * kShufThreads;
    for (uint32_t q = chunk * kShufThreads + threadIdx.x; q < a.squares; q += stride) {
        const SquarePlace p = shuf_place<8>(a, client, q);
        Square<2> sq;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint2 pk = s2[p.g0 + j * p.row_step];
            const uint32_t c[2] = {pk.x, pk.y};
            uint16_t v[8];
#pragma unroll
            for (int i = 0; i < 8; i++)
                v[i] = fp8::decode_to_bf16(static_cast<uint8_t>(c[i / 4] >> (8 * (i % 4))), scale);
            shuf_set_row(sq, j, v);
        }
        if (p.form == 2) sq.transpose();
        sq.store_run(p.client);
    }
}

// mxfp4: codes and scale bytes are indexed by the page-global STORED unit g:
// a row's 8 codes are the 4 bytes at codes[g], the group's scale byte sits
// behind all codes at page_elems / 2 + (g >> 2). A row is whole groups
// (shuffle_legal), so C/X, the squares per page and every loop stride are
// multiples of 4: the four lanes 4k..4k+3 hold squares 4m..4m+3 of ONE token
// slab in every iteration, all four in range or none, and row j of the four is
// units 4n..4n+3 of one stored row. __shfl_xor by 1 and 2 thus stays inside
// the group, as in quant_blocks_bf16_mxfp4_kernel, and exactly the lane with
// (g & 3) == 0 writes the scale.
__global__ __launch_bounds__(kShufThreads) void quant_blocks_bf16_mxfp4_shuf_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs, ShufArgs a) {
    uint32_t b;
    uint64_t pool, client;
    const uint32_t chunk = shuf_block_chunk(src_ptrs, dst_ptrs, a, &b, &pool, &client);
    uint32_t* codes = reinterpret_cast<uint32_t*>(pool);
    uint8_t* scales = reinterpret_cast<uint8_t*>(pool) + a.page_elems / 2;
    const uint32_t stride = a.chunks * kShufThreads;
    for (uint32_t q = chunk * kShufThreads + threadIdx.x; q < a.squares; q += stride) {
        const SquarePlace p = shuf_place<8>(a, client, q);
        Square<2> sq;
        sq.load_run(p.client);
        if (p.form == 2) sq.transpose();
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint64_t g = p.g0 + j * p.row_step;
            uint32_t key = 0;
#pragma unroll
            for (int i = 0; i < 8; i++)
                key = mxfp4::key_step(key, static_cast<uint16_t>(sq.get(j, i)));
            key = max(key, __shfl_xor(key, 1, 64));
            key = max(key, __shfl_xor(key, 2, 64));
            const uint8_t E = mxfp4::group_exponent(key);
            uint32_t out = 0;
#pragma unroll
            for (int i = 0; i < 8; i++)
                out |= static_cast<uint32_t>(
                           mxfp4::encode(static_cast<uint16_t>(sq.get(j, i)), E))
                       << (4 * i);
            codes[g] = out;
            if ((g & 3u) == 0) scales[g >> 2] = E;
        }
    }
}

// Decoding is lane-local: per row 4 code bytes plus the group's scale byte in,
// 8 bf16 out.
__global__ __launch_bounds__(kShufThreads) void dequant_blocks_mxfp4_bf16_shuf_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs, ShufArgs a) {
    uint32_t b;
    uint64_t pool, client;
    const uint32_t chunk = shuf_block_chunk(src_ptrs, dst_ptrs, a, &b, &pool, &client);
    const uint32_t* codes = reinterpret_cast<const uint32_t*>(pool);
    const uint8_t* scales = reinterpret_cast<const uint8_t*>(pool) + a.page_elems / 2;
    const uint32_t stride = a.chunks * kShufThreads;
    for (uint32_t q = chunk * kShufThreads + threadIdx.x; q < a.squares; q += stride) {
        const SquarePlace p = shuf_place<8>(a, client, q);
        Square<2> sq;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint64_t g = p.g0 + j * p.row_step;
            const uint32_t pk = codes[g];
            const uint8_t E = scales[g >> 2];
            uint16_t v[8];
#pragma unroll
            for (int i = 0; i < 8; i++)
                v[i] = mxfp4::decode(static_cast<uint8_t>((pk >> (4 * i)) & 0xfu), E);
            shuf_set_row(sq, j, v);
        }
        if (p.form == 2) sq.transpose();
        sq.store_run(p.client);
    }
}

static bool shuf_refuse(const char* what, const char* why) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", what, why);
    set_last_error(msg);
    return false;
}

static bool shuf_hip_ok(const char* what, hipError_t e) {
    return e == hipSuccess || shuf_refuse(what, hipGetErrorString(e));
}

// What both launchers do after the codec-specific checks: the refusals they
// share, the kernel arguments and the (block, chunk) grid. per_page is true
// for the fp8 quantizer (one workgroup per page).
static bool shuf_args(const char* what, PageCodec codec, size_t page_bytes, PageShuffle sh,
                      PageSegments seg, PageDir dir, bool aligned16, int n_blocks, bool per_page,
                      ShufArgs* a, uint32_t* grid) {
    if (!shuffle_legal(codec, page_bytes, sh, seg)) return shuf_refuse(what, "illegal page shuffle");
    if (!aligned16) return shuf_refuse(what, "needs 16-byte-aligned pointers");
    if (seg.n != 1 && seg.stride_bytes % 16 != 0)
        return shuf_refuse(what, "needs a segment stride of a multiple of 16 bytes");
    const uint32_t X = 16 / sh.elem_bytes;
    a->slabs = sh.tokens / X;
    a->cgroups = sh.cols / X;
    a->tokens = sh.tokens;
    a->heads = sh.heads;
    a->form0 = sh.form[0];
    a->form1 = sh.form[1];
    a->tiles_per_seg = sh.outer * sh.heads / seg.n;
    a->n_segs = seg.n;
    a->to_pool = dir == PageDir::kStore;
    a->seg_stride = seg.n > 1 ? seg.stride_bytes : 0;
    a->tile_bytes = static_cast<uint64_t>(sh.tokens) * sh.cols * sh.elem_bytes;
    a->page_elems = page_bytes / sh.elem_bytes;
    // Square indices are 32-bit in the kernels: one square is X * 16 bytes.
    const uint64_t squares = page_bytes / (16ull * X);
    if (squares > 0x7fffffffull) return shuf_refuse(what, "page too large");
    a->squares = static_cast<uint32_t>(squares);
    // About 4096 workgroups, as the copy kernels size their grids.
    const uint64_t n = n_blocks > 0 ? static_cast<uint64_t>(n_blocks) : 0;
    const uint64_t max_chunks = (squares + kShufThreads - 1) / kShufThreads;
    const uint64_t want = n ? (4096 + n - 1) / n : 1;
    a->chunks = per_page
                    ? 1u
                    : static_cast<uint32_t>(std::max<uint64_t>(std::min(want, max_chunks), 1));
    const uint64_t g = n * a->chunks;
    if (g > 0x7fffffffull) return shuf_refuse(what, "grid does not fit");
    *grid = static_cast<uint32_t>(g);
    return true;
}

bool launch_copy_blocks_shuf(int dev, Stream stream, const uint64_t* dev_src,
                             const uint64_t* dev_dst, int n_blocks, size_t bytes_per_block,
                             bool aligned16, PageSegments seg, PageDir dir, PageShuffle sh) {
    const char* what = "launch_copy_blocks_shuf";
    ShufArgs a;
    uint32_t grid;
    if (!shuf_args(what, PageCodec::kNone, bytes_per_block, sh, seg, dir, aligned16, n_blocks,
                   false, &a, &grid))
        return false;
    if (n_blocks <= 0) return true;
    if (!shuf_hip_ok(what, hipSetDevice(dev))) return false;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 g(grid), t(kShufThreads);
    switch (sh.elem_bytes) {
        case 1:
            hipLaunchKernelGGL(copy_blocks_shuf_kernel<1>, g, t, 0, s, dev_src, dev_dst, a);
            break;
        case 2:
            hipLaunchKernelGGL(copy_blocks_shuf_kernel<2>, g, t, 0, s, dev_src, dev_dst, a);
            break;
        default:
            hipLaunchKernelGGL(copy_blocks_shuf_kernel<4>, g, t, 0, s, dev_src, dev_dst, a);
            break;
    }
    return shuf_hip_ok(what, hipGetLastError());
}

bool launch_transform_blocks_shuf(int dev, Stream stream, PageCodec codec, PageDir dir,
                                  const uint64_t* dev_src, const uint64_t* dev_dst,
                                  float* dev_scales, int n_blocks, size_t elems_per_block,
                                  bool aligned16, PageSegments seg, PageShuffle sh) {
    const char* what = "launch_transform_blocks_shuf";
    if (!page_codec_known(static_cast<uint32_t>(codec)) || !page_codec_transforms(codec) ||
        elems_per_block == 0 || elems_per_block > SIZE_MAX / kPageElemBytes ||
        !page_legal(codec, elems_per_block * kPageElemBytes))
        return shuf_refuse(what, "not a page of a transforming codec");
    const size_t page_bytes = elems_per_block * kPageElemBytes;
    const bool store = dir == PageDir::kStore;
    ShufArgs a;
    uint32_t grid;
    if (!shuf_args(what, codec, page_bytes, sh, seg, dir, aligned16, n_blocks,
                   store && codec == PageCodec::kFp8, &a, &grid))
        return false;
    if (page_codec_info(codec).page_scale && !dev_scales)
        return shuf_refuse(what, "needs a scale per page");
    if (n_blocks <= 0) return true;
    if (!shuf_hip_ok(what, hipSetDevice(dev))) return false;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 g(grid), t(kShufThreads);
    switch (codec) {
        case PageCodec::kFp8:
            if (store)
                hipLaunchKernelGGL(quant_blocks_bf16_fp8_shuf_kernel, g, t, 0, s, dev_src, dev_dst,
                                   dev_scales, a);
            else
                hipLaunchKernelGGL(dequant_blocks_fp8_bf16_shuf_kernel, g, t, 0, s, dev_src,
                                   dev_dst, dev_scales, a);
            break;
        case PageCodec::kMxfp4:
            if (store)
                hipLaunchKernelGGL(quant_blocks_bf16_mxfp4_shuf_kernel, g, t, 0, s, dev_src,
                                   dev_dst, a);
            else
                hipLaunchKernelGGL(dequant_blocks_mxfp4_bf16_shuf_kernel, g, t, 0, s, dev_src,
                                   dev_dst, a);
            break;
        default:
            return false;
    }
    return shuf_hip_ok(what, hipGetLastError());
}

}  // namespace gpu
}  // namespace ifs
