// Transposed pages: paged-attention cache blocks <-> canonical pages, MI355X
// (gfx950).
//
// The CLIENT side of every page (source of kStore, destination of kLoad) is a
// paged-attention cache block (core/page_codec.h, PageTranspose; gpu.h;
// docs/design.md "transposed pages"): per half o and head h, C/x_o column
// blocks of T runs of x_o elements, i.e. K as [H, C/x, T, x] and V as
// [H, C, T]. The stored block is byte-identical to the one the contiguous
// kernels make of the canonical [outer, T, H, C] page.
//
// Unit of work. One TILE is one (block, o, h): T x C elements. On the client
// it is T*C*elem_bytes contiguous bytes inside its segment; on the stored side
// it is T rows of C elements, H*C elements apart. A workgroup is one tile
// (the fp8 quantizer, whose scale is the page's, is one workgroup per page and
// loops over the page's tiles). The descriptor pair is read once through LDS;
// the geometry rides in the kernel arguments.
//
// Data path: destination <- LDS tile <- source. Neither side can be walked in
// the other's order with 16-byte accesses: a client unit holds 16/(x_o*eb)
// runs of CONSECUTIVE TOKENS of one column block, a stored unit 16/eb
// consecutive columns of one token. So the source is read with 16-byte loads
// in its own order and written into an LDS tile indexed [t][c]; after one
// __syncthreads() the destination is written with 16-byte stores in its own
// order, reading the tile the other way. Per client unit k the run index
// k * runs_per_unit splits by ONE division by T (workgroup-uniform) into the
// column block and the first token; T % runs_per_unit == 0 (transpose_legal)
// keeps a unit inside its column block. Per stored unit one division by the
// units per row gives the token. Everything else is shifts by the run size,
// which is a template parameter picked by a workgroup-uniform switch.
//
// LDS row pitch. The tile's rows are C*eb bytes (a multiple of 16) with no
// padding: T * C * eb bytes of LDS per tile, 4 KiB for T = 16, C = 128 bf16,
// 8 KiB for T = 32, at most kMaxTransposeTile = 32 KiB, so five workgroups fit
// a CU's 160 KiB at the largest tile. The stored-order side moves 16 bytes per
// lane along a row and is conflict-free at any pitch. The client-order side
// moves one run per step, and with rows of a multiple of 256 bytes (V in bf16,
// C = 128) lanes that differ only in their token group may meet in a bank. A
// pitch of one 16-byte pad per row, which would spread them, was measured
// against this one on exactly that tile (docs/perf_notes.md): launch-to-sync
// time of the plain kernel on 4096 all-V pages of 64 KiB, both directions,
// three alternating runs a side, was 306-331 us padded against 310-335 us
// unpadded, about 2.1 TB/s of traffic either way, and the harness did not
// separate them either. The kernel waits on HBM, not on LDS, so the simpler
// pitch is kept. Whether the accesses conflict at all was not measured.
//
// Codecs act on the stored side only, with the codec headers' functions in
// the contiguous kernels' own expressions; the LDS tile always holds bf16.
//
// A translation unit of its own, compiled without packed fp32 instructions as
// quant_error.hip is (infinistore_amd/_build.py); the device functions of
// gpu.hip keep the code they have.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "fp8_codec.h"
#include "gpu.h"
#include "mxfp4_codec.h"

namespace ifs {
namespace gpu {

struct XposeArgs {
    uint32_t outer, tokens, heads;
    uint32_t row_bytes;       // one (token, head) row of the tile, LOGICAL bytes
    uint32_t run_shift0;      // log2(x_0 * elem_bytes): bytes of one client run, half 0
    uint32_t run_shift1;      // the same for half 1
    uint32_t tiles_per_seg;   // outer * heads / client segments
    uint32_t n_segs;          // client segments
    uint32_t to_pool;         // 1: client -> stored block, 0: stored block -> client
    uint64_t seg_stride;      // client bytes from one segment to the next
    uint64_t page_bytes;      // logical
};

template <int RB> struct XposeRun;
template <> struct XposeRun<1> { using type = uint8_t; };
template <> struct XposeRun<2> { using type = uint16_t; };
template <> struct XposeRun<4> { using type = uint32_t; };
template <> struct XposeRun<8> { using type = uint2; };
template <> struct XposeRun<16> { using type = uint4; };

// The client side of one tile, in client order: 16 bytes per lane in global
// memory, one run of RB bytes per step in LDS. kToLds: client -> tile.
template <int RB, bool kToLds>
__device__ __forceinline__ void xpose_client_runs(const XposeArgs& a, uint64_t ctile,
                                                  unsigned char* tile) {
    using R = typename XposeRun<RB>::type;
    constexpr uint32_t kRuns = 16 / RB;
    const uint32_t units = a.tokens * (a.row_bytes / 16);  // <= 2048
    uint4* c4 = reinterpret_cast<uint4*>(ctile);
    for (uint32_t k = threadIdx.x; k < units; k += blockDim.x) {
        const uint32_t r0 = k * kRuns;
        const uint32_t cb = r0 / a.tokens;
        const uint32_t t0 = r0 - cb * a.tokens;
        unsigned char* p = tile + t0 * a.row_bytes + cb * RB;
        uint4 pk;
        R* runs = reinterpret_cast<R*>(&pk);
        if (kToLds) {
            pk = c4[k];
#pragma unroll
            for (uint32_t j = 0; j < kRuns; j++)
                *reinterpret_cast<R*>(p + j * a.row_bytes) = runs[j];
        } else {
#pragma unroll
            for (uint32_t j = 0; j < kRuns; j++)
                runs[j] = *reinterpret_cast<const R*>(p + j * a.row_bytes);
            c4[k] = pk;
        }
    }
}

template <bool kToLds>
__device__ __forceinline__ void xpose_client_side(const XposeArgs& a, uint32_t o, uint64_t ctile,
                                                  unsigned char* tile) {
    switch (o ? a.run_shift1 : a.run_shift0) {  // workgroup-uniform
        case 0: xpose_client_runs<1, kToLds>(a, ctile, tile); break;
        case 1: xpose_client_runs<2, kToLds>(a, ctile, tile); break;
        case 2: xpose_client_runs<4, kToLds>(a, ctile, tile); break;
        case 3: xpose_client_runs<8, kToLds>(a, ctile, tile); break;
        default: xpose_client_runs<16, kToLds>(a, ctile, tile); break;
    }
}

// Client address of tile ti = o * heads + h of a page: its segment, and its
// place inside it. Once per tile, not per unit.
__device__ __forceinline__ uint64_t xpose_client_tile(const XposeArgs& a, uint64_t client,
                                                      uint32_t ti) {
    const uint32_t sg = ti / a.tiles_per_seg;
    return client + sg * a.seg_stride +
           static_cast<uint64_t>(ti - sg * a.tiles_per_seg) * a.tokens * a.row_bytes;
}

// The stored side of one tile, in stored order. move(g, lds) handles one
// 16-logical-byte unit: g is the unit's index in the whole stored page
// (((o*T + t)*H + h) * units_per_row + r), lds its place in the tile.
template <typename Move>
__device__ __forceinline__ void xpose_stored_rows(const XposeArgs& a, uint32_t o, uint32_t h,
                                                  unsigned char* tile, Move move) {
    const uint32_t ru = a.row_bytes / 16;
    const uint32_t units = a.tokens * ru;
    for (uint32_t u = threadIdx.x; u < units; u += blockDim.x) {
        const uint32_t t = u / ru;
        const uint32_t r = u - t * ru;
        const uint64_t g = (static_cast<uint64_t>(o * a.tokens + t) * a.heads + h) * ru + r;
        move(g, reinterpret_cast<uint4*>(tile + t * a.row_bytes) + r);
    }
}

// The prologue of the four (block, o, h) kernels: decodes the triple, reads
// block b's descriptor pair once through LDS as block_chunk_descs does, and
// hands out the pool and client base addresses whichever way the copy runs.
__device__ __forceinline__ void xpose_block_tile(const uint64_t* __restrict__ src_ptrs,
                                                 const uint64_t* __restrict__ dst_ptrs,
                                                 const XposeArgs& a, uint32_t* b, uint32_t* o,
                                                 uint32_t* h, uint64_t* pool, uint64_t* client) {
    const uint32_t per_block = a.outer * a.heads;
    *b = blockIdx.x / per_block;
    const uint32_t ti = blockIdx.x - *b * per_block;
    *o = ti / a.heads;
    *h = ti - *o * a.heads;
    __shared__ uint64_t lds[2];
    if (threadIdx.x == 0) {
        lds[0] = src_ptrs[*b];
        lds[1] = dst_ptrs[*b];
    }
    __syncthreads();
    *pool = a.to_pool ? lds[1] : lds[0];
    *client = xpose_client_tile(a, a.to_pool ? lds[0] : lds[1], ti);
}

extern __shared__ uint4 xpose_lds[];  // the tile: tokens * row_bytes bytes

// plain, both directions: raw elements of any legal size.
__global__ __launch_bounds__(kXposeThreads) void copy_blocks_xpose_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs, XposeArgs a) {
    unsigned char* tile = reinterpret_cast<unsigned char*>(xpose_lds);
    uint32_t b, o, h;
    uint64_t pool, client;
    xpose_block_tile(src_ptrs, dst_ptrs, a, &b, &o, &h, &pool, &client);
    uint4* p4 = reinterpret_cast<uint4*>(pool);
    if (a.to_pool) {
        xpose_client_side<true>(a, o, client, tile);
        __syncthreads();
        xpose_stored_rows(a, o, h, tile, [&](uint64_t g, uint4* l) { p4[g] = *l; });
    } else {
        xpose_stored_rows(a, o, h, tile, [&](uint64_t g, uint4* l) { *l = p4[g]; });
        __syncthreads();
        xpose_client_side<false>(a, o, client, tile);
    }
}

// fp8 quantize: one workgroup per page and two passes, because the scale is
// the PAGE's. The absmax does not depend on the order of the elements, so pass
// 1 reads the client page linearly, segment by segment. Pass 2 takes the
// page's outer * H tiles through the LDS path one after the other: 8 bf16 out
// of the tile -> 8 codes (uint2) per lane; stored byte = logical element
// index, so unit g's codes are the uint2 at index g.
__global__ __launch_bounds__(kXposeThreads) void quant_blocks_bf16_fp8_xpose_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs,
    float* __restrict__ scales, XposeArgs a) {
    unsigned char* tile = reinterpret_cast<unsigned char*>(xpose_lds);
    __shared__ uint64_t desc[2];  // the descriptor pair, read once as in xpose_block_tile
    if (threadIdx.x == 0) {
        desc[0] = src_ptrs[blockIdx.x];
        desc[1] = dst_ptrs[blockIdx.x];
    }
    __syncthreads();
    const uint64_t src = desc[0];
    uint2* d2 = reinterpret_cast<uint2*>(desc[1]);
    __shared__ uint32_t red[kXposeThreads / 64];
    __shared__ float scale_sh;
    uint32_t m = 0;  // largest finite bf16 magnitude, as bits
    const uint64_t seg16 = static_cast<uint64_t>(a.tiles_per_seg) * a.tokens * (a.row_bytes / 16);
    for (uint32_t sg = 0; sg < a.n_segs; sg++) {
        const uint4* src4 = reinterpret_cast<const uint4*>(src + sg * a.seg_stride);
        for (uint64_t u = threadIdx.x; u < seg16; u += blockDim.x) {
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
        for (int w = 1; w < static_cast<int>(blockDim.x) / 64; w++) mm = max(mm, red[w]);
        scale_sh = fp8::scale_from_absmax_bits(mm);
        scales[blockIdx.x] = scale_sh;
    }
    __syncthreads();
    const float inv = 1.f / scale_sh;
    for (uint32_t o = 0; o < a.outer; o++)
        for (uint32_t h = 0; h < a.heads; h++) {
            xpose_client_side<true>(a, o, xpose_client_tile(a, src, o * a.heads + h), tile);
            __syncthreads();
            xpose_stored_rows(a, o, h, tile, [&](uint64_t g, uint4* l) {
                uint4 pk = *l;
                const uint16_t* hw = reinterpret_cast<const uint16_t*>(&pk);
                uint8_t out[8];
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    float f = fp8::bits_f32(static_cast<uint32_t>(hw[i]) << 16);
                    out[i] = fp8::f32_to_e4m3(f * inv);
                }
                d2[g] = *reinterpret_cast<const uint2*>(out);
            });
            __syncthreads();  // the tile is free for the next one
        }
}

// fp8 dequantize: nothing needs a page-wide pass, so the workgroup is the
// tile, with block b's scale in scales[b]. 8 codes in (uint2) -> 8 bf16 into
// the tile per lane.
__global__ __launch_bounds__(kXposeThreads) void dequant_blocks_fp8_bf16_xpose_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs,
    const float* __restrict__ scales, XposeArgs a) {
    unsigned char* tile = reinterpret_cast<unsigned char*>(xpose_lds);
    uint32_t b, o, h;
    uint64_t pool, client;
    xpose_block_tile(src_ptrs, dst_ptrs, a, &b, &o, &h, &pool, &client);
    const float scale = scales[b];
    const uint2* s2 = reinterpret_cast<const uint2*>(pool);
    xpose_stored_rows(a, o, h, tile, [&](uint64_t g, uint4* l) {
        uint2 pk = s2[g];
        const uint8_t* c = reinterpret_cast<const uint8_t*>(&pk);
        uint16_t out[8];
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = fp8::decode_to_bf16(c[i], scale);
        *l = *reinterpret_cast<const uint4*>(out);
    });
    __syncthreads();
    xpose_client_side<false>(a, o, client, tile);
}

// mxfp4: codes and scale bytes are indexed by the page-global STORED unit g:
// the lane's 8 codes are the 4 bytes at codes[g], the group's scale byte sits
// behind all codes at page_elems / 2 + (g >> 2). The quantizer reads
// stored-order rows out of the tile with four lanes per 32-element group. A
// row is whole groups (transpose_legal), so the units per row, the units per
// tile and the workgroup size are multiples of 4: the four lanes 4k..4k+3 hold
// units 4j..4j+3 of ONE row in every iteration, all four inside the tile or
// none, and g agrees with the unit in its low two bits. __shfl_xor by 1 and 2
// thus stays inside the group, as in quant_blocks_bf16_mxfp4_kernel, and
// exactly the lane with (g & 3) == 0 writes the scale.
__global__ __launch_bounds__(kXposeThreads) void quant_blocks_bf16_mxfp4_xpose_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs, XposeArgs a) {
    unsigned char* tile = reinterpret_cast<unsigned char*>(xpose_lds);
    uint32_t b, o, h;
    uint64_t pool, client;
    xpose_block_tile(src_ptrs, dst_ptrs, a, &b, &o, &h, &pool, &client);
    uint32_t* codes = reinterpret_cast<uint32_t*>(pool);
    uint8_t* scales = reinterpret_cast<uint8_t*>(pool) + a.page_bytes / kPageElemBytes / 2;
    xpose_client_side<true>(a, o, client, tile);
    __syncthreads();
    xpose_stored_rows(a, o, h, tile, [&](uint64_t g, uint4* l) {
        uint4 pk = *l;
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
        codes[g] = out;
        if ((g & 3u) == 0) scales[g >> 2] = E;
    });
}

// Decoding is lane-local: 4 code bytes plus the group's scale byte in, 8 bf16
// into the tile.
__global__ __launch_bounds__(kXposeThreads) void dequant_blocks_mxfp4_bf16_xpose_kernel(
    const uint64_t* __restrict__ src_ptrs, const uint64_t* __restrict__ dst_ptrs, XposeArgs a) {
    unsigned char* tile = reinterpret_cast<unsigned char*>(xpose_lds);
    uint32_t b, o, h;
    uint64_t pool, client;
    xpose_block_tile(src_ptrs, dst_ptrs, a, &b, &o, &h, &pool, &client);
    const uint32_t* codes = reinterpret_cast<const uint32_t*>(pool);
    const uint8_t* scales =
        reinterpret_cast<const uint8_t*>(pool) + a.page_bytes / kPageElemBytes / 2;
    xpose_stored_rows(a, o, h, tile, [&](uint64_t g, uint4* l) {
        uint32_t pk = codes[g];
        uint8_t E = scales[g >> 2];
        uint16_t out[8];
#pragma unroll
        for (int i = 0; i < 8; i++)
            out[i] = mxfp4::decode(static_cast<uint8_t>((pk >> (4 * i)) & 0xfu), E);
        *l = *reinterpret_cast<const uint4*>(out);
    });
    __syncthreads();
    xpose_client_side<false>(a, o, client, tile);
}

static bool xpose_refuse(const char* what, const char* why) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", what, why);
    set_last_error(msg);
    return false;
}

static bool xpose_hip_ok(const char* what, hipError_t e) {
    return e == hipSuccess || xpose_refuse(what, hipGetErrorString(e));
}

// What both launchers do after the codec-specific checks: the refusals they
// share, the kernel arguments, the tile's LDS bytes and the (block, o, h)
// grid. need_grid is false for the fp8 quantizer (one workgroup per page).
static bool xpose_args(const char* what, PageCodec codec, size_t page_bytes, PageTranspose xp,
                       PageSegments seg, PageDir dir, bool aligned16, int n_blocks,
                       bool need_grid, XposeArgs* a, uint32_t* lds_bytes, uint32_t* grid) {
    if (!transpose_legal(codec, page_bytes, xp, seg))
        return xpose_refuse(what, "illegal page transpose");
    if (!aligned16) return xpose_refuse(what, "needs 16-byte-aligned pointers");
    if (seg.n != 1 && seg.stride_bytes % 16 != 0)
        return xpose_refuse(what, "needs a segment stride of a multiple of 16 bytes");
    a->outer = xp.outer;
    a->tokens = xp.tokens;
    a->heads = xp.heads;
    a->row_bytes = xp.cols * xp.elem_bytes;
    a->run_shift0 = static_cast<uint32_t>(__builtin_ctz(xp.inner[0] * xp.elem_bytes));
    a->run_shift1 = static_cast<uint32_t>(__builtin_ctz(xp.inner[1] * xp.elem_bytes));
    a->tiles_per_seg = xp.outer * xp.heads / seg.n;
    a->n_segs = seg.n;
    a->to_pool = dir == PageDir::kStore;
    a->seg_stride = seg.n > 1 ? seg.stride_bytes : 0;
    a->page_bytes = page_bytes;
    *lds_bytes = a->tokens * a->row_bytes;  // the tile: <= kMaxTransposeTile
    const uint64_t g = static_cast<uint64_t>(n_blocks > 0 ? n_blocks : 0) * xp.outer * xp.heads;
    if (need_grid && g > 0x7fffffffull) return xpose_refuse(what, "grid does not fit");
    *grid = static_cast<uint32_t>(g);
    return true;
}

bool launch_copy_blocks_xpose(int dev, Stream stream, const uint64_t* dev_src,
                              const uint64_t* dev_dst, int n_blocks, size_t bytes_per_block,
                              bool aligned16, PageSegments seg, PageDir dir, PageTranspose xp) {
    const char* what = "launch_copy_blocks_xpose";
    XposeArgs a;
    uint32_t lds, grid;
    if (!xpose_args(what, PageCodec::kNone, bytes_per_block, xp, seg, dir, aligned16, n_blocks,
                    true, &a, &lds, &grid))
        return false;
    if (n_blocks <= 0) return true;
    if (!xpose_hip_ok(what, hipSetDevice(dev))) return false;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(copy_blocks_xpose_kernel, dim3(grid), dim3(kXposeThreads), lds, s, dev_src,
                       dev_dst, a);
    return xpose_hip_ok(what, hipGetLastError());
}

bool launch_transform_blocks_xpose(int dev, Stream stream, PageCodec codec, PageDir dir,
                                   const uint64_t* dev_src, const uint64_t* dev_dst,
                                   float* dev_scales, int n_blocks, size_t elems_per_block,
                                   bool aligned16, PageSegments seg, PageTranspose xp) {
    const char* what = "launch_transform_blocks_xpose";
    const size_t page_bytes = elems_per_block * kPageElemBytes;
    if (!page_codec_known(static_cast<uint32_t>(codec)) || !page_codec_transforms(codec) ||
        elems_per_block == 0 || !page_legal(codec, page_bytes))
        return xpose_refuse(what, "not a page of a transforming codec");
    const bool store = dir == PageDir::kStore;
    XposeArgs a;
    uint32_t lds, grid;
    if (!xpose_args(what, codec, page_bytes, xp, seg, dir, aligned16, n_blocks,
                    !(store && codec == PageCodec::kFp8), &a, &lds, &grid))
        return false;
    if (page_codec_info(codec).page_scale && !dev_scales)
        return xpose_refuse(what, "needs a scale per page");
    if (n_blocks <= 0) return true;
    if (!xpose_hip_ok(what, hipSetDevice(dev))) return false;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 block(kXposeThreads);
    switch (codec) {
        case PageCodec::kFp8:
            if (store)
                hipLaunchKernelGGL(quant_blocks_bf16_fp8_xpose_kernel, dim3(n_blocks), block, lds,
                                   s, dev_src, dev_dst, dev_scales, a);
            else
                hipLaunchKernelGGL(dequant_blocks_fp8_bf16_xpose_kernel, dim3(grid), block, lds, s,
                                   dev_src, dev_dst, dev_scales, a);
            break;
        case PageCodec::kMxfp4:
            if (store)
                hipLaunchKernelGGL(quant_blocks_bf16_mxfp4_xpose_kernel, dim3(grid), block, lds, s,
                                   dev_src, dev_dst, a);
            else
                hipLaunchKernelGGL(dequant_blocks_mxfp4_bf16_xpose_kernel, dim3(grid), block, lds,
                                   s, dev_src, dev_dst, a);
            break;
        default:
            return false;
    }
    return xpose_hip_ok(what, hipGetLastError());
}

}  // namespace gpu
}  // namespace ifs
