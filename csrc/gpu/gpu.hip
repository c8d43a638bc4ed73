// MI355X (gfx950) HIP implementation: arenas, IPC, streams, and the batched
// block gather/scatter + fingerprint kernels. See gpu.h for the design notes.
//
// Kernels are written for CDNA4: 64-wide wavefronts, 16 B/lane vectorized
// global accesses (uint4), grid sized to cover 256 CUs with grid-stride
// loops (memory-bound kernel rule from the CDNA4 programming guide).
#include "gpu.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "../core/log.h"
#include "fp8_codec.h"
#include "mxfp4_codec.h"

namespace ifs {
namespace gpu {

static thread_local char g_err[256] = {0};
const char* last_error() { return g_err; }

static bool fail(const char* what, hipError_t e) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    ERROR("%s", g_err);
    return false;
}

#define HIP_OK(call)                                  \
    do {                                              \
        hipError_t _e = (call);                       \
        if (_e != hipSuccess) return fail(#call, _e); \
    } while (0)

static int cached_device_count() {
    static int n = []() {
        int c = 0;
        hipError_t e = hipGetDeviceCount(&c);
        if (e != hipSuccess) return 0;
        return c;
    }();
    return n;
}

bool available() { return cached_device_count() > 0; }
int device_count() { return cached_device_count(); }

std::string device_name(int dev) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return "unknown";
    return prop.name;
}

size_t device_total_mem(int dev) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    return prop.totalGlobalMem;
}

bool set_device(int dev) {
    HIP_OK(hipSetDevice(dev));
    return true;
}

void* alloc_device(int dev, size_t bytes) {
    if (hipSetDevice(dev) != hipSuccess) return nullptr;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        fail("hipMalloc", e);
        return nullptr;
    }
    return p;
}

void free_device(void* p) {
    if (p) hipFree(p);
}

void* alloc_host_pinned(size_t bytes) {
    if (available()) {
        void* p = nullptr;
        if (hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess) return p;
    }
    void* p = nullptr;
    if (posix_memalign(&p, 4096, bytes) != 0) return nullptr;
    return p;
}

void free_host_pinned(void* p) {
    if (!p) return;
    if (available()) {
        if (hipHostFree(p) == hipSuccess) return;
    }
    free(p);
}

bool memcpy_d2h(void* dst, const void* src, size_t n) {
    HIP_OK(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
    return true;
}
bool memcpy_h2d(void* dst, const void* src, size_t n) {
    HIP_OK(hipMemcpy(dst, src, n, hipMemcpyHostToDevice));
    return true;
}
bool memcpy_d2d(void* dst, const void* src, size_t n) {
    HIP_OK(hipMemcpy(dst, src, n, hipMemcpyDefault));
    return true;
}
bool memcpy_h2d_async(void* dst, const void* src, size_t n, Stream s) {
    HIP_OK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, reinterpret_cast<hipStream_t>(s)));
    return true;
}
bool memcpy_d2h_async(void* dst, const void* src, size_t n, Stream s) {
    HIP_OK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, reinterpret_cast<hipStream_t>(s)));
    return true;
}
bool memcpy_any_async(void* dst, const void* src, size_t n, Stream s) {
    HIP_OK(hipMemcpyAsync(dst, src, n, hipMemcpyDefault, reinterpret_cast<hipStream_t>(s)));
    return true;
}

// --- IPC -------------------------------------------------------------------
static_assert(sizeof(hipIpcMemHandle_t) == kIpcHandleSize, "hip ipc handle size");

bool ipc_export(const void* ptr, IpcHandle* handle, uint64_t* base_offset,
                uint64_t* alloc_size) {
    // Find the allocation base so tensors offset inside a caching-allocator
    // segment still round-trip exactly.
    void* base = nullptr;
    hipError_t e = hipPointerGetAttribute(&base, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR,
                                          reinterpret_cast<hipDeviceptr_t>(const_cast<void*>(ptr)));
    if (e != hipSuccess || base == nullptr) {
        base = const_cast<void*>(ptr);  // assume ptr is the base
    }
    *base_offset = reinterpret_cast<uintptr_t>(ptr) - reinterpret_cast<uintptr_t>(base);
    if (alloc_size) {
        size_t sz = 0;
        if (hipPointerGetAttribute(&sz, HIP_POINTER_ATTRIBUTE_RANGE_SIZE,
                                   reinterpret_cast<hipDeviceptr_t>(base)) != hipSuccess)
            sz = 0;  // unknown: caller decides
        *alloc_size = sz;
    }
    hipIpcMemHandle_t h;
    HIP_OK(hipIpcGetMemHandle(&h, base));
    memcpy(handle->bytes, &h, sizeof(h));
    return true;
}

void* ipc_open(const IpcHandle& handle, int src_device) {
    if (hipSetDevice(src_device) != hipSuccess) return nullptr;
    hipIpcMemHandle_t h;
    memcpy(&h, handle.bytes, sizeof(h));
    void* p = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
        fail("hipIpcOpenMemHandle", e);
        return nullptr;
    }
    return p;
}

bool ipc_close(void* base) {
    HIP_OK(hipIpcCloseMemHandle(base));
    return true;
}

bool is_device_pointer(const void* ptr) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) {
        (void)hipGetLastError();  // clear sticky error for untracked host ptrs
        return false;
    }
    return attr.type == hipMemoryTypeDevice;
}

int export_dmabuf(void* ptr, size_t size, uint64_t* offset) {
    *offset = 0;
#if HIP_VERSION >= 60000000 || defined(hipMemRangeHandleTypeDmaBufFd)
    int fd = -1;
    hipError_t e = hipMemGetHandleForAddressRange(&fd, reinterpret_cast<hipDeviceptr_t>(ptr),
                                                  size, hipMemRangeHandleTypeDmaBufFd, 0);
    if (e != hipSuccess) {
        fail("hipMemGetHandleForAddressRange", e);
        return -1;
    }
    return fd;
#else
    (void)ptr;
    (void)size;
    return -1;
#endif
}

bool enable_peer_access(int dev, int peer) {
    if (dev == peer) return true;
    int can = 0;
    HIP_OK(hipDeviceCanAccessPeer(&can, dev, peer));
    if (!can) return false;
    HIP_OK(hipSetDevice(dev));
    hipError_t e = hipDeviceEnablePeerAccess(peer, 0);
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return fail("enable_peer", e);
    return true;
}

// --- streams / events ------------------------------------------------------
Stream stream_create(int dev) {
    if (hipSetDevice(dev) != hipSuccess) return nullptr;
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    return reinterpret_cast<Stream>(s);
}
void stream_destroy(Stream s) {
    if (s) hipStreamDestroy(reinterpret_cast<hipStream_t>(s));
}
bool stream_sync(Stream s) {
    HIP_OK(hipStreamSynchronize(reinterpret_cast<hipStream_t>(s)));
    return true;
}
Event event_create(int dev) {
    if (hipSetDevice(dev) != hipSuccess) return nullptr;
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    return reinterpret_cast<Event>(e);
}
void event_destroy(Event e) {
    if (e) hipEventDestroy(reinterpret_cast<hipEvent_t>(e));
}
bool event_record(Event e, Stream s) {
    HIP_OK(hipEventRecord(reinterpret_cast<hipEvent_t>(e), reinterpret_cast<hipStream_t>(s)));
    return true;
}
bool event_sync(Event e) {
    HIP_OK(hipEventSynchronize(reinterpret_cast<hipEvent_t>(e)));
    return true;
}
bool event_query(Event e) {
    return hipEventQuery(reinterpret_cast<hipEvent_t>(e)) == hipSuccess;
}

// ---------------------------------------------------------------------------
// Kernels
// ---------------------------------------------------------------------------

// Batched block copy, vectorized: 16 B per lane per iteration. Replaces the
// reference's per-block cudaMemcpyAsync hot loop
// (/root/reference/src/infinistore.cpp:622-625, 747-748) with one launch per
// request. Lanes walk consecutive uint4 units, so a wave issues fully
// coalesced 1 KiB transactions; grid-stride covers all blocks.
// 2D mapping: workgroup (b, chunk) covers block b's units
// [chunk*T, ...] striding by chunks*T. Each workgroup reads its block's
// descriptor ONCE (lane 0 -> LDS broadcast), so the descriptor arrays can
// live in pinned HOST memory with negligible PCIe cost — the earlier
// per-unit desc[b] indexing either taxed PCIe at ~payload/64 (pinned) or
// forced per-job uploads that rocclr ran as single-workgroup blits at
// ~110 µs each (profiles/rocprof_bench_r02.txt).

// The shared prologue of the 2D-mapped kernels (vector copy, byte copy, mxfp4
// quantize and dequantize): lane 0 reads block b's descriptor pair, LDS
// broadcasts it into sd[0] = src, sd[1] = dst; returns the workgroup's chunk.
// chunk is written as blockIdx.x - b * chunks, not as `%`: with `%` the
// compiler sinks the division into the lane-0 branch and divides twice (one
// more SGPR in both copy kernels); this form compiles to the same
// instructions as the prologue written out in each kernel.
__device__ __forceinline__ uint32_t block_chunk_descs(const uint64_t* __restrict__ src_ptrs,
                                                      const uint64_t* __restrict__ dst_ptrs,
                                                      uint32_t chunks_per_block,
                                                      uint64_t (&sd)[2]) {
    uint32_t b = blockIdx.x / chunks_per_block;
    uint32_t chunk = blockIdx.x - b * chunks_per_block;
    __shared__ uint64_t lds[2];
    if (threadIdx.x == 0) {
        lds[0] = src_ptrs[b];
        lds[1] = dst_ptrs[b];
    }
    __syncthreads();
    sd[0] = lds[0];
    sd[1] = lds[1];
    return chunk;
}

__global__ void copy_blocks_vec_kernel(const uint64_t* __restrict__ src_ptrs,
                                       const uint64_t* __restrict__ dst_ptrs,
                                       uint32_t chunks_per_block,
                                       uint64_t units_per_block) {
    uint64_t sd[2];
    uint32_t chunk = block_chunk_descs(src_ptrs, dst_ptrs, chunks_per_block, sd);
    const uint4* s = reinterpret_cast<const uint4*>(sd[0]);
    uint4* d = reinterpret_cast<uint4*>(sd[1]);
    uint64_t stride = static_cast<uint64_t>(chunks_per_block) * blockDim.x;
    for (uint64_t u = static_cast<uint64_t>(chunk) * blockDim.x + threadIdx.x;
         u < units_per_block; u += stride)
        d[u] = s[u];
}

// Small-request variant: descriptors passed by value as kernel arguments —
// no staging H2D, shaving two async copies off the single-block latency path.
struct InlineDescs {
    uint64_t src[16];
    uint64_t dst[16];
};

__global__ void copy_blocks_vec_inline_kernel(InlineDescs descs, int n_blocks,
                                              uint64_t units_per_block) {
    uint64_t total = static_cast<uint64_t>(n_blocks) * units_per_block;
    uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
    for (uint64_t u = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; u < total;
         u += stride) {
        uint64_t b = u / units_per_block;
        uint64_t off = u - b * units_per_block;
        const uint4* s = reinterpret_cast<const uint4*>(descs.src[b]) + off;
        uint4* d = reinterpret_cast<uint4*>(descs.dst[b]) + off;
        *d = *s;
    }
}

bool launch_copy_blocks_inline(int dev, Stream stream, const uint64_t* src_ptrs,
                               const uint64_t* dst_ptrs, int n_blocks, size_t bytes_per_block) {
    if (n_blocks <= 0 || n_blocks > 16 || bytes_per_block % 16 != 0) return false;
    HIP_OK(hipSetDevice(dev));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    InlineDescs descs;
    for (int i = 0; i < n_blocks; i++) {
        descs.src[i] = src_ptrs[i];
        descs.dst[i] = dst_ptrs[i];
    }
    uint64_t upb = bytes_per_block / 16;
    uint64_t total = static_cast<uint64_t>(n_blocks) * upb;
    const int threads = 256;
    int grid = static_cast<int>(std::min<uint64_t>((total + threads - 1) / threads, 4096));
    hipLaunchKernelGGL(copy_blocks_vec_inline_kernel, dim3(grid), dim3(threads), 0, s, descs,
                       n_blocks, upb);
    HIP_OK(hipGetLastError());
    return true;
}

// Byte-granular fallback for unaligned pointers / sizes (same 2D mapping).
__global__ void copy_blocks_byte_kernel(const uint64_t* __restrict__ src_ptrs,
                                        const uint64_t* __restrict__ dst_ptrs,
                                        uint32_t chunks_per_block,
                                        uint64_t bytes_per_block) {
    uint64_t sd[2];
    uint32_t chunk = block_chunk_descs(src_ptrs, dst_ptrs, chunks_per_block, sd);
    const uint8_t* s = reinterpret_cast<const uint8_t*>(sd[0]);
    uint8_t* d = reinterpret_cast<uint8_t*>(sd[1]);
    uint64_t stride = static_cast<uint64_t>(chunks_per_block) * blockDim.x;
    for (uint64_t u = static_cast<uint64_t>(chunk) * blockDim.x + threadIdx.x;
         u < bytes_per_block; u += stride)
        d[u] = s[u];
}

// Enough workgroups to fill 256 CUs across 8 XCDs with headroom, but ONE
// descriptor read per workgroup.
static uint32_t copy_chunks_per_block(uint64_t units_per_block, uint64_t n_blocks, int threads) {
    uint64_t max_chunks = (units_per_block + threads - 1) / static_cast<uint64_t>(threads);
    uint64_t want = (4096 + n_blocks - 1) / n_blocks;
    uint64_t c = std::min<uint64_t>(std::max<uint64_t>(want, 1), max_chunks);
    return static_cast<uint32_t>(std::max<uint64_t>(c, 1));
}

// --- segmented pages ---------------------------------------------------------
// The client side of a page is n_segments pieces a fixed stride apart; the
// pool side is their concatenation (docs/design.md, "segmented pages"). The
// 2D mapping above becomes (block, segment, chunk): a workgroup decodes its
// triple ONCE from blockIdx.x, reads block b's descriptor pair once through
// LDS exactly as block_chunk_descs does, and moves both base pointers to its
// segment; the unit loop that follows is the contiguous kernels' loop over
// one segment, with no per-unit division. src_stride / dst_stride are the
// byte distances between a page's segments on either side: the client's
// stride on the segmented side, the segment's own (stored) size on the pool
// side, so the direction costs no branch.
__device__ __forceinline__ uint32_t block_seg_chunk_descs(const uint64_t* __restrict__ src_ptrs,
                                                          const uint64_t* __restrict__ dst_ptrs,
                                                          uint32_t n_segments,
                                                          uint32_t chunks_per_seg,
                                                          uint64_t (&sd)[2], uint32_t* seg) {
    uint32_t per_block = n_segments * chunks_per_seg;
    uint32_t b = blockIdx.x / per_block;
    uint32_t r = blockIdx.x - b * per_block;
    uint32_t s = r / chunks_per_seg;
    uint32_t chunk = r - s * chunks_per_seg;
    __shared__ uint64_t lds[2];
    if (threadIdx.x == 0) {
        lds[0] = src_ptrs[b];
        lds[1] = dst_ptrs[b];
    }
    __syncthreads();
    sd[0] = lds[0];
    sd[1] = lds[1];
    *seg = s;
    return chunk;
}

__global__ void copy_blocks_vec_seg_kernel(const uint64_t* __restrict__ src_ptrs,
                                           const uint64_t* __restrict__ dst_ptrs,
                                           uint32_t n_segments, uint32_t chunks_per_seg,
                                           uint64_t units_per_seg, uint64_t src_stride,
                                           uint64_t dst_stride) {
    uint64_t sd[2];
    uint32_t seg;
    uint32_t chunk =
        block_seg_chunk_descs(src_ptrs, dst_ptrs, n_segments, chunks_per_seg, sd, &seg);
    const uint4* s = reinterpret_cast<const uint4*>(sd[0] + seg * src_stride);
    uint4* d = reinterpret_cast<uint4*>(sd[1] + seg * dst_stride);
    uint64_t stride = static_cast<uint64_t>(chunks_per_seg) * blockDim.x;
    for (uint64_t u = static_cast<uint64_t>(chunk) * blockDim.x + threadIdx.x;
         u < units_per_seg; u += stride)
        d[u] = s[u];
}

__global__ void copy_blocks_byte_seg_kernel(const uint64_t* __restrict__ src_ptrs,
                                            const uint64_t* __restrict__ dst_ptrs,
                                            uint32_t n_segments, uint32_t chunks_per_seg,
                                            uint64_t bytes_per_seg, uint64_t src_stride,
                                            uint64_t dst_stride) {
    uint64_t sd[2];
    uint32_t seg;
    uint32_t chunk =
        block_seg_chunk_descs(src_ptrs, dst_ptrs, n_segments, chunks_per_seg, sd, &seg);
    const uint8_t* s = reinterpret_cast<const uint8_t*>(sd[0] + seg * src_stride);
    uint8_t* d = reinterpret_cast<uint8_t*>(sd[1] + seg * dst_stride);
    uint64_t stride = static_cast<uint64_t>(chunks_per_seg) * blockDim.x;
    for (uint64_t u = static_cast<uint64_t>(chunk) * blockDim.x + threadIdx.x;
         u < bytes_per_seg; u += stride)
        d[u] = s[u];
}

// Grid of a (block, segment, chunk) launch: chunks per segment chosen so that
// n_blocks * S * chunks meets the same ~4096-workgroup target as the
// contiguous kernels. False when the grid would not fit (never with at most
// kMaxPageSegments segments and a slot's worth of descriptors).
static bool seg_grid(uint64_t units_per_seg, int n_blocks, uint32_t n_segments, int threads,
                     uint32_t* chunks, uint32_t* grid) {
    uint64_t rows = static_cast<uint64_t>(n_blocks) * n_segments;
    *chunks = copy_chunks_per_block(units_per_seg, rows, threads);
    uint64_t g = rows * *chunks;
    if (g > 0x7fffffffull) return false;
    *grid = static_cast<uint32_t>(g);
    return true;
}

bool launch_copy_blocks(int dev, Stream stream, const uint64_t* dev_src_ptrs,
                        const uint64_t* dev_dst_ptrs, int n_blocks, size_t bytes_per_block,
                        bool aligned16, PageSegments seg, PageDir dir) {
    if (n_blocks <= 0 || bytes_per_block == 0) return true;
    if (!segments_legal(PageCodec::kNone, bytes_per_block, seg.n, seg.stride_bytes)) {
        snprintf(g_err, sizeof(g_err), "launch_copy_blocks: illegal page segments");
        return false;
    }
    HIP_OK(hipSetDevice(dev));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // threads=512 measured fastest for the grid-stride uint4 copy on gfx950
    // (90.7 us vs 93.4 us at 256 for 2048x128 KB; scripts/copybench.hip —
    // also faster than hipMemcpy D2D at 98.2 us).
    const int threads = 512;
    if (seg.n > 1) {
        const uint64_t seg_bytes = bytes_per_block / seg.n;
        const bool store = dir == PageDir::kStore;
        const uint64_t src_stride = store ? seg.stride_bytes : seg_bytes;
        const uint64_t dst_stride = store ? seg_bytes : seg.stride_bytes;
        const bool vec = aligned16 && seg_bytes % 16 == 0 && seg.stride_bytes % 16 == 0;
        const uint64_t units = vec ? seg_bytes / 16 : seg_bytes;
        uint32_t chunks, grid;
        if (!seg_grid(units, n_blocks, seg.n, threads, &chunks, &grid)) return false;
        if (vec)
            hipLaunchKernelGGL(copy_blocks_vec_seg_kernel, dim3(grid), dim3(threads), 0, s,
                               dev_src_ptrs, dev_dst_ptrs, seg.n, chunks, units, src_stride,
                               dst_stride);
        else
            hipLaunchKernelGGL(copy_blocks_byte_seg_kernel, dim3(grid), dim3(threads), 0, s,
                               dev_src_ptrs, dev_dst_ptrs, seg.n, chunks, units, src_stride,
                               dst_stride);
        HIP_OK(hipGetLastError());
        return true;
    }
    if (aligned16 && bytes_per_block % 16 == 0) {
        uint64_t upb = bytes_per_block / 16;
        uint32_t chunks = copy_chunks_per_block(upb, n_blocks, threads);
        dim3 grid(static_cast<uint32_t>(n_blocks) * chunks);
        hipLaunchKernelGGL(copy_blocks_vec_kernel, grid, dim3(threads), 0, s, dev_src_ptrs,
                           dev_dst_ptrs, chunks, upb);
    } else {
        uint32_t chunks = copy_chunks_per_block(bytes_per_block, n_blocks, threads);
        dim3 grid(static_cast<uint32_t>(n_blocks) * chunks);
        hipLaunchKernelGGL(copy_blocks_byte_kernel, grid, dim3(threads), 0, s, dev_src_ptrs,
                           dev_dst_ptrs, chunks, bytes_per_block);
    }
    HIP_OK(hipGetLastError());
    return true;
}

// --- fp8 KV-cache compression ----------------------------------------------
// MI355X-native extension (no reference equivalent): pages enter the pool
// quantized bf16 -> OCP fp8 e4m3fn with ONE scale per page (finite
// absmax/448), halving HBM footprint per cached page; reads dequantize
// back to bf16 on the way out. Both kernels are memory-bound streaming
// passes: one 512-thread workgroup per page, vectorized 8-elems-per-lane.
// The scalar codec lives in fp8_codec.h (shared with the host, where it is
// tested exhaustively): integer bit math, round-to-nearest-even in the
// normal AND subnormal range, so stored codes equal
// torch.clamp(x/scale, -448, 448).to(torch.float8_e4m3fn) bit for bit; NaN
// keeps the format's NaN code, +-inf saturates to +-448 and neither takes
// part in the scale (docs/design.md, "fp8 page codec").
// Both kernels issue 16-byte accesses on the bf16 side and 8-byte accesses
// on the fp8 side: callers guarantee 16-byte-aligned block pointers.

// One workgroup per page. Pass 1: workgroup absmax over the finite elements
// (wavefront shuffle reduce + LDS). Pass 2: scale + convert, 8 bf16 in (one
// uint4) -> 8 fp8 out (one uint2) per lane per iteration.
__global__ void quant_blocks_bf16_fp8_kernel(const uint64_t* __restrict__ src_ptrs,
                                             const uint64_t* __restrict__ dst_ptrs,
                                             float* __restrict__ scales,
                                             uint64_t elems_per_block) {
    const uint16_t* src = reinterpret_cast<const uint16_t*>(src_ptrs[blockIdx.x]);
    uint8_t* dst = reinterpret_cast<uint8_t*>(dst_ptrs[blockIdx.x]);
    __shared__ uint32_t red[8];  // 512 threads / 64-wide wavefronts
    __shared__ float scale_sh;
    uint32_t m = 0;  // largest finite bf16 magnitude, as bits
    uint64_t n8 = elems_per_block / 8;
    const uint4* src4 = reinterpret_cast<const uint4*>(src);
    for (uint64_t u = threadIdx.x; u < n8; u += blockDim.x) {
        uint4 pk = src4[u];
        const uint16_t* h = reinterpret_cast<const uint16_t*>(&pk);
#pragma unroll
        for (int i = 0; i < 8; i++) m = fp8::absmax_step(m, h[i]);
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
    float inv = 1.f / scale_sh;
    for (uint64_t u = threadIdx.x; u < n8; u += blockDim.x) {
        uint4 pk = src4[u];
        const uint16_t* h = reinterpret_cast<const uint16_t*>(&pk);
        uint8_t out[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            float f = fp8::bits_f32(static_cast<uint32_t>(h[i]) << 16);
            out[i] = fp8::f32_to_e4m3(f * inv);
        }
        reinterpret_cast<uint2*>(dst)[u] = *reinterpret_cast<const uint2*>(out);
    }
}

// Dequantize fp8 pages back into bf16 client memory (value * scale in fp32,
// round-to-nearest-even to bf16): 8 fp8 in (uint2) -> 8 bf16 out (uint4)
// per lane.
__global__ void dequant_blocks_fp8_bf16_kernel(const uint64_t* __restrict__ src_ptrs,
                                               const uint64_t* __restrict__ dst_ptrs,
                                               const float* __restrict__ scales,
                                               uint64_t elems_per_block) {
    const uint8_t* src = reinterpret_cast<const uint8_t*>(src_ptrs[blockIdx.x]);
    uint16_t* dst = reinterpret_cast<uint16_t*>(dst_ptrs[blockIdx.x]);
    float scale = scales[blockIdx.x];
    uint64_t n8 = elems_per_block / 8;
    for (uint64_t u = threadIdx.x; u < n8; u += blockDim.x) {
        uint2 pk = reinterpret_cast<const uint2*>(src)[u];
        const uint8_t* b = reinterpret_cast<const uint8_t*>(&pk);
        uint16_t out[8];
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = fp8::decode_to_bf16(b[i], scale);
        reinterpret_cast<uint4*>(dst)[u] = *reinterpret_cast<const uint4*>(out);
    }
}

// --- mxfp4 KV-cache compression ---------------------------------------------
// bf16 pages <-> OCP microscaling FP4: e2m1 codes, two per byte, followed by
// one e8m0 scale byte per group of 32 elements (block layout and rules:
// docs/design.md, "mxfp4 page codec"; scalar codec: mxfp4_codec.h). A scale
// covers 32 neighbouring elements only, so there is no page-wide reduction
// and each kernel is ONE streaming pass that touches every byte once. Four
// lanes share a group: on the bf16 side a lane moves one uint4 (8 elements),
// so a wave's accesses stay fully coalesced 16-byte ones; on the stored side
// it moves the 4 bytes holding its 8 codes. Work is laid out like the copy
// kernel's: workgroup (b, chunk), descriptor read once through LDS, so a
// request of few pages still fills the device.
// elems_per_block % 32 == 0 makes the lane-unit count a multiple of 4, and
// chunk * blockDim.x and the stride are multiples of 4 too: the four lanes of
// a quad always run the loop body together, and the cross-lane steps below
// only ever read lanes of the own quad.
constexpr int kMxfp4Threads = 4 * kMxfp4GroupsPerIter;

__global__ void quant_blocks_bf16_mxfp4_kernel(const uint64_t* __restrict__ src_ptrs,
                                               const uint64_t* __restrict__ dst_ptrs,
                                               uint32_t chunks_per_block,
                                               uint64_t elems_per_block) {
    uint64_t sd[2];
    uint32_t chunk = block_chunk_descs(src_ptrs, dst_ptrs, chunks_per_block, sd);
    const uint4* src4 = reinterpret_cast<const uint4*>(sd[0]);
    uint32_t* codes = reinterpret_cast<uint32_t*>(sd[1]);
    uint8_t* scales = reinterpret_cast<uint8_t*>(sd[1]) + elems_per_block / 2;
    uint64_t n8 = elems_per_block / 8;
    uint64_t stride = static_cast<uint64_t>(chunks_per_block) * blockDim.x;
    for (uint64_t u = static_cast<uint64_t>(chunk) * blockDim.x + threadIdx.x; u < n8;
         u += stride) {
        uint4 pk = src4[u];
        const uint16_t* h = reinterpret_cast<const uint16_t*>(&pk);
        uint32_t key = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) key = mxfp4::key_step(key, h[i]);
        key = max(key, __shfl_xor(key, 1, 64));
        key = max(key, __shfl_xor(key, 2, 64));
        uint8_t E = mxfp4::group_exponent(key);
        uint32_t out = 0;
#pragma unroll
        for (int i = 0; i < 8; i++)
            out |= static_cast<uint32_t>(mxfp4::encode(h[i], E)) << (4 * i);
        codes[u] = out;
        if ((u & 3u) == 0) scales[u >> 2] = E;
    }
}

__global__ void dequant_blocks_mxfp4_bf16_kernel(const uint64_t* __restrict__ src_ptrs,
                                                 const uint64_t* __restrict__ dst_ptrs,
                                                 uint32_t chunks_per_block,
                                                 uint64_t elems_per_block) {
    uint64_t sd[2];
    uint32_t chunk = block_chunk_descs(src_ptrs, dst_ptrs, chunks_per_block, sd);
    const uint32_t* codes = reinterpret_cast<const uint32_t*>(sd[0]);
    const uint8_t* scales = reinterpret_cast<const uint8_t*>(sd[0]) + elems_per_block / 2;
    uint4* dst4 = reinterpret_cast<uint4*>(sd[1]);
    uint64_t n8 = elems_per_block / 8;
    uint64_t stride = static_cast<uint64_t>(chunks_per_block) * blockDim.x;
    for (uint64_t u = static_cast<uint64_t>(chunk) * blockDim.x + threadIdx.x; u < n8;
         u += stride) {
        uint32_t pk = codes[u];
        uint8_t E = scales[u >> 2];  // the quad's four lanes read the same byte
        uint16_t out[8];
#pragma unroll
        for (int i = 0; i < 8; i++)
            out[i] = mxfp4::decode(static_cast<uint8_t>((pk >> (4 * i)) & 0xfu), E);
        dst4[u] = *reinterpret_cast<const uint4*>(out);
    }
}

// --- segmented forms of the four transforming kernels -------------------------
// The bf16 side is segmented (source of quantize, destination of dequantize);
// the stored block is byte-identical to the one the contiguous kernel makes
// of the concatenated page.

// fp8: still one 512-thread workgroup per page, because the scale is the
// PAGE's: pass 1 takes the absmax over every segment before pass 2 converts
// any. Segment loop outside, unit loop inside; seg_elems % 8 == 0.
__global__ void quant_blocks_bf16_fp8_seg_kernel(const uint64_t* __restrict__ src_ptrs,
                                                 const uint64_t* __restrict__ dst_ptrs,
                                                 float* __restrict__ scales,
                                                 uint32_t n_segments, uint64_t seg_elems,
                                                 uint64_t src_stride) {
    const uint64_t src = src_ptrs[blockIdx.x];
    uint2* dst = reinterpret_cast<uint2*>(dst_ptrs[blockIdx.x]);
    __shared__ uint32_t red[8];  // 512 threads / 64-wide wavefronts
    __shared__ float scale_sh;
    uint32_t m = 0;  // largest finite bf16 magnitude, as bits
    uint64_t n8 = seg_elems / 8;
    for (uint32_t sg = 0; sg < n_segments; sg++) {
        const uint4* src4 = reinterpret_cast<const uint4*>(src + sg * src_stride);
        for (uint64_t u = threadIdx.x; u < n8; u += blockDim.x) {
            uint4 pk = src4[u];
            const uint16_t* h = reinterpret_cast<const uint16_t*>(&pk);
#pragma unroll
            for (int i = 0; i < 8; i++) m = fp8::absmax_step(m, h[i]);
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
    float inv = 1.f / scale_sh;
    for (uint32_t sg = 0; sg < n_segments; sg++) {
        const uint4* src4 = reinterpret_cast<const uint4*>(src + sg * src_stride);
        uint2* dseg = dst + sg * n8;
        for (uint64_t u = threadIdx.x; u < n8; u += blockDim.x) {
            uint4 pk = src4[u];
            const uint16_t* h = reinterpret_cast<const uint16_t*>(&pk);
            uint8_t out[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                float f = fp8::bits_f32(static_cast<uint32_t>(h[i]) << 16);
                out[i] = fp8::f32_to_e4m3(f * inv);
            }
            dseg[u] = *reinterpret_cast<const uint2*>(out);
        }
    }
}

__global__ void dequant_blocks_fp8_bf16_seg_kernel(const uint64_t* __restrict__ src_ptrs,
                                                   const uint64_t* __restrict__ dst_ptrs,
                                                   const float* __restrict__ scales,
                                                   uint32_t n_segments, uint64_t seg_elems,
                                                   uint64_t dst_stride) {
    const uint2* src = reinterpret_cast<const uint2*>(src_ptrs[blockIdx.x]);
    const uint64_t dst = dst_ptrs[blockIdx.x];
    float scale = scales[blockIdx.x];
    uint64_t n8 = seg_elems / 8;
    for (uint32_t sg = 0; sg < n_segments; sg++) {
        const uint2* sseg = src + sg * n8;
        uint4* dst4 = reinterpret_cast<uint4*>(dst + sg * dst_stride);
        for (uint64_t u = threadIdx.x; u < n8; u += blockDim.x) {
            uint2 pk = sseg[u];
            const uint8_t* b = reinterpret_cast<const uint8_t*>(&pk);
            uint16_t out[8];
#pragma unroll
            for (int i = 0; i < 8; i++) out[i] = fp8::decode_to_bf16(b[i], scale);
            dst4[u] = *reinterpret_cast<const uint4*>(out);
        }
    }
}

// mxfp4: workgroup (b, s, chunk). The bf16 side is indexed by the segment's
// own unit u, the stored side by the page-global unit s * (seg_elems / 8) + u:
// codes at 4 * u_global, the scale byte at elems / 2 + (u_global >> 2).
// seg_elems % 32 == 0 makes seg_elems / 8 a multiple of 4, so u_global and u
// agree in their low two bits and the quad invariant written above
// kMxfp4Threads holds inside every segment.
__global__ void quant_blocks_bf16_mxfp4_seg_kernel(const uint64_t* __restrict__ src_ptrs,
                                                   const uint64_t* __restrict__ dst_ptrs,
                                                   uint32_t n_segments, uint32_t chunks_per_seg,
                                                   uint64_t seg_elems, uint64_t src_stride) {
    uint64_t sd[2];
    uint32_t seg;
    uint32_t chunk =
        block_seg_chunk_descs(src_ptrs, dst_ptrs, n_segments, chunks_per_seg, sd, &seg);
    uint64_t n8 = seg_elems / 8;
    const uint4* src4 = reinterpret_cast<const uint4*>(sd[0] + seg * src_stride);
    uint32_t* codes = reinterpret_cast<uint32_t*>(sd[1]) + seg * n8;
    uint8_t* scales =
        reinterpret_cast<uint8_t*>(sd[1]) + n_segments * seg_elems / 2 + seg * (n8 >> 2);
    uint64_t stride = static_cast<uint64_t>(chunks_per_seg) * blockDim.x;
    for (uint64_t u = static_cast<uint64_t>(chunk) * blockDim.x + threadIdx.x; u < n8;
         u += stride) {
        uint4 pk = src4[u];
        const uint16_t* h = reinterpret_cast<const uint16_t*>(&pk);
        uint32_t key = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) key = mxfp4::key_step(key, h[i]);
        key = max(key, __shfl_xor(key, 1, 64));
        key = max(key, __shfl_xor(key, 2, 64));
        uint8_t E = mxfp4::group_exponent(key);
        uint32_t out = 0;
#pragma unroll
        for (int i = 0; i < 8; i++)
            out |= static_cast<uint32_t>(mxfp4::encode(h[i], E)) << (4 * i);
        codes[u] = out;
        if ((u & 3u) == 0) scales[u >> 2] = E;
    }
}

__global__ void dequant_blocks_mxfp4_bf16_seg_kernel(const uint64_t* __restrict__ src_ptrs,
                                                     const uint64_t* __restrict__ dst_ptrs,
                                                     uint32_t n_segments,
                                                     uint32_t chunks_per_seg,
                                                     uint64_t seg_elems, uint64_t dst_stride) {
    uint64_t sd[2];
    uint32_t seg;
    uint32_t chunk =
        block_seg_chunk_descs(src_ptrs, dst_ptrs, n_segments, chunks_per_seg, sd, &seg);
    uint64_t n8 = seg_elems / 8;
    const uint32_t* codes = reinterpret_cast<const uint32_t*>(sd[0]) + seg * n8;
    const uint8_t* scales =
        reinterpret_cast<const uint8_t*>(sd[0]) + n_segments * seg_elems / 2 + seg * (n8 >> 2);
    uint4* dst4 = reinterpret_cast<uint4*>(sd[1] + seg * dst_stride);
    uint64_t stride = static_cast<uint64_t>(chunks_per_seg) * blockDim.x;
    for (uint64_t u = static_cast<uint64_t>(chunk) * blockDim.x + threadIdx.x; u < n8;
         u += stride) {
        uint32_t pk = codes[u];
        uint8_t E = scales[u >> 2];  // the quad's four lanes read the same byte
        uint16_t out[8];
#pragma unroll
        for (int i = 0; i < 8; i++)
            out[i] = mxfp4::decode(static_cast<uint8_t>((pk >> (4 * i)) & 0xfu), E);
        dst4[u] = *reinterpret_cast<const uint4*>(out);
    }
}

// Segmented requests of launch_transform_blocks (seg.n > 1, geometry legal).
static bool launch_transform_blocks_seg(int dev, hipStream_t s, PageCodec codec, bool store,
                                        const uint64_t* dev_src_ptrs,
                                        const uint64_t* dev_dst_ptrs, float* dev_scales,
                                        int n_blocks, size_t elems_per_block, PageSegments seg) {
    const uint64_t seg_elems = elems_per_block / seg.n;
    switch (codec) {
        case PageCodec::kFp8:
            HIP_OK(hipSetDevice(dev));
            if (store)
                hipLaunchKernelGGL(quant_blocks_bf16_fp8_seg_kernel, dim3(n_blocks), dim3(512),
                                   0, s, dev_src_ptrs, dev_dst_ptrs, dev_scales, seg.n,
                                   seg_elems, seg.stride_bytes);
            else
                hipLaunchKernelGGL(dequant_blocks_fp8_bf16_seg_kernel, dim3(n_blocks),
                                   dim3(512), 0, s, dev_src_ptrs, dev_dst_ptrs, dev_scales,
                                   seg.n, seg_elems, seg.stride_bytes);
            break;
        case PageCodec::kMxfp4: {
            uint32_t chunks, grid;
            if (!seg_grid(seg_elems / 8, n_blocks, seg.n, kMxfp4Threads, &chunks, &grid))
                return false;
            HIP_OK(hipSetDevice(dev));
            if (store)
                hipLaunchKernelGGL(quant_blocks_bf16_mxfp4_seg_kernel, dim3(grid),
                                   dim3(kMxfp4Threads), 0, s, dev_src_ptrs, dev_dst_ptrs, seg.n,
                                   chunks, seg_elems, seg.stride_bytes);
            else
                hipLaunchKernelGGL(dequant_blocks_mxfp4_bf16_seg_kernel, dim3(grid),
                                   dim3(kMxfp4Threads), 0, s, dev_src_ptrs, dev_dst_ptrs, seg.n,
                                   chunks, seg_elems, seg.stride_bytes);
            break;
        }
        default:
            return false;
    }
    HIP_OK(hipGetLastError());
    return true;
}

// The one entry for every transforming codec (gpu.h). A new codec is a kernel
// pair above and one case here.
bool launch_transform_blocks(int dev, Stream stream, PageCodec codec, PageDir dir,
                             const uint64_t* dev_src_ptrs, const uint64_t* dev_dst_ptrs,
                             float* dev_scales, int n_blocks, size_t elems_per_block,
                             PageSegments seg) {
    if (n_blocks <= 0) return true;
    if (!segments_legal(codec, elems_per_block * kPageElemBytes, seg.n, seg.stride_bytes)) {
        snprintf(g_err, sizeof(g_err), "launch_transform_blocks: illegal page segments");
        return false;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool store = dir == PageDir::kStore;
    if (seg.n > 1)
        return launch_transform_blocks_seg(dev, s, codec, store, dev_src_ptrs, dev_dst_ptrs,
                                           dev_scales, n_blocks, elems_per_block, seg);
    switch (codec) {
        case PageCodec::kFp8:
            if (elems_per_block % 8 != 0) return false;
            HIP_OK(hipSetDevice(dev));
            if (store)
                hipLaunchKernelGGL(quant_blocks_bf16_fp8_kernel, dim3(n_blocks), dim3(512), 0, s,
                                   dev_src_ptrs, dev_dst_ptrs, dev_scales, elems_per_block);
            else
                hipLaunchKernelGGL(dequant_blocks_fp8_bf16_kernel, dim3(n_blocks), dim3(512), 0,
                                   s, dev_src_ptrs, dev_dst_ptrs, dev_scales, elems_per_block);
            break;
        case PageCodec::kMxfp4: {
            if (elems_per_block == 0 || elems_per_block % mxfp4::kGroupElems != 0) return false;
            HIP_OK(hipSetDevice(dev));
            uint32_t chunks =
                copy_chunks_per_block(elems_per_block / 8, n_blocks, kMxfp4Threads);
            dim3 grid(static_cast<uint32_t>(n_blocks) * chunks);
            if (store)
                hipLaunchKernelGGL(quant_blocks_bf16_mxfp4_kernel, grid, dim3(kMxfp4Threads), 0,
                                   s, dev_src_ptrs, dev_dst_ptrs, chunks,
                                   static_cast<uint64_t>(elems_per_block));
            else
                hipLaunchKernelGGL(dequant_blocks_mxfp4_bf16_kernel, grid, dim3(kMxfp4Threads),
                                   0, s, dev_src_ptrs, dev_dst_ptrs, chunks,
                                   static_cast<uint64_t>(elems_per_block));
            break;
        }
        default:
            return false;
    }
    HIP_OK(hipGetLastError());
    return true;
}

// --- tensor sets ---------------------------------------------------------------
// The client side of a page spans n_tensors tensors (gpu.h, docs/design.md
// "tensor sets"): segment s of the page's S lies in tensor g = s / (S/G), at
// base[g] + offset + (s % (S/G)) * stride, the offset being the block's client
// descriptor. The mapping stays (block, segment, chunk) and the descriptor
// pair is read once through LDS by block_seg_chunk_descs; g is a function of
// blockIdx.x and kernel arguments alone, so base[g] is one scalar load per
// workgroup and the unit loops are the segmented kernels' loops.
//
// The table of bases rides in the KERNEL ARGUMENTS, not in the slot's pinned
// descriptor area. It is per request, not per block: 1 KiB that the launch
// copies into the kernarg segment, which the device reads through the scalar
// cache with a workgroup-uniform index, so no lane ever indexes it and nothing
// spills to scratch. In the pinned area every workgroup would fetch its base
// over PCIe (one more dependent host read before the first payload load, on
// top of the descriptor pair), the slot layout would change for every job, and
// fan-out sub-jobs on other streams would each stage their own copy. A kernel
// argument also ends the table's lifetime question: it is copied at launch.
struct TensorBases {
    uint64_t base[kMaxPageTensors];
};

__global__ void copy_blocks_vec_tset_kernel(const uint64_t* __restrict__ src_ptrs,
                                            const uint64_t* __restrict__ dst_ptrs,
                                            uint32_t n_segments, uint32_t segs_per_tensor,
                                            uint32_t chunks_per_seg, uint32_t to_pool,
                                            uint64_t units_per_seg, uint64_t stride,
                                            TensorBases tb) {
    uint64_t sd[2];
    uint32_t seg;
    uint32_t chunk =
        block_seg_chunk_descs(src_ptrs, dst_ptrs, n_segments, chunks_per_seg, sd, &seg);
    uint32_t g = seg / segs_per_tensor;
    uint32_t r = seg - g * segs_per_tensor;
    uint64_t client = tb.base[g] + r * stride;
    uint64_t pool = seg * (units_per_seg * 16);
    const uint4* s = reinterpret_cast<const uint4*>(sd[0] + (to_pool ? client : pool));
    uint4* d = reinterpret_cast<uint4*>(sd[1] + (to_pool ? pool : client));
    uint64_t step = static_cast<uint64_t>(chunks_per_seg) * blockDim.x;
    for (uint64_t u = static_cast<uint64_t>(chunk) * blockDim.x + threadIdx.x;
         u < units_per_seg; u += step)
        d[u] = s[u];
}

__global__ void copy_blocks_byte_tset_kernel(const uint64_t* __restrict__ src_ptrs,
                                             const uint64_t* __restrict__ dst_ptrs,
                                             uint32_t n_segments, uint32_t segs_per_tensor,
                                             uint32_t chunks_per_seg, uint32_t to_pool,
                                             uint64_t bytes_per_seg, uint64_t stride,
                                             TensorBases tb) {
    uint64_t sd[2];
    uint32_t seg;
    uint32_t chunk =
        block_seg_chunk_descs(src_ptrs, dst_ptrs, n_segments, chunks_per_seg, sd, &seg);
    uint32_t g = seg / segs_per_tensor;
    uint32_t r = seg - g * segs_per_tensor;
    uint64_t client = tb.base[g] + r * stride;
    uint64_t pool = seg * bytes_per_seg;
    const uint8_t* s = reinterpret_cast<const uint8_t*>(sd[0] + (to_pool ? client : pool));
    uint8_t* d = reinterpret_cast<uint8_t*>(sd[1] + (to_pool ? pool : client));
    uint64_t step = static_cast<uint64_t>(chunks_per_seg) * blockDim.x;
    for (uint64_t u = static_cast<uint64_t>(chunk) * blockDim.x + threadIdx.x;
         u < bytes_per_seg; u += step)
        d[u] = s[u];
}

// fp8: one 512-thread workgroup per page over ALL tensors, because the scale
// is the page's: pass 1 takes the absmax over every tensor's part before pass
// 2 converts any. Tensor loop outside (one scalar load of base[g] each), then
// the segmented kernel's segment and unit loops.
__global__ void quant_blocks_bf16_fp8_tset_kernel(const uint64_t* __restrict__ src_offs,
                                                  const uint64_t* __restrict__ dst_ptrs,
                                                  float* __restrict__ scales,
                                                  uint32_t n_tensors, uint32_t segs_per_tensor,
                                                  uint64_t seg_elems, uint64_t src_stride,
                                                  TensorBases tb) {
    const uint64_t off = src_offs[blockIdx.x];
    uint2* dst = reinterpret_cast<uint2*>(dst_ptrs[blockIdx.x]);
    __shared__ uint32_t red[8];  // 512 threads / 64-wide wavefronts
    __shared__ float scale_sh;
    uint32_t m = 0;  // largest finite bf16 magnitude, as bits
    uint64_t n8 = seg_elems / 8;
    for (uint32_t g = 0; g < n_tensors; g++) {
        const uint64_t src = tb.base[g] + off;
        for (uint32_t sg = 0; sg < segs_per_tensor; sg++) {
            const uint4* src4 = reinterpret_cast<const uint4*>(src + sg * src_stride);
            for (uint64_t u = threadIdx.x; u < n8; u += blockDim.x) {
                uint4 pk = src4[u];
                const uint16_t* h = reinterpret_cast<const uint16_t*>(&pk);
#pragma unroll
                for (int i = 0; i < 8; i++) m = fp8::absmax_step(m, h[i]);
            }
        }
    }
    for (int o = 32; o; o >>= 1) m = max(m, __shfl_down(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t mm = red[0];
        for (int w = 1; w < static_cast<int>(blockDim.x) / 64; w++) mm = max(mm, red[w]);
        scale_sh = fp8::scale_from_absmax_bits(mm);
        scales[blockIdx.x] = scale_sh;
    }
    __syncthreads();
    float inv = 1.f / scale_sh;
    for (uint32_t g = 0; g < n_tensors; g++) {
        const uint64_t src = tb.base[g] + off;
        for (uint32_t sg = 0; sg < segs_per_tensor; sg++) {
            const uint4* src4 = reinterpret_cast<const uint4*>(src + sg * src_stride);
            uint2* dseg = dst + (static_cast<uint64_t>(g) * segs_per_tensor + sg) * n8;
            for (uint64_t u = threadIdx.x; u < n8; u += blockDim.x) {
                uint4 pk = src4[u];
                const uint16_t* h = reinterpret_cast<const uint16_t*>(&pk);
                uint8_t out[8];
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    float f = fp8::bits_f32(static_cast<uint32_t>(h[i]) << 16);
                    out[i] = fp8::f32_to_e4m3(f * inv);
                }
                dseg[u] = *reinterpret_cast<const uint2*>(out);
            }
        }
    }
}

__global__ void dequant_blocks_fp8_bf16_tset_kernel(const uint64_t* __restrict__ src_ptrs,
                                                    const uint64_t* __restrict__ dst_offs,
                                                    const float* __restrict__ scales,
                                                    uint32_t n_tensors, uint32_t segs_per_tensor,
                                                    uint64_t seg_elems, uint64_t dst_stride,
                                                    TensorBases tb) {
    const uint2* src = reinterpret_cast<const uint2*>(src_ptrs[blockIdx.x]);
    const uint64_t off = dst_offs[blockIdx.x];
    float scale = scales[blockIdx.x];
    uint64_t n8 = seg_elems / 8;
    for (uint32_t g = 0; g < n_tensors; g++) {
        const uint64_t dst = tb.base[g] + off;
        for (uint32_t sg = 0; sg < segs_per_tensor; sg++) {
            const uint2* sseg = src + (static_cast<uint64_t>(g) * segs_per_tensor + sg) * n8;
            uint4* dst4 = reinterpret_cast<uint4*>(dst + sg * dst_stride);
            for (uint64_t u = threadIdx.x; u < n8; u += blockDim.x) {
                uint2 pk = sseg[u];
                const uint8_t* b = reinterpret_cast<const uint8_t*>(&pk);
                uint16_t out[8];
#pragma unroll
                for (int i = 0; i < 8; i++) out[i] = fp8::decode_to_bf16(b[i], scale);
                dst4[u] = *reinterpret_cast<const uint4*>(out);
            }
        }
    }
}

// mxfp4: workgroup (b, s, chunk) as in the segmented kernels; the stored side
// is indexed by the page-global unit s * (seg_elems / 8) + u with s counted
// over ALL tensors, so later tensors' codes and scale bytes land where the
// contiguous kernel puts them. The quad invariant holds inside every segment
// as it does there (seg_elems % 32 == 0).
__global__ void quant_blocks_bf16_mxfp4_tset_kernel(const uint64_t* __restrict__ src_offs,
                                                    const uint64_t* __restrict__ dst_ptrs,
                                                    uint32_t n_segments,
                                                    uint32_t segs_per_tensor,
                                                    uint32_t chunks_per_seg, uint64_t seg_elems,
                                                    uint64_t src_stride, TensorBases tb) {
    uint64_t sd[2];
    uint32_t seg;
    uint32_t chunk =
        block_seg_chunk_descs(src_offs, dst_ptrs, n_segments, chunks_per_seg, sd, &seg);
    uint32_t g = seg / segs_per_tensor;
    uint32_t r = seg - g * segs_per_tensor;
    uint64_t n8 = seg_elems / 8;
    const uint4* src4 = reinterpret_cast<const uint4*>(tb.base[g] + sd[0] + r * src_stride);
    uint32_t* codes = reinterpret_cast<uint32_t*>(sd[1]) + seg * n8;
    uint8_t* scales =
        reinterpret_cast<uint8_t*>(sd[1]) + n_segments * seg_elems / 2 + seg * (n8 >> 2);
    uint64_t step = static_cast<uint64_t>(chunks_per_seg) * blockDim.x;
    for (uint64_t u = static_cast<uint64_t>(chunk) * blockDim.x + threadIdx.x; u < n8;
         u += step) {
        uint4 pk = src4[u];
        const uint16_t* h = reinterpret_cast<const uint16_t*>(&pk);
        uint32_t key = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) key = mxfp4::key_step(key, h[i]);
        key = max(key, __shfl_xor(key, 1, 64));
        key = max(key, __shfl_xor(key, 2, 64));
        uint8_t E = mxfp4::group_exponent(key);
        uint32_t out = 0;
#pragma unroll
        for (int i = 0; i < 8; i++)
            out |= static_cast<uint32_t>(mxfp4::encode(h[i], E)) << (4 * i);
        codes[u] = out;
        if ((u & 3u) == 0) scales[u >> 2] = E;
    }
}

__global__ void dequant_blocks_mxfp4_bf16_tset_kernel(const uint64_t* __restrict__ src_ptrs,
                                                      const uint64_t* __restrict__ dst_offs,
                                                      uint32_t n_segments,
                                                      uint32_t segs_per_tensor,
                                                      uint32_t chunks_per_seg,
                                                      uint64_t seg_elems, uint64_t dst_stride,
                                                      TensorBases tb) {
    uint64_t sd[2];
    uint32_t seg;
    uint32_t chunk =
        block_seg_chunk_descs(src_ptrs, dst_offs, n_segments, chunks_per_seg, sd, &seg);
    uint32_t g = seg / segs_per_tensor;
    uint32_t r = seg - g * segs_per_tensor;
    uint64_t n8 = seg_elems / 8;
    const uint32_t* codes = reinterpret_cast<const uint32_t*>(sd[0]) + seg * n8;
    const uint8_t* scales =
        reinterpret_cast<const uint8_t*>(sd[0]) + n_segments * seg_elems / 2 + seg * (n8 >> 2);
    uint4* dst4 = reinterpret_cast<uint4*>(tb.base[g] + sd[1] + r * dst_stride);
    uint64_t step = static_cast<uint64_t>(chunks_per_seg) * blockDim.x;
    for (uint64_t u = static_cast<uint64_t>(chunk) * blockDim.x + threadIdx.x; u < n8;
         u += step) {
        uint32_t pk = codes[u];
        uint8_t E = scales[u >> 2];  // the quad's four lanes read the same byte
        uint16_t out[8];
#pragma unroll
        for (int i = 0; i < 8; i++)
            out[i] = mxfp4::decode(static_cast<uint8_t>((pk >> (4 * i)) & 0xfu), E);
        dst4[u] = *reinterpret_cast<const uint4*>(out);
    }
}

// What both tensor-set launchers check and build first: the geometry, the
// table itself, and whether every base keeps 16-byte alignment.
static bool tset_table(const char* what, PageCodec codec, size_t page_bytes, PageSegments seg,
                       TensorTable tset, TensorBases* tb, bool* bases16) {
    if (!tensors_legal(codec, page_bytes, seg.n, seg.stride_bytes, tset.n) || !tset.bases) {
        snprintf(g_err, sizeof(g_err), "%s: illegal tensor set geometry", what);
        return false;
    }
    *bases16 = true;
    memset(tb, 0, sizeof(*tb));
    for (uint32_t g = 0; g < tset.n; g++) {
        tb->base[g] = tset.bases[g];
        if (tset.bases[g] % 16 != 0) *bases16 = false;
    }
    return true;
}

bool launch_copy_blocks_tset(int dev, Stream stream, const uint64_t* dev_src,
                             const uint64_t* dev_dst, int n_blocks, size_t bytes_per_block,
                             bool aligned16, PageSegments seg, PageDir dir, TensorTable tset) {
    TensorBases tb;
    bool bases16;
    if (!tset_table("launch_copy_blocks_tset", PageCodec::kNone, bytes_per_block, seg, tset,
                    &tb, &bases16))
        return false;
    if (n_blocks <= 0 || bytes_per_block == 0) return true;
    const uint32_t per_tensor = seg.n / tset.n;
    const uint64_t stride = per_tensor > 1 ? seg.stride_bytes : 0;
    const uint64_t seg_bytes = bytes_per_block / seg.n;
    const bool vec = aligned16 && bases16 && seg_bytes % 16 == 0 && stride % 16 == 0;
    const uint64_t units = vec ? seg_bytes / 16 : seg_bytes;
    const int threads = 512;  // as launch_copy_blocks
    uint32_t chunks, grid;
    if (!seg_grid(units, n_blocks, seg.n, threads, &chunks, &grid)) {
        snprintf(g_err, sizeof(g_err), "launch_copy_blocks_tset: grid does not fit");
        return false;
    }
    HIP_OK(hipSetDevice(dev));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t to_pool = dir == PageDir::kStore;
    if (vec)
        hipLaunchKernelGGL(copy_blocks_vec_tset_kernel, dim3(grid), dim3(threads), 0, s, dev_src,
                           dev_dst, seg.n, per_tensor, chunks, to_pool, units, stride, tb);
    else
        hipLaunchKernelGGL(copy_blocks_byte_tset_kernel, dim3(grid), dim3(threads), 0, s,
                           dev_src, dev_dst, seg.n, per_tensor, chunks, to_pool, units, stride,
                           tb);
    HIP_OK(hipGetLastError());
    return true;
}

bool launch_transform_blocks_tset(int dev, Stream stream, PageCodec codec, PageDir dir,
                                  const uint64_t* dev_src, const uint64_t* dev_dst,
                                  float* dev_scales, int n_blocks, size_t elems_per_block,
                                  bool aligned16, PageSegments seg, TensorTable tset) {
    const char* what = "launch_transform_blocks_tset";
    TensorBases tb;
    bool bases16;
    if (!page_codec_transforms(codec) || elems_per_block == 0 ||
        !page_legal(codec, elems_per_block * kPageElemBytes)) {
        snprintf(g_err, sizeof(g_err), "%s: not a page of a transforming codec", what);
        return false;
    }
    if (!tset_table(what, codec, elems_per_block * kPageElemBytes, seg, tset, &tb, &bases16))
        return false;
    if (!aligned16 || !bases16) {
        snprintf(g_err, sizeof(g_err), "%s: %s needs 16-byte-aligned bases and offsets", what,
                 page_codec_info(codec).name);
        return false;
    }
    if (page_codec_info(codec).page_scale && !dev_scales) return false;
    if (n_blocks <= 0) return true;
    const uint32_t per_tensor = seg.n / tset.n;
    const uint64_t stride = per_tensor > 1 ? seg.stride_bytes : 0;
    const uint64_t seg_elems = elems_per_block / seg.n;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool store = dir == PageDir::kStore;
    switch (codec) {
        case PageCodec::kFp8:
            HIP_OK(hipSetDevice(dev));
            if (store)
                hipLaunchKernelGGL(quant_blocks_bf16_fp8_tset_kernel, dim3(n_blocks), dim3(512),
                                   0, s, dev_src, dev_dst, dev_scales, tset.n, per_tensor,
                                   seg_elems, stride, tb);
            else
                hipLaunchKernelGGL(dequant_blocks_fp8_bf16_tset_kernel, dim3(n_blocks),
                                   dim3(512), 0, s, dev_src, dev_dst, dev_scales, tset.n,
                                   per_tensor, seg_elems, stride, tb);
            break;
        case PageCodec::kMxfp4: {
            uint32_t chunks, grid;
            if (!seg_grid(seg_elems / 8, n_blocks, seg.n, kMxfp4Threads, &chunks, &grid)) {
                snprintf(g_err, sizeof(g_err), "%s: grid does not fit", what);
                return false;
            }
            HIP_OK(hipSetDevice(dev));
            if (store)
                hipLaunchKernelGGL(quant_blocks_bf16_mxfp4_tset_kernel, dim3(grid),
                                   dim3(kMxfp4Threads), 0, s, dev_src, dev_dst, seg.n,
                                   per_tensor, chunks, seg_elems, stride, tb);
            else
                hipLaunchKernelGGL(dequant_blocks_mxfp4_bf16_tset_kernel, dim3(grid),
                                   dim3(kMxfp4Threads), 0, s, dev_src, dev_dst, seg.n,
                                   per_tensor, chunks, seg_elems, stride, tb);
            break;
        }
        default:
            return false;
    }
    HIP_OK(hipGetLastError());
    return true;
}

// --- sliced reads --------------------------------------------------------------
// From each stored block take n_pieces pieces, piece p at LOGICAL byte
// offset + p * stride of the written page, and write their concatenation into
// the client page (gpu.h, docs/design.md "sliced reads"). Real pieces are
// small (one head group: 256 B to 2 KiB), so a workgroup per piece would idle
// most of its lanes. Instead L, the smallest power of two >= units per piece
// (capped at the workgroup), lanes share a piece and a workgroup covers
// blockDim.x / L pieces per step: threadIdx.x >> lane_shift picks the piece of
// the step, threadIdx.x & (L - 1) the unit lane, which strides by L inside the
// piece. Everything in the unit loop is a shift, a mask or an add. The
// workgroup is (block, chunk): chunk c of a block takes the steps c, c +
// chunks, ...; the chunk count meets the same ~4096-workgroup target as
// copy_chunks_per_block, and block b's descriptor pair is read once through
// LDS as in block_chunk_descs. Per piece, once: its logical byte inside the
// page (each kernel maps that to its stored address) and its client address
// dst + (p / pieces_per_seg) * seg_stride + (p % pieces_per_seg) * piece_bytes.
struct SliceArgs {
    uint32_t n_pieces;
    uint32_t chunks;          // workgroups per block
    uint32_t lane_shift;      // log2(L)
    uint32_t pieces_per_seg;  // n_pieces / client segments
    uint64_t units;           // per piece, in the kernel's unit
    uint64_t offset;          // logical bytes, as in PageSlice
    uint64_t stride;
    uint64_t piece_bytes;
    uint64_t seg_stride;      // client bytes from one segment to the next
    uint64_t page_bytes;      // logical size of the written page
};

// Walks the workgroup's pieces; move(b, src, logical_byte, client_addr, lane,
// L) runs one piece's unit loop (b for the per-block scale).
template <typename Move>
__device__ __forceinline__ void slice_for_each_piece(const uint64_t* __restrict__ src_ptrs,
                                                     const uint64_t* __restrict__ dst_ptrs,
                                                     const SliceArgs& a, Move move) {
    uint32_t b = blockIdx.x / a.chunks;
    uint32_t chunk = blockIdx.x - b * a.chunks;
    __shared__ uint64_t lds[2];
    if (threadIdx.x == 0) {
        lds[0] = src_ptrs[b];
        lds[1] = dst_ptrs[b];
    }
    __syncthreads();
    const uint64_t src = lds[0], dst = lds[1];
    const uint32_t L = 1u << a.lane_shift;
    const uint32_t per_step = blockDim.x >> a.lane_shift;
    const uint32_t lane = threadIdx.x & (L - 1);
    for (uint32_t p = chunk * per_step + (threadIdx.x >> a.lane_shift); p < a.n_pieces;
         p += a.chunks * per_step) {
        uint32_t sg = p / a.pieces_per_seg;
        uint32_t r = p - sg * a.pieces_per_seg;
        move(b, src, a.offset + p * a.stride, dst + sg * a.seg_stride + r * a.piece_bytes, lane,
             L);
    }
}

// plain: stored byte = logical byte. 16 bytes per lane; pointers, offset,
// piece, stride and client stride are all 16-byte multiples (the launcher
// picks the byte kernel otherwise).
__global__ void load_sliced_vec_kernel(const uint64_t* __restrict__ src_ptrs,
                                       const uint64_t* __restrict__ dst_ptrs, SliceArgs a) {
    slice_for_each_piece(src_ptrs, dst_ptrs, a,
                         [&](uint32_t, uint64_t src, uint64_t lbyte, uint64_t d, uint32_t lane,
                             uint32_t L) {
                             const uint4* s4 = reinterpret_cast<const uint4*>(src + lbyte);
                             uint4* d4 = reinterpret_cast<uint4*>(d);
                             for (uint64_t u = lane; u < a.units; u += L) d4[u] = s4[u];
                         });
}

__global__ void load_sliced_byte_kernel(const uint64_t* __restrict__ src_ptrs,
                                        const uint64_t* __restrict__ dst_ptrs, SliceArgs a) {
    slice_for_each_piece(src_ptrs, dst_ptrs, a,
                         [&](uint32_t, uint64_t src, uint64_t lbyte, uint64_t d, uint32_t lane,
                             uint32_t L) {
                             const uint8_t* s1 = reinterpret_cast<const uint8_t*>(src + lbyte);
                             uint8_t* d1 = reinterpret_cast<uint8_t*>(d);
                             for (uint64_t u = lane; u < a.units; u += L) d1[u] = s1[u];
                         });
}

// fp8: stored byte = logical ELEMENT index, so a piece's codes start at
// lbyte / 2: 8-byte aligned (offset and stride are multiples of 16 logical
// bytes), not 16. A lane loads 8 codes (uint2) and stores 8 bf16 (uint4). The
// block's one scale is scales[b]; nothing needs a page-wide pass, so the
// mapping is the copy's, not one workgroup per page.
__global__ void load_sliced_fp8_bf16_kernel(const uint64_t* __restrict__ src_ptrs,
                                            const uint64_t* __restrict__ dst_ptrs,
                                            const float* __restrict__ scales, SliceArgs a) {
    slice_for_each_piece(
        src_ptrs, dst_ptrs, a,
        [&](uint32_t b, uint64_t src, uint64_t lbyte, uint64_t d, uint32_t lane, uint32_t L) {
            const float scale = scales[b];
            const uint2* s2 = reinterpret_cast<const uint2*>(src + lbyte / kPageElemBytes);
            uint4* d4 = reinterpret_cast<uint4*>(d);
            for (uint64_t u = lane; u < a.units; u += L) {
                uint2 pk = s2[u];
                const uint8_t* c = reinterpret_cast<const uint8_t*>(&pk);
                uint16_t out[8];
#pragma unroll
                for (int i = 0; i < 8; i++) out[i] = fp8::decode_to_bf16(c[i], scale);
                d4[u] = *reinterpret_cast<const uint4*>(out);
            }
        });
}

// mxfp4: a lane's 8 codes are the 4 bytes at page-global unit
// g = lbyte / 16 + u, its scale byte sits behind all codes at
// page_elems / 2 + (g >> 2), page_elems being the WRITTEN page's. Decoding is
// lane-local: the quad shuffles exist only in the quantizer, so no quad of
// lanes has to run together here and any lane count per piece is fine. (A
// piece is whole 32-element groups, so u and g agree in their low two bits.)
__global__ void load_sliced_mxfp4_bf16_kernel(const uint64_t* __restrict__ src_ptrs,
                                              const uint64_t* __restrict__ dst_ptrs,
                                              SliceArgs a) {
    slice_for_each_piece(
        src_ptrs, dst_ptrs, a,
        [&](uint32_t, uint64_t src, uint64_t lbyte, uint64_t d, uint32_t lane, uint32_t L) {
            const uint64_t g0 = lbyte / 16;  // 8 elements of 2 bytes per unit
            const uint32_t* codes = reinterpret_cast<const uint32_t*>(src) + g0;
            const uint8_t* sc =
                reinterpret_cast<const uint8_t*>(src) + a.page_bytes / kPageElemBytes / 2;
            uint4* d4 = reinterpret_cast<uint4*>(d);
            for (uint64_t u = lane; u < a.units; u += L) {
                uint32_t pk = codes[u];
                uint8_t E = sc[(g0 + u) >> 2];
                uint16_t out[8];
#pragma unroll
                for (int i = 0; i < 8; i++)
                    out[i] = mxfp4::decode(static_cast<uint8_t>((pk >> (4 * i)) & 0xfu), E);
                d4[u] = *reinterpret_cast<const uint4*>(out);
            }
        });
}

bool launch_load_sliced(int dev, Stream stream, PageCodec codec, const uint64_t* dev_src_ptrs,
                        const uint64_t* dev_dst_ptrs, const float* dev_scales, int n_blocks,
                        PageSlice slice, PageSegments seg, bool aligned16) {
    if (n_blocks <= 0) return true;
    if (!slice_legal(codec, slice, seg)) {
        snprintf(g_err, sizeof(g_err), "launch_load_sliced: illegal page slice");
        return false;
    }
    const bool transforms = page_codec_transforms(codec);
    if (transforms && !aligned16) {
        snprintf(g_err, sizeof(g_err), "launch_load_sliced: %s needs 16-byte-aligned pointers",
                 page_codec_info(codec).name);
        return false;
    }
    if (page_codec_info(codec).page_scale && !dev_scales) return false;
    const bool many = slice.n > 1, segmented = seg.n > 1;
    // The transforming kernels' unit is 8 elements: 16 logical bytes.
    const bool vec = transforms ||
                     (aligned16 && slice.offset % 16 == 0 && slice.piece_bytes % 16 == 0 &&
                      (!many || slice.stride % 16 == 0) &&
                      (!segmented || seg.stride_bytes % 16 == 0));
    SliceArgs a;
    a.n_pieces = slice.n;
    a.units = vec ? slice.piece_bytes / 16 : slice.piece_bytes;
    a.lane_shift = 0;
    while ((1ull << a.lane_shift) < a.units && (1 << a.lane_shift) < kSliceThreads)
        a.lane_shift++;
    const uint32_t per_step = static_cast<uint32_t>(kSliceThreads) >> a.lane_shift;
    const uint64_t steps = (slice.n + per_step - 1) / per_step;
    a.chunks = copy_chunks_per_block(steps, n_blocks, 1);
    a.pieces_per_seg = slice.n / seg.n;
    a.offset = slice.offset;
    a.stride = many ? slice.stride : 0;
    a.piece_bytes = slice.piece_bytes;
    a.seg_stride = segmented ? seg.stride_bytes : 0;
    a.page_bytes = slice.page_bytes;
    const uint64_t g = static_cast<uint64_t>(n_blocks) * a.chunks;
    if (g > 0x7fffffffull) {
        snprintf(g_err, sizeof(g_err), "launch_load_sliced: grid does not fit");
        return false;
    }
    HIP_OK(hipSetDevice(dev));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(static_cast<uint32_t>(g)), block(kSliceThreads);
    switch (codec) {
        case PageCodec::kNone:
            if (vec)
                hipLaunchKernelGGL(load_sliced_vec_kernel, grid, block, 0, s, dev_src_ptrs,
                                   dev_dst_ptrs, a);
            else
                hipLaunchKernelGGL(load_sliced_byte_kernel, grid, block, 0, s, dev_src_ptrs,
                                   dev_dst_ptrs, a);
            break;
        case PageCodec::kFp8:
            hipLaunchKernelGGL(load_sliced_fp8_bf16_kernel, grid, block, 0, s, dev_src_ptrs,
                               dev_dst_ptrs, dev_scales, a);
            break;
        case PageCodec::kMxfp4:
            hipLaunchKernelGGL(load_sliced_mxfp4_bf16_kernel, grid, block, 0, s, dev_src_ptrs,
                               dev_dst_ptrs, a);
            break;
        default:
            return false;
    }
    HIP_OK(hipGetLastError());
    return true;
}

// --- fingerprint -----------------------------------------------------------
// Position-salted 64-bit mix (splitmix64 finalizer); XOR-combined across a
// block so the reduction is order-free, deterministic, and parallel.
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// One workgroup (256 threads) per KV block.
__global__ void hash_blocks_kernel(const uint64_t* __restrict__ ptrs, uint64_t bytes_per_block,
                                   uint64_t* __restrict__ out) {
    __shared__ uint64_t lds[256];
    int blk = blockIdx.x;
    const uint8_t* base = reinterpret_cast<const uint8_t*>(ptrs[blk]);
    uint64_t n_words = bytes_per_block / 8;
    uint64_t h = 0;
    // The fingerprint is defined over BYTES (little-endian 8-byte words), so
    // it must not depend on where the block starts. 8-byte loads need an
    // 8-byte-aligned base; any other base assembles each word from byte
    // loads. `base` comes from the descriptor, so the branch is uniform
    // across the workgroup.
    if ((reinterpret_cast<uint64_t>(base) & 7u) == 0) {
        const uint64_t* w = reinterpret_cast<const uint64_t*>(base);
        for (uint64_t i = threadIdx.x; i < n_words; i += blockDim.x)
            h ^= mix64(w[i] ^ (i * 0xff51afd7ed558ccdull));
    } else {
        for (uint64_t i = threadIdx.x; i < n_words; i += blockDim.x) {
            uint64_t word = 0;
#pragma unroll
            for (int k = 0; k < 8; k++)
                word |= static_cast<uint64_t>(base[i * 8 + k]) << (8 * k);
            h ^= mix64(word ^ (i * 0xff51afd7ed558ccdull));
        }
    }
    // Tail bytes (thread 0 only).
    if (threadIdx.x == 0) {
        uint64_t tail = 0;
        uint64_t tb = bytes_per_block - n_words * 8;
        for (uint64_t i = 0; i < tb; i++)
            tail |= static_cast<uint64_t>(base[n_words * 8 + i]) << (8 * i);
        if (tb) h ^= mix64(tail ^ (n_words * 0xff51afd7ed558ccdull));
    }
    lds[threadIdx.x] = h;
    __syncthreads();
    for (int s2 = blockDim.x / 2; s2 > 0; s2 >>= 1) {
        if (threadIdx.x < static_cast<unsigned>(s2)) lds[threadIdx.x] ^= lds[threadIdx.x + s2];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blk] = mix64(lds[0] ^ bytes_per_block);
}

bool launch_hash_blocks(int dev, Stream stream, const uint64_t* dev_ptrs, int n_blocks,
                        size_t bytes_per_block, uint64_t* dev_out_hashes) {
    if (n_blocks <= 0) return true;
    HIP_OK(hipSetDevice(dev));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(hash_blocks_kernel, dim3(n_blocks), dim3(256), 0, s, dev_ptrs,
                       bytes_per_block, dev_out_hashes);
    HIP_OK(hipGetLastError());
    return true;
}

}  // namespace gpu
}  // namespace ifs
