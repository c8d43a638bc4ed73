// HIP/ROCm layer for infinistore-amd (MI355X-native).
//
// Replaces the reference's CUDA-runtime call sites with an
// MI355X-first design: the pool lives in hipMalloc'd HBM3E, per-block
// hipMemcpyAsync loops are replaced by ONE batched gather/scatter HIP kernel
// launch per request (csrc/gpu/kernels.hip), and completion runs on pooled
// HIP streams with event FIFOs per shard.
//
// Everything here degrades gracefully when no GPU is present (CPU-only
// server mode, BASELINE config 1): `available()` is false and callers fall
// back to host arenas + memcpy.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "../core/page_codec.h"

namespace ifs {
namespace gpu {

bool available();
int device_count();
std::string device_name(int dev);
size_t device_total_mem(int dev);

// --- memory ----------------------------------------------------------------
void* alloc_device(int dev, size_t bytes);           // hipMalloc on device
void free_device(void* p);
void* alloc_host_pinned(size_t bytes);               // hipHostMalloc (falls back to aligned_alloc)
void free_host_pinned(void* p);
bool memcpy_d2h(void* dst, const void* src, size_t n);
bool memcpy_h2d(void* dst, const void* src, size_t n);
bool memcpy_d2d(void* dst, const void* src, size_t n);  // same or peer device
// Async variants on a stream (hipMemcpyAsync).
using Stream = void*;
bool memcpy_h2d_async(void* dst, const void* src, size_t n, Stream s);
bool memcpy_d2h_async(void* dst, const void* src, size_t n, Stream s);
bool memcpy_any_async(void* dst, const void* src, size_t n, Stream s);

// --- IPC -------------------------------------------------------------------
constexpr size_t kIpcHandleSize = 64;  // == HIP_IPC_HANDLE_SIZE
struct IpcHandle {
    uint8_t bytes[kIpcHandleSize];
};

// Export `ptr`'s allocation; also reports the offset of ptr inside that
// allocation so importers can reconstruct the exact address (works with the
// PyTorch caching allocator, unlike the reference which needs
// PYTORCH_NO_CUDA_MEMORY_CACHING).
// alloc_size (optional): the containing allocation's byte size — callers
// must refuse the IPC path for allocations >= 2 GiB (hipIpcOpenMemHandle
// hangs forever importing them under dmabuf IPC on this ROCm/driver stack;
// scripts/ipc_size_probe.py bisected the threshold).
bool ipc_export(const void* ptr, IpcHandle* handle, uint64_t* base_offset,
                uint64_t* alloc_size = nullptr);
void* ipc_open(const IpcHandle& handle, int src_device);
bool ipc_close(void* base);

// Enable xGMI peer access dev -> peer (idempotent). Returns false if the
// pair cannot peer.
bool enable_peer_access(int dev, int peer);

// True if ptr is device (HBM) memory — hipPointerGetAttributes probe, the
// HIP analog of the reference's host-vs-device MR classification.
bool is_device_pointer(const void* ptr);

// Export a dmabuf fd covering [ptr, ptr+size) of device memory (the amdgpu
// path for registering HBM with an RDMA NIC: ibv_reg_dmabuf_mr). Returns
// the fd or -1; *offset is the start offset inside the dmabuf.
int export_dmabuf(void* ptr, size_t size, uint64_t* offset);

// --- streams / events (opaque wrappers so non-HIP TUs can hold them) -------
using Event = void*;
Stream stream_create(int dev);
void stream_destroy(Stream s);
bool stream_sync(Stream s);
Event event_create(int dev);
void event_destroy(Event e);
bool event_record(Event e, Stream s);
bool event_sync(Event e);      // blocking wait
bool event_query(Event e);     // true if complete
bool set_device(int dev);

// --- batched block copy ----------------------------------------------------
// One launch copies n_blocks of `bytes_per_block` from src_ptrs[i] to
// dst_ptrs[i]. The pointer arrays must be device-VISIBLE: device memory or
// pinned host (hipHostMalloc — ROCm unified addressing; each workgroup reads
// its 16 B descriptor once, so keeping descriptors in pinned host memory
// avoids any per-launch SDMA upload). Chooses the vectorized 16 B/lane
// kernel when every pointer and the size are 16-byte aligned, else a
// byte-granular fallback.
// Segmented pages (core/page_codec.h): with seg.n > 1 the CLIENT side of every
// block is seg.n pieces seg.stride_bytes apart, the source for kStore and the
// destination for kLoad; the pool side stays contiguous. The geometry rides in
// the kernel arguments: a workgroup is (block, segment, chunk) and still reads
// its block's descriptor pair once. The vector kernel additionally needs the
// segment size and the stride to be 16-byte multiples, else the byte kernel
// runs. seg.n == 1 runs the contiguous kernels; an illegal geometry
// (segments_legal) returns false before any launch.
bool launch_copy_blocks(int dev, Stream s, const uint64_t* dev_src_ptrs,
                        const uint64_t* dev_dst_ptrs, int n_blocks, size_t bytes_per_block,
                        bool aligned16, PageSegments seg = {}, PageDir dir = PageDir::kStore);

// Small batches (n <= 16, 16B-aligned): descriptors passed as kernel args
// from HOST arrays — no device staging needed.
bool launch_copy_blocks_inline(int dev, Stream s, const uint64_t* src_ptrs,
                               const uint64_t* dst_ptrs, int n_blocks, size_t bytes_per_block);

// --- KV page compression -----------------------------------------------------
// Convert n blocks of bf16 (elems_per_block each) into stored blocks of
// `codec` (kStore), or stored blocks back into bf16 (kLoad). Sizes per codec:
// core/page_codec.h. Every block pointer is 16-byte aligned (the CALLER
// checks: the descriptors may be device memory). kNone is refused: plain
// pages go through launch_copy_blocks.
//  * fp8 (fp8_codec.h): e4m3fn blocks of half the byte size and one scale
//    (finite absmax/448) per block, written to dev_scales[i] by kStore and
//    read from it by kLoad. Both kernels move 16 bytes per lane:
//    elems_per_block % 8 == 0 (checked here).
//  * mxfp4 (mxfp4_codec.h): OCP MXFP4 blocks of elems/2 + elems/32 bytes:
//    e2m1 codes, two per byte, then one e8m0 scale byte per 32 elements. The
//    scales live inside the block, so dev_scales is ignored.
//    elems_per_block % 32 == 0 (checked here).
// Segmented pages: with seg.n > 1 the bf16 side (source of kStore,
// destination of kLoad) is segmented as for launch_copy_blocks; the stored
// block is byte-identical to the contiguous page's. fp8 keeps ONE scale over
// all segments; mxfp4 indexes codes and scale bytes by the page-global unit.
// Segment and stride rules: segments_legal (checked here).
bool launch_transform_blocks(int dev, Stream s, PageCodec codec, PageDir dir,
                             const uint64_t* dev_src_ptrs, const uint64_t* dev_dst_ptrs,
                             float* dev_scales, int n_blocks, size_t elems_per_block,
                             PageSegments seg = {});
// Groups of 32 elements that one workgroup of either mxfp4 kernel covers per
// loop iteration (four lanes per group).
constexpr int kMxfp4GroupsPerIter = 64;

// --- tensor sets --------------------------------------------------------------
// The client side of every page spans tset.n tensors (core/page_codec.h,
// tensors_legal; docs/design.md, "tensor sets"): seg.n is the TOTAL segment
// count S, and segment s of block i lives at
//   tset.bases[s / (S/G)] + client_desc[i] + (s % (S/G)) * seg.stride_bytes.
// The client descriptor (src for kStore, dst for kLoad) is therefore a byte
// OFFSET, the same inside every tensor; the pool descriptor is a pointer, and
// both arrays are device-visible as above. tset.bases is HOST memory: the
// table is copied into the kernel arguments at launch, so it need not outlive
// the call.
struct TensorTable {
    const uint64_t* bases = nullptr;  // n device addresses, host array
    uint32_t n = 0;
};
// Plain pages: the 16 B/lane kernel when aligned16 holds (every offset and
// pool pointer is a multiple of 16; the CALLER checks, the descriptors may be
// device memory) and every base, the segment size and, where one is applied,
// the stride are multiples of 16 too; else the byte kernel. False before any
// launch for a geometry tensors_legal refuses or a grid that does not fit.
bool launch_copy_blocks_tset(int dev, Stream s, const uint64_t* dev_src, const uint64_t* dev_dst,
                             int n_blocks, size_t bytes_per_block, bool aligned16,
                             PageSegments seg, PageDir dir, TensorTable tset);
// Transforming codecs, scales as for launch_transform_blocks: fp8 keeps ONE
// scale per page over all tensors, mxfp4 indexes codes and scale bytes by the
// page-global unit. There is no byte fallback: additionally false, before any
// launch, unless aligned16 holds and every base is a multiple of 16.
bool launch_transform_blocks_tset(int dev, Stream s, PageCodec codec, PageDir dir,
                                  const uint64_t* dev_src, const uint64_t* dev_dst,
                                  float* dev_scales, int n_blocks, size_t elems_per_block,
                                  bool aligned16, PageSegments seg, TensorTable tset);

// --- sliced reads -------------------------------------------------------------
// Load direction only (core/page_codec.h, PageSlice; docs/design.md, "sliced
// reads"): from each stored block take slice.n pieces of slice.piece_bytes
// LOGICAL bytes, piece p at logical byte slice.offset + p * slice.stride of
// the page the block was written with, and write their concatenation, the
// sliced page, to the client page, itself split into seg.n segments when
// seg.n > 1. Descriptors are what they are elsewhere (stored block base,
// client page base, device-visible); the geometry rides in the kernel
// arguments. One kernel per stored format: plain 16 B/lane, plain byte-wise
// (chosen when the client pointers, offset, piece, stride or client stride are
// not all 16-byte multiples), fp8 -> bf16 with block i's scale in
// dev_scales[i], mxfp4 -> bf16 (dev_scales ignored). aligned16 says that every
// descriptor pointer is 16-byte aligned (the CALLER checks). Returns false
// before any launch for an illegal geometry (slice_legal), a transforming
// codec without aligned16, or a grid that does not fit.
bool launch_load_sliced(int dev, Stream s, PageCodec codec, const uint64_t* dev_src_ptrs,
                        const uint64_t* dev_dst_ptrs, const float* dev_scales, int n_blocks,
                        PageSlice slice, PageSegments seg, bool aligned16);
// Workgroup size of the four sliced kernels, public so that tests compute the
// edges of the lane mapping from it.
constexpr int kSliceThreads = 512;

// --- block fingerprint ------------------------------------------------------
// 64-bit position-salted fingerprint per block -> out_hashes[i] (device mem).
bool launch_hash_blocks(int dev, Stream s, const uint64_t* dev_ptrs, int n_blocks,
                        size_t bytes_per_block, uint64_t* dev_out_hashes);

const char* last_error();

}  // namespace gpu
}  // namespace ifs
