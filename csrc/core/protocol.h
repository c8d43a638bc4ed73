// Wire protocol for infinistore-amd.
//
// Wire-compatible with the reference store's protocol
// (cf. /root/reference/src/protocol.h:39-71 for the 9-byte header, op chars
// and status codes, and /root/reference/src/*.fbs for the four flatbuffers
// tables) — reimplemented from scratch on top of the clean-room flatbuffers
// core in wire.h.
//
// Extensions over the reference (all additive):
//  * LocalMetaRequest gains field id 4 `base_offset:ulong` — the byte offset
//    of the tensor pointer inside its IPC-exported allocation, which lets
//    clients use tensors that are not at the base of a hipMalloc allocation
//    (the reference requires PYTORCH_NO_CUDA_MEMORY_CACHING instead).
//  * New ops for the TCP data fabric (RDMA-semantics emulation when no
//    RDMA NIC is present): OP_TCP_PUT 'P', OP_TCP_GET 'G'.
#pragma once

#include <cstdint>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "wire.h"

namespace ifs {

// ---- framing --------------------------------------------------------------
constexpr uint32_t kMagic = 0xdeadbeef;

#pragma pack(push, 1)
struct Header {
    uint32_t magic;
    char op;
    uint32_t body_size;
};
#pragma pack(pop)
static_assert(sizeof(Header) == 9, "header must be 9 bytes");

// ---- ops ------------------------------------------------------------------
constexpr char OP_R = 'R';                  // local-GPU read
constexpr char OP_W = 'W';                  // local-GPU write
constexpr char OP_SYNC = 'S';               // local sync (inflight count)
constexpr char OP_RDMA_EXCHANGE = 'E';      // fabric negotiation
constexpr char OP_RDMA_ALLOCATE = 'D';      // allocate blocks for remote write
constexpr char OP_RDMA_READ = 'A';          // remote read request
constexpr char OP_RDMA_WRITE_COMMIT = 'T';  // commit written blocks
constexpr char OP_CHECK_EXIST = 'C';
constexpr char OP_GET_MATCH_LAST_IDX = 'M';
// Extensions (TCP data fabric):
constexpr char OP_TCP_PUT = 'P';  // inline block data put (emulated RDMA_WRITE)
constexpr char OP_TCP_GET = 'G';  // inline block data get (emulated server push)
constexpr char OP_DELETE = 'X';   // delete keys (extension: engine-driven eviction)
constexpr char OP_STATS = 'Q';    // server stats JSON over the wire (extension)
// Packed fast-path local ops (extension): same semantics as OP_W/OP_R but a
// flat binary layout the hot path can build/parse at memcpy speed — the
// flatbuffers LocalMetaRequest ops remain accepted for wire compatibility.
// Body: PackedLocalHdr, [PackedLocalSegExt when kLocalFlagSegmented is set,]
// [PackedLocalSliceExt when kLocalFlagSliced is set,] [PackedLocalTensorExt
// when kLocalFlagTensorSet is set,] u64 offsets[n], NUL-separated key bytes
// (n keys).
constexpr char OP_W_FAST = 'w';
constexpr char OP_R_FAST = 'r';
// Shared-memory ring handshake (extension, same-host clients): body is the
// shm_open name of a client-created segment (csrc/core/shm_ring.h); after a
// FINISH response the client sends OP_W_FAST/OP_R_FAST/OP_SYNC through the
// ring instead of the socket.
constexpr char OP_SHM_SETUP = 'h';
// Tensor sets (extension; docs/design.md, "tensor sets"): register an ordered
// list of client tensors on this connection once, then name it in packed
// requests by id. Socket only. Register body: PackedTensorSetHdr + n_tensors
// PackedTensorRec; the reply is FINISH + u32 set id, or a bare error status.
// Release body: u32 set id; the reply is a bare status.
constexpr char OP_TSET_REGISTER = 't';
constexpr char OP_TSET_RELEASE = 'u';
// Live sets one connection may hold.
constexpr uint32_t kMaxTensorSetsPerConn = 16;

#pragma pack(push, 1)
struct PackedLocalHdr {
    int32_t device;
    int32_t pid;
    uint64_t base_ptr;
    uint64_t base_offset;
    uint32_t block_size;
    uint32_t n_blocks;
    uint32_t flags;
    uint32_t rsvd;
    uint8_t ipc[64];
};
#pragma pack(pop)
static_assert(sizeof(PackedLocalHdr) == 104, "packed local header size");

// Follows PackedLocalHdr when kLocalFlagSegmented is set: the geometry of the
// request's pages in CLIENT memory (docs/design.md, "segmented pages"). The
// header keeps its size: its own rsvd word carries the allocation size.
#pragma pack(push, 1)
struct PackedLocalSegExt {
    uint32_t n_segments;
    uint32_t rsvd;            // 0
    uint64_t segment_stride;  // bytes from one segment of a page to the next
};
#pragma pack(pop)
static_assert(sizeof(PackedLocalSegExt) == 16, "packed local segment extension size");

// Follows PackedLocalHdr, and PackedLocalSegExt when that is present, when
// kLocalFlagSliced is set: the POOL-side geometry of a read (core/page_codec.h,
// PageSlice; docs/design.md, "sliced reads"). All values are logical bytes.
// The header's block_size is the sliced page: n_pieces * piece_bytes.
#pragma pack(push, 1)
struct PackedLocalSliceExt {
    uint32_t n_pieces;
    uint32_t rsvd;         // 0
    uint64_t page_bytes;   // logical size of the page the keys were written with
    uint64_t offset;       // logical byte of piece 0 inside that page
    uint64_t piece_bytes;
    uint64_t stride;       // logical bytes from one piece to the next
};
#pragma pack(pop)
static_assert(sizeof(PackedLocalSliceExt) == 40, "packed local slice extension size");

// Follows PackedLocalHdr and the segment and slice extensions when
// kLocalFlagTensorSet is set, so that the existing prefixes parse as before:
// the request's pages span the tensors of a registered set. The header's ipc,
// base_ptr and base_offset are then ignored, and offsets[] are relative to
// each tensor.
#pragma pack(push, 1)
struct PackedLocalTensorExt {
    uint32_t set_id;
    uint32_t n_tensors;  // must equal the registered count
    uint64_t rsvd;       // 0
};
#pragma pack(pop)
static_assert(sizeof(PackedLocalTensorExt) == 16, "packed local tensor-set extension size");

// OP_TSET_REGISTER body: this header, then n_tensors records in set order.
#pragma pack(push, 1)
struct PackedTensorSetHdr {
    int32_t pid;
    int32_t device;
    uint32_t n_tensors;
    uint32_t rsvd;  // 0
};
struct PackedTensorRec {
    uint64_t base_ptr;      // the allocation's base in the client's address space
    uint64_t base_offset;   // the tensor's first byte inside the allocation
    uint64_t extent_bytes;  // the tensor's size: no page part may reach past it
    uint32_t alloc_mb;      // allocation size in MB (0 = unknown), as PackedLocalHdr.rsvd
    uint32_t rsvd;          // 0
    uint8_t ipc[64];
};
#pragma pack(pop)
static_assert(sizeof(PackedTensorSetHdr) == 16 && sizeof(PackedTensorRec) == 96,
              "tensor set registration sizes");

// PackedLocalHdr.flags: defer the response until the copy completes (one
// round trip instead of request-ack + sync).
constexpr uint32_t kLocalFlagSyncResponse = 1;
// Store the (bf16) payload quantized to fp8 e4m3 with one scale per block —
// half the HBM per cached page; reads dequantize transparently (extension,
// csrc/gpu/gpu.hip quant kernels).
constexpr uint32_t kLocalFlagQuantFp8 = 2;
// Store the (bf16) payload as OCP MXFP4: e2m1 codes plus one e8m0 scale per
// 32 elements inside the stored block, 17/64 of the bf16 bytes (extension,
// csrc/gpu/mxfp4_codec.h). Setting both quant flags is INVALID_REQ.
constexpr uint32_t kLocalFlagQuantMxfp4 = 4;
// Each page is n_segments equal pieces of client memory, segment_stride bytes
// apart, given by the PackedLocalSegExt that follows the header (extension;
// packed ops only). The stored block is that of the concatenated page.
constexpr uint32_t kLocalFlagSegmented = 8;
// Read n_pieces strided pieces of each stored page instead of the whole page,
// given by the PackedLocalSliceExt that follows the header and the segment
// extension (extension; OP_R_FAST only, INVALID_REQ on OP_W_FAST).
constexpr uint32_t kLocalFlagSliced = 16;
// The pages span the tensors of a registered set, named by the
// PackedLocalTensorExt that follows the other extensions (extension; both
// packed ops). Together with kLocalFlagSliced it is INVALID_REQ.
constexpr uint32_t kLocalFlagTensorSet = 32;

std::string op_name(char op);

// ---- status codes ---------------------------------------------------------
constexpr int INVALID_REQ = 400;
constexpr int FINISH = 200;
constexpr int TASK_ACCEPTED = 202;
constexpr int INTERNAL_ERROR = 500;
constexpr int KEY_NOT_FOUND = 404;
constexpr int RETRY = 408;
constexpr int SYSTEM_ERROR = 503;
constexpr int OUT_OF_MEMORY = 507;

constexpr size_t kProtocolBufferSize = 4u << 20;  // max body for one request

// Flow-control constants (same roles as the reference's WR constants,
// protocol.h:23-34; the TCP fabric uses them to bound in-flight bytes).
constexpr int kMaxWrBatch = 32;
constexpr int kMaxOutstandingWrites = 4096;

// ---- typed messages -------------------------------------------------------
struct RemoteBlockWire {  // matches flatbuffers struct RemoteBlock (16 B)
    uint32_t rkey;
    uint32_t pad_ = 0;
    uint64_t remote_addr;
};
static_assert(sizeof(RemoteBlockWire) == 16, "RemoteBlock wire size");

struct KeyOffset {
    std::string key;
    uint64_t offset;
};

struct LocalMetaMsg {
    int32_t device = 0;
    std::vector<uint8_t> ipc_handle;
    int32_t block_size = 0;
    std::vector<KeyOffset> blocks;
    uint64_t base_offset = 0;  // extension, field id 4
    int32_t pid = 0;           // extension, field id 5: client pid — enables a
    uint64_t base_ptr = 0;     // field id 6: same-process fast path (an IPC
                               // handle cannot be opened in its own process)
};

struct RemoteMetaMsg {
    std::vector<std::string> keys;
    int32_t block_size = 0;
    uint32_t rkey = 0;
    std::vector<uint64_t> remote_addrs;
    int8_t op = 0;
};

// Serializers produce a complete flatbuffer (root offset included).
std::vector<uint8_t> build_local_meta(const LocalMetaMsg& m);
bool parse_local_meta(const uint8_t* buf, size_t len, LocalMetaMsg* out);

std::vector<uint8_t> build_remote_meta(const RemoteMetaMsg& m);
bool parse_remote_meta(const uint8_t* buf, size_t len, RemoteMetaMsg* out);

std::vector<uint8_t> build_allocate_response(const std::vector<RemoteBlockWire>& blocks);
bool parse_allocate_response(const uint8_t* buf, size_t len, std::vector<RemoteBlockWire>* out);

std::vector<uint8_t> build_match_request(const std::vector<std::string>& keys);
bool parse_match_request(const uint8_t* buf, size_t len, std::vector<std::string>* out);

// Packed fast-path body (OP_W_FAST / OP_R_FAST). The builder writes the
// segment extension, and sets kLocalFlagSegmented, only for n_segments > 1:
// a contiguous request is byte for byte what it was before the extension
// existed. Offsets are in bytes; keys_blob holds the n NUL-separated keys.
// Likewise the slice extension and kLocalFlagSliced are written only for a
// slice with n_pieces != 0 (its rsvd is written as given, 0 from every real
// caller); without one the body is what it was before slices existed.
std::vector<uint8_t> build_packed_local(PackedLocalHdr h, uint32_t n_segments,
                                        uint64_t segment_stride, const uint64_t* offsets,
                                        const char* keys_blob, size_t blob_len,
                                        const PackedLocalSliceExt* slice = nullptr,
                                        const PackedLocalTensorExt* tset = nullptr);
// (The tensor-set extension and kLocalFlagTensorSet are written only when
// `tset` is given; the segment extension is then written for n_segments > 1
// as always, n_segments being the total over all tensors.)

// OP_TSET_REGISTER body and its parser (false: truncated, rsvd set, or a
// count outside 1..kMaxPageTensors).
std::vector<uint8_t> build_tensor_set(int32_t pid, int32_t device,
                                      const std::vector<PackedTensorRec>& recs);
bool parse_tensor_set(const uint8_t* body, size_t body_len, PackedTensorSetHdr* hdr,
                      std::vector<PackedTensorRec>* recs);

// Parsed view of a packed body: (key, byte offset) per block, the key views
// pointing into the body. The server moves `blocks` into its request view,
// so parsing stays one pass and one allocation.
struct PackedLocalReq {
    PackedLocalHdr hdr;
    uint32_t n_segments = 1;
    uint64_t segment_stride = 0;
    PackedLocalSliceExt slice{};  // n_pieces == 0: whole pages
    bool has_tset = false;
    PackedLocalTensorExt tset{};
    std::vector<std::pair<std::string_view, uint64_t>> blocks;
};
// False (the server answers INVALID_REQ) for a truncated body or extension,
// a non-zero extension rsvd, more than one quant flag, or a geometry that
// segments_legal refuses: for the request's codec on OP_W_FAST, for plain
// pages on OP_R_FAST (the read path re-checks every entry against its own
// codec once the index has told it what the keys hold). kLocalFlagSliced is
// refused on OP_W_FAST; on OP_R_FAST also when block_size is not n_pieces *
// piece_bytes or slice_legal refuses the geometry under plain rules. With
// kLocalFlagTensorSet the geometry rule is tensors_legal instead of
// segments_legal (same codec choice), and the flag together with
// kLocalFlagSliced is refused.
bool parse_packed_local(char op, const uint8_t* body, size_t body_len, PackedLocalReq* out);

// Sentinel for duplicate-key allocations: the server returns rkey=0, addr=0
// for keys that already exist; clients skip writing those blocks (first write
// wins, matching the reference's dedup semantics).
inline bool is_fake_remote_block(uint32_t rkey, uint64_t addr) { return rkey == 0 && addr == 0; }

}  // namespace ifs
