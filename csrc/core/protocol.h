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
// when kLocalFlagTensorSet is set,] [PackedLocalPermExt when
// kLocalFlagPermuted is set,] [PackedLocalXposeExt when kLocalFlagTransposed
// is set,] [PackedLocalCastExt when kLocalFlagCast is set,] [PackedLocalRotExt
// and its rot_dim float32 table when kLocalFlagRotated is set,]
// [PackedLocalShufExt when kLocalFlagShuffled is set,] u64 offsets[n],
// NUL-separated key bytes (n keys).
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

// Follows PackedLocalHdr and every other extension when kLocalFlagPermuted is
// set: the order of the pieces of the request's pages in CLIENT memory
// (core/page_codec.h, PagePermute; docs/design.md, "permuted pages").
#pragma pack(push, 1)
struct PackedLocalPermExt {
    uint32_t outer;
    uint32_t rows;
    uint32_t cols;
    uint32_t rsvd;         // 0
    uint64_t piece_bytes;  // logical bytes; outer * rows * cols pieces are block_size
};
#pragma pack(pop)
static_assert(sizeof(PackedLocalPermExt) == 24, "packed local permute extension size");

// Follows PackedLocalHdr and every other extension when kLocalFlagTransposed
// is set: the element order of the request's pages in CLIENT memory
// (core/page_codec.h, PageTranspose; docs/design.md, "transposed pages").
#pragma pack(push, 1)
struct PackedLocalXposeExt {
    uint32_t outer;
    uint32_t tokens;
    uint32_t heads;
    uint32_t cols;
    uint32_t elem_bytes;
    uint32_t inner_k;  // x_0, in elements
    uint32_t inner_v;  // x_1
    uint32_t rsvd;     // 0
};
#pragma pack(pop)
static_assert(sizeof(PackedLocalXposeExt) == 32, "packed local transpose extension size");

// Follows PackedLocalHdr and every other extension when kLocalFlagCast is set:
// the element type of the request's pages in CLIENT memory (core/page_codec.h,
// PageCast; docs/design.md, "cast pages").
#pragma pack(push, 1)
struct PackedLocalCastExt {
    uint32_t elem_type;  // 1: OCP e4m3fn codes
    uint32_t halves;     // 1 or 2
    float scale[2];      // element value = code value * scale[half]
};
#pragma pack(pop)
static_assert(sizeof(PackedLocalCastExt) == 16, "packed local cast extension size");

// Follows PackedLocalHdr and every other extension when kLocalFlagRotated is
// set, itself followed by rot_dim float32 values, (cos, sin) of pair 0, of
// pair 1, ...: the rotation a READ applies to the K half of each page
// (core/page_codec.h, PageRotate; docs/design.md, "rotated reads").
#pragma pack(push, 1)
struct PackedLocalRotExt {
    uint32_t style;     // 1: NeoX halves, 2: GPT-J interleaved
    uint32_t halves;    // 1 or 2; half 0 is rotated
    uint32_t heads;
    uint32_t head_dim;  // elements
    uint32_t rot_dim;   // elements, <= head_dim
    uint32_t rsvd;      // 0
};
#pragma pack(pop)
static_assert(sizeof(PackedLocalRotExt) == 24, "packed local rotate extension size");

// Follows PackedLocalHdr and every other extension when kLocalFlagShuffled is
// set: the element order of the request's pages in CLIENT memory
// (core/page_codec.h, PageShuffle; docs/design.md, "shuffled pages").
#pragma pack(push, 1)
struct PackedLocalShufExt {
    uint32_t outer;
    uint32_t tokens;
    uint32_t heads;
    uint32_t cols;
    uint32_t elem_bytes;
    uint32_t form_k;  // form of half 0: 1 (K form) or 2 (V form)
    uint32_t form_v;  // form of half 1
    uint32_t rsvd;    // 0
};
#pragma pack(pop)
static_assert(sizeof(PackedLocalShufExt) == 32, "packed local shuffle extension size");

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
// The client holds each page with two piece axes exchanged, as the
// PackedLocalPermExt after the other extensions says (extension; both packed
// ops). The stored block is the canonical page's. Together with
// kLocalFlagSliced or kLocalFlagTensorSet it is INVALID_REQ.
constexpr uint32_t kLocalFlagPermuted = 64;
// The client holds each page as a paged-attention cache block (per head, K as
// [cols/x, tokens, x] and V as [cols, tokens]), as the PackedLocalXposeExt
// after all other extensions says (extension; both packed ops). The stored
// block is the canonical page's. Together with kLocalFlagSliced,
// kLocalFlagTensorSet or kLocalFlagPermuted it is INVALID_REQ.
constexpr uint32_t kLocalFlagTransposed = 128;
// The client holds each page as one-byte e4m3fn codes with a scale per half,
// as the PackedLocalCastExt after all other extensions says (extension; both
// packed ops). block_size stays the LOGICAL bf16 byte count and the stored
// block is the bf16 page's; the client page is half of it, and a segment
// extension next to this flag speaks of client bytes. Together with
// kLocalFlagSliced, kLocalFlagTensorSet, kLocalFlagPermuted or
// kLocalFlagTransposed it is INVALID_REQ.
constexpr uint32_t kLocalFlagCast = 256;
// Rotate the K half of each page by the (cos, sin) table that follows the
// PackedLocalRotExt after all other extensions (extension; OP_R_FAST only,
// INVALID_REQ on OP_W_FAST). The pages are bf16 and block_size is the written
// page. Together with kLocalFlagSliced, kLocalFlagTensorSet,
// kLocalFlagPermuted, kLocalFlagTransposed or kLocalFlagCast it is
// INVALID_REQ.
constexpr uint32_t kLocalFlagRotated = 512;
// The client holds each page as a shuffled cache block (per head, K as
// [cols/X, tokens, X] and V as [tokens/X, cols, X], X = 16 / elem_bytes), as
// the PackedLocalShufExt after all other extensions says (extension; both
// packed ops). The stored block is the canonical page's. Together with
// kLocalFlagSliced, kLocalFlagTensorSet, kLocalFlagPermuted,
// kLocalFlagTransposed, kLocalFlagCast or kLocalFlagRotated it is INVALID_REQ.
constexpr uint32_t kLocalFlagShuffled = 1024;

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
                                        const PackedLocalTensorExt* tset = nullptr,
                                        const PackedLocalPermExt* perm = nullptr,
                                        const PackedLocalXposeExt* xpose = nullptr,
                                        const PackedLocalCastExt* cast = nullptr,
                                        const PackedLocalRotExt* rot = nullptr,
                                        const float* rot_table = nullptr,
                                        const PackedLocalShufExt* shuf = nullptr);
// (The shuffle extension and kLocalFlagShuffled are written only for a `shuf`
// with tokens != 0, its rsvd as given.)
// (The rotate extension, the rot_dim floats at rot_table and kLocalFlagRotated
// are written only for a `rot` with style != 0, its rsvd as given.)
// (The cast extension and kLocalFlagCast are written only for a `cast` with
// elem_type != 0.)
// (The permute extension and kLocalFlagPermuted are written only for a `perm`
// with rows != 0, its rsvd as given; the transpose extension and
// kLocalFlagTransposed likewise only for an `xpose` with tokens != 0.)
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
    PackedLocalPermExt perm{};  // rows == 0: not permuted
    PackedLocalXposeExt xpose{};  // tokens == 0: not transposed
    PackedLocalCastExt cast{};    // elem_type == 0: not cast
    PackedLocalRotExt rot{};      // style == 0: not rotated
    std::vector<float> rot_table;  // rot.rot_dim values when rotated
    PackedLocalShufExt shuf{};     // tokens == 0: not shuffled
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
// kLocalFlagSliced is refused. kLocalFlagPermuted is refused next to either
// of those two flags, and when permute_legal refuses the geometry for
// block_size (same codec choice as for segments). kLocalFlagTransposed is
// refused next to any of those three flags, and when transpose_legal refuses
// the geometry for block_size (same codec choice again). kLocalFlagCast is
// refused next to any of those four flags, and when cast_legal refuses the
// extension for block_size and the segments (same codec choice), which it
// judges in place of segments_legal. kLocalFlagRotated is refused on
// OP_W_FAST, next to any of those five flags, with a cut table, and when
// rotate_legal refuses the geometry or the table for block_size and the
// segments under plain rules. kLocalFlagShuffled is refused next to any of
// those six flags, and when shuffle_legal refuses the geometry for block_size
// (same codec choice as for segments).
bool parse_packed_local(char op, const uint8_t* body, size_t body_len, PackedLocalReq* out);

// Sentinel for duplicate-key allocations: the server returns rkey=0, addr=0
// for keys that already exist; clients skip writing those blocks (first write
// wins, matching the reference's dedup semantics).
inline bool is_fake_remote_block(uint32_t rkey, uint64_t addr) { return rkey == 0 && addr == 0; }

}  // namespace ifs
