#include "protocol.h"

#include <cstring>

#include "page_codec.h"

namespace ifs {

std::string op_name(char op) {
    switch (op) {
        case OP_R: return "local_read";
        case OP_W: return "local_write";
        case OP_SYNC: return "sync";
        case OP_RDMA_EXCHANGE: return "exchange";
        case OP_RDMA_ALLOCATE: return "allocate";
        case OP_RDMA_READ: return "rdma_read";
        case OP_RDMA_WRITE_COMMIT: return "write_commit";
        case OP_CHECK_EXIST: return "check_exist";
        case OP_GET_MATCH_LAST_IDX: return "match_last_index";
        case OP_TCP_PUT: return "tcp_put";
        case OP_TCP_GET: return "tcp_get";
        case OP_DELETE: return "delete";
        case OP_STATS: return "stats";
        case OP_W_FAST: return "local_write_fast";
        case OP_R_FAST: return "local_read_fast";
        case OP_SHM_SETUP: return "shm_setup";
        default: return "unknown";
    }
}

// --- LocalMetaRequest: device(0), ipc_handle(1), block_size(2), blocks(3),
//     base_offset(4 — extension). Block: key(0), offset(1).
std::vector<uint8_t> build_local_meta(const LocalMetaMsg& m) {
    wire::Builder b(512 + m.blocks.size() * 64);
    // Build Block subtables first (file-later objects are pushed first).
    std::vector<wire::Builder::Offset> block_offs;
    block_offs.reserve(m.blocks.size());
    for (auto it = m.blocks.rbegin(); it != m.blocks.rend(); ++it) {
        auto koff = b.create_string(it->key);
        b.start_table();
        b.add_offset(0, koff);
        b.add_scalar<uint64_t>(1, it->offset, 0);
        block_offs.push_back(b.end_table());
    }
    // block_offs built in reverse; restore order for the vector.
    std::vector<wire::Builder::Offset> ordered(block_offs.rbegin(), block_offs.rend());
    auto blocks_vec = b.create_offset_vector(ordered);
    auto ipc_vec = b.create_vector<uint8_t>(m.ipc_handle.data(), m.ipc_handle.size());
    b.start_table();
    b.add_scalar<int32_t>(0, m.device, 0);
    b.add_offset(1, ipc_vec);
    b.add_scalar<int32_t>(2, m.block_size, 0);
    b.add_offset(3, blocks_vec);
    b.add_scalar<uint64_t>(4, m.base_offset, 0);
    b.add_scalar<int32_t>(5, m.pid, 0);
    b.add_scalar<uint64_t>(6, m.base_ptr, 0);
    auto root = b.end_table();
    b.finish(root);
    return b.release();
}

bool parse_local_meta(const uint8_t* buf, size_t len, LocalMetaMsg* out) {
    wire::Reader r(buf, len);
    if (!r.ok()) return false;
    auto t = r.root();
    if (!t.valid()) return false;
    out->device = t.scalar<int32_t>(0, 0);
    out->ipc_handle = t.scalar_vector<uint8_t>(1);
    out->block_size = t.scalar<int32_t>(2, 0);
    out->base_offset = t.scalar<uint64_t>(4, 0);
    out->pid = t.scalar<int32_t>(5, 0);
    out->base_ptr = t.scalar<uint64_t>(6, 0);
    out->blocks.clear();
    size_t n = t.vec_len(3);
    out->blocks.reserve(n);
    for (size_t i = 0; i < n; i++) {
        auto bt = t.table_at_vec(3, i);
        if (!bt.valid()) return false;
        out->blocks.push_back({bt.string_field(0), bt.scalar<uint64_t>(1, 0)});
    }
    return true;
}

// --- RemoteMetaRequest: keys(0), block_size(1), rkey(2), remote_addrs(3), op(4)
std::vector<uint8_t> build_remote_meta(const RemoteMetaMsg& m) {
    wire::Builder b(256 + m.keys.size() * 48 + m.remote_addrs.size() * 8);
    std::vector<wire::Builder::Offset> key_offs;
    key_offs.reserve(m.keys.size());
    for (auto it = m.keys.rbegin(); it != m.keys.rend(); ++it) key_offs.push_back(b.create_string(*it));
    std::vector<wire::Builder::Offset> ordered(key_offs.rbegin(), key_offs.rend());
    auto keys_vec = b.create_offset_vector(ordered);
    auto addrs_vec = b.create_vector<uint64_t>(m.remote_addrs.data(), m.remote_addrs.size());
    b.start_table();
    b.add_offset(0, keys_vec);
    b.add_scalar<int32_t>(1, m.block_size, 0);
    b.add_scalar<uint32_t>(2, m.rkey, 0);
    b.add_offset(3, addrs_vec);
    b.add_scalar<int8_t>(4, m.op, 0);
    auto root = b.end_table();
    b.finish(root);
    return b.release();
}

bool parse_remote_meta(const uint8_t* buf, size_t len, RemoteMetaMsg* out) {
    wire::Reader r(buf, len);
    if (!r.ok()) return false;
    auto t = r.root();
    if (!t.valid()) return false;
    out->keys = t.string_vector(0);
    out->block_size = t.scalar<int32_t>(1, 0);
    out->rkey = t.scalar<uint32_t>(2, 0);
    out->remote_addrs = t.scalar_vector<uint64_t>(3);
    out->op = t.scalar<int8_t>(4, 0);
    return true;
}

// --- RdmaAllocateResponse: blocks(0) = vector of RemoteBlock struct (16 B)
std::vector<uint8_t> build_allocate_response(const std::vector<RemoteBlockWire>& blocks) {
    wire::Builder b(64 + blocks.size() * 16);
    auto vec = b.create_struct_vector(blocks.data(), blocks.size(), sizeof(RemoteBlockWire), 8);
    b.start_table();
    b.add_offset(0, vec);
    auto root = b.end_table();
    b.finish(root);
    return b.release();
}

bool parse_allocate_response(const uint8_t* buf, size_t len, std::vector<RemoteBlockWire>* out) {
    wire::Reader r(buf, len);
    if (!r.ok()) return false;
    auto t = r.root();
    if (!t.valid()) return false;
    *out = t.scalar_vector<RemoteBlockWire>(0);
    return true;
}

// --- GetMatchLastIndexRequest: keys(0)
std::vector<uint8_t> build_match_request(const std::vector<std::string>& keys) {
    wire::Builder b(64 + keys.size() * 48);
    std::vector<wire::Builder::Offset> key_offs;
    key_offs.reserve(keys.size());
    for (auto it = keys.rbegin(); it != keys.rend(); ++it) key_offs.push_back(b.create_string(*it));
    std::vector<wire::Builder::Offset> ordered(key_offs.rbegin(), key_offs.rend());
    auto keys_vec = b.create_offset_vector(ordered);
    b.start_table();
    b.add_offset(0, keys_vec);
    auto root = b.end_table();
    b.finish(root);
    return b.release();
}

bool parse_match_request(const uint8_t* buf, size_t len, std::vector<std::string>* out) {
    wire::Reader r(buf, len);
    if (!r.ok()) return false;
    auto t = r.root();
    if (!t.valid()) return false;
    *out = t.string_vector(0);
    return true;
}

std::vector<uint8_t> build_packed_local(PackedLocalHdr h, uint32_t n_segments,
                                        uint64_t segment_stride, const uint64_t* offsets,
                                        const char* keys_blob, size_t blob_len,
                                        const PackedLocalSliceExt* slice,
                                        const PackedLocalTensorExt* tset) {
    const size_t n = h.n_blocks;
    const bool seg = n_segments != 1;
    const bool sliced = slice && slice->n_pieces != 0;
    if (seg) h.flags |= kLocalFlagSegmented;
    if (sliced) h.flags |= kLocalFlagSliced;
    if (tset) h.flags |= kLocalFlagTensorSet;
    const size_t seg_ext = seg ? sizeof(PackedLocalSegExt) : 0;
    const size_t slice_end = seg_ext + (sliced ? sizeof(PackedLocalSliceExt) : 0);
    const size_t ext = slice_end + (tset ? sizeof(PackedLocalTensorExt) : 0);
    std::vector<uint8_t> body(sizeof(h) + ext + n * 8 + blob_len);
    memcpy(body.data(), &h, sizeof(h));
    if (seg) {
        PackedLocalSegExt e{n_segments, 0, segment_stride};
        memcpy(body.data() + sizeof(h), &e, sizeof(e));
    }
    if (sliced) memcpy(body.data() + sizeof(h) + seg_ext, slice, sizeof(*slice));
    if (tset) memcpy(body.data() + sizeof(h) + slice_end, tset, sizeof(*tset));
    if (n) memcpy(body.data() + sizeof(h) + ext, offsets, n * 8);
    if (blob_len) memcpy(body.data() + sizeof(h) + ext + n * 8, keys_blob, blob_len);
    return body;
}

bool parse_packed_local(char op, const uint8_t* body, size_t body_len, PackedLocalReq* out) {
    if (body_len < sizeof(PackedLocalHdr)) return false;
    PackedLocalHdr& h = out->hdr;
    memcpy(&h, body, sizeof(h));
    size_t pos = sizeof(h);
    out->n_segments = 1;
    out->segment_stride = 0;
    // Over a tensor set the geometry is judged once the set's extension has
    // been read, by tensors_legal.
    const bool has_tset = (h.flags & kLocalFlagTensorSet) != 0;
    if (has_tset && (h.flags & kLocalFlagSliced)) return false;
    if (h.flags & kLocalFlagSegmented) {
        if (body_len < pos + sizeof(PackedLocalSegExt)) return false;
        PackedLocalSegExt e;
        memcpy(&e, body + pos, sizeof(e));
        pos += sizeof(e);
        if (e.rsvd != 0) return false;
        PageCodec codec = PageCodec::kNone;
        if (op == OP_W_FAST && !page_codec_from_flags(h.flags, &codec)) return false;
        if (!has_tset && !segments_legal(codec, h.block_size, e.n_segments, e.segment_stride))
            return false;
        out->n_segments = e.n_segments;
        out->segment_stride = e.segment_stride;
    }
    out->slice = PackedLocalSliceExt{};
    if (h.flags & kLocalFlagSliced) {
        if (op != OP_R_FAST) return false;  // slices are a read-side geometry
        if (body_len < pos + sizeof(PackedLocalSliceExt)) return false;
        PackedLocalSliceExt e;
        memcpy(&e, body + pos, sizeof(e));
        pos += sizeof(e);
        if (e.rsvd != 0) return false;
        // Plain rules, like the segments above; a zero-piece extension fails
        // slice_legal, so a parsed request is sliced exactly when n_pieces != 0.
        if (!slice_legal(PageCodec::kNone, slice_from_wire(e),
                         PageSegments{out->n_segments, out->segment_stride}))
            return false;
        if (h.block_size != e.n_pieces * e.piece_bytes) return false;
        out->slice = e;
    }
    out->has_tset = has_tset;
    out->tset = PackedLocalTensorExt{};
    if (has_tset) {
        if (body_len < pos + sizeof(PackedLocalTensorExt)) return false;
        PackedLocalTensorExt e;
        memcpy(&e, body + pos, sizeof(e));
        pos += sizeof(e);
        if (e.rsvd != 0) return false;
        PageCodec codec = PageCodec::kNone;
        if (op == OP_W_FAST && !page_codec_from_flags(h.flags, &codec)) return false;
        if (!tensors_legal(codec, h.block_size, out->n_segments, out->segment_stride,
                           e.n_tensors))
            return false;
        out->tset = e;
    }
    const size_t n = h.n_blocks;
    const size_t off_end = pos + n * 8;
    if (body_len < off_end) return false;
    const uint8_t* offs = body + pos;  // n little-endian u64, any alignment
    const char* kp = reinterpret_cast<const char*>(body + off_end);
    const char* kend = reinterpret_cast<const char*>(body + body_len);
    out->blocks.clear();
    out->blocks.reserve(n);
    for (size_t i = 0; i < n; i++) {
        const char* nul = static_cast<const char*>(memchr(kp, 0, kend - kp));
        const char* ke = nul ? nul : kend;
        if (kp > kend || (i + 1 < n && !nul)) return false;
        uint64_t off;
        memcpy(&off, offs + i * 8, 8);
        out->blocks.push_back({std::string_view(kp, ke - kp), off});
        kp = nul ? nul + 1 : kend;
    }
    return true;
}

std::vector<uint8_t> build_tensor_set(int32_t pid, int32_t device,
                                      const std::vector<PackedTensorRec>& recs) {
    PackedTensorSetHdr h{pid, device, static_cast<uint32_t>(recs.size()), 0};
    std::vector<uint8_t> body(sizeof(h) + recs.size() * sizeof(PackedTensorRec));
    memcpy(body.data(), &h, sizeof(h));
    if (!recs.empty())
        memcpy(body.data() + sizeof(h), recs.data(), recs.size() * sizeof(PackedTensorRec));
    return body;
}

bool parse_tensor_set(const uint8_t* body, size_t body_len, PackedTensorSetHdr* hdr,
                      std::vector<PackedTensorRec>* recs) {
    if (body_len < sizeof(*hdr)) return false;
    memcpy(hdr, body, sizeof(*hdr));
    if (hdr->rsvd != 0 || hdr->n_tensors < 1 || hdr->n_tensors > kMaxPageTensors) return false;
    if (body_len != sizeof(*hdr) + hdr->n_tensors * sizeof(PackedTensorRec)) return false;
    recs->resize(hdr->n_tensors);
    memcpy(recs->data(), body + sizeof(*hdr), hdr->n_tensors * sizeof(PackedTensorRec));
    for (const PackedTensorRec& r : *recs)
        if (r.rsvd != 0) return false;
    return true;
}

}  // namespace ifs
