// Page codecs: the formats a stored block can have, one table row each.
//
// Everything that defines a format outside its kernels is here: the wire
// flag that asks for it, which logical page sizes it takes, how many bytes
// the stored block has, and whether a per-page scale travels next to the
// block. Server, shard, launcher, bindings and the Python client all derive
// their size and alignment rules from this table (docs/design.md, "page
// codecs"). Host-only: no HIP includes.
#pragma once

#include <cstddef>
#include <cstdint>

#include "protocol.h"

namespace ifs {

// What a stored block holds. The values are the snapshot file's codec word
// (0 and 1 predate mxfp4), so they never change.
enum class PageCodec : uint8_t { kNone = 0, kFp8 = 1, kMxfp4 = 2 };

// Which way a transform runs: kStore converts a logical page into its stored
// block (write path), kLoad converts a stored block back (read path).
enum class PageDir : uint8_t { kStore, kLoad };

// The compressed codecs take bf16 pages.
constexpr size_t kPageElemBytes = 2;

struct PageCodecInfo {
    const char* name;
    uint32_t flag;           // PackedLocalHdr.flags bit that requests it
    uint32_t page_multiple;  // logical page bytes are a multiple of this
    uint32_t num, den;       // stored bytes = page * num / den, exactly
    bool page_scale;         // one fp32 scale per page in BlockEntry::scale
};

// Indexed by PageCodec. fp8: one byte per bf16 element (page / 2), 16 bytes
// per lane. mxfp4: e2m1 codes (page / 4) plus one e8m0 scale byte per 32
// elements (page / 64), whole 32-element groups only.
constexpr PageCodecInfo kPageCodecs[] = {
    {"none", 0, 1, 1, 1, false},
    {"fp8", kLocalFlagQuantFp8, 16, 1, 2, true},
    {"mxfp4", kLocalFlagQuantMxfp4, 64, 17, 64, false},
};
constexpr size_t kNumPageCodecs = sizeof(kPageCodecs) / sizeof(kPageCodecs[0]);
static_assert(kPageCodecs[1].page_multiple % kPageCodecs[1].den == 0 &&
                  kPageCodecs[2].page_multiple % kPageCodecs[2].den == 0,
              "a legal page divides exactly into its stored size");

inline bool page_codec_known(uint32_t id) { return id < kNumPageCodecs; }

inline const PageCodecInfo& page_codec_info(PageCodec c) {
    return kPageCodecs[static_cast<size_t>(c)];
}

// Codec a request's flags ask for; false when more than one quant flag is set.
inline bool page_codec_from_flags(uint32_t flags, PageCodec* out) {
    *out = PageCodec::kNone;
    for (size_t i = 1; i < kNumPageCodecs; i++) {
        if (!(flags & kPageCodecs[i].flag)) continue;
        if (*out != PageCodec::kNone) return false;
        *out = static_cast<PageCodec>(i);
    }
    return true;
}

// Codecs other than kNone convert while moving. Their kernels move 16 bytes
// per lane and have no byte fallback: every page address, logical or stored,
// must be 16-byte aligned.
inline bool page_codec_transforms(PageCodec c) { return c != PageCodec::kNone; }

inline bool page_legal(PageCodec c, size_t page) {
    return page % page_codec_info(c).page_multiple == 0;
}

// Stored bytes of a legal page.
inline size_t stored_bytes(PageCodec c, size_t page) {
    const PageCodecInfo& i = page_codec_info(c);
    return page / i.den * i.num;
}

// Read side: does a block of `stored` bytes hold a logical page of `page`?
inline bool stored_matches(PageCodec c, size_t stored, size_t page) {
    const PageCodecInfo& i = page_codec_info(c);
    // 128-bit products: a size near 2^64 off the wire must not wrap into a match.
    using u128 = unsigned __int128;
    return static_cast<u128>(stored) * i.den == static_cast<u128>(page) * i.num;
}

// Read side, whole-page request: may a block of `stored` bytes answer a read
// of `page` bytes? A plain block serves any page up to its own size, and a
// shorter read returns the block's first `page` bytes (the reference's
// behaviour, kept); a larger one would run past the block into its neighbour
// or out of the arena. A compressed block has no usable prefix: the page must
// be the written one. Sliced and tensor-set reads do not come here: they take
// stored_matches for every codec. The plain case reads no table row: the read
// sweep calls this per block under the stripe lock.
inline bool stored_serves(PageCodec c, size_t stored, size_t page) {
    if (!page_codec_transforms(c)) return page <= stored;
    return stored_matches(c, stored, page);
}

// Segmented pages (docs/design.md, "segmented pages"): on the CLIENT side of
// one request a page may be n_segments equal pieces, piece s starting
// s * stride_bytes after the page's offset; the stored block is that of their
// concatenation. The bound is a condition, not a tuning value: with at most
// 16384 descriptors per launch it keeps every grid far below 2^31 workgroups.
constexpr uint32_t kMaxPageSegments = 1024;

// Client-side geometry of a request's pages; the default is "contiguous".
struct PageSegments {
    uint32_t n = 1;
    uint64_t stride_bytes = 0;
};

// The one predicate every layer uses (wire parser, server, shard, launchers,
// bindings, Python client). n_segments == 1 is the contiguous page and the
// stride is ignored. Plain pages take any segment size and stride; the
// transforming kernels move whole 8- (fp8) or 32-element (mxfp4) groups of
// 16-byte accesses, so a segment is a multiple of the codec's page multiple
// and the stride keeps every segment 16-byte aligned.
inline bool segments_legal(PageCodec c, size_t page_bytes, uint64_t n_segments,
                           uint64_t stride_bytes) {
    if (n_segments < 1 || n_segments > kMaxPageSegments) return false;
    if (page_bytes % n_segments != 0) return false;
    if (n_segments == 1) return true;
    const size_t seg = page_bytes / n_segments;
    if (seg == 0 || stride_bytes < seg) return false;  // segments never overlap
    if (page_codec_transforms(c)) {
        if (seg % page_codec_info(c).page_multiple != 0) return false;
        if (stride_bytes % 16 != 0) return false;
    }
    return true;
}

// Tensor sets (docs/design.md, "tensor sets"): on the CLIENT side of one
// request a page may span n_tensors tensors, an equal part of the page in each
// and every part at the SAME byte offset inside its own tensor. A part may
// itself be segmented: with n_segments segments in the whole page, segment s
// lives at base[s / (S/G)] + offset + (s % (S/G)) * stride_bytes. The stored
// block is still that of the concatenation. The bound is a condition, not a
// tuning value: the table of bases is 1 KiB, and the largest current open
// models have 126 layers. kMaxPageSegments still bounds the total S.
constexpr uint32_t kMaxPageTensors = 128;

// The one predicate for a page over a tensor set, used by every layer as
// segments_legal is. n_segments is the TOTAL over all tensors. With one
// segment per tensor (S/G == 1) no stride is ever applied, so it is ignored;
// the whole page otherwise obeys segments_legal.
inline bool tensors_legal(PageCodec c, size_t page_bytes, uint64_t n_segments,
                          uint64_t stride_bytes, uint64_t n_tensors) {
    if (n_tensors < 1 || n_tensors > kMaxPageTensors) return false;
    if (n_segments < 1 || n_segments % n_tensors != 0) return false;
    // A stride that is never applied stands in as the segment's own size,
    // which segments_legal accepts exactly when the segment itself is legal.
    if (n_segments == n_tensors) stride_bytes = page_bytes / n_segments;
    return segments_legal(c, page_bytes, n_segments, stride_bytes);
}

// Sliced reads (docs/design.md, "sliced reads"): on the POOL side of a read a
// request may take n equal pieces of the stored page, piece p starting at
// logical byte offset + p * stride; the client receives their concatenation,
// the sliced page, and client-side PageSegments apply to it as to a whole
// page. All values are LOGICAL (bf16) bytes for every codec; mapping them to
// stored bytes is the kernels' business. The bound is a condition, not a
// tuning value: with at most 16384 descriptors per launch it keeps every grid
// below 2^31 workgroups.
constexpr uint32_t kMaxSlicePieces = 4096;

// Pool-side geometry of a READ; n == 0 (the default) is the whole page.
struct PageSlice {
    uint32_t n = 0;            // pieces
    uint64_t page_bytes = 0;   // logical size of the page the key was WRITTEN with
    uint64_t offset = 0;       // logical byte of piece 0 inside that page
    uint64_t piece_bytes = 0;  // logical size of one piece
    uint64_t stride = 0;      // logical bytes between pieces (ignored for n == 1)
};

// The one predicate for a slice (wire parser, server, shard, launcher,
// bindings, Python client); a whole-page read (n == 0) never comes here.
// Pieces never overlap and never leave the written page. A transforming
// kernel moves whole 8-element lane units and, for mxfp4, whole 32-element
// groups: offset, piece and stride are multiples of the codec's page
// multiple. A piece never straddles a client segment (n % S == 0), and the
// sliced page obeys segments_legal like any other page.
inline bool slice_legal(PageCodec c, const PageSlice& sl, const PageSegments& seg = {}) {
    if (sl.n < 1 || sl.n > kMaxSlicePieces) return false;
    if (sl.piece_bytes == 0) return false;
    const bool many = sl.n > 1;
    if (many && sl.stride < sl.piece_bytes) return false;
    // offset + (n - 1) * stride + piece_bytes <= page_bytes, without overflow
    if (sl.piece_bytes > sl.page_bytes) return false;
    uint64_t room = sl.page_bytes - sl.piece_bytes;
    if (sl.offset > room) return false;
    room -= sl.offset;
    if (many && sl.stride > room / (sl.n - 1)) return false;
    if (page_codec_transforms(c)) {
        const uint32_t m = page_codec_info(c).page_multiple;
        if (!page_legal(c, sl.page_bytes)) return false;
        if (sl.offset % m != 0 || sl.piece_bytes % m != 0) return false;
        if (many && sl.stride % m != 0) return false;
    }
    if (seg.n != 1) {
        if (seg.n == 0 || sl.n % seg.n != 0) return false;
        // n * piece_bytes <= page_bytes here, so the product cannot overflow
        if (!segments_legal(c, sl.n * sl.piece_bytes, seg.n, seg.stride_bytes)) return false;
    }
    return true;
}

// Does the request carry a slice at all?
inline bool slice_is_set(const PageSlice& sl) { return sl.n != 0; }

// The slice as the wire extension carries it, and back.
inline PackedLocalSliceExt slice_to_wire(const PageSlice& sl) {
    return {sl.n, 0, sl.page_bytes, sl.offset, sl.piece_bytes, sl.stride};
}
inline PageSlice slice_from_wire(const PackedLocalSliceExt& e) {
    return {e.n_pieces, e.page_bytes, e.offset, e.piece_bytes, e.stride};
}

}  // namespace ifs
