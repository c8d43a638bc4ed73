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

// Permuted pages (docs/design.md, "permuted pages"): on the CLIENT side of a
// request a page may hold its pieces in the other order of two axes. A page is
// outer * rows * cols pieces of piece_bytes LOGICAL bytes; piece (o, r, c)
// starts at logical byte ((o*rows + r)*cols + c) * piece_bytes of the STORED
// (canonical) page and at ((o*cols + c)*rows + r) * piece_bytes of the client
// page, to which PageSegments then apply as to any page. For a KV block,
// outer = 2, rows = T, cols = H and the piece is one head of one token: the
// store keeps [2, T, H, hd] whether the engine's cache is that or [2, H, T, hd].
// The bound is a condition, not a tuning value: it keeps every piece index,
// and the products of two of them that the kernels form, inside 32 bits.
constexpr uint32_t kMaxPermPieces = 1u << 20;

// Client-side piece order of a request's pages; rows == 0 (the default) is
// "not permuted".
struct PagePermute {
    uint32_t outer = 0, rows = 0, cols = 0;
    uint64_t piece_bytes = 0;
};

inline bool permute_is_set(const PagePermute& p) { return p.rows != 0; }

// The one predicate for a permuted page (wire parser, server, shard,
// launchers, bindings, Python client). The pieces tile the page exactly. A
// transforming kernel moves whole 8-element lane units and, for mxfp4, whole
// 32-element groups: the piece is a multiple of the codec's page multiple. A
// piece never straddles a client segment, and the page obeys segments_legal
// like any other. rows == 1 or cols == 1 is legal: it is the identity.
inline bool permute_legal(PageCodec c, size_t page_bytes, const PagePermute& p,
                          const PageSegments& seg = {}) {
    if (p.outer < 1 || p.rows < 1 || p.cols < 1 || p.piece_bytes == 0) return false;
    // 128-bit products: three 32-bit counts and a 64-bit size off the wire
    // must not wrap into a match.
    using u128 = unsigned __int128;
    const u128 pieces = static_cast<u128>(p.outer) * p.rows * p.cols;
    if (pieces > kMaxPermPieces) return false;
    if (pieces * p.piece_bytes != static_cast<u128>(page_bytes)) return false;
    if (page_codec_transforms(c) && p.piece_bytes % page_codec_info(c).page_multiple != 0)
        return false;
    if (seg.n != 1) {
        if (seg.n == 0 || static_cast<uint64_t>(pieces) % seg.n != 0) return false;
        if (!segments_legal(c, page_bytes, seg.n, seg.stride_bytes)) return false;
    }
    return true;
}

// The geometry as the wire extension carries it, and back.
inline PackedLocalPermExt permute_to_wire(const PagePermute& p) {
    return {p.outer, p.rows, p.cols, 0, p.piece_bytes};
}
inline PagePermute permute_from_wire(const PackedLocalPermExt& e) {
    return {e.outer, e.rows, e.cols, e.piece_bytes};
}

// Transposed pages (docs/design.md, "transposed pages"): on the CLIENT side of
// a request a page may be the classic paged-attention cache block. A page is
// outer (1 or 2) halves of tokens x heads x cols elements of elem_bytes; with
// T, H, C those extents and x_o = inner[o], element (o, t, h, c) sits at
// element ((o*T + t)*H + h)*C + c of the STORED (canonical) page and at
// (((o*H + h)*(C/x_o) + c/x_o)*T + t)*x_o + c%x_o of the client page, to which
// PageSegments then apply as to any page. K of a paged-attention block is
// x_0 = 16 / elem_bytes ([H, hd/x, T, x]) and V is x_1 = 1 ([H, hd, T]). The
// bound is a condition, not a tuning value: one (o, h) tile of T x C elements
// is what a workgroup holds in LDS, with room for further resident workgroups.
constexpr uint32_t kMaxTransposeTile = 32u << 10;

// Client-side element order of a request's pages; tokens == 0 (the default)
// is "not transposed".
struct PageTranspose {
    uint32_t outer = 0, tokens = 0, heads = 0, cols = 0, elem_bytes = 0;
    uint32_t inner[2] = {0, 0};
};

inline bool transpose_is_set(const PageTranspose& x) { return x.tokens != 0; }

// The one predicate for a transposed page (wire parser, server, shard,
// launchers, bindings, Python client). Both sides move in 16-byte units: a
// client run of x_o elements is at most one unit and T runs fill whole units,
// a stored (token, head) row is whole units and, under a transforming codec
// (bf16 only), whole groups of the codec, so an mxfp4 group never leaves its
// row. Both x_o are checked whatever outer is. A tile never straddles a client
// segment, and the page obeys segments_legal like any other.
inline bool transpose_legal(PageCodec c, size_t page_bytes, const PageTranspose& x,
                            const PageSegments& seg = {}) {
    if (x.outer < 1 || x.outer > 2 || x.tokens < 1 || x.heads < 1 || x.cols < 1) return false;
    if (x.elem_bytes != 1 && x.elem_bytes != 2 && x.elem_bytes != 4) return false;
    if (page_codec_transforms(c) && x.elem_bytes != kPageElemBytes) return false;
    for (uint32_t xo : x.inner) {
        if (xo == 0 || (xo & (xo - 1)) != 0 || xo > 16 || x.cols % xo != 0) return false;
        if (xo * x.elem_bytes > 16) return false;
        if (x.tokens % (16 / (xo * x.elem_bytes)) != 0) return false;
    }
    const uint64_t row = static_cast<uint64_t>(x.cols) * x.elem_bytes;
    if (row % 16 != 0 || row % page_codec_info(c).page_multiple != 0) return false;
    // 128-bit products: five 32-bit values off the wire must not wrap into a match.
    using u128 = unsigned __int128;
    if (static_cast<u128>(x.outer) * x.tokens * x.heads * row != static_cast<u128>(page_bytes))
        return false;
    if (static_cast<u128>(x.tokens) * row > kMaxTransposeTile) return false;
    if (seg.n != 1) {
        if (seg.n == 0 || (static_cast<uint64_t>(x.outer) * x.heads) % seg.n != 0) return false;
        if (!segments_legal(c, page_bytes, seg.n, seg.stride_bytes)) return false;
    }
    return true;
}

// The geometry as the wire extension carries it, and back.
inline PackedLocalXposeExt transpose_to_wire(const PageTranspose& x) {
    return {x.outer, x.tokens, x.heads, x.cols, x.elem_bytes, x.inner[0], x.inner[1], 0};
}
inline PageTranspose transpose_from_wire(const PackedLocalXposeExt& e) {
    return {e.outer, e.tokens, e.heads, e.cols, e.elem_bytes, {e.inner_k, e.inner_v}};
}

// Cast pages (docs/design.md, "cast pages"): on the CLIENT side of a request a
// page may hold one-byte OCP e4m3fn codes instead of bf16, element value =
// code value * scale[h], h being the half (of `halves`, 1 or 2: K and V) the
// element lies in. The logical page stays the bf16 page: page_bytes, the
// header's block_size and every stored block are what a bf16 writer holding
// the dequantized values has, and the client page is page_bytes / 2 bytes.
// PageSegments apply to the CLIENT page: the segments are equal parts of its
// bytes and the stride is in client bytes.
constexpr uint32_t kCastE4m3 = 1;

// Client-side element type of a request's pages; elem_type == 0 (the default)
// is "not cast".
struct PageCast {
    uint32_t elem_type = 0;
    uint32_t halves = 0;
    float scale[2] = {0.f, 0.f};
};

inline bool cast_is_set(const PageCast& c) { return c.elem_type != 0; }

// A scale is a finite, positive, normal float32 (judged on its bits, so no
// denormal mode bends it).
inline bool cast_scale_legal(float s) {
    const uint32_t u = __builtin_bit_cast(uint32_t, s);
    return u >= 0x00800000u && u < 0x7f800000u;
}

// The one predicate for a cast page (wire parser, server, shard, launchers,
// bindings, Python client). The kernels move 8-element lane units (8 client
// bytes, 16 bf16 bytes) and, under mxfp4, 32-element groups: neither
// straddles a half or a client segment. With halves == 1 the second scale is
// still carried and still judged. The stride keeps every client segment
// 16-byte aligned; it and the segment size are CLIENT bytes.
inline bool cast_legal(PageCodec c, size_t page_bytes, const PageCast& cast,
                       const PageSegments& seg = {}) {
    if (cast.elem_type != kCastE4m3) return false;
    if (cast.halves != 1 && cast.halves != 2) return false;
    if (!cast_scale_legal(cast.scale[0]) || !cast_scale_legal(cast.scale[1])) return false;
    if (page_bytes == 0 || page_bytes % kPageElemBytes != 0 || !page_legal(c, page_bytes))
        return false;
    const uint64_t elems = page_bytes / kPageElemBytes;  // = client bytes
    const uint64_t unit = c == PageCodec::kMxfp4 ? 32 : 8;
    if (elems % cast.halves != 0 || (elems / cast.halves) % unit != 0) return false;
    if (seg.n < 1 || seg.n > kMaxPageSegments) return false;
    if (seg.n > 1) {
        if (elems % seg.n != 0) return false;
        const uint64_t cseg = elems / seg.n;
        if (cseg % unit != 0) return false;
        if (seg.stride_bytes < cseg || seg.stride_bytes % 16 != 0) return false;
    }
    return true;
}

// The cast as the wire extension carries it, and back.
inline PackedLocalCastExt cast_to_wire(const PageCast& c) {
    return {c.elem_type, c.halves, {c.scale[0], c.scale[1]}};
}
inline PageCast cast_from_wire(const PackedLocalCastExt& e) {
    return {e.elem_type, e.halves, {e.scale[0], e.scale[1]}};
}

// Rotated reads (docs/design.md, "rotated reads"): a READ may shift the rotary
// position embedding of the keys it loads. The page is [halves, T, heads,
// head_dim] bf16, T implied by the page size; half 0 (K) is rotated, half 1
// (V) is copied. With P = rot_dim / 2 pairs per head and (cos_i, sin_i) =
// table[2i], table[2i + 1], pair i of every (token, head) row is channels
// (i, i + P) under style 1 (NeoX halves) and (2i, 2i + 1) under style 2 (GPT-J
// interleaved); channels at or above rot_dim are copied (partial rotary). For
// a pair (a, b) of decoded bf16 values, in float32,
//     out_a = fma(a, cos, -(b * sin)),  out_b = fma(b, cos, a * sin),
// each rounded to bf16 (gpu/rotate_math.h). The bound is a condition, not a
// tuning value: the table is 1 KiB, as the tensor-set table is.
constexpr uint32_t kMaxRotatePairs = 128;
constexpr uint32_t kRotateNeox = 1, kRotateGptj = 2;

// Read-side rotation of a request's pages; style == 0 (the default) is "not
// rotated". table points at rot_dim floats in host memory that outlive the
// struct's use; Shard::CopyJob keeps its own copy.
struct PageRotate {
    uint32_t style = 0;
    uint32_t halves = 0;
    uint32_t heads = 0, head_dim = 0, rot_dim = 0;  // elements
    const float* table = nullptr;
};

inline bool rotate_is_set(const PageRotate& r) { return r.style != 0; }

// The one predicate for a rotated read (wire parser, server, shard, launcher,
// bindings, Python client). The kernels move 8-element lane units and, under
// mxfp4, decode whole 32-element groups: a unit never holds both rotated and
// copied channels, never half a pair and never parts of two heads, so
// head_dim is a multiple of 8 under both styles. A client segment holds whole
// (token, head) rows, and its stride keeps every unit 16-byte aligned under
// every codec, because there is no byte path. Every table entry is finite
// (judged on its bits).
inline bool rotate_legal(PageCodec c, size_t page_bytes, const PageRotate& r,
                         const PageSegments& seg = {}) {
    if (r.style != kRotateNeox && r.style != kRotateGptj) return false;
    if (r.halves != 1 && r.halves != 2) return false;
    if (r.heads < 1 || r.head_dim < 1 || r.rot_dim < 1 || r.rot_dim > r.head_dim) return false;
    if (r.rot_dim % 2 != 0) return false;
    const uint32_t pairs = r.rot_dim / 2;
    if (pairs > kMaxRotatePairs) return false;
    if (r.head_dim % 8 != 0) return false;
    if (r.style == kRotateNeox ? pairs % 8 != 0 : r.rot_dim % 8 != 0) return false;
    if (c == PageCodec::kMxfp4) {
        if (r.head_dim % 32 != 0 || r.rot_dim % 32 != 0) return false;
        if (r.style == kRotateNeox && pairs % 32 != 0) return false;
    }
    // 128-bit products: three 32-bit values off the wire must not wrap.
    using u128 = unsigned __int128;
    const u128 row = static_cast<u128>(r.head_dim) * kPageElemBytes;
    const u128 token = row * r.halves * r.heads;
    if (page_bytes == 0 || static_cast<u128>(page_bytes) % token != 0) return false;
    if (!page_legal(c, page_bytes)) return false;
    if (!segments_legal(c, page_bytes, seg.n, seg.stride_bytes)) return false;
    if (seg.n > 1) {
        if (static_cast<u128>(page_bytes / seg.n) % row != 0) return false;
        if (seg.stride_bytes % 16 != 0) return false;
    }
    if (!r.table) return false;
    for (uint32_t i = 0; i < r.rot_dim; i++)
        if ((__builtin_bit_cast(uint32_t, r.table[i]) & 0x7f800000u) == 0x7f800000u) return false;
    return true;
}

// The geometry as the wire extension carries it, and back; the table travels
// behind the extension.
inline PackedLocalRotExt rotate_to_wire(const PageRotate& r) {
    return {r.style, r.halves, r.heads, r.head_dim, r.rot_dim, 0};
}
inline PageRotate rotate_from_wire(const PackedLocalRotExt& e, const float* table) {
    return {e.style, e.halves, e.heads, e.head_dim, e.rot_dim, table};
}

// Shuffled pages (docs/design.md, "shuffled pages"): on the CLIENT side of a
// request a page may be the shuffled cache block that assembly paged-attention
// kernels read. A page is outer (1 or 2) halves of tokens x heads x cols
// elements of elem_bytes; with T, H, C those extents and X = 16 / elem_bytes,
// element (o, t, h, c) sits at element ((o*T + t)*H + h)*C + c of the STORED
// (canonical) page and, on the client, in tile o*H + h of T*C elements at
//     form 1 (K, [C/X, T, X]):  ((c/X)*T + t)*X + c%X
//     form 2 (V, [T/X, C, X]):  ((t/X)*C + c)*X + t%X
// to which PageSegments then apply as to any page. A SQUARE is X tokens x X
// channels: X 16-byte units of X consecutive stored rows, and X*16 contiguous
// client bytes, held as they are under form 1 and transposed under form 2.

// Client-side element order of a request's pages; tokens == 0 (the default)
// is "not shuffled". form[o] is half o's form; a one-half page uses form[0].
struct PageShuffle {
    uint32_t outer = 0, tokens = 0, heads = 0, cols = 0, elem_bytes = 0;
    uint32_t form[2] = {0, 0};
};

inline bool shuffle_is_set(const PageShuffle& x) { return x.tokens != 0; }

// The one predicate for a shuffled page (wire parser, server, shard,
// launchers, bindings, Python client). Whole squares tile every (half, head)
// tile; under a transforming codec the elements are bf16 and, for mxfp4, a
// (token, head) row is whole 32-element groups, so a group never leaves its
// row. Both forms are judged whatever outer is. The two bounds are conditions,
// not tuning values: the kernels count the squares of a tile and the tiles of
// a page in 32 bits. A tile never straddles a client segment, and the page
// obeys segments_legal like any other. There is no bound on the tile's size.
inline bool shuffle_legal(PageCodec c, size_t page_bytes, const PageShuffle& x,
                          const PageSegments& seg = {}) {
    if (x.outer < 1 || x.outer > 2 || x.tokens < 1 || x.heads < 1 || x.cols < 1) return false;
    if (x.elem_bytes != 1 && x.elem_bytes != 2 && x.elem_bytes != 4) return false;
    if (page_codec_transforms(c) && x.elem_bytes != kPageElemBytes) return false;
    for (uint32_t f : x.form)
        if (f != 1 && f != 2) return false;
    const uint32_t X = 16 / x.elem_bytes;
    if (x.tokens % X != 0 || x.cols % X != 0) return false;
    if (c == PageCodec::kMxfp4 && x.cols % 32 != 0) return false;
    // 128-bit products: five 32-bit values off the wire must not wrap into a match.
    using u128 = unsigned __int128;
    if (static_cast<u128>(x.outer) * x.tokens * x.heads * x.cols * x.elem_bytes !=
        static_cast<u128>(page_bytes))
        return false;
    if (static_cast<uint64_t>(x.tokens / X) * (x.cols / X) > 0xffffffffull) return false;
    if (static_cast<uint64_t>(x.outer) * x.heads > 0xffffffffull) return false;
    if (seg.n == 0 || (static_cast<uint64_t>(x.outer) * x.heads) % seg.n != 0) return false;
    return segments_legal(c, page_bytes, seg.n, seg.stride_bytes);
}

// The geometry as the wire extension carries it, and back.
inline PackedLocalShufExt shuffle_to_wire(const PageShuffle& x) {
    return {x.outer, x.tokens, x.heads, x.cols, x.elem_bytes, x.form[0], x.form[1], 0};
}
inline PageShuffle shuffle_from_wire(const PackedLocalShufExt& e) {
    return {e.outer, e.tokens, e.heads, e.cols, e.elem_bytes, {e.form_k, e.form_v}};
}

}  // namespace ifs
