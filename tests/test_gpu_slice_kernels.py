"""The four sliced-load kernels, launched directly (`_dbg_load_sliced` calls
gpu::launch_load_sliced with pinned descriptors, as the shard does), at the
edges of their lane mapping.

Every comparison is bit for bit against the reference decode of the WHOLE
stored block (`_kernel_refs.fp8_dequant_ref`, `_mxfp4_refs.dequant_ref`; the
stored bytes themselves for plain pages), sliced afterwards with numpy. The
references are computed once per module for 64 KiB pages; a smaller page is a
prefix of them (every codec decodes element by element, fp8 with the block's
one scale). Stored blocks sit in a guarded `Region`, client pages in a guarded
`SegArena`; after each launch the whole stored tensor must be unchanged and
every client byte outside the pieces still sentinel.

Lane mapping under test (csrc/gpu/gpu.hip, "sliced reads"): L is the smallest
power of two >= units per piece, capped at the 512-thread workgroup; a
workgroup covers 512 / L pieces per step; chunks per block =
min(ceil(4096 / descriptors), steps)."""

import functools

import numpy as np
import pytest
import torch

from infinistore_amd import _native

from _kernel_refs import Region, SENTINEL, fp8_dequant_ref, bf16_bits, assert_bf16_bits_equal
from _seg_refs import SegArena
import _mxfp4_refs as mx

pytestmark = pytest.mark.gpu

NONE, FP8, MXFP4 = 0, 1, 2
THREADS = 512
MAX_PAGE = 64 << 10  # logical bytes
ELEMS = MAX_PAGE // 2
N_DISTINCT = 5
# kind -> (codec, bytes per lane unit, bytes every slice value is a multiple of)
KINDS = {"vec": (NONE, 16, 16), "byte": (NONE, 1, 1), "fp8": (FP8, 16, 16),
         "mxfp4": (MXFP4, 16, 64)}


def test_constants():
    assert _native._SLICE_THREADS == THREADS


# --- stored blocks and their whole-page decode, once per module --------------
@functools.lru_cache(maxsize=None)
def master(codec):
    """(stored_of(page_bytes) -> (N_DISTINCT, stored) uint8, logical (N_DISTINCT,
    MAX_PAGE) uint8, scales)."""
    rs = np.random.RandomState(40 + codec)
    if codec == NONE:
        data = rs.randint(0, 256, (N_DISTINCT, MAX_PAGE), dtype=np.uint8)
        return (lambda page: data[:, :page]), data, [0.0] * N_DISTINCT
    if codec == FP8:
        codes = rs.randint(0, 256, (N_DISTINCT, ELEMS), dtype=np.uint8)
        # NaN (both signs) and +-448 in every block, also in the last unit
        for pos, c in ((3, 0x7F), (9, 0xFF), (17, 0x7E), (26, 0xFE),
                       (ELEMS - 1, 0x7F), (ELEMS - 2, 0xFE), (ELEMS - 8, 0x7E)):
            codes[:, pos] = c
        scales = np.array([1.0, 0.03125, 2.5e-3, 317.0, 7.7e-9], dtype=np.float32)
        want = bf16_bits(fp8_dequant_ref(torch.from_numpy(codes), scales))
        logical = np.ascontiguousarray(want).view(np.uint8).reshape(N_DISTINCT, MAX_PAGE)
        return (lambda page: codes[:, :page // 2]), logical, [float(s) for s in scales]
    packed = rs.randint(0, 256, (N_DISTINCT, ELEMS // 2), dtype=np.uint8)
    E = rs.randint(1, 251, (N_DISTINCT, ELEMS // mx.GROUP)).astype(np.uint8)
    E[:, 5] = mx.E_NAN  # groups with the NaN scale: early, in the middle ...
    E[:, 517] = mx.E_NAN
    E[1::2, -1] = mx.E_NAN  # ... and the page's last group, in every other block
    blocks = np.concatenate([packed, E], axis=1)
    want = mx.dequant_ref(blocks, ELEMS)
    logical = np.ascontiguousarray(want).view(np.uint8).reshape(N_DISTINCT, MAX_PAGE)

    def stored_of(page):
        pe = page // 2
        return np.concatenate([packed[:, :pe // 2], E[:, :pe // mx.GROUP]], axis=1)

    return stored_of, logical, [0.0] * N_DISTINCT


def lanes_per_piece(units):
    L = 1
    while L < units and L < THREADS:
        L *= 2
    return L


def run(kind, geo, *, S=1, arrangement="gapped", n_desc=N_DISTINCT, misalign=0, gap=48,
        expect_ok=True):
    """One launch. geo = (n, page_bytes, offset, piece_bytes, stride). The
    descriptor list cycles through N_DISTINCT blocks n_desc times over."""
    codec = KINDS[kind][0]
    n, page, offset, piece, stride = geo
    stored_of, logical, scales = master(codec)
    what = f"{kind} geo={geo} S={S} n_desc={n_desc} misalign={misalign}"
    # every piece inside the written page, checked before anything is launched
    assert page <= MAX_PAGE and offset + (n - 1) * stride + piece <= page, what
    blocks = stored_of(page)
    nb = min(n_desc, N_DISTINCT)
    stored = Region(nb, blocks.shape[1], fill="sentinel", seed=n + piece)
    stored.set_blocks(torch.from_numpy(np.ascontiguousarray(blocks[:nb])))
    before = stored.t.clone()
    sliced = n * piece
    assert sliced % S == 0
    client = SegArena(nb, S, sliced // S, arrangement, misalign=misalign, gap=gap,
                      seed=piece + n)
    ids = [i % nb for i in range(n_desc)]
    ok = _native._dbg_load_sliced(codec, [stored.ptrs[i] for i in ids],
                                  [client.ptrs[i] for i in ids], [scales[i] for i in ids],
                                  geo, S, client.stride if S > 1 else 0, 0)
    torch.cuda.synchronize()
    assert torch.equal(stored.t, before), "the stored side was written"
    if not expect_ok:
        assert ok is False, what
        assert client.untouched(), what + ": a refused launch wrote"
        return
    assert ok is True, what
    idx = (offset + np.arange(n)[:, None] * stride + np.arange(piece)[None, :]).reshape(-1)
    want = logical[:nb][:, idx]
    got = client.pages().cpu().numpy()
    if codec == NONE:
        assert np.array_equal(got, want), what
    else:
        assert_bf16_bits_equal(np.ascontiguousarray(got).view(np.uint16),
                               np.ascontiguousarray(want).view(np.uint16), what)
    assert client.guards_intact(), what + ": bytes outside the pieces were written"


def legal_page(end, m):
    """Smallest legal page (a multiple of 64 covers every codec) holding `end`."""
    return -(-max(end, 64) // 64) * 64


def geometries(n, piece, m):
    """The geometry variants of one (count, piece): offset 0 with stride ==
    piece; a non-zero offset and a gap, the slice ending on the page's last
    byte; a stride much larger than the piece. Each (n, page, off, piece, stride)."""
    out = [(n, legal_page(n * piece, m) + 64, 0, piece, piece)]
    gap = piece + 3 * m
    span = (n - 1) * gap + piece
    page = legal_page(span + 5 * m, m)
    if page <= MAX_PAGE:
        out.append((n, page, page - span, piece, gap))
    wide = 8 * piece + m
    if (n - 1) * wide + piece + 2 * m <= MAX_PAGE:
        out.append((n, legal_page((n - 1) * wide + piece + 2 * m, m), 2 * m, piece, wide))
    return out


PIECE_UNITS = {"vec": [1, 3, 63, 64, 65, 512, 513], "byte": [1, 3, 63, 64, 65, 512, 513],
               "fp8": [1, 3, 63, 64, 65, 512, 513],
               # whole 32-element groups: multiples of 4 lane units
               "mxfp4": [4, 12, 60, 64, 68, 512, 516]}


@pytest.mark.parametrize("kind,units", [(k, u) for k in KINDS for u in PIECE_UNITS[k]])
def test_lane_mapping_edges(kind, units):
    _, unit, m = KINDS[kind]
    piece = units * unit
    per_step = THREADS // lanes_per_piece(units)
    counts = sorted({1, per_step - 1, per_step, per_step + 1} - {0})
    for n in counts:
        if n * piece > MAX_PAGE - 192:
            continue
        geos = geometries(n, piece, m)
        assert geos[0][2] == 0 and geos[0][4] == piece
        for geo in geos:
            if kind == "byte":  # an odd offset keeps the plain pages on the byte kernel
                n_, page, off, p_, st = geo
                geo = (n_, page + 1, off + 1, p_, st)
            run(kind, geo)


@pytest.mark.parametrize("kind", list(KINDS))
def test_workgroups_that_loop_and_that_do_not(kind):
    """65-unit pieces (68 for mxfp4): L = 128, four pieces per step. The
    descriptor list repeats five small blocks (identical copies land on
    identical bytes), so the grid edges are reached with a few KiB of data."""
    _, unit, m = KINDS[kind]
    units = 68 if kind == "mxfp4" else 65
    piece = units * unit
    odd = 1 if kind == "byte" else 0
    # 57 pieces: 15 steps. 5 descriptors: chunks = 15, one step per workgroup.
    tight = (57, legal_page(57 * piece + 64, m), odd, piece, piece)
    run(kind, tight, n_desc=5)
    # 400 descriptors: chunks = ceil(4096 / 400) = 11 < 15: some workgroups take two steps
    run(kind, tight, n_desc=400)
    # 4100 descriptors exceed the workgroup target: chunks = 1, one workgroup
    # walks all three steps of its block (9 pieces)
    run(kind, (9, legal_page(9 * piece + 64, m), odd, piece, piece), n_desc=4100)


@pytest.mark.parametrize("which", ["client", "offset", "piece", "stride"])
def test_byte_kernel_each_misalignment(which):
    for d in range(1, 16):
        n, off, piece, stride, mis = 6, 32, 48, 80, 0
        if which == "client":
            mis = d
        elif which == "offset":
            off += d
        elif which == "piece":
            piece += d
            stride = 96
        else:
            stride += d
        run("byte", (n, 1024, off, piece, stride), misalign=mis)
    # and with every one of them misaligned at once
    run("byte", (6, 1024, 33, 49, 83), misalign=7)


def test_fp8_eight_byte_aligned_stored_side():
    # offsets of 8 elements (16 logical bytes) put the stored side on 8-byte,
    # not 16-byte, boundaries; so does a stride of an odd number of units
    for off_units in (1, 3, 5):
        run("fp8", (8, 4096, 16 * off_units, 32, 16 * 7))
    # NaN and +-448 codes sit in the first units and in the page's last one
    run("fp8", (2, MAX_PAGE, 0, 64, MAX_PAGE - 64))
    run("fp8", (1, MAX_PAGE, MAX_PAGE - 16, 16, 0))


def test_mxfp4_scale_bytes_far_from_the_first():
    last = MAX_PAGE - 64
    run("mxfp4", (1, MAX_PAGE, last, 64, 0))  # exactly the page's last group (NaN scale)
    run("mxfp4", (4, MAX_PAGE, last - 3 * 4096, 64, 4096))  # ends on the last group
    run("mxfp4", (3, MAX_PAGE, 517 * 64 - 64, 192, 8192))  # around the NaN group 517
    run("mxfp4", (2, MAX_PAGE, 5 * 64, 64, 512 * 64))  # NaN groups 5 and 517
    # a smaller written page: its scale bytes start at page_elems / 2
    run("mxfp4", (4, 8192, 8192 - 4 * 1024, 128, 1024))


@pytest.mark.parametrize("kind", list(KINDS))
def test_client_segments(kind):
    _, unit, m = KINDS[kind]
    T, piece = 4, 4 * m
    odd = 1 if kind == "byte" else 0
    geo = (2 * T, legal_page(2 * T * 4 * piece + 64, m), odd + 0, piece, 4 * piece)
    run(kind, geo, S=2, arrangement="kv_major")  # K pieces, then V a plane further
    run(kind, geo, S=2 * T, arrangement="gapped")  # S == n: every piece its own segment
    run(kind, geo, S=4, arrangement="gapped")
    if kind == "byte":  # a misaligned client stride alone also takes the byte kernel
        run(kind, (8, 4096, 0, 64, 256), S=2, arrangement="gapped", gap=41)


@pytest.mark.parametrize("kind", list(KINDS))
def test_refusals_leave_the_destination_alone(kind):
    _, unit, m = KINDS[kind]
    p = 4 * m
    good = (4, 64 * m, 2 * m, p, 3 * p)
    run(kind, good)
    bad = [
        (0, 64 * m, 0, p, p),  # no pieces
        (4097, 4097 * p, 0, p, p),  # more than kMaxSlicePieces
        (4, 64 * m, 0, 0, p),  # empty pieces
        (4, 64 * m, 0, p, p - m),  # pieces overlap
        (4, 64 * m, 64 * m - (3 * 3 * p + p) + m, p, 3 * p),  # one step past the page
        (4, 3 * 3 * p + p - 1, 0, p, 3 * p),  # the page one byte too small
        (1, 64 * m, 64 * m, p, 0),
    ]
    if KINDS[kind][0] != NONE:  # each value off the codec's multiple, in turn
        bad += [(4, 64 * m, 2 * m + 16 if m == 64 else 2 * m + 8, p, 3 * p),
                (4, 64 * m, 2 * m, p + m // 2, 3 * p),
                (4, 64 * m, 2 * m, p, 3 * p + m // 2)]
    if KINDS[kind][0] != NONE:
        bad.append((4, 64 * m + 8, 2 * m, p, 3 * p))  # not a legal page of the codec
    for geo in bad:
        n, piece = max(geo[0], 1), max(geo[3], 16)
        # build the arenas for a legal twin, then launch the illegal geometry
        codec = KINDS[kind][0]
        stored_of, _, scales = master(codec)
        blocks = stored_of(64 * m)
        stored = Region(2, blocks.shape[1], fill="sentinel")
        stored.set_blocks(torch.from_numpy(np.ascontiguousarray(blocks[:2])))
        client = SegArena(2, 1, min(n, 8) * piece, "gapped")
        ok = _native._dbg_load_sliced(codec, stored.ptrs, client.ptrs, scales[:2], geo, 1, 0, 0)
        torch.cuda.synchronize()
        assert ok is False, (kind, geo)
        assert client.untouched(), (kind, geo)
    # client segments: n % S, and a client stride smaller than a segment
    run(kind, (8, 64 * m, 0, p, 2 * p), S=2, arrangement="kv_major")
    for S, seg_stride in ((3, 1 << 16), (2, 4 * p - m), (0, 1 << 16), (16, 1 << 16)):
        codec = KINDS[kind][0]
        stored_of, _, scales = master(codec)
        blocks = stored_of(64 * m)
        stored = Region(2, blocks.shape[1], fill="sentinel")
        stored.set_blocks(torch.from_numpy(np.ascontiguousarray(blocks[:2])))
        client = SegArena(2, 1, 8 * p, "gapped")
        ok = _native._dbg_load_sliced(codec, stored.ptrs, client.ptrs, scales[:2],
                                      (8, 64 * m, 0, p, 2 * p), S, seg_stride, 0)
        torch.cuda.synchronize()
        assert ok is False and client.untouched(), (kind, S, seg_stride)


@pytest.mark.parametrize("kind", ["fp8", "mxfp4"])
def test_transforming_codec_needs_aligned_client_pointers(kind):
    m = KINDS[kind][2]
    geo = (4, 64 * m, 0, 2 * m, 4 * m)
    run(kind, geo)
    for mis in (1, 2, 4, 8, 15):
        run(kind, geo, misalign=mis, expect_ok=False)
    if kind == "fp8":  # with a segmented client too
        run(kind, geo, S=2, arrangement="gapped", misalign=8, expect_ok=False)


def test_sentinel_is_not_in_the_way():
    # the guards are checked against SENTINEL, so the comparison above is only
    # as good as the data is different from it: no reference page is all 0xA5
    for codec in (NONE, FP8, MXFP4):
        logical = master(codec)[1]
        assert (logical != SENTINEL).mean() > 0.9
