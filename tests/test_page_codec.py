"""The page-codec table (csrc/core/page_codec.h) through its host-only
bindings: stored sizes against the formulas the docs state, the refusals, and
agreement between the native rows and the Python client's quant mapping.
write_pages' own argument checks need a GPU tensor and a local connection:
tests/test_gpu_mxfp4.py::test_write_pages_refusals_are_value_errors."""

import pytest

from infinistore_amd import _native
from infinistore_amd.lib import InfinityConnection

PLAIN, FP8, MXFP4 = 0, 2, 4  # request flags (docs/protocol.md)
PAGES = [16, 64, 131072, 246720]  # bytes; 246720 = 123360 bf16 elements


@pytest.mark.parametrize("page", PAGES)
def test_stored_bytes_match_documented_formulas(page):
    assert _native._dbg_page_codec(PLAIN, page) == (0, page)
    assert _native._dbg_page_codec(FP8, page) == (1, page // 2)
    if page % 64 == 0:
        assert _native._dbg_page_codec(MXFP4, page) == (2, page // 4 + page // 64)
    # the sync-response flag is no codec's business
    assert _native._dbg_page_codec(FP8 | 1, page) == (1, page // 2)


def test_mxfp4_refuses_the_one_page_skipped_above():
    assert [p for p in PAGES if p % 64] == [16]
    with pytest.raises(ValueError):
        _native._dbg_page_codec(MXFP4, 16)


@pytest.mark.parametrize("flags,page", [(FP8, 8), (FP8, 24), (MXFP4, 32), (MXFP4, 96)]
                         + [(FP8 | MXFP4, p) for p in [1] + PAGES])
def test_refusals(flags, page):
    with pytest.raises(ValueError):
        _native._dbg_page_codec(flags, page)


def test_plain_takes_any_page():
    assert _native._dbg_page_codec(PLAIN, 1) == (0, 1)


# The read-size rule (docs/protocol.md, "read sizes"), written out here with
# Python's unbounded integers and without the table: a plain block serves any
# whole-page read up to its own size; an fp8 block holds one byte per bf16
# element; an mxfp4 block holds 17 bytes per 32 elements.
def _matches_rule(codec, stored, page):
    if codec == 0:
        return stored == page
    if codec == 1:
        return 2 * stored == page
    return 64 * stored == 17 * page


def _serves_rule(codec, stored, page):
    return page <= stored if codec == 0 else _matches_rule(codec, stored, page)


U64 = 2 ** 64 - 1
# Pages (bytes): legal for every codec, legal for fp8 only, legal for none of
# the compressed codecs, and the largest values a size_t holds. 2^63 and 2^64-64
# are where a 64-bit product of the size with the codec's ratio wraps.
RULE_PAGES = [1, 2, 16, 64, 1000, 1024, 8256, 246720, 2 ** 32, 2 ** 63 - 64, 2 ** 63,
              U64 - 63, U64 - 1, U64]


def _stored_candidates(codec, page):
    exact = {0: page, 1: page // 2, 2: page // 64 * 17}[codec]
    near = {exact - 1, exact, exact + 1, page - 1, page, page + 1, 0, 2 ** 63, U64}
    # the values at which a wrapped 64-bit compare would falsely agree
    den, num = {0: (1, 1), 1: (2, 1), 2: (64, 17)}[codec]
    near |= {(page * num % 2 ** 64) // den, exact + 2 ** 63, exact + 2 ** 64 // den}
    return sorted(s for s in near if 0 <= s <= U64)


@pytest.mark.parametrize("codec", [0, 1, 2])
def test_read_size_predicates_against_the_written_rule(codec):
    checked = 0
    for page in RULE_PAGES:
        for stored in _stored_candidates(codec, page):
            assert _native._dbg_stored_serves(codec, stored, page) == \
                _serves_rule(codec, stored, page), (codec, stored, page)
            assert _native._dbg_stored_matches(codec, stored, page) == \
                _matches_rule(codec, stored, page), (codec, stored, page)
            checked += 1
    assert checked >= 5 * len(RULE_PAGES)  # candidates coincide for tiny pages


@pytest.mark.parametrize("flags,page", [(PLAIN, 1000), (PLAIN, 16384), (FP8, 1024),
                                        (FP8, 246720), (MXFP4, 1024), (MXFP4, 246720)])
def test_a_written_block_serves_its_own_page_and_no_larger_one(flags, page):
    codec, stored = _native._dbg_page_codec(flags, page)
    assert _native._dbg_stored_serves(codec, stored, page)
    assert not _native._dbg_stored_serves(codec, stored, page + 1)
    assert not _native._dbg_stored_serves(codec, stored, 2 * page)
    assert not _native._dbg_stored_serves(codec, stored - 1, page)
    assert _native._dbg_stored_serves(codec, stored + 1, page) == (codec == 0)
    # only a plain block has a usable prefix
    assert _native._dbg_stored_serves(codec, stored, page - 1) == (codec == 0)
    assert _native._dbg_stored_serves(codec, stored, page // 2) == (codec == 0)


def test_read_size_predicates_refuse_an_unknown_codec():
    for fn in (_native._dbg_stored_serves, _native._dbg_stored_matches):
        with pytest.raises(ValueError):
            fn(3, 16, 16)


def test_python_mapping_agrees_with_native_rows():
    rows = _native._page_codec_rows()
    assert [r[0] for r in rows] == ["none", "fp8", "mxfp4"]
    assert rows[0][1:] == (0, 1)
    assert {name: (flag, mult) for name, flag, mult in rows[1:]} == InfinityConnection.QUANT_MODES
    assert InfinityConnection.FLAG_QUANT_FP8 == FP8
    assert InfinityConnection.FLAG_QUANT_MXFP4 == MXFP4
    for cid, (name, flag, mult) in enumerate(rows):
        # the smallest legal bf16 page of each codec, and one element less
        assert _native._dbg_page_codec(flag, 2 * mult)[0] == cid
        if mult > 1:
            with pytest.raises(ValueError):
                _native._dbg_page_codec(flag, 2 * (mult - 1))
