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
