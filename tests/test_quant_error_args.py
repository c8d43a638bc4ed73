"""quant_error's argument checks that need no launch, hence no GPU: they run
before the device is looked at, on CPU tensors."""

import pytest
import torch

import infinistore_amd as ifs
from infinistore_amd import _native

BF16 = torch.zeros(4096, dtype=torch.bfloat16)
QUANTS = list(ifs.InfinityConnection.QUANT_MODES)


@pytest.mark.parametrize("quant", [None, "int8", "FP8"])
def test_unknown_quant(quant):
    assert ifs.QuantErrorFields() == tuple(range(_native._QUANT_ERROR_FIELDS))
    with pytest.raises(ValueError, match="quant"):
        ifs.quant_error(BF16, [0], 64, quant)


@pytest.mark.parametrize("quant", QUANTS)
@pytest.mark.parametrize("kw, why", [
    (dict(cache=BF16.float(), offsets=[0], page_size=64), "bf16"),
    (dict(cache=BF16.reshape(64, 64).t(), offsets=[0], page_size=64), "contiguous"),
    (dict(cache=BF16, offsets=[0], page_size=64, tensors=[BF16]), "either"),
    (dict(cache=None, offsets=[0], page_size=64), "either"),
    (dict(cache=None, offsets=[0], page_size=32 * 129, tensors=[BF16] * 129), "tensors"),
    (dict(cache=BF16, offsets=[4096 - 32], page_size=64), "outside"),
    (dict(cache=BF16, offsets=[0], page_size=4096, segments=2, segment_stride=2064), "outside"),
    (dict(cache=None, offsets=[2048], page_size=64, tensors=[BF16, BF16[:2048]]), "outside"),
])
def test_refused_before_any_launch(quant, kw, why):
    with pytest.raises(ValueError, match=why):
        ifs.quant_error(quant=quant, **kw)


@pytest.mark.parametrize("quant", QUANTS)
def test_page_multiples_are_the_codec_table_rows(quant):
    """A page size passes the geometry checks (and reaches the device check)
    exactly when it is a multiple of the codec row's."""
    multiple = {name: m for name, _flag, m in _native._page_codec_rows()}[quant]
    for page in range(0, 4 * multiple + 1):
        with pytest.raises(ValueError) as e:
            ifs.quant_error(BF16, [0], page, quant)
        assert ("CUDA" in str(e.value)) == (page > 0 and page % multiple == 0), (page, e.value)
