"""The two mxfp4 kernels of csrc/gpu/gpu.hip at their edge shapes, launched
directly through `_dbg_mxfp4_quant_blocks` / `_dbg_mxfp4_dequant_blocks`
(descriptors in pinned host memory, as the shard does) and compared byte for
byte with the numpy reference (tests/_mxfp4_refs.py). Blocks sit in guarded,
permuted `Region`s: every address is checked on the host before a launch, and
every byte outside the N/2 + N/32 stored bytes must keep its sentinel."""

import numpy as np
import pytest
import torch

from infinistore_amd import _native

from _kernel_refs import SENTINEL, Region, assert_bf16_bits_equal
from _mxfp4_refs import (
    GROUP,
    dequant_ref,
    every_finite_pattern_pages,
    finite_patterns,
    quant_ref,
    special_groups,
    stored_bytes,
)

pytestmark = pytest.mark.gpu

DEV = 0
G = _native._MXFP4_GROUPS_PER_ITER  # groups one workgroup covers per iteration


def _as_blocks(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1))


def run_mxfp4(bits: np.ndarray, what=""):
    """(n, N) uint16 bf16 bits through the quantize kernel, then both the
    kernel-encoded and the reference-encoded blocks through the dequantize
    kernel. Returns the stored blocks (n, N/2 + N/32) uint8."""
    n, N = bits.shape
    sb = stored_bytes(N)
    want_blocks = quant_ref(bits)
    want_bits = dequant_ref(want_blocks, N)

    src = Region(n, 2 * N, fill="sentinel", seed=N)
    src.set_blocks(_as_blocks(bits))
    mid = Region(n, sb, fill="sentinel", seed=N + 1)
    assert all(p % 16 == 0 for p in src.ptrs + mid.ptrs)
    _native._dbg_mxfp4_quant_blocks(src.ptrs, mid.ptrs, N, DEV)
    got_blocks = mid.blocks().cpu().numpy()
    bad = np.argwhere(got_blocks != want_blocks)
    assert bad.size == 0, (
        f"{what}: {len(bad)} stored bytes differ, first block {bad[0][0]} byte {bad[0][1]} "
        f"(codes end at {N // 2}): got {got_blocks[tuple(bad[0])]:#04x} "
        f"want {want_blocks[tuple(bad[0])]:#04x}")
    assert mid.guards_intact(), f"{what}: quantize wrote outside its N/2 + N/32 bytes"
    assert np.array_equal(src.blocks().cpu().numpy().view(np.uint16), bits), \
        f"{what}: quantize modified its source"
    assert src.guards_intact()

    ref_mid = Region(n, sb, fill="sentinel", seed=N + 3)
    ref_mid.set_blocks(torch.from_numpy(want_blocks))
    for enc, name in ((mid, "kernel-encoded"), (ref_mid, "reference-encoded")):
        out = Region(n, 2 * N, fill="sentinel", seed=N + 2)
        _native._dbg_mxfp4_dequant_blocks(enc.ptrs, out.ptrs, N, DEV)
        got = out.blocks().cpu().numpy().view(np.uint16)
        assert_bf16_bits_equal(got, want_bits, f"{what} dequant of {name}")
        assert out.guards_intact(), f"{what}: dequantize wrote outside its blocks"
        assert enc.guards_intact()
    return got_blocks


def random_finite_pages(n, N, seed) -> np.ndarray:
    """Random finite bf16 bit patterns over all exponents; every other page
    instead draws each group from a window of four exponents, so that its
    elements do not all vanish under the group's scale."""
    rs = np.random.RandomState(seed)
    fin = finite_patterns()
    bits = fin[rs.randint(0, fin.size, (n, N))]
    base = rs.randint(0, 0x7F80 - 0x200, (n, N // GROUP, 1))
    windowed = (base + rs.randint(0, 0x200, (n, N // GROUP, GROUP))) | (
        rs.randint(0, 2, (n, N // GROUP, GROUP)) << 15)
    bits[1::2] = windowed.reshape(n, N)[1::2]
    bits = bits.astype(np.uint16)
    assert ((bits & 0x7FFF) < 0x7F80).all()
    return bits


@pytest.mark.parametrize("n_blocks", [1, 3, 17])
@pytest.mark.parametrize("groups", [1, 2, G - 1, G, G + 1, 3 * G + 1])
def test_mxfp4_shapes(groups, n_blocks):
    N = groups * GROUP
    run_mxfp4(random_finite_pages(n_blocks, N, groups * 100 + n_blocks),
              f"groups={groups} n={n_blocks}")


def test_mxfp4_many_one_group_pages():
    """4097 one-group pages: more blocks than the launcher's workgroup
    target, so chunks-per-block clamps to 1."""
    run_mxfp4(random_finite_pages(4097, GROUP, 5), "4097 x 1 group")


def test_mxfp4_every_finite_pattern():
    pages = every_finite_pattern_pages()
    blocks = run_mxfp4(pages, "every finite pattern")
    N = pages.shape[1]
    assert (blocks[:, N // 2:] != 0xFF).all(), "no NaN group among finite values"
    codes = blocks[1, : N // 2]
    seen = set(np.unique(codes & 0xF)) | set(np.unique(codes >> 4))
    assert seen == set(range(16)), "the windowed page reaches every code"


def test_mxfp4_special_groups():
    """The special groups (all zero, all -0, only inf, one NaN, subnormals
    only, largest finite) next to ordinary ones, in two orders."""
    sp = special_groups()
    names = list(sp)
    plain = random_finite_pages(1, 2 * GROUP, 8)[0].reshape(2, GROUP)
    order0 = [sp[k] for k in names] + [plain[0], plain[1]]
    order1 = [plain[1]] + [sp[k] for k in reversed(names)] + [plain[0]]
    pages = np.stack([np.concatenate(order0), np.concatenate(order1)])
    N = pages.shape[1]
    blocks = run_mxfp4(pages, "special groups")
    scales = dict(zip(names, blocks[0, N // 2: N // 2 + len(names)]))
    assert scales == {"all_zero": 127, "all_negative_zero": 127, "only_inf": 127,
                      "one_nan": 0xFF, "subnormals_only": 0, "largest_finite": 252}
    out = dequant_ref(blocks, N)[0].reshape(-1, GROUP)
    assert (out[names.index("all_zero")] == 0).all()
    assert (out[names.index("all_negative_zero")] == 0x8000).all(), "-0 keeps its sign"
    assert ((out[names.index("one_nan")] & 0x7FFF) > 0x7F80).all(), "a NaN group is all NaN"
    inf_mag = out[names.index("only_inf")] & 0x7FFF
    assert (inf_mag == 0x40C0).all(), "inf saturates to +-6 under scale 1"


def test_mxfp4_refusals():
    """Refused on the host before any launch: elems % 32 != 0, a misaligned
    source or destination, mismatched list lengths."""
    N = 64
    pages = Region(3, 2 * N, fill="pattern")
    stored = Region(3, stored_bytes(N), fill="sentinel", seed=1)
    odd_pages = Region(3, 2 * N, misalign=[0, 2, 0], fill="pattern")
    odd_stored = Region(3, stored_bytes(N), misalign=[0, 0, 8], fill="sentinel", seed=1)
    for src, dst, elems in [(pages, stored, 48), (pages, stored, 16), (pages, stored, 0),
                            (odd_pages, stored, N), (pages, odd_stored, N)]:
        with pytest.raises(ValueError):
            _native._dbg_mxfp4_quant_blocks(src.ptrs, dst.ptrs, elems, DEV)
        assert bool((dst.t == SENTINEL).all())
    with pytest.raises(ValueError):
        _native._dbg_mxfp4_quant_blocks(pages.ptrs[:2], stored.ptrs, N, DEV)
    assert bool((stored.t == SENTINEL).all())

    enc = Region(3, stored_bytes(N), fill="pattern", seed=4)
    odd_enc = Region(3, stored_bytes(N), misalign=[4, 0, 0], fill="pattern", seed=4)
    out = Region(3, 2 * N, fill="sentinel", seed=2)
    odd_out = Region(3, 2 * N, misalign=[2, 0, 0], fill="sentinel", seed=2)
    for src, dst, elems in [(enc, out, 48), (enc, out, 16), (enc, out, 0),
                            (odd_enc, out, N), (enc, odd_out, N)]:
        with pytest.raises(ValueError):
            _native._dbg_mxfp4_dequant_blocks(src.ptrs, dst.ptrs, elems, DEV)
        assert bool((dst.t == SENTINEL).all())
    with pytest.raises(ValueError):
        _native._dbg_mxfp4_dequant_blocks(enc.ptrs, out.ptrs[:1], N, DEV)
    assert bool((out.t == SENTINEL).all())
