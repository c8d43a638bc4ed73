"""References and helpers shared by the kernel tests (plain module, no
fixtures): the pure-Python fingerprint, a torch/numpy fp8 page codec that
follows the rules in docs/design.md ("fp8 page codec"), and a guarded block
arena for launching kernels on exactly known, bounds-checked addresses."""

import numpy as np
import torch

M64 = (1 << 64) - 1


# --- fingerprint -----------------------------------------------------------
def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def fingerprint_ref(data: bytes, block_size: int):
    """Pure-Python reference of the hash_blocks kernel: one fingerprint per
    `block_size` bytes of `data`."""
    out = []
    for b0 in range(0, len(data), block_size):
        blk = data[b0 : b0 + block_size]
        h = 0
        nw = len(blk) // 8
        for i in range(nw):
            w = int.from_bytes(blk[i * 8 : i * 8 + 8], "little")
            h ^= mix64(w ^ ((i * 0xFF51AFD7ED558CCD) & M64))
        tb = len(blk) - nw * 8
        if tb:
            tail = int.from_bytes(blk[nw * 8 :], "little")
            h ^= mix64(tail ^ ((nw * 0xFF51AFD7ED558CCD) & M64))
        out.append(mix64(h ^ block_size))
    return out


# --- fp8 page codec ----------------------------------------------------------
FP8_MAX = 448.0
MIN_SCALE = np.float32(2.0 ** -126)
BF16_MAX_BITS = 0x7F7F  # largest finite bf16


def bf16_from_bits(bits) -> torch.Tensor:
    """uint16 bit patterns (any integer array-like) -> CPU bf16 tensor."""
    a = np.array(bits, dtype=np.uint16)  # own, writable copy
    return torch.from_numpy(a.view(np.int16)).view(torch.bfloat16)


def bf16_bits(t: torch.Tensor) -> np.ndarray:
    """bf16 tensor (any device) -> uint16 numpy bits."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def all_bf16_patterns() -> torch.Tensor:
    return bf16_from_bits(np.arange(65536, dtype=np.uint32).astype(np.uint16))


def every_pattern_page(variant: str) -> torch.Tensor:
    """One 65536-element page holding every bf16 bit pattern. "untouched"
    keeps NaN and inf; "absmax_448" / "absmax_3" replace the non-finite
    patterns and everything above that magnitude by 0, so the page's absmax
    is exactly 448 (scale 1: every subnormal tie is hit) or 3."""
    page = all_bf16_patterns().clone()
    if variant == "untouched":
        return page
    amax = {"absmax_448": 448.0, "absmax_3": 3.0}[variant]
    x = page.float()
    page[~torch.isfinite(x) | (x.abs() > amax)] = 0
    assert page.float().abs().max().item() == amax
    return page


def fp8_encode_ref(y: torch.Tensor) -> torch.Tensor:
    """Already-scaled f32 values -> e4m3fn codes (uint8): torch's cast after
    the clamp to the format's finite range."""
    return torch.clamp(y, -FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def fp8_scales_ref(pages: torch.Tensor) -> np.ndarray:
    """(n_pages, elems) bf16 -> float32 scales: finite absmax / 448, 1 for a
    page without a nonzero finite element, never below 2^-126."""
    x = pages.cpu().float()
    mag = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x))
    m = mag.max(dim=1).values.numpy().astype(np.float32)
    s = np.maximum(m / np.float32(FP8_MAX), MIN_SCALE).astype(np.float32)
    s[m == 0] = np.float32(1.0)
    return s


def fp8_quant_ref(pages: torch.Tensor):
    """(n_pages, elems) bf16 -> (codes uint8 (n_pages, elems), scales)."""
    scales = fp8_scales_ref(pages)
    inv = (np.float32(1.0) / scales).astype(np.float32)
    y = pages.cpu().float() * torch.from_numpy(inv)[:, None]
    return fp8_encode_ref(y), scales


def fp8_dequant_ref(codes: torch.Tensor, scales) -> torch.Tensor:
    """codes uint8 (n_pages, elems) + scales -> bf16 (n_pages, elems)."""
    s = torch.from_numpy(np.asarray(scales, dtype=np.float32))[:, None]
    return (codes.cpu().view(torch.float8_e4m3fn).float() * s).to(torch.bfloat16)


def assert_codes_equal(got, want, what=""):
    """Bit equality of e4m3fn codes; NaN codes compare as 'is NaN'."""
    got = np.asarray(got, dtype=np.uint8).reshape(-1)
    want = np.asarray(want, dtype=np.uint8).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g_nan, w_nan = (got & 0x7F) == 0x7F, (want & 0x7F) == 0x7F
    bad = np.flatnonzero((g_nan != w_nan) | (~w_nan & (got != want)))
    assert bad.size == 0, (
        f"{what}: {bad.size} codes differ, first at {bad[0]}: "
        f"got {got[bad[0]]:#04x} want {want[bad[0]]:#04x}")


def assert_bf16_bits_equal(got, want, what=""):
    """Bit equality of bf16 values given as uint16 bits; NaN compares as
    'is NaN'."""
    got = np.asarray(got, dtype=np.uint16).reshape(-1)
    want = np.asarray(want, dtype=np.uint16).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g_nan, w_nan = (got & 0x7FFF) > 0x7F80, (want & 0x7FFF) > 0x7F80
    bad = np.flatnonzero((g_nan != w_nan) | (~w_nan & (got != want)))
    assert bad.size == 0, (
        f"{what}: {bad.size} values differ, first at {bad[0]}: "
        f"got {got[bad[0]]:#06x} want {want[bad[0]]:#06x}")


# --- guarded block arena -----------------------------------------------------
SENTINEL = 0xA5


class Region:
    """One uint8 device tensor holding `n_blocks` blocks of `nbytes`, each at
    a 16-byte-aligned address plus its `misalign` (0..15), in permuted slot
    order, with at least `guard` untouched bytes before, between and after
    the blocks. fill="pattern" writes seeded random bytes everywhere,
    fill="sentinel" writes SENTINEL everywhere. Every block is asserted to lie
    inside the tensor when the region is built — before any launch."""

    def __init__(self, n_blocks, nbytes, *, misalign=0, guard=64, fill="sentinel",
                 seed=0, device="cuda:0"):
        assert n_blocks > 0 and nbytes > 0 and guard >= 16
        mis = np.broadcast_to(np.asarray(misalign, dtype=np.int64), (n_blocks,))
        assert mis.min() >= 0 and mis.max() < 16
        self.n_blocks, self.nbytes = n_blocks, nbytes
        stride = -(-(nbytes + 16 + guard) // 16) * 16
        lead = -(-guard // 16) * 16
        total = lead + n_blocks * stride + 32
        if fill == "pattern":
            g = torch.Generator(device="cpu").manual_seed(seed)
            self.t = torch.randint(0, 256, (total,), dtype=torch.uint8, generator=g).to(device)
        else:
            self.t = torch.full((total,), SENTINEL, dtype=torch.uint8, device=device)
        self.base = self.t.data_ptr()
        pad = (-self.base) % 16
        slots = np.random.RandomState(seed + 1).permutation(n_blocks).astype(np.int64)
        self.offs = pad + lead + slots * stride + mis  # byte offsets into self.t
        self.ptrs = [self.base + int(o) for o in self.offs]
        self.assert_in_bounds()

    def assert_in_bounds(self):
        end = self.base + self.t.numel()
        for p in self.ptrs:
            assert self.base <= p and p + self.nbytes <= end, (p, self.nbytes, self.base, end)
        o = np.sort(self.offs)
        assert (np.diff(o) >= self.nbytes + 16).all(), "blocks must not touch"

    def _index(self):
        offs = torch.from_numpy(self.offs).to(self.t.device)
        return offs[:, None] + torch.arange(self.nbytes, device=self.t.device)[None, :]

    def blocks(self) -> torch.Tensor:
        """(n_blocks, nbytes) uint8 copy of the blocks, in descriptor order."""
        return self.t[self._index()]

    def set_blocks(self, data: torch.Tensor):
        self.t[self._index()] = data.to(self.t.device).view(torch.uint8).reshape(
            self.n_blocks, self.nbytes)

    def guards_intact(self) -> bool:
        outside = torch.ones(self.t.numel(), dtype=torch.bool, device=self.t.device)
        outside[self._index().reshape(-1)] = False
        return bool((self.t[outside] == SENTINEL).all())


def assert_copied(src: Region, dst: Region, what=""):
    """Every destination block holds its source block's bytes and every byte
    outside the destination blocks still holds the sentinel."""
    got, want = dst.blocks(), src.blocks()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()[0].tolist()
        raise AssertionError(
            f"{what}: block {bad[0]} byte {bad[1]} differs "
            f"({int((got != want).sum())} bytes wrong)")
    assert dst.guards_intact(), f"{what}: bytes outside the destination blocks were written"
