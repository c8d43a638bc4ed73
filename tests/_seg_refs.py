"""Client-side arena for the segmented-page kernel tests (plain module, no
fixtures): the segmented counterpart of `_kernel_refs.Region`. One uint8
device tensor holds `n_blocks` pages of `n_segments` segments of `seg_bytes`,
filled with a pattern (a source) or the sentinel (a destination), with
untouched bytes around everything a kernel may write. Every segment is
asserted to lie inside the tensor, and not to touch another, when the arena is
built — before any launch."""

import numpy as np
import torch

from _kernel_refs import SENTINEL


class SegArena:
    """arrangement="gapped": the segments of a page lie `seg_bytes + gap`
    apart (stride), pages in permuted slots with guards between them, so
    every byte between two segments can be checked.
    arrangement="kv_major": segment s of slot b lies at
    `s * plane + b * seg_bytes`, slots permuted, stride = plane — a
    `[S, n_blocks, seg]` cache; `gap` bytes of guard separate the planes.
    `misalign` (0..15) is added to every page's base address; the stride is
    the same for all pages, as a request's is."""

    def __init__(self, n_blocks, n_segments, seg_bytes, arrangement, *, gap=48, misalign=0,
                 guard=64, fill="sentinel", seed=0, device="cuda:0"):
        assert n_blocks > 0 and n_segments > 0 and seg_bytes > 0 and guard >= 16
        assert 0 <= misalign < 16 and gap >= 0
        self.n_blocks, self.n_segments, self.seg_bytes = n_blocks, n_segments, seg_bytes
        self.nbytes = n_segments * seg_bytes  # the logical page
        slots = np.random.RandomState(seed + 1).permutation(n_blocks).astype(np.int64)
        lead = -(-guard // 16) * 16
        if arrangement == "gapped":
            self.stride = seg_bytes + gap
            slot = -(-(n_segments * self.stride + 16 + guard) // 16) * 16
            offs = lead + slots * slot
            total = lead + n_blocks * slot + 32
        elif arrangement == "kv_major":
            self.stride = n_blocks * seg_bytes + gap  # the plane
            offs = lead + slots * seg_bytes
            total = lead + n_segments * self.stride + guard + 32
        else:
            raise ValueError(arrangement)
        if fill == "pattern":
            g = torch.Generator(device="cpu").manual_seed(seed)
            self.t = torch.randint(0, 256, (total,), dtype=torch.uint8, generator=g).to(device)
        else:
            self.t = torch.full((total,), SENTINEL, dtype=torch.uint8, device=device)
        self.base = self.t.data_ptr()
        pad = (-self.base) % 16
        self.offs = pad + offs + misalign  # byte offset of each page's segment 0
        self.ptrs = [self.base + int(o) for o in self.offs]
        self.assert_in_bounds()

    def seg_offs(self) -> np.ndarray:
        """(n_blocks, n_segments) byte offsets of every segment."""
        return self.offs[:, None] + np.arange(self.n_segments, dtype=np.int64)[None, :] * self.stride

    def assert_in_bounds(self):
        so = self.seg_offs().reshape(-1)
        assert so.min() >= 0 and so.max() + self.seg_bytes <= self.t.numel(), (
            so.min(), so.max(), self.seg_bytes, self.t.numel())
        o = np.sort(so)
        assert (np.diff(o) >= self.seg_bytes).all(), "segments must not overlap"

    def _index(self):
        so = torch.from_numpy(self.seg_offs()).to(self.t.device)  # (n, S)
        idx = so[:, :, None] + torch.arange(self.seg_bytes, device=self.t.device)[None, None, :]
        return idx.reshape(self.n_blocks, self.nbytes)

    def pages(self) -> torch.Tensor:
        """(n_blocks, n_segments * seg_bytes) uint8: each page's segments
        concatenated, in descriptor order — the logical pages."""
        return self.t[self._index()]

    def set_pages(self, data: torch.Tensor):
        self.t[self._index()] = data.to(self.t.device).contiguous().view(torch.uint8).reshape(
            self.n_blocks, self.nbytes)

    def guards_intact(self) -> bool:
        outside = torch.ones(self.t.numel(), dtype=torch.bool, device=self.t.device)
        outside[self._index().reshape(-1)] = False
        return bool((self.t[outside] == SENTINEL).all())

    def untouched(self) -> bool:
        return bool((self.t == SENTINEL).all())
