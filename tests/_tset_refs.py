"""Client-side arena for the tensor-set tests (plain module, no fixtures).
Every tensor of the set is its own guarded `SegArena` (tests/_seg_refs.py),
built with the same block permutation and geometry, so that block i sits at
the SAME byte offset in each of them; the set's page i is the concatenation,
in table order, of each tensor's part. A tensor may have `extra` unused planes
(kv_major only), which makes the tensors differ in size while offsets and
stride stay common; those planes belong to the guard. The table of bases is
deliberately NOT in address order."""

import numpy as np
import torch

from _kernel_refs import SENTINEL
from _seg_refs import SegArena


class TensorSetArena:
    """n_tensors tensors, `per_tensor` segments of `seg_bytes` in each, for
    `n_blocks` pages of n_tensors * per_tensor * seg_bytes bytes.
    `misalign[g]` (0..15) moves tensor g's base off a 16-byte boundary;
    `off_shift` is added to every offset (and taken off every base), so
    offsets are nonzero and, when it is odd, misaligned themselves."""

    def __init__(self, n_tensors, n_blocks, per_tensor, seg_bytes, arrangement="gapped", *,
                 gap=48, misalign=None, extra=None, off_shift=4096, fill="sentinel", seed=0,
                 device="cuda:0"):
        G = n_tensors
        misalign = list(misalign) if misalign is not None else [0] * G
        extra = list(extra) if extra is not None else [0] * G
        assert len(misalign) == G and len(extra) == G
        assert arrangement == "kv_major" or not any(extra), "extra planes need kv_major"
        self.n_tensors, self.n_blocks = G, n_blocks
        self.per_tensor, self.seg_bytes = per_tensor, seg_bytes
        self.n_segments = G * per_tensor
        self.part_bytes = per_tensor * seg_bytes
        self.nbytes = G * self.part_bytes  # the logical page
        parts = [SegArena(n_blocks, per_tensor + extra[g], seg_bytes, arrangement, gap=gap,
                          misalign=misalign[g], fill=fill, seed=seed, device=device)
                 for g in range(G)]
        # not in address order: descending, and for three or more rotated by
        # one as well, so the table is neither ascending nor descending
        order = sorted(range(G), key=lambda g: -parts[g].base)
        if G >= 3:
            order = order[1:] + order[:1]
        self.parts = [parts[g] for g in order]
        self.misalign = [misalign[g] for g in order]
        addr = [p.base for p in self.parts]
        assert G == 1 or addr != sorted(addr), "the table must not be in address order"
        self.stride = self.parts[0].stride
        rel = self.parts[0].offs - self.parts[0].offs.min()
        for p in self.parts:
            assert p.stride == self.stride
            assert np.array_equal(p.offs - p.offs.min(), rel), "offsets must be common"
        self.offsets = [int(o) + off_shift for o in rel]
        self.bases = [int(p.base + p.offs.min()) - off_shift for p in self.parts]
        for b, m in zip(self.bases, self.misalign):
            assert (b + off_shift) % 16 == m
        # every part of every page inside its own tensor, checked before any launch
        for b, p in zip(self.bases, self.parts):
            for o in self.offsets:
                lo = b + o
                hi = lo + (per_tensor - 1) * self.stride + seg_bytes
                assert p.base <= lo and hi <= p.base + p.t.numel(), (lo, hi, p.base, p.t.numel())

    def pages(self) -> torch.Tensor:
        """(n_blocks, nbytes) uint8: the logical pages, tensors in table order."""
        return torch.cat([p.pages()[:, :self.part_bytes] for p in self.parts], dim=1)

    def set_pages(self, data: torch.Tensor):
        data = data.contiguous().view(torch.uint8).reshape(self.n_blocks, self.nbytes)
        for g, p in enumerate(self.parts):
            full = p.pages()
            full[:, :self.part_bytes] = data[:, g * self.part_bytes:(g + 1) * self.part_bytes].to(
                full.device)
            p.set_pages(full)

    def guards_intact(self) -> bool:
        """Nothing outside the pages' own segments was written: each tensor's
        guards, and its unused planes."""
        for p in self.parts:
            if not p.guards_intact():
                return False
            if not bool((p.pages()[:, self.part_bytes:] == SENTINEL).all()):
                return False
        return True

    def untouched(self) -> bool:
        return all(p.untouched() for p in self.parts)

    def snapshot(self):
        return [p.t.clone() for p in self.parts]

    def unchanged_since(self, snap) -> bool:
        return all(torch.equal(p.t, s) for p, s in zip(self.parts, snap))
