"""vLLM-shaped KV-cache connector adapter.

Presents the interface shape of vLLM v1's KV connector (scheduler-side
prefix-hit query + worker-side per-layer save/load hooks with async waits)
on top of :class:`PagedKVConnector`, so an engine that manages paged KV
caches through block tables can plug the store in without writing any
store-specific code. vLLM itself is NOT imported — the adapter is
duck-typed against the engine objects it needs (per-layer cache tensors +
block tables), which is also what makes it testable here.

Engine model assumed (vLLM-style paged attention):

* per layer, one physical cache tensor in one of two layouts
  (``kv_layout``):

  - ``"block_major"`` (default): ``cache[layer].view(num_blocks, -1)`` —
    physical block ``b`` of layer ``l`` occupies elements
    ``[b*page_elems, (b+1)*page_elems)``. The
    ``[num_blocks, 2, block_tokens, n_kv, head]`` layout satisfies this.
  - ``"kv_major"``: ``[2, num_blocks, block_tokens, n_kv, head]``, as
    FlashAttention-style and several ROCm paged-attention back ends
    allocate. The K half of block ``b`` occupies elements
    ``[b*page_elems/2, (b+1)*page_elems/2)`` and its V half lies
    ``cache.numel()/2`` further on. Each block still travels as ONE page
    under ONE key: a segmented page of two segments
    (docs/design.md, "segmented pages"), stored exactly as the
    block-major page ``cat(K[b], V[b])`` would be — so a prefill engine
    with one layout and a decode engine with the other share pages.
* a request's logical page ``p`` lives in physical block
  ``block_table[p]`` (an arbitrary permutation — the adapter maps through
  it on both save and load, so prefill and decode engines can use
  completely different physical placements).
* page keys are the token-prefix hash chain (``token_page_hashes``), so a
  page key commits to the whole prefix and `get_match_last_index` answers
  "how many leading pages are cached" in one round trip.

Reference behavior being packaged: the layer-by-layer streaming pattern of
/root/reference/infinistore/example/demo_prefill.py:58-90 and the prefix
lookup of /root/reference/src/infinistore.cpp:1092-1108.
"""

from typing import Dict, List, Optional, Sequence

import torch

from .kv_connector import PagedKVConnector, token_page_hashes
from .lib import PageSlice


class InfiniStoreKVAdapter:
    """vLLM-v1-shaped connector over a PagedKVConnector.

    Scheduler side:
        ``get_num_new_matched_tokens(token_ids, num_computed_tokens)``
    Worker side (prefill):
        ``save_kv_layer(layer, kv_cache, token_ids, block_table)`` per
        layer, then ``wait_for_save()``.
    Worker side (decode):
        ``start_load_kv(kv_caches, token_ids, block_table)`` once, then
        ``wait_for_layer_load(layer)`` right before each layer's attention.

    Args:
        host, port: store address.
        model_tag: namespace (model + dtype + layout version).
        n_layers: engine layer count.
        block_tokens: tokens per engine block (= store page).
        page_elems: elements per page per layer (``2*block_tokens*n_kv*hd``
            for the usual K+V layout).
        local: same-host GPU path (IPC + HIP gather) vs the fabric path.
        quant: "fp8" or "mxfp4" to store pages compressed (bf16 engines
            only; "mxfp4" needs page_elems % 32 == 0).
        kv_layout: "block_major" or "kv_major" (see the module docstring).
            page_elems counts K plus V in both. "kv_major" needs the local
            path (ValueError with local=False).
        stored_kv_heads, head_range, head_dim: mixed tensor-parallel decode.
            The pages in the store are a prefill engine's
            ``[2, block_tokens, stored_kv_heads, head_dim]``; this engine owns
            the KV heads ``head_range = (h0, h1)`` of them, so its own
            page_elems is ``2*block_tokens*(h1-h0)*head_dim`` (checked) and
            every load is a sliced read (docs/design.md, "sliced reads") that
            fetches only those heads. Works in both layouts and needs the
            local path. Such an adapter is load-only: save_kv_layer raises
            ValueError. Keys and prefix lookups are the prefill engine's.
        layer_pages: "per_layer" (default): one key per (layer, block), one
            request per layer. "fused": one key per block for ALL layers
            (docs/design.md, "tensor sets"): the engine's per-layer tensors
            are registered once as a tensor set, save_kv_layer only records
            its arguments, wait_for_save issues ONE write, start_load_kv ONE
            read, and wait_for_layer_load waits on that one ticket. Works
            with both kv_layout values; needs the local path and layer
            tensors of one size; with head_range it raises ValueError
            (slices over a tensor set are not supported). The key scheme
            drops the layer index, so fused and per-layer pages of one model
            tag never collide, and neither kind of adapter sees the other's
            pages. With quant="fp8" the page's one scale spans all layers.
    """

    KV_LAYOUTS = ("block_major", "kv_major")
    LAYER_PAGES = ("per_layer", "fused")

    def __init__(self, host: str, port: int, model_tag: str, n_layers: int,
                 block_tokens: int, page_elems: int, local: bool = True,
                 quant: Optional[str] = None, kv_layout: str = "block_major",
                 stored_kv_heads: Optional[int] = None,
                 head_range: Optional[Sequence[int]] = None,
                 head_dim: Optional[int] = None, layer_pages: str = "per_layer"):
        if layer_pages not in self.LAYER_PAGES:
            raise ValueError(f"layer_pages must be one of {self.LAYER_PAGES}")
        if layer_pages == "fused":
            if head_range is not None:
                raise ValueError('layer_pages="fused" cannot be combined with head_range: '
                                 "a tensor set takes no slice")
            if not local:
                raise ValueError('layer_pages="fused" uses tensor sets, which need the '
                                 "local GPU path")
        self.fused = layer_pages == "fused"
        self._recorded: Dict[int, tuple] = {}  # fused: layer -> save_kv_layer arguments
        self._fused_ticket = None
        self._fused_result: Optional[bool] = None
        self._page_slice = None
        if head_range is not None:
            if stored_kv_heads is None or head_dim is None:
                raise ValueError("head_range needs stored_kv_heads and head_dim")
            if not local:
                raise ValueError("head_range uses sliced reads, which need the "
                                 "local GPU path")
            h0, h1 = (int(h) for h in head_range)
            if not 0 <= h0 < h1 <= stored_kv_heads or head_dim <= 0:
                raise ValueError("head_range must be 0 <= h0 < h1 <= stored_kv_heads")
            if page_elems != 2 * block_tokens * (h1 - h0) * head_dim:
                raise ValueError("with head_range=(h0, h1) page_elems is "
                                 "2*block_tokens*(h1-h0)*head_dim")
            self._page_slice = PageSlice(
                page_size=2 * block_tokens * stored_kv_heads * head_dim,
                offset=h0 * head_dim, piece=(h1 - h0) * head_dim,
                stride=stored_kv_heads * head_dim, count=2 * block_tokens)
        elif stored_kv_heads is not None or head_dim is not None:
            raise ValueError("stored_kv_heads and head_dim go with head_range")
        if kv_layout not in self.KV_LAYOUTS:
            raise ValueError(f"kv_layout must be one of {self.KV_LAYOUTS}")
        if kv_layout == "kv_major":
            if not local:
                raise ValueError('kv_layout="kv_major" uses segmented pages, '
                                 "which need the local GPU path")
            if page_elems % 2 != 0:
                raise ValueError("kv_major needs an even page_elems (K plus V)")
        self.kv_layout = kv_layout
        self.block_tokens = block_tokens
        self.page_elems = page_elems
        self.n_layers = n_layers
        self._conn = PagedKVConnector(host, port, model_tag, n_layers,
                                      local=local, quant=quant)
        self._load_tickets: Dict[int, object] = {}
        self._load_fallback: Dict[int, tuple] = {}
        self._key_cache: Dict[tuple, List[str]] = {}

    def close(self):
        self._conn.close()

    # -- scheduler side -------------------------------------------------------
    def get_num_new_matched_tokens(self, token_ids: Sequence[int],
                                   num_computed_tokens: int = 0) -> int:
        """Prefix-hit fast path: how many tokens beyond
        ``num_computed_tokens`` can be served from the store (whole pages
        only). One `get_match_last_index` round trip."""
        keys = self._page_keys(token_ids)
        if not keys:
            return 0
        hit_pages = (self._conn.cached_pages_fused(keys) if self.fused
                     else self._conn.cached_pages(keys))
        hit_tokens = hit_pages * self.block_tokens
        return max(0, hit_tokens - num_computed_tokens)

    # -- worker side: prefill save -------------------------------------------
    def save_kv_layer(self, layer: int, kv_cache: torch.Tensor,
                      token_ids: Sequence[int],
                      block_table: Sequence[int],
                      skip_leading_pages: int = 0) -> None:
        """Stream layer ``layer``'s full pages of this request into the
        store (async; overlaps later layers' compute). ``kv_cache`` is the
        engine's physical cache tensor for this layer (block-major);
        ``block_table[p]`` names the physical block of logical page ``p``.
        ``skip_leading_pages`` skips pages already known cached (prefix
        hits reported by the scheduler)."""
        if self._page_slice is not None:
            raise ValueError("an adapter with head_range is load-only: slices "
                             "are a read-side geometry")
        keys = self._page_keys(token_ids)
        n_pages = len(keys)
        if n_pages > len(block_table):
            raise ValueError(f"block_table has {len(block_table)} entries for "
                             f"{n_pages} full pages")
        s = skip_leading_pages
        if self.fused:
            # One write for all layers at wait_for_save: record only.
            if not 0 <= layer < self.n_layers:
                raise ValueError(f"layer {layer} of {self.n_layers}")
            self._recorded[layer] = (kv_cache, tuple(token_ids), tuple(block_table), s)
            return
        if s >= n_pages:
            return
        offsets = self._offsets(block_table, range(s, n_pages))
        self._conn.save_layer(layer, kv_cache.view(-1), keys[s:], offsets,
                              self.page_elems, **self._geometry(kv_cache))

    def wait_for_save(self):
        """Barrier: all save_kv_layer uploads committed (readable by any
        client, including other hosts). A fused adapter issues its one
        write here, from what save_kv_layer recorded for every layer."""
        if self.fused and self._recorded:
            rec, self._recorded = self._recorded, {}
            if sorted(rec) != list(range(self.n_layers)):
                raise ValueError("a fused save needs save_kv_layer for every layer: got "
                                 f"{sorted(rec)}")
            _, token_ids, block_table, skip = rec[0]
            if any(r[1:] != rec[0][1:] for r in rec.values()):
                raise ValueError("a fused save needs the same token_ids, block_table and "
                                 "skip_leading_pages for every layer")
            keys = self._page_keys(token_ids)
            if skip < len(keys):
                kvs = [rec[li][0] for li in range(self.n_layers)]
                offsets = self._offsets(block_table, range(skip, len(keys)))
                self._conn.save_all_layers(kvs, keys[skip:], offsets, self.page_elems,
                                           **self._geometry(kvs[0]))
        self._conn.flush()

    # -- worker side: decode load ----------------------------------------------
    def start_load_kv(self, kv_caches: List[torch.Tensor],
                      token_ids: Sequence[int],
                      block_table: Sequence[int],
                      n_pages: Optional[int] = None) -> int:
        """Kick off the gather of every layer's cached pages straight into
        the engine's cache tensors (ticketed async reads on the local path;
        all layers' gathers are in flight at once). Returns the number of
        pages being loaded. Call ``wait_for_layer_load(l)`` before layer
        ``l``'s attention reads its pages."""
        keys = self._page_keys(token_ids)
        if n_pages is not None:
            keys = keys[:n_pages]
        if not keys:
            return 0
        if len(keys) > len(block_table):
            raise ValueError(f"block_table has {len(block_table)} entries for "
                             f"{len(keys)} pages")
        offsets = self._offsets(block_table, range(len(keys)))
        self._load_tickets.clear()
        self._load_fallback.clear()
        if self.fused:
            # One read for all layers; every wait_for_layer_load waits on it.
            self._fused_result = None
            self._fused_ticket = self._conn.load_all_layers_async(
                list(kv_caches), keys, offsets, self.page_elems,
                **self._geometry(kv_caches[0]))
            if self._fused_ticket is None:
                self._fused_result = False
            return len(keys)
        for li in range(self.n_layers):
            tk = self._conn.load_layer_async(li, kv_caches[li].view(-1), keys,
                                             offsets, self.page_elems,
                                             **self._geometry(kv_caches[li]))
            if tk is not None:
                self._load_tickets[li] = tk
            else:  # fabric path (or ring unavailable): blocking load at wait
                self._load_fallback[li] = (kv_caches[li], keys, offsets)
        return len(keys)

    def wait_for_layer_load(self, layer: int) -> bool:
        """Block until layer ``layer``'s pages have landed. False = a page
        was missing or the read failed (caller recomputes that layer)."""
        if self.fused:
            if self._fused_result is None:
                if self._fused_ticket is None:
                    return True  # nothing pending (e.g. 0 pages)
                self._fused_result = self._conn.wait_load(self._fused_ticket)
                self._fused_ticket = None
            return self._fused_result
        tk = self._load_tickets.pop(layer, None)
        if tk is not None:
            return self._conn.wait_load(tk)
        fb = self._load_fallback.pop(layer, None)
        if fb is not None:
            kv, keys, offsets = fb
            return self._conn.load_layer(layer, kv.view(-1), keys, offsets,
                                         self.page_elems, **self._geometry(kv))
        return True  # nothing pending for this layer (e.g. 0 pages)

    # -- maintenance -----------------------------------------------------------
    def evict_request(self, token_ids: Sequence[int]) -> int:
        """Drop all layers of this sequence's pages from the store."""
        if self.fused:
            return self._conn.evict_fused(self._page_keys(token_ids))
        return self._conn.evict(self._page_keys(token_ids))

    # -- internals -------------------------------------------------------------
    def _offsets(self, block_table: Sequence[int], pages) -> List[int]:
        """Element offset of each logical page's block (its K half for
        kv_major) in the flattened layer tensor."""
        step = self.page_elems // 2 if self.kv_layout == "kv_major" else self.page_elems
        return [int(block_table[p]) * step for p in pages]

    def _geometry(self, kv_cache: torch.Tensor) -> dict:
        """Segment arguments for one layer tensor: none for block_major; K
        and V halves a plane (half the tensor) apart for kv_major. With a
        head_range, the slice every load takes (saves never get here)."""
        geo = {}
        if self._page_slice is not None:
            geo["page_slice"] = self._page_slice
        if self.kv_layout == "kv_major":
            geo.update(segments=2, segment_stride=kv_cache.numel() // 2)
        return geo

    def _page_keys(self, token_ids: Sequence[int]) -> List[str]:
        ck = tuple(token_ids)
        got = self._key_cache.get(ck)
        if got is not None:
            return got
        keys = token_page_hashes(list(token_ids), self.block_tokens,
                                 self._conn.model_tag)
        if len(self._key_cache) < 256:
            self._key_cache[ck] = keys
        return keys
