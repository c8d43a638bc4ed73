"""Paged-KV connector: the integration layer an inference engine (vLLM-style
disaggregated prefill/decode) uses to stream per-layer KV pages into the
store and pull prefix hits back out.

This is the pattern the reference documents through its examples
(/root/reference/infinistore/example/demo_prefill.py, docs/source/design.rst:
54-63) packaged as a reusable class: page keys are a hash chain over token
pages (so `get_match_last_index` answers "how many leading pages of this
sequence are cached"), writes stream layer-by-layer during prefill, reads
gather straight into the decode engine's KV tensors.

Framework-agnostic: anything that exposes per-layer KV page tensors can use
it (duck-typed; vLLM not required).
"""

import hashlib
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import lib


def token_page_hashes(token_ids: Sequence[int], page_size: int,
                      model_tag: str) -> List[str]:
    """Hash-chain page keys: key_i = H(model_tag, key_{i-1}, tokens_of_page_i).
    A page's key therefore commits to the whole prefix, which is what makes
    key-presence monotone (the property get_match_last_index relies on)."""
    keys = []
    prev = model_tag.encode()
    for start in range(0, len(token_ids) - len(token_ids) % page_size, page_size):
        page = token_ids[start : start + page_size]
        h = hashlib.blake2b(digest_size=16)
        h.update(prev)
        h.update(bytes(str(list(page)), "utf-8"))
        digest = h.hexdigest()
        keys.append(digest)
        prev = digest.encode()
    return keys


class PagedKVConnector:
    """Streams paged KV between an engine and an infinistore-amd server.

    Args:
        host, port: server address.
        model_tag: disambiguates models sharing one store.
        n_layers: layer count (layer index becomes part of the key).
        local: use the local-GPU IPC path (same host) vs the fabric path.
    """

    def __init__(self, host: str, port: int, model_tag: str, n_layers: int,
                 local: bool = True, quant: Optional[str] = None):
        """quant="fp8": store KV pages fp8-compressed (half HBM per page,
        ~3-bit mantissa; reads return bf16). quant="mxfp4": OCP MXFP4 pages
        (17/32 byte per element, one power-of-two scale per 32 elements;
        page size a multiple of 32 elements). Local path + bf16 KV only."""
        self.model_tag = model_tag
        self.n_layers = n_layers
        self.quant = quant
        cfg = lib.ClientConfig(
            host_addr=host,
            service_port=port,
            connection_type=lib.TYPE_LOCAL_GPU if local else lib.TYPE_RDMA,
            link_type="Ethernet" if not local else "Ethernet",
        )
        self.conn = lib.InfinityConnection(cfg)
        self.conn.connect()
        self.local = local
        self._registered = set()
        self._tensor_sets = {}  # (ptr, numel) per layer -> registered TensorSet

    def close(self):
        self.conn.close()

    # -- lookup ---------------------------------------------------------------
    def cached_pages(self, page_keys: List[str]) -> int:
        """How many leading pages of this sequence are fully cached (all
        layers present). Probes layer keys of the LAST layer written per page
        (layers are written 0..n-1, so the last layer's presence implies the
        rest on the prefill side)."""
        probe = [self._key(self.n_layers - 1, k) for k in page_keys]
        try:
            return self.conn.get_match_last_index(probe) + 1
        except Exception:
            return 0

    # -- prefill side ---------------------------------------------------------
    def save_layer(self, layer: int, kv: torch.Tensor, page_keys: List[str],
                   page_offsets, page_elems: int, segments: int = 1,
                   segment_stride: int = 0):
        """Store this layer's pages of `kv` (offsets in elements). Call per
        layer as prefill produces them; uploads overlap later layers'
        compute (writes are async until sync()). segments / segment_stride:
        segmented pages, as in InfinityConnection.write_pages (local path
        only, ValueError on the fabric path)."""
        keys = [self._key(layer, k) for k in page_keys]
        if self.local:
            self.conn.write_pages(kv, keys, page_offsets, page_elems,
                                  quant=self.quant, segments=segments,
                                  segment_stride=segment_stride)
        elif segments != 1:
            raise ValueError("segmented pages use the local GPU path")
        else:
            self._ensure_mr(kv)
            es = kv.element_size()
            blocks = self.conn.allocate_rdma(keys, page_elems * es)
            self.conn.rdma_write_cache(kv, list(page_offsets), page_elems, blocks)

    def flush(self):
        self.conn.sync()

    # -- decode side ----------------------------------------------------------
    def load_layer(self, layer: int, kv_out: torch.Tensor, page_keys: List[str],
                   page_offsets, page_elems: int, segments: int = 1,
                   segment_stride: int = 0, page_slice=None) -> bool:
        """Gather this layer's cached pages into the engine's KV tensor.
        Returns False if any page is missing (caller falls back to compute).
        segments / segment_stride / page_slice: as in
        InfinityConnection.read_pages (page_elems is then the sliced page); a
        refused geometry raises ValueError."""
        keys = [self._key(layer, k) for k in page_keys]
        if segments != 1 and not self.local:
            raise ValueError("segmented pages use the local GPU path")
        if page_slice is not None and not self.local:
            raise ValueError("sliced reads use the local GPU path")
        self._check_segments(kv_out, page_offsets, page_elems, segments,
                             segment_stride, page_slice)
        try:
            if self.local:
                self.conn.read_pages(kv_out, keys, page_offsets, page_elems,
                                     segments=segments,
                                     segment_stride=segment_stride,
                                     page_slice=page_slice)
            else:
                self._ensure_mr(kv_out)
                blocks = [(k, int(o)) for k, o in zip(keys, page_offsets)]
                self.conn.read_cache(kv_out, blocks, page_elems)
            self.conn.sync()
            return True
        except Exception:
            return False

    def load_layer_async(self, layer: int, kv_out: torch.Tensor,
                         page_keys: List[str], page_offsets, page_elems: int,
                         segments: int = 1, segment_stride: int = 0,
                         page_slice=None):
        """Ticketed prefetch (local path): push the gather and return a
        ticket; call wait_load(ticket) before touching kv_out. Lets decode
        overlap the next request's KV fetch with current compute. Returns
        None if any page was missing or the path is unavailable (caller
        falls back to load_layer / recompute). page_slice as in load_layer."""
        if not self.local:
            if segments != 1:
                raise ValueError("segmented pages use the local GPU path")
            if page_slice is not None:
                raise ValueError("sliced reads use the local GPU path")
            return None
        keys = [self._key(layer, k) for k in page_keys]
        self._check_segments(kv_out, page_offsets, page_elems, segments,
                             segment_stride, page_slice)
        try:
            return self.conn.read_pages_async(kv_out, keys, page_offsets,
                                              page_elems, segments=segments,
                                              segment_stride=segment_stride,
                                              page_slice=page_slice)
        except Exception:
            return None

    # -- all layers under one key (tensor sets) --------------------------------
    # Engines allocate one KV tensor per layer. Registered once as a tensor
    # set (docs/design.md, "tensor sets"), block b of ALL layers travels as one
    # page of n_layers * page_elems elements under ONE key: one request per
    # save and one per load instead of n_layers of each. Local path only. The
    # key scheme drops the layer index, so fused and per-layer keys of one
    # page hash never collide. With quant="fp8" the page's single scale spans
    # all layers.
    def save_all_layers(self, kvs, page_keys: List[str], page_offsets, page_elems: int,
                        segments: int = 1, segment_stride: int = 0):
        """Store block `page_offsets[i]` (elements, the same in every layer
        tensor) of all `kvs` under page_keys[i]. page_elems, segments and
        segment_stride describe ONE layer's part, as in save_layer."""
        ts = self._tensor_set(kvs)
        self.conn.write_pages(None, [self._fused_key(k) for k in page_keys], page_offsets,
                              page_elems * len(kvs), quant=self.quant,
                              segments=segments * len(kvs), segment_stride=segment_stride,
                              tensor_set=ts)

    def load_all_layers(self, kvs_out, page_keys: List[str], page_offsets, page_elems: int,
                        segments: int = 1, segment_stride: int = 0) -> bool:
        """Gather the pages into all layer tensors with one request. False if
        any page is missing; a refused geometry raises ValueError."""
        tk = self.load_all_layers_async(kvs_out, page_keys, page_offsets, page_elems,
                                        segments, segment_stride)
        return tk is not None and self.wait_load(tk)

    def load_all_layers_async(self, kvs_out, page_keys: List[str], page_offsets,
                              page_elems: int, segments: int = 1, segment_stride: int = 0):
        """Ticketed form of load_all_layers: one ticket for all layers (None
        if the request failed at once); wait_load(ticket) before use."""
        ts = self._tensor_set(kvs_out)
        offs = np.asarray(page_offsets, dtype=np.uint64)
        total = segments * len(kvs_out)
        self.conn._check_tensor_set(ts, offs, page_elems * len(kvs_out), total, segment_stride)
        try:
            return self.conn.read_pages_async(None, [self._fused_key(k) for k in page_keys],
                                              offs, page_elems * len(kvs_out), segments=total,
                                              segment_stride=segment_stride, tensor_set=ts)
        except Exception:
            return None

    def cached_pages_fused(self, page_keys: List[str]) -> int:
        """cached_pages for pages saved with save_all_layers."""
        try:
            return self.conn.get_match_last_index([self._fused_key(k) for k in page_keys]) + 1
        except Exception:
            return 0

    def evict_fused(self, page_keys: List[str]) -> int:
        return self.conn.delete_keys([self._fused_key(k) for k in page_keys])

    def _tensor_set(self, kvs):
        """The registered set of these layer tensors, registered on first use.
        A connection holds few sets: the oldest is released for a new one."""
        if not self.local:
            raise ValueError("all-layer pages use tensor sets, which need the local GPU path")
        if len(kvs) != self.n_layers:
            raise ValueError(f"{len(kvs)} layer tensors for {self.n_layers} layers")
        ident = tuple((t.data_ptr(), t.numel()) for t in kvs)
        ts = self._tensor_sets.get(ident)
        if ts is None:
            if len(self._tensor_sets) >= self.conn.MAX_TENSOR_SETS:
                self.conn.sync()  # nothing of the set to be released is in flight
                self.conn.release_tensor_set(self._tensor_sets.pop(next(iter(self._tensor_sets))))
            ts = self.conn.register_tensor_set([t.view(-1) for t in kvs])
            self._tensor_sets[ident] = ts
        return ts

    def _fused_key(self, page_hash: str) -> str:
        return f"{self.model_tag}/ALL/{page_hash}"

    def wait_load(self, ticket) -> bool:
        try:
            self.conn.wait_read(ticket)
            return True
        except Exception:
            return False

    def evict(self, page_keys: List[str]) -> int:
        """Drop a sequence's pages (all layers)."""
        keys = [self._key(layer, k) for layer in range(self.n_layers)
                for k in page_keys]
        return self.conn.delete_keys(keys)

    # -- internals ------------------------------------------------------------
    def _check_segments(self, kv: torch.Tensor, page_offsets, page_elems: int,
                        segments: int, segment_stride: int, page_slice=None):
        # The loads turn every failure into False / None; a refused geometry
        # is the caller's mistake and stays a ValueError.
        if page_slice is not None:
            self.conn._check_slice(kv.numel(), page_offsets, page_elems, page_slice,
                                   segments, segment_stride)
        self.conn._check_segments(kv.numel(), kv.element_size(), page_offsets,
                                  page_elems, segments, segment_stride)

    def _key(self, layer: int, page_hash: str) -> str:
        return f"{self.model_tag}/L{layer}/{page_hash}"

    def _ensure_mr(self, t: torch.Tensor):
        ptr = t.data_ptr()
        if ptr not in self._registered:
            self.conn.register_mr(t)
            self._registered.add(ptr)


def gpu_page_hashes(kv: torch.Tensor, page_offsets, page_elems: int,
                    prev_digest: Optional[int] = None) -> List[int]:
    """GPU-side alternative to token_page_hashes: fingerprint the KV pages
    themselves with the fingerprint kernel (no host readback). Useful for
    content-addressed dedup rather than token-prefix reuse."""
    fps = lib.fingerprint_blocks(kv, list(page_offsets), page_elems)
    out = []
    prev = prev_digest or 0
    for f in fps:
        prev = (prev * 1099511628211 + f) % (1 << 64)
        out.append(prev)
    return out
