"""infinistore-amd client/server Python API.

API parity with the reference store's `infinistore/lib.py`
(/root/reference/infinistore/lib.py): `InfinityConnection` with the same
method names and unit conventions (offsets/page_size are in tensor
*elements*; conversion to bytes happens here), `ClientConfig`/`ServerConfig`
kwargs classes with `verify()`, `Logger`, `check_supported`,
`register_server`, `purge_kv_map`, `get_kvmap_len`, `DisableTorchCaching`.

Differences (MI355X-native build):
  * The server runs on a dedicated C++ thread — `register_server(config)`
    just starts it; an optional leading asyncio-loop argument is accepted
    and ignored for source compatibility with the reference signature.
  * TYPE_RDMA works with no RDMA NIC: the connection negotiates a data
    fabric at setup time and falls back to the TCP inline-data fabric
    (`link_type` may also be "TCP" to request it explicitly).
  * check_supported() probes ROCm/HIP + amdgpu instead of nv_peer_mem.
"""

import os
import time
import asyncio
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _build

_build.ensure_native()

from . import _native  # noqa: E402

# connection types
TYPE_LOCAL_GPU = "LOCAL_GPU"
TYPE_RDMA = "RDMA"
# rdma link types ("TCP" = inline-data fabric; auto-negotiated anyway)
LINK_ETHERNET = "Ethernet"
LINK_IB = "IB"
LINK_TCP = "TCP"


class ClientConfig(_native.ClientConfig):
    """Client configuration (kwargs: connection_type, host_addr, dev_name,
    ib_port, link_type, service_port, log_level)."""

    def __init__(self, **kwargs):
        super().__init__()
        self.connection_type = kwargs.get("connection_type", "") or ""
        self.host_addr = kwargs.get("host_addr", "") or ""
        self.dev_name = kwargs.get("dev_name", "")
        self.ib_port = kwargs.get("ib_port", 1)
        self.link_type = kwargs.get("link_type", "Ethernet")
        self.service_port = kwargs.get("service_port", 0) or 0
        if "INFINISTORE_LOG_LEVEL" in os.environ:
            self.log_level = os.environ["INFINISTORE_LOG_LEVEL"]
        else:
            self.log_level = kwargs.get("log_level", "warning")

    def __repr__(self):
        return (
            f"ClientConfig(service_port={self.service_port}, "
            f"log_level='{self.log_level}', host_addr='{self.host_addr}', "
            f"connection_type='{self.connection_type}', "
            f"dev_name='{self.dev_name}', ib_port={self.ib_port}, "
            f"link_type='{self.link_type}')"
        )

    def verify(self):
        if self.connection_type not in [TYPE_LOCAL_GPU, TYPE_RDMA]:
            raise Exception("Invalid connection type")
        if self.host_addr == "":
            raise Exception("Host address is empty")
        if self.service_port == 0:
            raise Exception("Service port is 0")
        if self.log_level not in ["error", "debug", "info", "warning"]:
            raise Exception("log level should be error, debug, info or warning")
        if self.ib_port < 1:
            raise Exception("ib port of device should be greater than 0")
        if self.connection_type == TYPE_RDMA and self.link_type not in [
            LINK_IB,
            LINK_ETHERNET,
            LINK_TCP,
        ]:
            raise Exception("link type should be IB, Ethernet or TCP for RDMA connection")


class ServerConfig(_native.ServerConfig):
    """Server configuration (kwargs: manage_port, service_port, log_level,
    dev_name, ib_port, link_type, prealloc_size (GB per shard),
    minimal_allocate_size (KB), num_stream, auto_increase, devices,
    cpu_only)."""

    def __init__(self, **kwargs):
        super().__init__()
        self.manage_port = kwargs.get("manage_port", 0)
        self.service_port = kwargs.get("service_port", 0)
        self.log_level = kwargs.get("log_level", "warning")
        self.dev_name = kwargs.get("dev_name", "")
        self.ib_port = kwargs.get("ib_port", 1)
        self.link_type = kwargs.get("link_type", "Ethernet")
        self.prealloc_size = kwargs.get("prealloc_size", 16)
        self.minimal_allocate_size = kwargs.get("minimal_allocate_size", 64)
        self.num_stream = kwargs.get("num_stream", 4)
        self.auto_increase = kwargs.get("auto_increase", False)
        self.devices = kwargs.get("devices", [])
        self.cpu_only = kwargs.get("cpu_only", False)
        self.cpu_shards = kwargs.get("cpu_shards", 1)
        self.auto_evict = kwargs.get("auto_evict", False)
        self.ttl_seconds = kwargs.get("ttl_seconds", 0)
        self.io_threads = kwargs.get("io_threads", 3)
        self.extend_size = kwargs.get("extend_size", 10)

    def __repr__(self):
        return (
            f"ServerConfig(service_port={self.service_port}, manage_port={self.manage_port}, "
            f"log_level='{self.log_level}', prealloc_size={self.prealloc_size}, "
            f"minimal_allocate_size={self.minimal_allocate_size}, "
            f"num_stream={self.num_stream}, devices={list(self.devices)}, "
            f"cpu_only={self.cpu_only})"
        )

    def verify(self):
        if self.service_port == 0:
            raise Exception("Service port is 0")
        if self.manage_port == 0:
            raise Exception("Manage port is 0")
        if self.log_level not in ["error", "debug", "info", "warning"]:
            raise Exception("log level should be error, debug, info or warning")
        if self.ib_port < 1:
            raise Exception("ib port of device should be greater than 0")
        if self.link_type not in [LINK_IB, LINK_ETHERNET, LINK_TCP]:
            raise Exception("link type should be IB, Ethernet or TCP")
        if self.minimal_allocate_size < 16:
            raise Exception("minimal allocate size should be greater than 16")


class Logger:
    @staticmethod
    def info(msg):
        _native.log_msg("info", str(msg))

    @staticmethod
    def debug(msg):
        _native.log_msg("debug", str(msg))

    @staticmethod
    def error(msg):
        _native.log_msg("error", str(msg))

    @staticmethod
    def warn(msg):
        _native.log_msg("warning", str(msg))

    @staticmethod
    def set_log_level(level):
        _native.set_log_level(level)


def get_kvmap_len():
    """Number of keys stored in the (in-process) server."""
    return _native.get_kvmap_len()


def purge_kv_map():
    """Drop every key from the (in-process) server; returns the count."""
    return _native.purge_kv_map()


def snapshot_pool(path: str):
    """Dump every committed page to `path` for a warm restart (extension —
    the reference cache is volatile). Returns (entries, payload_bytes)."""
    ok, n, b = _native.server_snapshot(path)
    if not ok:
        raise Exception(f"snapshot to {path} failed")
    return n, b


def restore_pool(path: str):
    """Load a snapshot back into the pool (existing keys win; stops cleanly
    when the pool fills). Returns (entries, payload_bytes)."""
    ok, n, b = _native.server_restore(path)
    if not ok:
        raise Exception(f"restore from {path} failed")
    return n, b


def get_server_stats():
    """JSON string with server counters (extension over the reference)."""
    return _native.server_stats()


def compact_pool():
    """Defragment the (in-process) server's pools by moving committed idle
    blocks to lower addresses with the batched copy kernel. Returns
    (moved_blocks, moved_bytes). Extension over the reference."""
    return _native.server_compact()


def register_server(*args):
    """Start the in-process server.

    Accepts `register_server(config)` or the reference's
    `register_server(loop, config)` (the loop argument is ignored: the
    server owns a dedicated C++ event-loop thread instead of borrowing
    uvloop's uv_loop_t*, cf. reference lib.py:179-205).
    """
    config = args[-1]
    config.verify()
    if not _native.start_server(config):
        raise Exception("Failed to start server")


def unregister_server():
    _native.stop_server()


def check_supported():
    """Probe platform support: ROCm GPUs present? amdgpu loaded? Logs
    warnings (the reference probes nv_peer_mem + ibv_devinfo instead)."""
    if not _native.gpu_available():
        Logger.warn("no ROCm GPU visible — server will run with a CPU (DRAM) pool")
        return False
    try:
        with open("/proc/modules") as f:
            mods = f.read()
        if "amdgpu" not in mods:
            Logger.warn("amdgpu module not listed in /proc/modules")
    except OSError:
        pass
    return True


class DisableTorchCaching:
    """Context manager that disables the torch caching allocator for tensors
    allocated inside it. With this build it is OPTIONAL for the local path:
    the wire protocol carries the offset of a tensor inside its allocation,
    so IPC round-trips work with the caching allocator too. Kept for API
    compatibility with the reference (lib.py:254-274)."""

    def __enter__(self):
        os.environ["PYTORCH_NO_CUDA_MEMORY_CACHING"] = "1"
        return self

    def __exit__(self, exc_type, exc_value, traceback):
        os.environ.pop("PYTORCH_NO_CUDA_MEMORY_CACHING", None)


def _remap_device_id(tensor: torch.Tensor) -> int:
    device_id = tensor.device.index
    if device_id is None:
        return 0
    visible = os.environ.get("CUDA_VISIBLE_DEVICES", "") or os.environ.get(
        "HIP_VISIBLE_DEVICES", ""
    )
    if visible:
        return int(visible.split(",")[device_id])
    return device_id


class PageSlice(NamedTuple):
    """Pool-side geometry of a sliced read, in ELEMENTS of the cache tensor:
    from every stored page of `page_size` elements take `count` pieces of
    `piece` elements, piece p starting at element offset + p * stride of the
    page. The reader receives the concatenation, a page of count * piece
    elements (docs/design.md, "sliced reads"). Read-only: there is no sliced
    write. E.g. the heads h0..h1 of a [2, T, H, hd] page:
    PageSlice(2*T*H*hd, h0*hd, (h1-h0)*hd, H*hd, 2*T)."""

    page_size: int  # of the page as it was WRITTEN
    offset: int  # of piece 0 inside that page
    piece: int
    stride: int = 0  # from one piece to the next (ignored for count == 1)
    count: int = 1


class TensorSet:
    """A registered tensor set (InfinityConnection.register_tensor_set): the
    server-side id and the tensors, which it keeps alive."""

    def __init__(self, conn, set_id: int, tensors):
        self.conn = conn
        self.set_id = set_id
        self.tensors = list(tensors)

    def __len__(self):
        return len(self.tensors)


class InfinityConnection:
    """Connection to an infinistore-amd server (local IPC path or
    RDMA-semantics path over the negotiated fabric)."""

    OP_R = "R"
    OP_W = "W"
    OP_SYNC = "S"
    OP_RDMA_READ = "A"

    def __init__(self, config: ClientConfig):
        config.verify()
        self.conn = _native.Connection()
        self.local_connected = False
        self.rdma_connected = False
        self.config = config
        Logger.set_log_level(config.log_level)

    # -- connect ------------------------------------------------------------
    def connect(self):
        if self.local_connected:
            raise Exception("Already connected to local instance")
        if self.rdma_connected:
            raise Exception("Already connected to remote instance")
        ret = self.conn.init_connection(self.config)
        if ret < 0:
            raise Exception("Failed to initialize remote connection")
        if self.config.connection_type == TYPE_LOCAL_GPU:
            if self.config.host_addr not in ["127.0.0.1", "localhost"]:
                raise Exception("Local GPU connection must be to localhost")
            self.local_connected = True
        else:
            ret = self.conn.setup_rdma(self.config)
            if ret < 0:
                raise Exception("Failed to setup RDMA connection")
            self.rdma_connected = True

    async def connect_async(self):
        if self.config.connection_type == TYPE_LOCAL_GPU:
            raise Exception("Local GPU connection is not supported in async mode")
        loop = asyncio.get_running_loop()

        def blocking_connect():
            if self.conn.init_connection(self.config) < 0:
                raise Exception("Failed to initialize remote connection")
            if self.conn.setup_rdma(self.config) < 0:
                raise Exception("Failed to setup RDMA connection")
            self.rdma_connected = True

        await loop.run_in_executor(None, blocking_connect)

    def close(self):
        self.conn.close_conn()
        self.local_connected = False
        self.rdma_connected = False

    # -- local (IPC) path ---------------------------------------------------
    @staticmethod
    def _pack_blocks(blocks, element_size):
        """(keys_blob, offsets_bytes, n): keys NUL-joined, offsets in bytes as
        u64 — the packed fast-path arguments (avoids per-tuple marshalling)."""
        n = len(blocks)
        if n == 0:
            return b"", b"", 0
        keys, offsets = zip(*blocks)
        blob = "\x00".join(keys).encode()
        offs = np.fromiter(offsets, dtype=np.uint64, count=n) * np.uint64(element_size)
        return blob, offs.tobytes(), n

    def local_gpu_write_cache(
        self, cache: torch.Tensor, blocks: List[Tuple[str, int]], page_size: int
    ):
        """Write pages of `cache` (offsets in elements) under string keys."""
        self._verify(cache)
        assert self.local_connected
        element_size = cache.element_size()
        blob, offs, n = self._pack_blocks(blocks, element_size)
        ret = self.conn.rw_local_fast(
            self.OP_W,
            blob,
            offs,
            n,
            page_size * element_size,
            cache.data_ptr(),
            _remap_device_id(cache),
        )
        if ret < 0:
            raise Exception(f"Failed to write to infinistore, ret = {ret}")
        return 0

    # -- vectorized page API (extension) ------------------------------------
    # Same semantics as local_gpu_write_cache/read_cache but takes keys and
    # offsets as parallel sequences; `offsets` may be a reusable
    # np.ndarray(dtype=uint64) of ELEMENT offsets, skipping per-call tuple
    # marshalling on the hot path. `keys` may also be a pre-serialized bytes
    # blob (the NUL-joined key list, e.g. via pack_keys) — engines that hold
    # a page hash chain can serialize it once and skip the per-request join.
    @staticmethod
    def pack_keys(keys: List[str]) -> bytes:
        """Serialize a key list for the write_pages/read_pages blob form."""
        return "\0".join(keys).encode()

    # quant mode -> (wire flag, page_size multiple in bf16 elements). The
    # native codec table (csrc/core/page_codec.h) is the authority;
    # tests/test_page_codec.py checks that the two agree.
    QUANT_MODES = {"fp8": (2, 8), "mxfp4": (4, 32)}
    FLAG_QUANT_FP8 = QUANT_MODES["fp8"][0]  # store bf16 pages fp8-compressed
    FLAG_QUANT_MXFP4 = QUANT_MODES["mxfp4"][0]  # store bf16 pages as OCP MXFP4

    # Segmented pages (csrc/core/page_codec.h, docs/design.md): the most
    # segments one page may have; tests/test_page_segments.py checks it
    # against the native constant.
    MAX_PAGE_SEGMENTS = 1024

    @classmethod
    def _check_segments(cls, numel: int, element_size: int, offsets, page_size: int,
                        segments: int, segment_stride: int,
                        quant: Optional[str] = None) -> None:
        """Refuse (ValueError) a segmented request the store cannot serve,
        before anything is sent: segments_legal's rules applied in elements,
        plus the bound check that keeps every segment inside the tensor.
        `quant` names the codec whose rules apply (None: plain pages; reads
        pass None, the server checks each stored page's own codec)."""
        if segments == 1:
            return
        if not 1 <= segments <= cls.MAX_PAGE_SEGMENTS:
            raise ValueError(f"segments must be in 1..{cls.MAX_PAGE_SEGMENTS}")
        if page_size <= 0 or page_size % segments != 0:
            raise ValueError("page_size must be a positive multiple of segments")
        seg = page_size // segments
        if segment_stride < seg:
            raise ValueError("segment_stride is smaller than a segment: the segments "
                             "of a page would overlap")
        if quant is not None:
            multiple = cls.QUANT_MODES[quant][1]
            if seg % multiple != 0:
                raise ValueError(f"{quant} quant needs segments of a multiple of "
                                 f"{multiple} elements")
            if (segment_stride * element_size) % 16 != 0:
                raise ValueError(f"{quant} quant needs a segment_stride that is a "
                                 "multiple of 16 bytes")
        if len(offsets) and (int(max(offsets)) + (segments - 1) * segment_stride + seg
                             > numel):
            raise ValueError("a segmented page extends outside the tensor")

    # Sliced reads (csrc/core/page_codec.h, docs/design.md): the most pieces
    # one slice may have; tests/test_page_slice.py checks it against the
    # native constant.
    MAX_SLICE_PIECES = 4096

    @classmethod
    def _check_slice(cls, numel: int, offsets, page_size: int, page_slice,
                     segments: int = 1, segment_stride: int = 0) -> None:
        """Refuse (ValueError) a sliced read the store cannot serve, before
        anything is sent: slice_legal's plain rules in elements (the server
        checks each stored page's own codec), page_size == count * piece, and
        the bound check that keeps every sliced page inside the tensor."""
        sl = PageSlice(*page_slice)
        if not 1 <= sl.count <= cls.MAX_SLICE_PIECES:
            raise ValueError(f"PageSlice.count must be in 1..{cls.MAX_SLICE_PIECES}")
        if sl.piece <= 0:
            raise ValueError("PageSlice.piece must be positive")
        if sl.offset < 0 or sl.page_size <= 0:
            raise ValueError("PageSlice.offset and page_size must not be negative")
        if sl.count > 1 and sl.stride < sl.piece:
            raise ValueError("PageSlice.stride is smaller than a piece: the pieces "
                             "would overlap")
        span = (sl.count - 1) * sl.stride if sl.count > 1 else 0
        if sl.offset + span + sl.piece > sl.page_size:
            raise ValueError("the slice extends outside the stored page")
        if page_size != sl.count * sl.piece:
            raise ValueError("page_size must be PageSlice.count * PageSlice.piece, the "
                             "size of the sliced page")
        if segments > 1 and sl.count % segments != 0:
            raise ValueError("PageSlice.count must be a multiple of segments: a piece "
                             "never straddles a segment")
        if segments == 1 and len(offsets) and int(max(offsets)) + page_size > numel:
            raise ValueError("a sliced page extends outside the tensor")
        # segments > 1: _check_segments bounds the segmented sliced page

    @staticmethod
    def _slice_arg(page_slice):
        """The native (n_pieces, page, offset, piece, stride) tuple, or None."""
        if page_slice is None:
            return None
        sl = PageSlice(*page_slice)
        return (sl.count, sl.page_size, sl.offset, sl.piece, sl.stride)

    # Tensor sets (csrc/core/page_codec.h, docs/design.md): the most tensors
    # one set may have and the most sets one connection may hold.
    MAX_PAGE_TENSORS = 128
    MAX_TENSOR_SETS = 16

    def register_tensor_set(self, tensors) -> "TensorSet":
        """Register an ordered list of tensors (one device, one dtype, e.g. an
        engine's per-layer KV tensors) on this connection, once. The returned
        TensorSet stands in for `cache` in write_pages / read_pages /
        read_pages_async (``tensor_set=``): a page is then the concatenation,
        in set order, of one equal part from each tensor, every part at the
        SAME offset inside its own tensor, so one key and one request move a
        block of all layers. The set keeps the tensors alive. Local path
        only."""
        tensors = list(tensors)
        if not self.local_connected:
            raise ValueError("tensor sets use the local GPU path")
        if not 1 <= len(tensors) <= self.MAX_PAGE_TENSORS:
            raise ValueError(f"a tensor set has 1..{self.MAX_PAGE_TENSORS} tensors")
        for t in tensors:
            if t.device != tensors[0].device or t.dtype != tensors[0].dtype:
                raise ValueError("the tensors of a set share one device and one dtype")
            if not t.is_contiguous():
                raise ValueError("the tensors of a set must be contiguous")
        for t in tensors:
            self._verify(t)
        es = tensors[0].element_size()
        set_id = self.conn.register_tensor_set(
            [t.data_ptr() for t in tensors], [t.numel() * es for t in tensors],
            _remap_device_id(tensors[0]))
        if set_id <= 0:
            raise Exception(f"Failed to register the tensor set, ret = {set_id}")
        return TensorSet(self, set_id, tensors)

    def release_tensor_set(self, ts: "TensorSet") -> None:
        """Release a registered set: its id is unknown to the server from then
        on, and the TensorSet can no longer be used."""
        if ts.conn is not self or ts.set_id is None:
            raise ValueError("not a live tensor set of this connection")
        ret = self.conn.release_tensor_set(ts.set_id)
        ts.set_id = None
        ts.tensors = []
        if ret < 0:
            raise Exception(f"Failed to release the tensor set, ret = {ret}")

    def _check_tensor_set(self, ts, offsets, page_size: int, segments: int,
                          segment_stride: int, quant: Optional[str] = None) -> None:
        """Refuse (ValueError) a request over a tensor set the store cannot
        serve, before anything is sent: tensors_legal's rules in elements and
        the bound check that keeps every part inside every tensor."""
        if not self.local_connected:
            raise ValueError("tensor sets use the local GPU path")
        if not isinstance(ts, TensorSet) or ts.conn is not self or ts.set_id is None:
            raise ValueError("not a live tensor set of this connection")
        G = len(ts.tensors)
        if not 1 <= segments <= self.MAX_PAGE_SEGMENTS or segments % G != 0:
            raise ValueError("segments is the total over all tensors: a multiple of their "
                             f"number, at most {self.MAX_PAGE_SEGMENTS}")
        if page_size <= 0 or page_size % segments != 0:
            raise ValueError("page_size must be a positive multiple of segments")
        seg, per = page_size // segments, segments // G
        if per > 1 and segment_stride < seg:
            raise ValueError("segment_stride is smaller than a segment: the segments "
                             "of a page would overlap")
        es = ts.tensors[0].element_size()
        if quant is not None:
            multiple = self.QUANT_MODES[quant][1]
            if ts.tensors[0].dtype != torch.bfloat16:
                raise ValueError(f"{quant} quant requires bf16 tensors")
            if seg % multiple != 0:
                raise ValueError(f"{quant} quant needs segments of a multiple of "
                                 f"{multiple} elements")
            if per > 1 and (segment_stride * es) % 16 != 0:
                raise ValueError(f"{quant} quant needs a segment_stride that is a "
                                 "multiple of 16 bytes")
            if any(t.data_ptr() % 16 for t in ts.tensors) or (offsets % np.uint64(8)).any():
                raise ValueError(f"{quant} quant needs 16-byte-aligned tensors and page "
                                 "offsets that are multiples of 8 elements")
        span = (per - 1) * segment_stride + seg if per > 1 else seg
        if len(offsets) and int(max(offsets)) + span > min(t.numel() for t in ts.tensors):
            raise ValueError("a page part extends outside a tensor of the set")

    def _rw_tensor_set(self, op, ts, keys, offs, page_size, sync, flags, segments,
                       segment_stride, ticketed=False):
        if not isinstance(keys, (bytes, bytearray, memoryview)):
            keys = self.pack_keys(keys)
        es = ts.tensors[0].element_size()
        per = segments // len(ts.tensors)
        return self.conn.rw_tset_blob(
            op, keys, offs, es, page_size * es, ts.set_id, len(ts.tensors),
            _remap_device_id(ts.tensors[0]), sync, flags, segments,
            segment_stride if per > 1 else 0, ticketed)

    def write_pages(self, cache: Optional[torch.Tensor], keys, offsets, page_size: int,
                    sync: bool = False, quant: Optional[str] = None,
                    segments: Optional[int] = None, segment_stride: int = 0,
                    tensor_set=None, **unsupported):
        """sync=True completes the write in ONE round trip (the response is
        sent when the copy finishes); sync=False (default) returns after the
        server accepts, so uploads overlap compute — call sync() later.

        quant="fp8": store the pages quantized to fp8 e4m3 (one absmax/448
        scale per page) at HALF the HBM footprint; requires a bf16 cache
        tensor and page_size % 8 == 0 (ValueError otherwise, like every
        refused quant argument), and reads of these keys dequantize back to
        bf16 transparently. Doubles effective cache capacity at ~3-bit mantissa
        precision — the usual KV-cache quantization trade.

        quant="mxfp4": store the pages as OCP microscaling FP4 — e2m1
        elements {0, .5, 1, 1.5, 2, 3, 4, 6} with one power-of-two (e8m0)
        scale per 32 consecutive elements, kept inside the stored block. A
        page takes 17/32 of a byte per element: 3.76x smaller than bf16 and
        1.88x smaller than quant="fp8". Requires a bf16 cache,
        page_size % 32 == 0, a 16-byte-aligned cache and page offsets that
        are multiples of 8 elements (ValueError otherwise, before anything
        is sent). Reads dequantize transparently and must use the written
        page_size. Values round to nearest (ties to even) after scaling by
        the group's absmax exponent; +-inf and anything above the group's
        range saturate to +-6 x scale; a group holding a NaN reads back as
        all NaN (e2m1 has no NaN code, so the OCP convention marks the
        group's scale); -0 keeps its sign.

        segments=S > 1: each page is S equal pieces of `cache`, piece s
        starting at offset + s * segment_stride (elements), e.g. S=2 and
        segment_stride=cache.numel() // 2 for a K/V-split
        ``[2, num_blocks, ...]`` cache. The stored page is the concatenation
        of the pieces, byte-identical to a contiguous write of it, so any
        reader, contiguous or segmented with any S, can fetch it. Local path
        only; an illegal geometry or a page that leaves the tensor is a
        ValueError before anything is sent.

        tensor_set=ts (from register_tensor_set) in place of `cache` (pass
        None): each page spans all tensors of the set, `offsets` are relative
        to every tensor, page_size is the whole page across all tensors and
        `segments` the total (default: one per tensor; a multiple of the number of tensors; with one
        segment per tensor segment_stride is ignored). fp8 then keeps one
        scale over the parts of all tensors.

        Slices are read-only: write_pages has no page_slice parameter, and
        passing one is a ValueError."""
        if "page_slice" in unsupported:
            raise ValueError("page_slice is read-only: there is no sliced write")
        if unsupported:
            raise TypeError(f"write_pages() got an unexpected keyword argument "
                            f"{next(iter(unsupported))!r}")
        if tensor_set is not None:
            if cache is not None:
                raise ValueError("pass either cache or tensor_set")
            if quant is not None and quant not in self.QUANT_MODES:
                raise ValueError(f"unsupported quant mode {quant!r}")
            if segments is None:  # not given: one segment per tensor
                segments = len(getattr(tensor_set, "tensors", ())) or 1
            offs = np.asarray(offsets, dtype=np.uint64)
            self._check_tensor_set(tensor_set, offs, page_size, segments, segment_stride, quant)
            flags = self.QUANT_MODES[quant][0] if quant is not None else 0
            ret, _ = self._rw_tensor_set(self.OP_W, tensor_set, keys, offs, page_size, sync,
                                         flags, segments, segment_stride)
            if ret < 0:
                raise Exception(f"Failed to write to infinistore, ret = {ret}")
            return 0
        segments = 1 if segments is None else segments
        self._verify(cache)
        if segments != 1 and not self.local_connected:
            raise ValueError("segmented pages use the local GPU path")
        assert self.local_connected, "write_pages uses the local GPU path"
        flags = 0
        if quant is not None:
            if quant not in self.QUANT_MODES:
                raise ValueError(f"unsupported quant mode {quant!r}")
            flags, multiple = self.QUANT_MODES[quant]
            if cache.dtype != torch.bfloat16:
                raise ValueError(f"{quant} quant requires a bf16 cache")
            if page_size <= 0 or page_size % multiple != 0:
                raise ValueError(f"{quant} quant needs page_size % {multiple} == 0")
        es = cache.element_size()
        offs = np.asarray(offsets, dtype=np.uint64)
        if quant is not None:
            # the quantize kernel loads 16 bytes (8 bf16) per lane
            if cache.data_ptr() % 16 != 0 or (offs % np.uint64(8)).any():
                raise ValueError(
                    f"{quant} quant needs a 16-byte-aligned cache and page offsets "
                    "that are multiples of 8 elements")
        self._check_segments(cache.numel(), es, offs, page_size, segments,
                             segment_stride, quant)
        if isinstance(keys, (bytes, bytearray, memoryview)):
            ret = self.conn.rw_local_blob(
                self.OP_W, keys, offs, es, page_size * es,
                cache.data_ptr(), _remap_device_id(cache), sync, flags,
                segments, segment_stride,
            )
        else:
            ret = self.conn.rw_local_keys(
                self.OP_W, keys, offs, es, page_size * es,
                cache.data_ptr(), _remap_device_id(cache), sync, flags,
                segments, segment_stride,
            )
        if ret < 0:
            raise Exception(f"Failed to write to infinistore, ret = {ret}")
        return 0

    def read_pages(self, cache: Optional[torch.Tensor], keys, offsets, page_size: int,
                   segments: Optional[int] = None, segment_stride: int = 0,
                   page_slice: Optional[PageSlice] = None, tensor_set=None):
        """segments / segment_stride: scatter each page into that many equal
        pieces of `cache` (see write_pages), however the page was written.
        Local path only.

        page_slice: fetch only that strided part of every stored page (see
        PageSlice), e.g. a decode rank's heads of pages a prefill engine
        stored under another tensor-parallel degree. page_size is then the
        SLICED page, count * piece, and segments apply to it (count must be a
        multiple of segments). Every key must have been written with
        page_slice.page_size elements; for fp8 and mxfp4 pages offset, piece
        and stride are multiples of 8 and 32 elements (the server answers
        INVALID_REQ otherwise). Only the requested elements are read and
        dequantized. Local path only; an illegal geometry or a page that
        leaves the tensor is a ValueError before anything is sent.

        tensor_set=ts in place of `cache` (pass None): scatter each page over
        the tensors of the set (see write_pages), however it was written.
        Not together with page_slice."""
        if tensor_set is not None:
            offs = self._tensor_set_read_args(cache, tensor_set, offsets, page_size,
                                              segments, segment_stride, page_slice)
            segments = len(tensor_set.tensors) if segments is None else segments
            ret, _ = self._rw_tensor_set(self.OP_R, tensor_set, keys, offs, page_size, False,
                                         0, segments, segment_stride)
            if ret < 0:
                raise Exception(f"Failed to read from infinistore, ret = {ret}")
            return
        segments = 1 if segments is None else segments
        self._verify(cache)
        if segments != 1 and not self.local_connected:
            raise ValueError("segmented pages use the local GPU path")
        if page_slice is not None and not self.local_connected:
            raise ValueError("sliced reads use the local GPU path")
        es = cache.element_size()
        if self.local_connected:
            offs = np.asarray(offsets, dtype=np.uint64)
            if page_slice is not None:
                self._check_slice(cache.numel(), offs, page_size, page_slice, segments,
                                  segment_stride)
            self._check_segments(cache.numel(), es, offs, page_size, segments,
                                 segment_stride)
            if isinstance(keys, (bytes, bytearray, memoryview)):
                ret = self.conn.rw_local_blob(
                    self.OP_R, keys, offs, es, page_size * es,
                    cache.data_ptr(), _remap_device_id(cache), False, 0,
                    segments, segment_stride, self._slice_arg(page_slice),
                )
            else:
                ret = self.conn.rw_local_keys(
                    self.OP_R, keys, offs, es, page_size * es,
                    cache.data_ptr(), _remap_device_id(cache), False, 0,
                    segments, segment_stride, self._slice_arg(page_slice),
                )
        elif self.rdma_connected:
            blocks = [(k, int(o) * es) for k, o in zip(keys, offsets)]
            ret = self.conn.r_rdma(blocks, page_size * es, cache.data_ptr())
        else:
            raise Exception("Not connected to any instance")
        if ret < 0:
            raise Exception(f"Failed to read from infinistore, ret = {ret}")

    def _tensor_set_read_args(self, cache, tensor_set, offsets, page_size, segments,
                              segment_stride, page_slice):
        if cache is not None:
            raise ValueError("pass either cache or tensor_set")
        if page_slice is not None:
            raise ValueError("page_slice and tensor_set cannot be combined")
        if segments is None:  # not given: one segment per tensor
            segments = len(getattr(tensor_set, "tensors", ())) or 1
        offs = np.asarray(offsets, dtype=np.uint64)
        self._check_tensor_set(tensor_set, offs, page_size, segments, segment_stride)
        return offs

    def read_pages_async(self, cache: Optional[torch.Tensor], keys, offsets, page_size: int,
                         segments: Optional[int] = None, segment_stride: int = 0,
                         page_slice: Optional[PageSlice] = None, tensor_set=None):
        """Ticketed read (local path, shm ring): pushes the request and
        returns a ticket; call wait_read(ticket) before using the data. Lets
        an engine overlap its own work (or further requests) with the copy —
        e.g. prefetching the next sequence's KV pages while decoding. Falls
        back to a blocking read (ticket 0) when the ring is unavailable.
        segments / segment_stride / page_slice / tensor_set as in read_pages."""
        if tensor_set is not None:
            offs = self._tensor_set_read_args(cache, tensor_set, offsets, page_size,
                                              segments, segment_stride, page_slice)
            segments = len(tensor_set.tensors) if segments is None else segments
            ret, ticket = self._rw_tensor_set(self.OP_R, tensor_set, keys, offs, page_size,
                                              True, 0, segments, segment_stride, ticketed=True)
            if ret < 0:
                raise Exception(f"Failed to read from infinistore, ret = {ret}")
            return ticket
        segments = 1 if segments is None else segments
        self._verify(cache)
        if segments != 1 and not self.local_connected:
            raise ValueError("segmented pages use the local GPU path")
        if page_slice is not None and not self.local_connected:
            raise ValueError("sliced reads use the local GPU path")
        assert self.local_connected, "read_pages_async uses the local GPU path"
        es = cache.element_size()
        offs = np.asarray(offsets, dtype=np.uint64)
        if page_slice is not None:
            self._check_slice(cache.numel(), offs, page_size, page_slice, segments,
                              segment_stride)
        self._check_segments(cache.numel(), es, offs, page_size, segments,
                             segment_stride)
        if not isinstance(keys, (bytes, bytearray, memoryview)):
            keys = self.pack_keys(keys)
        ret, ticket = self.conn.rw_local_blob_async(
            self.OP_R, keys, offs, es, page_size * es,
            cache.data_ptr(), _remap_device_id(cache), segments, segment_stride,
            self._slice_arg(page_slice),
        )
        if ret < 0:
            raise Exception(f"Failed to read from infinistore, ret = {ret}")
        return ticket

    def wait_read(self, ticket: int):
        ret = self.conn.wait_local_ticket(ticket)
        if ret < 0:
            raise Exception(f"Async read failed, ret = {ret}")

    def read_cache(self, cache: torch.Tensor, blocks: List[Tuple[str, int]], page_size: int):
        """Read pages into `cache` (offsets in elements)."""
        self._verify(cache)
        element_size = cache.element_size()
        if self.local_connected:
            blob, offs, n = self._pack_blocks(blocks, element_size)
            ret = self.conn.rw_local_fast(
                self.OP_R,
                blob,
                offs,
                n,
                page_size * element_size,
                cache.data_ptr(),
                _remap_device_id(cache),
            )
        elif self.rdma_connected:
            blocks_in_bytes = [(key, offset * element_size) for key, offset in blocks]
            ret = self.conn.r_rdma(
                blocks_in_bytes, page_size * element_size, cache.data_ptr()
            )
        else:
            raise Exception("Not connected to any instance")
        if ret < 0:
            raise Exception(f"Failed to read from infinistore, ret = {ret}")

    async def read_cache_async(
        self, cache: torch.Tensor, blocks: List[Tuple[str, int]], page_size: int
    ):
        if not self.rdma_connected:
            raise Exception("this function is only valid for connected rdma")
        self._verify(cache)
        element_size = cache.element_size()
        blocks_in_bytes = [(key, offset * element_size) for key, offset in blocks]
        loop = asyncio.get_running_loop()
        future = loop.create_future()

        def _callback():
            loop.call_soon_threadsafe(future.set_result, 0)

        ret = self.conn.r_rdma_async(
            blocks_in_bytes, page_size * element_size, cache.data_ptr(), _callback
        )
        if ret < 0:
            raise Exception(f"Failed to read from infinistore, ret = {ret}")
        return await future

    # -- RDMA-semantics path --------------------------------------------------
    def register_mr(self, cache: torch.Tensor):
        self._verify(cache)
        if not self.rdma_connected:
            raise Exception("this function is only valid for connected rdma")
        ret = self.conn.register_mr(cache.data_ptr(), cache.numel() * cache.element_size())
        if ret < 0:
            raise Exception("register memory region failed")
        return ret

    def allocate_rdma(self, keys: List[str], page_size_in_bytes: int):
        if not self.rdma_connected:
            raise Exception("this function is only valid for connected rdma")
        ret = self.conn.allocate_rdma(keys, page_size_in_bytes)
        if len(ret) == 0:
            raise Exception("allocate memory failed")
        return ret

    async def allocate_rdma_async(self, keys: List[str], page_size_in_bytes: int):
        if not self.rdma_connected:
            raise Exception("this function is only valid for connected rdma")
        loop = asyncio.get_running_loop()
        future = loop.create_future()

        def _callback(remote_blocks):
            loop.call_soon_threadsafe(future.set_result, remote_blocks)

        self.conn.allocate_rdma_async(keys, page_size_in_bytes, _callback)
        return await future

    def rdma_write_cache(
        self, cache: torch.Tensor, offsets: List[int], page_size, remote_blocks: List
    ):
        assert self.rdma_connected
        self._verify(cache)
        element_size = cache.element_size()
        offsets_in_bytes = [offset * element_size for offset in offsets]
        ret = self.conn.w_rdma(
            offsets_in_bytes,
            page_size * element_size,
            [tuple(b) for b in remote_blocks],
            cache.data_ptr(),
        )
        if ret < 0:
            raise Exception(f"Failed to write to infinistore, ret = {ret}")
        return 0

    async def rdma_write_cache_async(
        self, cache: torch.Tensor, offsets: List[int], page_size, remote_blocks: List
    ):
        if not self.rdma_connected:
            raise Exception("this function is only valid for connected rdma")
        self._verify(cache)
        element_size = cache.element_size()
        offsets_in_bytes = [offset * element_size for offset in offsets]
        loop = asyncio.get_running_loop()
        future = loop.create_future()

        def _callback():
            loop.call_soon_threadsafe(future.set_result, 0)

        self.conn.w_rdma_async(
            offsets_in_bytes,
            page_size * element_size,
            [tuple(b) for b in remote_blocks],
            cache.data_ptr(),
            _callback,
        )
        return await future

    # -- sync / queries -------------------------------------------------------
    def sync(self):
        if self.local_connected:
            n = 0
            timeout = 1.0
            start = time.time()
            while True:
                ret = self.conn.sync_local()
                if ret < 0:
                    raise Exception(f"Failed to sync with infinistore, ret = {ret}")
                if ret == 0:
                    return
                if time.time() - start > timeout:
                    raise Exception("Timeout waiting for inflight requests")
                time.sleep(ret * 0.0005)
                n += 1
        elif self.rdma_connected:
            ret = self.conn.sync_rdma()
            if ret < 0:
                raise Exception(f"Failed to sync with infinistore, ret = {ret}")
        else:
            raise Exception("Not connected to any instance")

    def check_exist(self, key: str):
        ret = self.conn.check_exist(key)
        if ret < 0:
            raise Exception("Failed to check if this key exists")
        return ret == 0

    def get_match_last_index(self, keys: List[str]):
        ret = self.conn.get_match_last_index(keys)
        if ret < 0:
            raise Exception("can't find a match")
        return ret

    def get_server_stats_remote(self) -> str:
        """Server stats JSON fetched over the wire (extension) — works from
        any client, no management port needed."""
        return self.conn.get_stats()

    def delete_keys(self, keys: List[str]) -> int:
        """Delete keys from the store; returns the number removed.
        Extension over the reference (which only offers wholesale purge) —
        lets the inference engine evict cold prefixes."""
        ret = self.conn.delete_keys(keys)
        if ret < 0:
            raise Exception("Failed to delete keys")
        return ret

    # -- internal -------------------------------------------------------------
    def _verify(self, cache: torch.Tensor):
        if (not self.rdma_connected) and cache.device.type != "cuda":
            raise Exception("Tensor must be on CUDA device for local GPU connection")
        if cache.is_contiguous() is False:
            raise Exception("Tensor must be contiguous")


def fingerprint_blocks(cache: torch.Tensor, offsets: List[int], page_size: int):
    """GPU-accelerated 64-bit fingerprints of pages of `cache` (offsets and
    page_size in elements) — one HIP kernel launch. Use to build prefix-hash
    key chains for `get_match_last_index` without reading the KV data back to
    the host. Extension over the reference (new capability)."""
    if cache.device.type != "cuda":
        raise Exception("fingerprint_blocks requires a CUDA (ROCm) tensor")
    if not cache.is_contiguous():
        raise Exception("Tensor must be contiguous")
    es = cache.element_size()
    return _native.hash_blocks(
        cache.data_ptr(),
        [o * es for o in offsets],
        page_size * es,
        cache.device.index or 0,
    )
