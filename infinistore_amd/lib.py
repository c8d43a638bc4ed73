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


class PagePermute(NamedTuple):
    """Client-side piece order of a page (docs/design.md, "permuted pages"):
    the tensor holds each page as [outer, cols, rows, piece] while the store
    keeps, and every other reader sees, [outer, rows, cols, piece]. The piece
    is page_size // (outer * rows * cols) elements. E.g. a head-major
    [2, H, T, hd] cache block sharing keys with token-major [2, T, H, hd]
    engines: PagePermute(2, T, H)."""

    outer: int
    rows: int
    cols: int


class PageTranspose(NamedTuple):
    """Client-side element order of a page (docs/design.md, "transposed
    pages"): the tensor holds each page as a paged-attention cache block, per
    half and head K as [head_dim // inner_k, tokens, inner_k] and V as
    [head_dim // inner_v, tokens, inner_v], while the store keeps, and every
    other reader sees, [halves, tokens, heads, head_dim]. All values are in
    elements. vLLM's key_cache [blocks, H, hd/x, T, x] and value_cache
    [blocks, H, hd, T] of a bf16 model: PageTranspose(T, H, hd, 8), with
    segments=2 when K and V are the two halves of one allocation."""

    tokens: int
    heads: int
    head_dim: int
    inner_k: int
    inner_v: int = 1
    halves: int = 2


class PageShuffle(NamedTuple):
    """Client-side element order of a page (docs/design.md, "shuffled pages"):
    the tensor holds each page as the shuffled cache block that assembly
    paged-attention kernels read, per half and head one tile of tokens x
    head_dim elements, with X = 16 // elem_bytes, as [head_dim // X, tokens, X]
    (form "k") or [tokens // X, head_dim, X] (form "v"), while the store keeps,
    and every other reader sees, [halves, tokens, heads, head_dim]. forms[o] is
    half o's form; a one-half page (separate key and value tensors) uses
    forms[0]. elem_bytes must be the tensor's element size. A bf16 engine's
    key_cache [blocks, H, hd/8, T, 8] and value_cache [blocks, H, T/8, hd, 8] in
    one [2, blocks, ...] allocation: PageShuffle(T, H, hd) with segments=2."""

    tokens: int
    heads: int
    head_dim: int
    elem_bytes: int = 2
    halves: int = 2
    forms: tuple = ("k", "v")


class PageCast:
    """Client-side element type of a page (docs/design.md, "cast pages"): the
    tensor (torch.float8_e4m3fn or uint8) holds each page as one-byte OCP
    e4m3fn codes, element value = code value * scales[h] with h the half of
    the page (K, then V) the element lies in, vLLM's kv_cache_dtype="fp8"
    convention with k_scale and v_scale. The store keeps, and every other
    reader sees, the bf16 page of the dequantized values. scales: one or two
    finite, positive, normal float32 values; halves defaults to their number,
    and PageCast([s], halves=2) applies one scale to both halves."""

    __slots__ = ("scales", "halves")

    def __init__(self, scales, halves: Optional[int] = None):
        scales = [scales] if isinstance(scales, (int, float)) else list(scales)
        if len(scales) not in (1, 2):
            raise ValueError("PageCast takes one or two scales")
        self.scales = tuple(float(np.float32(x)) for x in scales)
        self.halves = len(scales) if halves is None else int(halves)
        if self.halves not in (1, 2) or self.halves < len(scales):
            raise ValueError("PageCast.halves is 1 or 2, and at least the number of scales")

    def wire(self):
        """What the native calls take: (elem_type, halves, scale_k, scale_v)."""
        return (1, self.halves, self.scales[0], self.scales[-1])

    def __repr__(self):
        return f"PageCast(scales={self.scales}, halves={self.halves})"


class PageRotate:
    """Read-side rotation of cached keys (docs/design.md, "rotated reads"): a
    read delivers every page, [halves, T, heads, head_dim] bf16 with T implied
    by the page size, with the rotary pairs of its K half (half 0) turned by
    one angle per pair, which moves keys that carry RoPE for position p to
    position p + delta. cos_sin is a float32 array [P, 2] of (cos, sin), P =
    rot_dim / 2; rot_dim defaults to head_dim, and channels at or above it
    are copied (partial rotary). style "neox" pairs channel i with i + P,
    "gptj" pairs 2i with 2i + 1. V, the second half when halves == 2, is
    copied. One table, hence one position delta, per request."""

    STYLES = {"neox": 1, "gptj": 2}
    __slots__ = ("heads", "head_dim", "rot_dim", "style", "halves", "cos_sin")

    def __init__(self, heads: int, head_dim: int, cos_sin, rot_dim: Optional[int] = None,
                 style: str = "neox", halves: int = 2):
        if style not in self.STYLES:
            raise ValueError(f"PageRotate.style is one of {tuple(self.STYLES)}")
        self.heads, self.head_dim, self.halves = int(heads), int(head_dim), int(halves)
        self.rot_dim = self.head_dim if rot_dim is None else int(rot_dim)
        self.style = style
        self.cos_sin = np.ascontiguousarray(cos_sin, dtype=np.float32)
        if self.cos_sin.ndim != 2 or self.cos_sin.shape[1] != 2:
            raise ValueError("PageRotate.cos_sin is a [rot_dim / 2, 2] array of (cos, sin)")
        if self.cos_sin.shape[0] * 2 != self.rot_dim:
            raise ValueError("PageRotate.cos_sin has one (cos, sin) row per pair, rot_dim / 2")

    @classmethod
    def from_delta(cls, delta, heads: int, head_dim: int, theta: float = 10000.0,
                   rot_dim: Optional[int] = None, style: str = "neox", halves: int = 2):
        """The table that moves keys by `delta` positions: pair i turns by
        delta * theta ** (-2i / rot_dim), computed in float64 and rounded to
        float32."""
        rd = int(head_dim if rot_dim is None else rot_dim)
        i = np.arange(rd // 2, dtype=np.float64)
        ang = np.float64(delta) * np.float64(theta) ** (-2.0 * i / rd)
        return cls(heads, head_dim, np.stack([np.cos(ang), np.sin(ang)], axis=1), rd, style,
                   halves)

    def wire(self):
        """What the native calls take: (style, halves, heads, head_dim,
        rot_dim, float32 table)."""
        return (self.STYLES[self.style], self.halves, self.heads, self.head_dim, self.rot_dim,
                self.cos_sin.reshape(-1))

    def __repr__(self):
        return (f"PageRotate(heads={self.heads}, head_dim={self.head_dim}, "
                f"rot_dim={self.rot_dim}, style={self.style!r}, halves={self.halves})")


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

    # kMaxPermPieces in csrc/core/page_codec.h: the pieces one permuted page
    # may have; tests/test_page_permute.py checks it against the native value.
    MAX_PERM_PIECES = 1 << 20

    def _permute_arg(self, page_permute, page_size: int, segments: int, quant=None,
                     page_slice=None, tensor_set=None):
        """Refuse (ValueError) a permuted request the store cannot serve,
        before anything is sent: permute_legal's rules applied in elements.
        Returns None, or what the native calls take: (outer, rows, cols,
        piece) with the piece in elements."""
        if page_permute is None:
            return None
        if page_slice is not None or tensor_set is not None:
            raise ValueError("page_permute cannot be combined with page_slice or tensor_set")
        if not self.local_connected:
            raise ValueError("permuted pages use the local GPU path")
        pm = PagePermute(*page_permute)
        if min(pm) < 1:
            raise ValueError("PagePermute outer, rows and cols must be >= 1")
        pieces = pm.outer * pm.rows * pm.cols
        if pieces > self.MAX_PERM_PIECES:
            raise ValueError(f"a permuted page has at most {self.MAX_PERM_PIECES} pieces")
        if page_size <= 0 or page_size % pieces != 0:
            raise ValueError("page_size must be a positive multiple of outer * rows * cols")
        if segments < 1 or pieces % segments != 0:
            raise ValueError("outer * rows * cols must be a multiple of segments: a piece "
                             "never straddles a segment")
        piece = page_size // pieces
        if quant is not None and piece % self.QUANT_MODES[quant][1] != 0:
            raise ValueError(f"{quant} quant needs pieces of a multiple of "
                             f"{self.QUANT_MODES[quant][1]} elements")
        return (pm.outer, pm.rows, pm.cols, piece)

    # PageCodec ids of csrc/core/page_codec.h, for the native predicates.
    QUANT_CODECS = {None: 0, "fp8": 1, "mxfp4": 2}

    def _transpose_arg(self, page_transpose, cache, offsets, page_size: int, segments: int,
                       segment_stride: int, quant=None, page_slice=None, tensor_set=None,
                       page_permute=None):
        """Refuse (ValueError) a transposed request the store cannot serve,
        before anything is sent; the geometry rule is the native
        transpose_legal. Returns None, or what the native calls take:
        (halves, tokens, heads, head_dim, element bytes, inner_k, inner_v)."""
        if page_transpose is None:
            return None
        if page_slice is not None or tensor_set is not None or page_permute is not None:
            raise ValueError("page_transpose cannot be combined with page_slice, tensor_set "
                             "or page_permute")
        if not self.local_connected:
            raise ValueError("transposed pages use the local GPU path")
        xp = PageTranspose(*page_transpose)
        es = cache.element_size()
        geo = (xp.halves, xp.tokens, xp.heads, xp.head_dim, es, xp.inner_k, xp.inner_v)
        if min(geo) < 1 or max(geo) >= 1 << 32 or not 0 < page_size < 1 << 60:
            raise ValueError("PageTranspose values and page_size must be positive")
        if quant is not None and cache.dtype != torch.bfloat16:
            raise ValueError(f"{quant} quant requires a bf16 cache")
        if not _native._dbg_transpose_legal(self.QUANT_CODECS[quant], page_size * es, geo,
                                            segments, segment_stride * es):
            raise ValueError(
                "illegal page transpose: page_size is halves * tokens * heads * head_dim; "
                "inner_k and inner_v are powers of two dividing head_dim, at most 16 bytes, "
                "with tokens runs filling whole 16-byte units; a head_dim row is a multiple "
                "of 16 bytes (of 32 elements with mxfp4); tokens * head_dim is at most "
                f"{_native._MAX_TRANSPOSE_TILE} bytes; halves * heads is a multiple of segments")
        offs = np.asarray(offsets, dtype=np.uint64)
        if (cache.data_ptr() % 16 != 0 or (offs * np.uint64(es) % np.uint64(16)).any()
                or (segments != 1 and segment_stride * es % 16 != 0)):
            raise ValueError("transposed pages need a 16-byte-aligned cache, page offsets and "
                             "segment stride")
        return geo

    SHUFFLE_FORMS = {"k": 1, "v": 2}

    def _shuffle_arg(self, page_shuffle, cache, offsets, page_size: int, segments: int,
                     segment_stride: int, quant=None, page_slice=None, tensor_set=None,
                     page_permute=None, page_transpose=None, page_cast=None, page_rotate=None):
        """Refuse (ValueError) a shuffled request the store cannot serve,
        before anything is sent; the geometry rule is the native
        shuffle_legal. Returns what the native calls take: (halves, tokens,
        heads, head_dim, element bytes, form_k, form_v)."""
        if (page_slice is not None or tensor_set is not None or page_permute is not None
                or page_transpose is not None or page_cast is not None
                or page_rotate is not None):
            raise ValueError("page_shuffle cannot be combined with page_slice, tensor_set, "
                             "page_permute, page_transpose, page_cast or page_rotate")
        if not self.local_connected:
            raise ValueError("shuffled pages use the local GPU path")
        sh = PageShuffle(*page_shuffle)
        forms = tuple(sh.forms) if isinstance(sh.forms, (tuple, list)) else ()
        if not 1 <= len(forms) <= 2 or any(f not in self.SHUFFLE_FORMS for f in forms):
            raise ValueError('PageShuffle forms are one or two of "k" and "v"')
        fk, fv = self.SHUFFLE_FORMS[forms[0]], self.SHUFFLE_FORMS[forms[-1]]
        es = cache.element_size()
        if sh.elem_bytes != es:
            raise ValueError(f"PageShuffle elem_bytes is {sh.elem_bytes}, the cache's element "
                             f"size is {es}")
        if quant is not None and quant not in self.QUANT_MODES:
            raise ValueError(f"unsupported quant mode {quant!r}")
        if quant is not None and cache.dtype != torch.bfloat16:
            raise ValueError(f"{quant} quant requires a bf16 cache")
        geo = (sh.halves, sh.tokens, sh.heads, sh.head_dim, es, fk, fv)
        if (min(geo) < 1 or max(geo) >= 1 << 32 or not 0 < page_size < 1 << 60
                or not 0 < segments < 1 << 32 or segment_stride < 0):
            raise ValueError("PageShuffle values, page_size and segments must be positive")
        if not _native._dbg_shuffle_legal(self.QUANT_CODECS[quant], page_size * es, geo,
                                          segments, segment_stride * es):
            raise ValueError(
                "illegal page shuffle: page_size is halves * tokens * heads * head_dim with "
                "halves 1 or 2; tokens and head_dim are multiples of 16 // elem_bytes "
                "(head_dim of 32 with mxfp4); a quant needs 2-byte elements; halves * heads is "
                f"a multiple of segments, at most {self.MAX_PAGE_SEGMENTS}, with a "
                "segment_stride of at least one segment")
        offs = np.asarray(offsets, dtype=np.uint64)
        if (cache.data_ptr() % 16 != 0 or (offs * np.uint64(es) % np.uint64(16)).any()
                or (segments != 1 and segment_stride * es % 16 != 0)):
            raise ValueError("shuffled pages need a 16-byte-aligned cache, page offsets and "
                             "segment stride")
        if len(offs) and (int(offs.max()) + (segments - 1) * segment_stride
                          + page_size // segments > cache.numel()):
            raise ValueError("a shuffled page extends outside the tensor")
        return geo

    def _rw_shuffled(self, op, cache, keys, offsets, page_size, segments, segment_stride, shuf,
                     sync=False, flags=0, ticketed=False):
        """One shuffled request. Returns the ticket (0 unless ticketed)."""
        offs = np.asarray(offsets, dtype=np.uint64)
        es = cache.element_size()
        args = (es, page_size * es, cache.data_ptr(), _remap_device_id(cache))
        ticket = 0
        if ticketed:
            if not isinstance(keys, (bytes, bytearray, memoryview)):
                keys = self.pack_keys(keys)
            ret, ticket = self.conn.rw_local_blob_async(
                op, keys, offs, *args, segments, segment_stride, None, None, None, None, None,
                shuf)
        elif isinstance(keys, (bytes, bytearray, memoryview)):
            ret = self.conn.rw_local_blob(op, keys, offs, *args, sync, flags, segments,
                                          segment_stride, None, None, None, None, None, shuf)
        else:
            ret = self.conn.rw_local_keys(op, keys, offs, *args, sync, flags, segments,
                                          segment_stride, None, None, None, None, None, shuf)
        if ret < 0:
            what = "write to" if op == self.OP_W else "read from"
            raise Exception(f"Failed to {what} infinistore, ret = {ret}")
        return ticket

    CAST_DTYPES = (torch.float8_e4m3fn, torch.uint8)

    def _cast_arg(self, page_cast, cache, offsets, page_size: int, segments: int,
                  segment_stride: int, quant=None, page_slice=None, tensor_set=None,
                  page_permute=None, page_transpose=None):
        """Refuse (ValueError) a cast request the store cannot serve, before
        anything is sent; the geometry rule is the native cast_legal. Returns
        what the native calls take: (1, halves, scale_k, scale_v)."""
        if (page_slice is not None or tensor_set is not None or page_permute is not None
                or page_transpose is not None):
            raise ValueError("page_cast cannot be combined with page_slice, tensor_set, "
                             "page_permute or page_transpose")
        if not self.local_connected:
            raise ValueError("cast pages use the local GPU path")
        if not isinstance(page_cast, PageCast):
            raise ValueError("page_cast must be a PageCast")
        if cache.dtype not in self.CAST_DTYPES:
            raise ValueError("page_cast needs a torch.float8_e4m3fn or uint8 cache")
        if quant is not None and quant not in self.QUANT_MODES:
            raise ValueError(f"unsupported quant mode {quant!r}")
        if not 0 < page_size < 1 << 60 or not 0 < segments < 1 << 32 or segment_stride < 0:
            raise ValueError("page_size and segments must be positive")
        if not _native._dbg_cast_legal(self.QUANT_CODECS[quant], page_size * 2, page_cast.wire(),
                                       segments, segment_stride):
            raise ValueError(
                "illegal page cast: scales are finite, positive, normal float32 values; "
                "page_size / halves is a multiple of 8 elements (32 with mxfp4); segments "
                "are equal parts of a multiple of 8 (32) elements, at most "
                f"{self.MAX_PAGE_SEGMENTS}, with a segment_stride of at least one segment "
                "and a multiple of 16")
        offs = np.asarray(offsets, dtype=np.uint64)
        if cache.data_ptr() % 16 != 0 or (offs % np.uint64(16)).any():
            raise ValueError("cast pages need a 16-byte-aligned cache and page offsets")
        if len(offs) and (int(offs.max()) + (segments - 1) * segment_stride
                          + page_size // segments > cache.numel()):
            raise ValueError("a cast page extends outside the tensor")
        return page_cast.wire()

    def _rw_cast(self, op, cache, keys, offsets, page_size, segments, segment_stride, cast,
                 sync=False, flags=0, ticketed=False):
        """One cast request: element size 1, block size the LOGICAL bf16 bytes,
        offsets and stride in client bytes. Returns the ticket (0 unless
        ticketed)."""
        offs = np.asarray(offsets, dtype=np.uint64)
        args = (1, page_size * 2, cache.data_ptr(), _remap_device_id(cache))
        ticket = 0
        if ticketed:
            if not isinstance(keys, (bytes, bytearray, memoryview)):
                keys = self.pack_keys(keys)
            ret, ticket = self.conn.rw_local_blob_async(
                op, keys, offs, *args, segments, segment_stride, None, None, None, cast)
        elif isinstance(keys, (bytes, bytearray, memoryview)):
            ret = self.conn.rw_local_blob(op, keys, offs, *args, sync, flags, segments,
                                          segment_stride, None, None, None, cast)
        else:
            ret = self.conn.rw_local_keys(op, keys, offs, *args, sync, flags, segments,
                                          segment_stride, None, None, None, cast)
        if ret < 0:
            what = "write to" if op == self.OP_W else "read from"
            raise Exception(f"Failed to {what} infinistore, ret = {ret}")
        return ticket

    def _rotate_arg(self, page_rotate, cache, offsets, page_size: int, segments: int,
                    segment_stride: int, page_slice=None, tensor_set=None, page_permute=None,
                    page_transpose=None, page_cast=None):
        """Refuse (ValueError) a rotated read the store cannot serve, before
        anything is sent; the geometry rule is the native rotate_legal under
        plain rules (the server judges every entry against its own codec).
        Returns what the native calls take, PageRotate.wire()."""
        if (page_slice is not None or tensor_set is not None or page_permute is not None
                or page_transpose is not None or page_cast is not None):
            raise ValueError("page_rotate cannot be combined with page_slice, tensor_set, "
                             "page_permute, page_transpose or page_cast")
        if not self.local_connected:
            raise ValueError("rotated reads use the local GPU path")
        if not isinstance(page_rotate, PageRotate):
            raise ValueError("page_rotate must be a PageRotate")
        if cache.dtype != torch.bfloat16:
            raise ValueError("page_rotate needs a torch.bfloat16 cache")
        if not 0 < page_size < 1 << 60 or not 0 < segments < 1 << 32 or segment_stride < 0:
            raise ValueError("page_size and segments must be positive")
        rot = page_rotate.wire()
        if not _native._dbg_rotate_legal(0, page_size * 2, rot, segments, segment_stride * 2):
            raise ValueError(
                "illegal page rotation: halves is 1 or 2; head_dim is a multiple of 8 and "
                "rot_dim <= head_dim an even number of at most "
                f"{2 * _native._MAX_ROTATE_PAIRS} channels, rot_dim / 2 a multiple of 8 "
                "(neox) or rot_dim a multiple of 8 (gptj); page_size is a multiple of halves * "
                "heads * head_dim; segments hold whole (token, head) rows with a "
                "segment_stride of a multiple of 8 elements; the table is finite")
        offs = np.asarray(offsets, dtype=np.uint64)
        if cache.data_ptr() % 16 != 0 or (offs % np.uint64(8)).any():
            raise ValueError("rotated reads need a 16-byte-aligned cache and page offsets")
        if len(offs) and (int(offs.max()) + (segments - 1) * segment_stride
                          + page_size // segments > cache.numel()):
            raise ValueError("a rotated page extends outside the tensor")
        return rot

    def _read_rotated(self, cache, keys, offsets, page_size, segments, segment_stride, rot,
                      ticketed=False):
        """One rotated read. Returns the ticket (0 unless ticketed)."""
        offs = np.asarray(offsets, dtype=np.uint64)
        args = (2, page_size * 2, cache.data_ptr(), _remap_device_id(cache))
        ticket = 0
        if ticketed:
            if not isinstance(keys, (bytes, bytearray, memoryview)):
                keys = self.pack_keys(keys)
            ret, ticket = self.conn.rw_local_blob_async(
                self.OP_R, keys, offs, *args, segments, segment_stride, None, None, None, None,
                rot)
        elif isinstance(keys, (bytes, bytearray, memoryview)):
            ret = self.conn.rw_local_blob(self.OP_R, keys, offs, *args, False, 0, segments,
                                          segment_stride, None, None, None, None, rot)
        else:
            ret = self.conn.rw_local_keys(self.OP_R, keys, offs, *args, False, 0, segments,
                                          segment_stride, None, None, None, None, rot)
        if ret < 0:
            raise Exception(f"Failed to read from infinistore, ret = {ret}")
        return ticket

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
                    tensor_set=None, page_permute: Optional[PagePermute] = None,
                    page_transpose: Optional[PageTranspose] = None,
                    page_cast: Optional[PageCast] = None,
                    page_shuffle: Optional[PageShuffle] = None, **unsupported):
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

        page_permute=PagePermute(outer, rows, cols): `cache` holds each page
        as [outer, cols, rows, piece] (e.g. a head-major [2, H, T, hd] block)
        and the stored page is the [outer, rows, cols, piece] one,
        byte-identical to what a writer in that layout stores, so every
        reader serves it. Works with every quant and with segments (which
        apply to the page as `cache` holds it); local path only, not with
        tensor_set; an illegal geometry is a ValueError before anything is
        sent.

        page_transpose=PageTranspose(tokens, heads, head_dim, inner_k):
        `cache` holds each page as a paged-attention cache block (see
        PageTranspose) and the stored page is the token-major
        [halves, tokens, heads, head_dim] one, byte-identical to what a
        token-major writer stores. Works with every quant and with segments;
        local path only, not with tensor_set or page_permute; cache, offsets
        and stride must be 16-byte aligned; an illegal geometry is a
        ValueError before anything is sent.

        page_cast=PageCast([k_scale, v_scale]): `cache` is an fp8 engine's
        cache (torch.float8_e4m3fn or uint8, see PageCast); page_size, offsets
        and segment_stride stay in elements, one byte each. The stored page is
        what a bf16 writer holding code * scale would have stored, under every
        quant, so bf16 engines read it as usual. Works with segments; local
        path only, not with tensor_set, page_permute or page_transpose; cache
        and offsets must be 16-byte aligned; anything the server would refuse
        is a ValueError before anything is sent.

        page_shuffle=PageShuffle(tokens, heads, head_dim): `cache` holds each
        page as a shuffled cache block (see PageShuffle) and the stored page
        is the token-major [halves, tokens, heads, head_dim] one,
        byte-identical to what a token-major writer stores. Works with every
        quant and with segments; local path only, with none of the other page_*
        arguments or tensor_set; cache, offsets and stride must be 16-byte
        aligned; an illegal geometry is a ValueError before anything is sent.

        Slices are read-only: write_pages has no page_slice parameter, and
        passing one is a ValueError."""
        if page_shuffle is not None and "page_rotate" in unsupported:
            raise ValueError("page_shuffle cannot be combined with page_slice, tensor_set, "
                             "page_permute, page_transpose, page_cast or page_rotate")
        if "page_slice" in unsupported:
            raise ValueError("page_slice is read-only: there is no sliced write")
        if unsupported:
            raise TypeError(f"write_pages() got an unexpected keyword argument "
                            f"{next(iter(unsupported))!r}")
        if page_shuffle is not None:
            segments = 1 if segments is None else segments
            if tensor_set is None:
                self._verify(cache)
            shuf = self._shuffle_arg(page_shuffle, cache, offsets, page_size, segments,
                                     segment_stride, quant, None,
                                     tensor_set, page_permute, page_transpose, page_cast)
            self._rw_shuffled(self.OP_W, cache, keys, offsets, page_size, segments,
                              segment_stride, shuf, sync,
                              self.QUANT_MODES[quant][0] if quant else 0)
            return 0
        if tensor_set is not None:
            if page_permute is not None:
                raise ValueError("page_permute cannot be combined with page_slice or "
                                 "tensor_set")
            if page_transpose is not None:
                raise ValueError("page_transpose cannot be combined with page_slice, "
                                 "tensor_set or page_permute")
            if page_cast is not None:
                raise ValueError("page_cast cannot be combined with page_slice, tensor_set, "
                                 "page_permute or page_transpose")
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
        if page_cast is not None:
            cast = self._cast_arg(page_cast, cache, offsets, page_size, segments, segment_stride,
                                  quant, None, None, page_permute, page_transpose)
            self._rw_cast(self.OP_W, cache, keys, offsets, page_size, segments, segment_stride,
                          cast, sync, self.QUANT_MODES[quant][0] if quant else 0)
            return 0
        if segments != 1 and not self.local_connected:
            raise ValueError("segmented pages use the local GPU path")
        if page_permute is not None and not self.local_connected:
            raise ValueError("permuted pages use the local GPU path")
        if page_transpose is not None and not self.local_connected:
            raise ValueError("transposed pages use the local GPU path")
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
        perm = self._permute_arg(page_permute, page_size, segments, quant)
        xpose = self._transpose_arg(page_transpose, cache, offs, page_size, segments,
                                    segment_stride, quant, None, None, page_permute)
        if isinstance(keys, (bytes, bytearray, memoryview)):
            ret = self.conn.rw_local_blob(
                self.OP_W, keys, offs, es, page_size * es,
                cache.data_ptr(), _remap_device_id(cache), sync, flags,
                segments, segment_stride, None, perm, xpose,
            )
        else:
            ret = self.conn.rw_local_keys(
                self.OP_W, keys, offs, es, page_size * es,
                cache.data_ptr(), _remap_device_id(cache), sync, flags,
                segments, segment_stride, None, perm, xpose,
            )
        if ret < 0:
            raise Exception(f"Failed to write to infinistore, ret = {ret}")
        return 0

    def read_pages(self, cache: Optional[torch.Tensor], keys, offsets, page_size: int,
                   segments: Optional[int] = None, segment_stride: int = 0,
                   page_slice: Optional[PageSlice] = None, tensor_set=None,
                   page_permute: Optional[PagePermute] = None,
                   page_transpose: Optional[PageTranspose] = None,
                   page_cast: Optional[PageCast] = None,
                   page_rotate: Optional[PageRotate] = None,
                   page_shuffle: Optional[PageShuffle] = None):
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
        Not together with page_slice.

        page_permute: deliver each page as [outer, cols, rows, piece] (see
        write_pages), however it was written. page_size must be the written
        one. Not together with page_slice or tensor_set.

        page_transpose: deliver each page as a paged-attention cache block
        (see write_pages), however it was written. page_size must be the
        written one. Not together with page_slice, tensor_set or
        page_permute.

        page_cast: deliver each page as e4m3fn codes under the given scales
        (see write_pages), however it was written: the stored element is
        decoded to bf16 as for a bf16 reader, then divided by its half's scale
        and rounded to e4m3fn (saturating at +-448). page_size must be the
        written one. Not together with page_slice, tensor_set, page_permute
        or page_transpose.

        page_rotate: deliver each bf16 page with the rotary pairs of its K
        half turned by the given table (see PageRotate), however it was
        written (plain, fp8 or mxfp4): the stored element is decoded to bf16
        as for any reader, rotated in float32 and rounded to bf16 once.
        page_size must be the written one. Works with segments (kv-major
        caches); local path only, bf16 only, 16-byte-aligned cache and
        offsets; not together with page_slice, tensor_set, page_permute,
        page_transpose or page_cast; anything the server would refuse is a
        ValueError before anything is sent.

        page_shuffle: deliver each page as a shuffled cache block (see
        write_pages), however it was written. page_size must be the written
        one. With none of the other page_* arguments or tensor_set."""
        if page_shuffle is not None:
            segments = 1 if segments is None else segments
            if tensor_set is None:
                self._verify(cache)
            shuf = self._shuffle_arg(page_shuffle, cache, offsets, page_size, segments,
                                     segment_stride, None, page_slice, tensor_set, page_permute,
                                     page_transpose, page_cast, page_rotate)
            self._rw_shuffled(self.OP_R, cache, keys, offsets, page_size, segments,
                              segment_stride, shuf)
            return
        if page_rotate is not None:
            segments = 1 if segments is None else segments
            if tensor_set is None:
                self._verify(cache)
            rot = self._rotate_arg(page_rotate, cache, offsets, page_size, segments,
                                   segment_stride, page_slice, tensor_set, page_permute,
                                   page_transpose, page_cast)
            self._read_rotated(cache, keys, offsets, page_size, segments, segment_stride, rot)
            return
        if page_cast is not None:
            segments = 1 if segments is None else segments
            if tensor_set is None:
                self._verify(cache)
            cast = self._cast_arg(page_cast, cache, offsets, page_size, segments, segment_stride,
                                  None, page_slice, tensor_set, page_permute, page_transpose)
            self._rw_cast(self.OP_R, cache, keys, offsets, page_size, segments, segment_stride,
                          cast)
            return
        if tensor_set is not None:
            self._permute_arg(page_permute, page_size, 1, None, page_slice, tensor_set)
            self._transpose_arg(page_transpose, None, None, page_size, 1, 0, None, page_slice,
                                tensor_set, page_permute)
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
        perm = self._permute_arg(page_permute, page_size, segments, None, page_slice)
        xpose = self._transpose_arg(page_transpose, cache, offsets, page_size, segments,
                                    segment_stride, None, page_slice, None, page_permute)
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
                    segments, segment_stride, self._slice_arg(page_slice), perm, xpose,
                )
            else:
                ret = self.conn.rw_local_keys(
                    self.OP_R, keys, offs, es, page_size * es,
                    cache.data_ptr(), _remap_device_id(cache), False, 0,
                    segments, segment_stride, self._slice_arg(page_slice), perm, xpose,
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
                         page_slice: Optional[PageSlice] = None, tensor_set=None,
                         page_permute: Optional[PagePermute] = None,
                         page_transpose: Optional[PageTranspose] = None,
                         page_cast: Optional[PageCast] = None,
                         page_rotate: Optional[PageRotate] = None,
                         page_shuffle: Optional[PageShuffle] = None):
        """Ticketed read (local path, shm ring): pushes the request and
        returns a ticket; call wait_read(ticket) before using the data. Lets
        an engine overlap its own work (or further requests) with the copy —
        e.g. prefetching the next sequence's KV pages while decoding. Falls
        back to a blocking read (ticket 0) when the ring is unavailable.
        segments / segment_stride / page_slice / tensor_set / page_permute /
        page_transpose / page_cast / page_rotate / page_shuffle as in
        read_pages."""
        if page_shuffle is not None:
            segments = 1 if segments is None else segments
            if tensor_set is None:
                self._verify(cache)
            shuf = self._shuffle_arg(page_shuffle, cache, offsets, page_size, segments,
                                     segment_stride, None, page_slice, tensor_set, page_permute,
                                     page_transpose, page_cast, page_rotate)
            return self._rw_shuffled(self.OP_R, cache, keys, offsets, page_size, segments,
                                     segment_stride, shuf, ticketed=True)
        if page_rotate is not None:
            segments = 1 if segments is None else segments
            if tensor_set is None:
                self._verify(cache)
            rot = self._rotate_arg(page_rotate, cache, offsets, page_size, segments,
                                   segment_stride, page_slice, tensor_set, page_permute,
                                   page_transpose, page_cast)
            return self._read_rotated(cache, keys, offsets, page_size, segments,
                                      segment_stride, rot, ticketed=True)
        if page_cast is not None:
            segments = 1 if segments is None else segments
            if tensor_set is None:
                self._verify(cache)
            cast = self._cast_arg(page_cast, cache, offsets, page_size, segments, segment_stride,
                                  None, page_slice, tensor_set, page_permute, page_transpose)
            return self._rw_cast(self.OP_R, cache, keys, offsets, page_size, segments,
                                 segment_stride, cast, ticketed=True)
        if tensor_set is not None:
            self._permute_arg(page_permute, page_size, 1, None, page_slice, tensor_set)
            self._transpose_arg(page_transpose, None, None, page_size, 1, 0, None, page_slice,
                                tensor_set, page_permute)
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
        perm = self._permute_arg(page_permute, page_size, segments, None, page_slice)
        xpose = self._transpose_arg(page_transpose, cache, offsets, page_size, segments,
                                    segment_stride, None, page_slice, None, page_permute)
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
            self._slice_arg(page_slice), perm, xpose,
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


class QuantErrorFields(NamedTuple):
    """Indices into the last axis of quant_error's result."""

    sum_sq: int = 0  # sum of x^2
    sum_sq_err: int = 1  # sum of (x - x^)^2
    max_abs_err: int = 2  # max |x - x^|
    absmax: int = 3  # max |x|
    nonfinite: int = 4  # elements whose x or x^ is not finite


QUANT_ERROR_FIELDS = QuantErrorFields()


def quant_error(cache: Optional[torch.Tensor], offsets, page_size: int, quant: str,
                segments: int = 1, segment_stride: int = 0, tensors=None) -> torch.Tensor:
    """What the pages would lose under ``quant`` ("fp8" or "mxfp4"), measured
    on the GPU without storing anything: no connection, no server, no pool
    space. With x an element and x^ what read_pages returns for it after
    write_pages(quant=quant), bit for bit, the result is a float64 CPU tensor
    ``[len(offsets), parts, 5]`` holding, per page and part (QuantErrorFields):
    sum x^2, sum (x - x^)^2, max |x - x^|, max |x| and the number of elements
    whose x or x^ is not finite; the first four run over the other elements.

    cache, offsets, page_size, segments and segment_stride mean what they mean
    in write_pages (elements of a bf16 GPU tensor); a part is a segment, or the
    whole page when segments == 1. tensors=[...] (pass cache=None) is the
    tensor-set form: the page spans all tensors, offsets are per-tensor
    element offsets, page_size the whole page, segments the total (default
    one per tensor), and a part is one tensor's share. The fp8 scale is the
    PAGE's, so a quiet part that shares a page with a loud one shows a larger
    relative error than it would alone. Permuted pages need no form of their
    own: a permutation of whole pieces changes neither the fp8 error nor the
    mxfp4 groups. Every request write_pages would refuse is a ValueError."""
    modes = InfinityConnection.QUANT_MODES
    if quant not in modes:
        raise ValueError(f"unsupported quant mode {quant!r}")
    flag, multiple = modes[quant]
    if (cache is None) == (tensors is None):
        raise ValueError("pass either cache or tensors")
    group = [cache] if tensors is None else list(tensors)
    if not 1 <= len(group) <= InfinityConnection.MAX_PAGE_TENSORS:
        raise ValueError(f"tensors holds 1..{InfinityConnection.MAX_PAGE_TENSORS} tensors")
    for t in group:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16:
            raise ValueError(f"{quant} quant requires bf16 tensors")
        if not t.is_contiguous():
            raise ValueError("the tensors must be contiguous")
        if t.device != group[0].device:
            raise ValueError("the tensors share one device")
    es = group[0].element_size()
    if tensors is not None and segments == 1:
        segments = len(group)  # not given: one segment per tensor
    if page_size <= 0 or page_size % multiple != 0:
        raise ValueError(f"{quant} quant needs page_size % {multiple} == 0")
    codec = _native._dbg_page_codec(flag, page_size * es)[0]
    if tensors is None:
        legal = _native._dbg_segments_legal(codec, page_size * es, segments, segment_stride * es)
        per = segments
    else:
        legal = _native._dbg_tensors_legal(codec, page_size * es, segments,
                                           segment_stride * es, len(group))
        per = segments // len(group)
    if not legal:
        raise ValueError(f"illegal page geometry for {quant}: a segment is a multiple of "
                         f"{multiple} elements, segments do not overlap, and the stride "
                         "keeps them 16-byte aligned")
    offs = np.asarray(offsets, dtype=np.uint64)
    if any(t.data_ptr() % 16 for t in group) or (offs * np.uint64(es) % np.uint64(16)).any():
        raise ValueError(f"{quant} quant needs 16-byte-aligned tensors and page offsets")
    seg = page_size // segments
    span = (per - 1) * segment_stride + seg if per > 1 else seg
    if len(offs) and int(offs.max()) + span > min(t.numel() for t in group):
        raise ValueError("a page extends outside its tensor")
    if group[0].device.type != "cuda":
        raise ValueError("quant_error requires CUDA (ROCm) tensors")
    parts = len(group) if tensors is not None else segments
    flat = _native.quant_error(
        0 if tensors is not None else cache.data_ptr(), [int(o) * es for o in offs],
        page_size, flag, group[0].device.index or 0, segments,
        segment_stride * es if per > 1 else 0,
        [t.data_ptr() for t in group] if tensors is not None else [])
    return torch.tensor(flat, dtype=torch.float64).reshape(
        len(offs), parts, len(QUANT_ERROR_FIELDS))
