// Python bindings for infinistore-amd (module: infinistore_amd._native).
//
// Mirrors the reference's pybind surface (/root/reference/src/pybind.cpp:36-210:
// Connection, ClientConfig/ServerConfig, register_server, purge_kv_map,
// get_kvmap_len, log) with two deliberate changes:
//  * The server runs on its own C++ thread (start_server/stop_server) instead
//    of borrowing uvloop's uv_loop_t* through a PyCapsule.
//  * allocate_rdma returns a list of (rkey, remote_addr) tuples and w_rdma
//    accepts the same — no numpy dtype marshalling required.
#include <pybind11/functional.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>

#include "client/client.h"
#include "core/log.h"
#include "fabric/wr_flow.h"
#include "core/protocol.h"
#include "core/mempool.h"
#include "gpu/fp8_codec.h"
#include "gpu/mxfp4_codec.h"
#include "gpu/gpu.h"
#include "server/completed_prefix.h"
#include "server/server.h"

namespace py = pybind11;
using namespace ifs;

namespace {

// Hold a Python callback so it can be copied/destroyed on C++ worker threads:
// the shared_ptr deleter re-acquires the GIL for the final decref.
std::shared_ptr<py::function> hold_callback(py::function cb) {
    return std::shared_ptr<py::function>(new py::function(std::move(cb)), [](py::function* p) {
        py::gil_scoped_acquire acq;
        delete p;
    });
}

std::unique_ptr<Server> g_server;

struct ServerConfigPy {
    int manage_port = 0;
    int service_port = 0;
    std::string log_level = "warning";
    std::string dev_name = "";
    int ib_port = 1;
    std::string link_type = "Ethernet";
    int prealloc_size = 16;           // GB per shard
    int minimal_allocate_size = 64;   // KB
    int num_stream = 4;
    bool auto_increase = false;
    std::vector<int> devices;         // GPU ordinals to shard over; empty=auto
    bool cpu_only = false;            // force CPU pool even if GPUs exist
    int cpu_shards = 1;               // CPU-mode shard count
    bool auto_evict = false;          // LRU-evict on allocation failure
    int ttl_seconds = 0;              // key time-to-live (0 = forever)
    int io_threads = 3;               // worker IO loops (0 = single loop)
    int extend_size = 10;             // GB per auto-extend arena
};

bool start_server(const ServerConfigPy& cfg) {
    if (g_server && g_server->running()) {
        ERROR("server already running");
        return false;
    }
    ServerOptions opt;
    opt.service_port = cfg.service_port;
    opt.prealloc_bytes = static_cast<size_t>(cfg.prealloc_size) << 30;
    opt.block_granule = static_cast<size_t>(cfg.minimal_allocate_size) << 10;
    opt.auto_extend = cfg.auto_increase;
    opt.n_streams = cfg.num_stream > 0 ? cfg.num_stream : 4;
    opt.cpu_shards = cfg.cpu_shards;
    opt.log_level = cfg.log_level;
    opt.dev_name = cfg.dev_name;
    opt.ib_port = cfg.ib_port;
    opt.link_type = cfg.link_type;
    opt.auto_evict = cfg.auto_evict;
    opt.ttl_seconds = cfg.ttl_seconds;
    opt.io_threads = cfg.io_threads;
    opt.extend_bytes = static_cast<size_t>(cfg.extend_size) << 30;
    if (!cfg.cpu_only && gpu::available()) {
        if (!cfg.devices.empty()) {
            opt.devices = cfg.devices;
        } else {
            opt.devices.resize(static_cast<size_t>(gpu::device_count()));
            for (int i = 0; i < gpu::device_count(); i++) opt.devices[static_cast<size_t>(i)] = i;
        }
    }
    g_server.reset(new Server(opt));
    return g_server->start();
}

void stop_server() {
    if (g_server) {
        g_server->stop();
        g_server.reset();
    }
}

size_t purge_kv_map_py() { return g_server ? g_server->purge() : 0; }
size_t get_kvmap_len_py() { return g_server ? g_server->kvmap_len() : 0; }
std::string server_stats_py() { return g_server ? g_server->stats_json() : "{}"; }
std::pair<size_t, size_t> server_compact_py() {
    return g_server ? g_server->compact() : std::make_pair<size_t, size_t>(0, 0);
}

// GPU fingerprint helper: hash n blocks of a device tensor in one kernel
// launch (block i at base + offsets[i], each `block_size` bytes).
std::vector<uint64_t> hash_blocks_py(uintptr_t base, std::vector<uint64_t> offsets,
                                     size_t block_size, int device) {
    size_t n = offsets.size();
    std::vector<uint64_t> out(n, 0);
    if (n == 0) return out;
    if (!gpu::available()) throw std::runtime_error("hash_blocks: no GPU available");
    std::vector<uint64_t> ptrs(n);
    for (size_t i = 0; i < n; i++) ptrs[i] = base + offsets[i];
    auto* d_ptrs = static_cast<uint64_t*>(gpu::alloc_device(device, n * 8));
    auto* d_out = static_cast<uint64_t*>(gpu::alloc_device(device, n * 8));
    gpu::Stream s = d_ptrs && d_out ? gpu::stream_create(device) : nullptr;
    bool ok = s && gpu::memcpy_h2d(d_ptrs, ptrs.data(), n * 8) &&
              gpu::launch_hash_blocks(device, s, d_ptrs, static_cast<int>(n), block_size,
                                      d_out) &&
              gpu::stream_sync(s) && gpu::memcpy_d2h(out.data(), d_out, n * 8);
    std::string err = ok ? "" : gpu::last_error();
    gpu::stream_destroy(s);
    gpu::free_device(d_ptrs);
    gpu::free_device(d_out);
    if (!ok) throw std::runtime_error("hash_blocks failed: " + err);
    return out;
}

// ---- direct kernel entry points (debug/test surface) ----------------------
// Descriptors and scales sit in pinned host memory exactly as in
// Shard::submit_copy, so a test that goes through these runs what production
// runs. Every request the kernel cannot serve is refused before any launch.

// Pinned host array, freed on scope exit.
template <typename T>
struct Pinned {
    T* p;
    explicit Pinned(size_t n) : p(static_cast<T*>(gpu::alloc_host_pinned(n * sizeof(T)))) {
        if (!p) throw std::runtime_error("alloc_host_pinned failed");
    }
    ~Pinned() { gpu::free_host_pinned(p); }
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
};

struct ScopedStream {
    gpu::Stream s;
    explicit ScopedStream(int device) : s(gpu::stream_create(device)) {
        if (!s) throw std::runtime_error("stream_create failed");
    }
    ~ScopedStream() { gpu::stream_destroy(s); }
    ScopedStream(const ScopedStream&) = delete;
    ScopedStream& operator=(const ScopedStream&) = delete;
};

void require_gpu_and_pairs(const char* what, const std::vector<uint64_t>& src,
                           const std::vector<uint64_t>& dst) {
    if (!gpu::available()) throw std::runtime_error(std::string(what) + ": no GPU available");
    if (src.size() != dst.size())
        throw std::invalid_argument(std::string(what) + ": src/dst length mismatch");
    if (src.size() > static_cast<size_t>(INT32_MAX))
        throw std::invalid_argument(std::string(what) + ": too many blocks");
}

bool all_aligned16(const std::vector<uint64_t>& a, const std::vector<uint64_t>& b) {
    for (uint64_t p : a)
        if (p % 16) return false;
    for (uint64_t p : b)
        if (p % 16) return false;
    return true;
}

void copy_blocks_py(const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst,
                    size_t bytes_per_block, int device, const std::string& path) {
    require_gpu_and_pairs("_dbg_copy_blocks", src, dst);
    const bool vec = path == "vec", inl = path == "inline";
    if (!vec && !inl && path != "byte")
        throw std::invalid_argument("_dbg_copy_blocks: path must be vec, byte or inline");
    if (bytes_per_block == 0) throw std::invalid_argument("_dbg_copy_blocks: empty blocks");
    if ((vec || inl) && (bytes_per_block % 16 != 0 || !all_aligned16(src, dst)))
        throw std::invalid_argument("_dbg_copy_blocks: " + path +
                                    " path needs 16-byte-aligned pointers and size");
    if (inl && src.size() > 16)
        throw std::invalid_argument("_dbg_copy_blocks: inline path takes at most 16 blocks");
    size_t n = src.size();
    if (n == 0) return;
    Pinned<uint64_t> h_src(n), h_dst(n);
    memcpy(h_src.p, src.data(), n * 8);
    memcpy(h_dst.p, dst.data(), n * 8);
    ScopedStream st(device);
    bool ok = inl ? gpu::launch_copy_blocks_inline(device, st.s, h_src.p, h_dst.p,
                                                   static_cast<int>(n), bytes_per_block)
                  : gpu::launch_copy_blocks(device, st.s, h_src.p, h_dst.p,
                                            static_cast<int>(n), bytes_per_block, vec);
    // Always drain the stream before the pinned descriptors go away.
    bool synced = gpu::stream_sync(st.s);
    if (!ok || !synced)
        throw std::runtime_error(std::string("_dbg_copy_blocks failed: ") + gpu::last_error());
}

// The one body behind the four `_dbg_*quant*` kernel bindings: checks from the
// codec table, then the production launcher. kStore returns the per-page
// scales (empty for codecs that keep theirs inside the block); kLoad takes
// them in `scales`.
std::vector<float> transform_blocks_py(const char* what, PageCodec codec, PageDir dir,
                                       const std::vector<uint64_t>& src,
                                       const std::vector<uint64_t>& dst,
                                       std::vector<float> scales, size_t elems_per_block,
                                       int device) {
    const PageCodecInfo& info = page_codec_info(codec);
    const bool store = dir == PageDir::kStore;
    require_gpu_and_pairs(what, src, dst);
    if (elems_per_block == 0 || !page_legal(codec, elems_per_block * kPageElemBytes))
        throw std::invalid_argument(std::string(what) + ": elems_per_block % " +
                                    std::to_string(info.page_multiple / kPageElemBytes) +
                                    " != 0");
    if (!all_aligned16(src, dst))
        throw std::invalid_argument(std::string(what) + ": pointers must be 16-byte aligned");
    size_t n = src.size();
    if (info.page_scale && !store && scales.size() != n)
        throw std::invalid_argument(std::string(what) + ": one scale per block");
    scales.resize(info.page_scale ? n : 0);
    if (n == 0) return scales;
    Pinned<uint64_t> h_src(n), h_dst(n);
    Pinned<float> h_scale(n);
    memcpy(h_src.p, src.data(), n * 8);
    memcpy(h_dst.p, dst.data(), n * 8);
    memcpy(h_scale.p, scales.data(), scales.size() * sizeof(float));
    ScopedStream st(device);
    bool ok = gpu::launch_transform_blocks(device, st.s, codec, dir, h_src.p, h_dst.p,
                                           h_scale.p, static_cast<int>(n), elems_per_block);
    bool synced = gpu::stream_sync(st.s);
    if (!ok || !synced)
        throw std::runtime_error(std::string(what) + " failed: " + gpu::last_error());
    memcpy(scales.data(), h_scale.p, scales.size() * sizeof(float));
    return scales;
}

// ---- segmented forms (docs/design.md, "segmented pages") ------------------
// The client side of every block is n_segments pieces segment_stride BYTES
// apart, the pool side contiguous; descriptors in pinned host memory as above.

PageCodec codec_from_id(const char* what, int codec) {
    if (codec < 0 || !page_codec_known(static_cast<uint32_t>(codec)))
        throw std::invalid_argument(std::string(what) + ": unknown codec id");
    return static_cast<PageCodec>(codec);
}

void copy_blocks_seg_py(const std::vector<uint64_t>& client, const std::vector<uint64_t>& pool,
                        size_t bytes_per_block, uint32_t n_segments, uint64_t segment_stride,
                        bool to_pool, int device, const std::string& path) {
    const char* what = "_dbg_copy_blocks_seg";
    require_gpu_and_pairs(what, client, pool);
    const bool vec = path == "vec";
    if (!vec && path != "byte")
        throw std::invalid_argument(std::string(what) + ": path must be vec or byte");
    if (bytes_per_block == 0) throw std::invalid_argument(std::string(what) + ": empty blocks");
    if (!segments_legal(PageCodec::kNone, bytes_per_block, n_segments, segment_stride))
        throw std::invalid_argument(std::string(what) + ": illegal page segments");
    if (vec && (bytes_per_block % 16 != 0 || (bytes_per_block / n_segments) % 16 != 0 ||
                (n_segments > 1 && segment_stride % 16 != 0) || !all_aligned16(client, pool)))
        throw std::invalid_argument(std::string(what) +
                                    ": vec path needs 16-byte-aligned pointers, segment size "
                                    "and stride");
    size_t n = client.size();
    if (n == 0) return;
    const std::vector<uint64_t>& src = to_pool ? client : pool;
    const std::vector<uint64_t>& dst = to_pool ? pool : client;
    Pinned<uint64_t> h_src(n), h_dst(n);
    memcpy(h_src.p, src.data(), n * 8);
    memcpy(h_dst.p, dst.data(), n * 8);
    ScopedStream st(device);
    bool ok = gpu::launch_copy_blocks(device, st.s, h_src.p, h_dst.p, static_cast<int>(n),
                                      bytes_per_block, vec,
                                      PageSegments{n_segments, segment_stride},
                                      to_pool ? PageDir::kStore : PageDir::kLoad);
    bool synced = gpu::stream_sync(st.s);
    if (!ok || !synced)
        throw std::runtime_error(std::string(what) + " failed: " + gpu::last_error());
}

// kStore: src is the segmented bf16 side, dst the stored blocks; kLoad the
// other way round. Scales as in transform_blocks_py.
std::vector<float> transform_blocks_seg_py(const char* what, int codec_id, PageDir dir,
                                           const std::vector<uint64_t>& src,
                                           const std::vector<uint64_t>& dst,
                                           std::vector<float> scales, size_t elems_per_block,
                                           uint32_t n_segments, uint64_t segment_stride,
                                           int device) {
    const PageCodec codec = codec_from_id(what, codec_id);
    if (!page_codec_transforms(codec))
        throw std::invalid_argument(std::string(what) + ": codec does not transform");
    const PageCodecInfo& info = page_codec_info(codec);
    const bool store = dir == PageDir::kStore;
    require_gpu_and_pairs(what, src, dst);
    if (elems_per_block == 0 || !page_legal(codec, elems_per_block * kPageElemBytes))
        throw std::invalid_argument(std::string(what) + ": illegal page size");
    if (!segments_legal(codec, elems_per_block * kPageElemBytes, n_segments, segment_stride))
        throw std::invalid_argument(std::string(what) + ": illegal page segments");
    if (!all_aligned16(src, dst))
        throw std::invalid_argument(std::string(what) + ": pointers must be 16-byte aligned");
    size_t n = src.size();
    if (info.page_scale && !store && scales.size() != n)
        throw std::invalid_argument(std::string(what) + ": one scale per block");
    scales.resize(info.page_scale ? n : 0);
    if (n == 0) return scales;
    Pinned<uint64_t> h_src(n), h_dst(n);
    Pinned<float> h_scale(n);
    memcpy(h_src.p, src.data(), n * 8);
    memcpy(h_dst.p, dst.data(), n * 8);
    memcpy(h_scale.p, scales.data(), scales.size() * sizeof(float));
    ScopedStream st(device);
    bool ok = gpu::launch_transform_blocks(device, st.s, codec, dir, h_src.p, h_dst.p,
                                           h_scale.p, static_cast<int>(n), elems_per_block,
                                           PageSegments{n_segments, segment_stride});
    bool synced = gpu::stream_sync(st.s);
    if (!ok || !synced)
        throw std::runtime_error(std::string(what) + " failed: " + gpu::last_error());
    memcpy(scales.data(), h_scale.p, scales.size() * sizeof(float));
    return scales;
}

// ---- tensor sets (docs/design.md, "tensor sets") -----------------------------
// The two tensor-set launchers, called directly. The client side is `bases`
// (one device address per tensor) plus one byte offset per block, the same in
// every tensor; the pool side one pointer per block. Both return what the
// launcher returns, so a refusal is False, not an exception; aligned16 is
// computed from offsets and pool pointers as Shard::submit_copy does.
// force_byte passes aligned16 = false, which selects the byte kernel for
// aligned operands too.
bool copy_blocks_tset_py(const std::vector<uint64_t>& bases, const std::vector<uint64_t>& offs,
                         const std::vector<uint64_t>& pool, size_t bytes_per_block,
                         uint32_t n_segments, uint64_t segment_stride, bool to_pool, int device,
                         bool force_byte) {
    const char* what = "_dbg_copy_blocks_tset";
    require_gpu_and_pairs(what, offs, pool);
    size_t n = offs.size();
    if (n == 0) return true;
    py::gil_scoped_release rel;
    Pinned<uint64_t> h_client(n), h_pool(n);
    memcpy(h_client.p, offs.data(), n * 8);
    memcpy(h_pool.p, pool.data(), n * 8);
    ScopedStream st(device);
    bool ok = gpu::launch_copy_blocks_tset(
        device, st.s, to_pool ? h_client.p : h_pool.p, to_pool ? h_pool.p : h_client.p,
        static_cast<int>(n), bytes_per_block, !force_byte && all_aligned16(offs, pool),
        PageSegments{n_segments, segment_stride}, to_pool ? PageDir::kStore : PageDir::kLoad,
        gpu::TensorTable{bases.data(), static_cast<uint32_t>(bases.size())});
    // Always drain the stream before the pinned descriptors go away.
    if (!gpu::stream_sync(st.s))
        throw std::runtime_error(std::string(what) + " failed: " + gpu::last_error());
    return ok;
}

// to_pool quantizes (the scales come back), else dequantizes (they go in).
std::pair<bool, std::vector<float>> transform_blocks_tset_py(
    int codec_id, bool to_pool, const std::vector<uint64_t>& bases,
    const std::vector<uint64_t>& offs, const std::vector<uint64_t>& pool,
    std::vector<float> scales, size_t elems_per_block, uint32_t n_segments,
    uint64_t segment_stride, int device) {
    const char* what = "_dbg_transform_blocks_tset";
    const PageCodec codec = codec_from_id(what, codec_id);
    require_gpu_and_pairs(what, offs, pool);
    size_t n = offs.size();
    const bool page_scale = page_codec_info(codec).page_scale;
    if (page_scale && !to_pool && scales.size() != n)
        throw std::invalid_argument(std::string(what) + ": one scale per block");
    scales.resize(page_scale ? n : 0);
    if (n == 0) return {true, scales};
    py::gil_scoped_release rel;
    Pinned<uint64_t> h_client(n), h_pool(n);
    Pinned<float> h_scale(n);
    memcpy(h_client.p, offs.data(), n * 8);
    memcpy(h_pool.p, pool.data(), n * 8);
    memcpy(h_scale.p, scales.data(), scales.size() * sizeof(float));
    ScopedStream st(device);
    bool ok = gpu::launch_transform_blocks_tset(
        device, st.s, codec, to_pool ? PageDir::kStore : PageDir::kLoad,
        to_pool ? h_client.p : h_pool.p, to_pool ? h_pool.p : h_client.p, h_scale.p,
        static_cast<int>(n), elems_per_block, all_aligned16(offs, pool),
        PageSegments{n_segments, segment_stride},
        gpu::TensorTable{bases.data(), static_cast<uint32_t>(bases.size())});
    if (!gpu::stream_sync(st.s))
        throw std::runtime_error(std::string(what) + " failed: " + gpu::last_error());
    if (ok) memcpy(scales.data(), h_scale.p, scales.size() * sizeof(float));
    return {ok, scales};
}

// ---- sliced reads (docs/design.md, "sliced reads") ---------------------------
// A slice from Python: None, or (n_pieces, page, offset, piece, stride) in
// units of `unit` bytes (the tensor's element size; 1 for the byte-level
// debug entries).
PageSlice slice_from_py(const char* what, const py::object& o, uint64_t unit) {
    PageSlice sl;
    if (o.is_none()) return sl;
    py::tuple t = o.cast<py::tuple>();
    if (t.size() != 5)
        throw std::invalid_argument(std::string(what) +
                                    ": a slice is (n_pieces, page, offset, piece, stride)");
    sl.n = t[0].cast<uint32_t>();
    sl.page_bytes = t[1].cast<uint64_t>() * unit;
    sl.offset = t[2].cast<uint64_t>() * unit;
    sl.piece_bytes = t[3].cast<uint64_t>() * unit;
    sl.stride = t[4].cast<uint64_t>() * unit;
    return sl;
}

// The sliced-load launcher, called directly: stored blocks -> client pages.
// Returns what the launcher returns, so a refusal is False, not an exception;
// aligned16 is computed from the pointers as Shard::submit_copy does.
bool load_sliced_py(int codec_id, const std::vector<uint64_t>& stored,
                    const std::vector<uint64_t>& client, const std::vector<float>& scales,
                    const py::object& slice, uint32_t n_segments, uint64_t segment_stride,
                    int device) {
    const char* what = "_dbg_load_sliced";
    const PageCodec codec = codec_from_id(what, codec_id);
    const PageSlice sl = slice_from_py(what, slice, 1);
    require_gpu_and_pairs(what, stored, client);
    size_t n = stored.size();
    if (page_codec_info(codec).page_scale && scales.size() != n)
        throw std::invalid_argument(std::string(what) + ": one scale per block");
    if (n == 0) return true;
    py::gil_scoped_release rel;
    Pinned<uint64_t> h_src(n), h_dst(n);
    Pinned<float> h_scale(n);
    memcpy(h_src.p, stored.data(), n * 8);
    memcpy(h_dst.p, client.data(), n * 8);
    memcpy(h_scale.p, scales.data(), std::min(scales.size(), n) * sizeof(float));
    ScopedStream st(device);
    bool ok = gpu::launch_load_sliced(device, st.s, codec, h_src.p, h_dst.p, h_scale.p,
                                      static_cast<int>(n), sl,
                                      PageSegments{n_segments, segment_stride},
                                      all_aligned16(stored, client));
    // Always drain the stream before the pinned descriptors go away.
    if (!gpu::stream_sync(st.s))
        throw std::runtime_error(std::string(what) + " failed: " + gpu::last_error());
    return ok;
}

// (codec id, stored bytes) of a request with these flags and this logical
// page size, by the codec table alone (host-only).
std::pair<int, size_t> page_codec_py(uint32_t flags, size_t page_bytes) {
    PageCodec codec;
    if (!page_codec_from_flags(flags, &codec))
        throw std::invalid_argument("_dbg_page_codec: more than one quant flag");
    if (!page_legal(codec, page_bytes))
        throw std::invalid_argument(std::string("_dbg_page_codec: ") +
                                    page_codec_info(codec).name + " pages are multiples of " +
                                    std::to_string(page_codec_info(codec).page_multiple) +
                                    " bytes");
    return {static_cast<int>(codec), stored_bytes(codec, page_bytes)};
}

// ---- jobs through a real Shard (debug/test surface) -------------------------
// Builds a Shard with the given stream, slot and descriptor limits, submits
// the jobs from n_threads threads (job i on thread i % n_threads, copy jobs
// first, list order within a thread), waits until every job was refused or
// called back, destroys the Shard and reports what happened to each job.
// All callbacks point into ShardRun, which the caller (and, after a timeout,
// the reaper thread) keeps alive until the Shard is gone.
struct ShardRun {
    struct Result {
        bool submitted = false;
        int done_calls = 0;
        bool ok = false;
        std::vector<float> scales;  // the shared vector as done() found it
    };
    std::unique_ptr<Shard> shard;
    std::vector<Shard::CopyJob> copy_jobs;
    std::vector<Shard::FabricJob> fabric_jobs;
    std::vector<std::shared_ptr<std::vector<float>>> scales;  // per copy job
    std::vector<Result> results;  // copy jobs, then fabric jobs
    std::vector<char> open;       // neither refused nor called back yet
    std::vector<std::thread> submitters;
    std::mutex mu;
    std::condition_variable cv;
    size_t outstanding = 0;
    bool reaped = false;

    void close(size_t i) {  // mu held
        if (!open[i]) return;
        open[i] = 0;
        outstanding--;
        cv.notify_all();
    }
    void on_done(size_t i, bool ok) {
        std::lock_guard<std::mutex> lk(mu);
        Result& r = results[i];
        r.done_calls++;
        r.ok = ok;
        if (i < scales.size() && scales[i]) r.scales = *scales[i];
        close(i);
    }
    void submit(size_t i) {
        if (i < copy_jobs.size()) {
            bool submitted = shard->submit_copy(std::move(copy_jobs[i]));
            std::lock_guard<std::mutex> lk(mu);
            results[i].submitted = submitted;
            if (!submitted) close(i);
        } else {
            shard->submit_fabric(std::move(fabric_jobs[i - copy_jobs.size()]));
            std::lock_guard<std::mutex> lk(mu);
            results[i].submitted = true;
        }
    }
};

// slices (null for _dbg_shard_run): one entry per copy job, None or the job's
// slice in bytes as slice_from_py takes it. tsets (null but for
// _dbg_shard_run_tset): one entry per copy job, None or (bases,
// segs_per_tensor); the job's client-side descriptors are then byte offsets.
py::tuple shard_run_impl(const char* what, int device, int n_streams, int slots_per_stream,
                         size_t max_descs_per_slot, const py::list& copy_jobs,
                         const py::list& fabric_jobs, int n_threads, double timeout_s,
                         const py::list* slices, const py::list* tsets = nullptr) {
    if (slices && slices->size() != copy_jobs.size())
        throw std::invalid_argument(std::string(what) + ": one slice (or None) per copy job");
    if (tsets && tsets->size() != copy_jobs.size())
        throw std::invalid_argument(std::string(what) +
                                    ": one tensor set (or None) per copy job");
    if (device < -1) throw std::invalid_argument(std::string(what) + ": device is -1 or an ordinal");
    if (device >= 0 && (!gpu::available() || device >= gpu::device_count()))
        throw std::runtime_error(std::string(what) + ": no such GPU available");
    if (n_streams < 1 || n_streams > 8 || slots_per_stream < 1 || slots_per_stream > 64 ||
        max_descs_per_slot < 1 || max_descs_per_slot > 16384)
        throw std::invalid_argument(std::string(what) + ": stream, slot or descriptor limit");
    if (n_threads < 1 || n_threads > 64 || !(timeout_s > 0))
        throw std::invalid_argument(std::string(what) + ": n_threads in 1..64, timeout_s > 0");

    auto st = std::make_shared<ShardRun>();
    ShardRun* run = st.get();
    const size_t n_copy = copy_jobs.size(), n_all = n_copy + fabric_jobs.size();
    st->results.resize(n_all);
    st->open.assign(n_all, 1);
    st->outstanding = n_all;
    for (size_t i = 0; i < n_copy; i++) {
        py::tuple t = copy_jobs[i].cast<py::tuple>();
        if (t.size() != 9) throw std::invalid_argument(std::string(what) + ": copy job of 9");
        Shard::CopyJob j;
        j.src = t[0].cast<std::vector<uint64_t>>();
        j.dst = t[1].cast<std::vector<uint64_t>>();
        j.bytes_per_block = t[2].cast<size_t>();
        j.codec = codec_from_id(what, t[3].cast<int>());
        j.dir = t[4].cast<bool>() ? PageDir::kStore : PageDir::kLoad;
        j.n_segments = t[5].cast<uint32_t>();
        j.segment_stride = t[6].cast<uint64_t>();
        if (!t[7].is_none())
            j.scales = std::make_shared<std::vector<float>>(t[7].cast<std::vector<float>>());
        j.scales_off = t[8].cast<size_t>();
        if (slices) j.slice = slice_from_py(what, (*slices)[i], 1);
        if (tsets && !py::object((*tsets)[i]).is_none()) {
            py::tuple ts = (*tsets)[i].cast<py::tuple>();
            if (ts.size() != 2)
                throw std::invalid_argument(std::string(what) +
                                            ": a tensor set is (bases, segs_per_tensor)");
            j.tensor_bases = std::make_shared<const std::vector<uint64_t>>(
                ts[0].cast<std::vector<uint64_t>>());
            j.segs_per_tensor = ts[1].cast<uint32_t>();
        }
        j.done = [run, i](bool ok) { run->on_done(i, ok); };
        st->scales.push_back(j.scales);
        st->copy_jobs.push_back(std::move(j));
    }
    // A put travels in `host` (the request body), a get lands in `raw_host`
    // (the response buffer), as in the server; the caller's buffer is copied
    // in before and, for a get, back out afterwards.
    std::vector<py::buffer_info> host_bufs;
    for (size_t k = 0; k < fabric_jobs.size(); k++) {
        py::tuple t = fabric_jobs[k].cast<py::tuple>();
        if (t.size() != 5) throw std::invalid_argument(std::string(what) + ": fabric job of 5");
        Shard::FabricJob j;
        j.is_put = t[0].cast<bool>();
        host_bufs.push_back(t[1].cast<py::buffer>().request(/*writable=*/true));
        const py::buffer_info& info = host_bufs.back();
        j.block_ptrs = t[2].cast<std::vector<uint64_t>>();
        j.host_offsets = t[3].cast<std::vector<size_t>>();
        j.bytes_per_block = t[4].cast<size_t>();
        const size_t len = static_cast<size_t>(info.size) * static_cast<size_t>(info.itemsize);
        if (!PyBuffer_IsContiguous(info.view(), 'C'))
            throw std::invalid_argument(std::string(what) + ": host buffer must be contiguous");
        if (j.block_ptrs.size() != j.host_offsets.size())
            throw std::invalid_argument(std::string(what) + ": one host offset per block");
        for (size_t off : j.host_offsets)
            if (off > len || j.bytes_per_block > len - off)
                throw std::invalid_argument(std::string(what) + ": host offset out of bounds");
        const uint8_t* p = static_cast<const uint8_t*>(info.ptr);
        if (j.is_put) {
            j.host = std::make_shared<std::vector<uint8_t>>(p, p + len);
        } else {
            j.raw_host = std::shared_ptr<uint8_t[]>(new uint8_t[len ? len : 1]);
            memcpy(j.raw_host.get(), p, len);
        }
        const size_t i = n_copy + k;
        j.done = [run, i](bool ok) { run->on_done(i, ok); };
        st->fabric_jobs.push_back(std::move(j));
    }
    std::vector<std::shared_ptr<uint8_t[]>> get_bufs;
    for (auto& j : st->fabric_jobs) get_bufs.push_back(j.raw_host);

    std::string timed_out;
    {
        py::gil_scoped_release rel;
        ShardOptions opt;
        opt.device = device;
        opt.pool_bytes = 4 * opt.block_granule;  // the pool itself is not used
        opt.n_streams = n_streams;
        opt.slots_per_stream = slots_per_stream;
        opt.max_descs_per_slot = max_descs_per_slot;
        st->shard.reset(new Shard(opt));
        if (!st->shard->init()) {
            st->shard.reset();
            throw std::runtime_error(std::string(what) + ": Shard::init failed");
        }
        for (int t = 0; t < n_threads; t++)
            st->submitters.emplace_back([run, t, n_threads, n_all] {
                for (size_t i = static_cast<size_t>(t); i < n_all; i += n_threads) run->submit(i);
            });
        bool finished;
        {
            std::unique_lock<std::mutex> lk(st->mu);
            finished = st->cv.wait_for(lk, std::chrono::duration<double>(timeout_s),
                                       [&] { return st->outstanding == 0; });
            if (!finished)
                for (size_t i = 0; i < n_all; i++)
                    if (st->open[i]) timed_out += " " + std::to_string(i);
        }
        if (finished) {
            for (auto& t : st->submitters) t.join();
            st->shard.reset();  // drains every stream's FIFO
        } else {
            // Stop the Shard off this thread: its destructor wakes submitters
            // blocked on a slot (their submit then returns false) and joins
            // the completion threads, which cannot end while an event never
            // fires. Wait for that a bounded time, then report either way.
            std::thread([st] {
                st->shard.reset();
                for (auto& t : st->submitters) t.join();
                std::lock_guard<std::mutex> lk(st->mu);
                st->reaped = true;
                st->cv.notify_all();
            }).detach();
            std::unique_lock<std::mutex> lk(st->mu);
            st->cv.wait_for(lk, std::chrono::seconds(10), [&] { return st->reaped; });
        }
    }
    if (!timed_out.empty())
        throw std::runtime_error(std::string(what) + ": timed out, jobs outstanding:" + timed_out);

    py::list copy_out, fabric_out;
    std::lock_guard<std::mutex> lk(st->mu);
    for (size_t i = 0; i < n_all; i++) {
        const ShardRun::Result& r = st->results[i];
        if (i < n_copy) {
            py::dict d;
            d["submitted"] = r.submitted;
            d["done_calls"] = r.done_calls;
            d["ok"] = r.ok;
            d["scales"] = py::cast(r.done_calls ? r.scales
                                                : (st->scales[i] ? *st->scales[i]
                                                                 : std::vector<float>()));
            copy_out.append(d);
        } else {
            const size_t k = i - n_copy;
            if (get_bufs[k]) {
                const py::buffer_info& info = host_bufs[k];
                memcpy(info.ptr, get_bufs[k].get(),
                       static_cast<size_t>(info.size) * static_cast<size_t>(info.itemsize));
            }
            fabric_out.append(py::make_tuple(r.done_calls, r.ok));
        }
    }
    return py::make_tuple(copy_out, fabric_out);
}

py::tuple shard_run_py(int device, int n_streams, int slots_per_stream,
                       size_t max_descs_per_slot, const py::list& copy_jobs,
                       const py::list& fabric_jobs, int n_threads, double timeout_s) {
    return shard_run_impl("_dbg_shard_run", device, n_streams, slots_per_stream,
                          max_descs_per_slot, copy_jobs, fabric_jobs, n_threads, timeout_s,
                          nullptr);
}

// Shard::completion_loop's search (server/completed_prefix.h) over a modelled
// queue: has_slot[i] says whether task i is real; at the k-th question
// fired_at_query[k] (its last value from then on) real tasks, in FIFO order,
// have fired. Returns the prefix and the indices asked about, in order.
std::pair<size_t, std::vector<size_t>> completed_prefix_py(
    const std::vector<bool>& has_slot, const std::vector<size_t>& fired_at_query) {
    std::vector<size_t> rank(has_slot.size(), 0);  // real tasks before task i
    size_t reals = 0;
    for (size_t i = 0; i < has_slot.size(); i++) {
        rank[i] = reals;
        if (has_slot[i]) reals++;
    }
    std::vector<size_t> asked;
    size_t prefix = completed_prefix(
        has_slot.size(), [&](size_t i) { return static_cast<bool>(has_slot[i]); },
        [&](size_t i) {
            if (!has_slot[i])
                throw std::logic_error("completed_prefix asked about a null-slot task");
            size_t fired = 0;
            if (!fired_at_query.empty())
                fired = fired_at_query[std::min(asked.size(), fired_at_query.size() - 1)];
            asked.push_back(i);
            return rank[i] < fired;
        });
    return {prefix, asked};
}

}  // namespace

PYBIND11_MODULE(_native, m) {
    m.doc() = "infinistore-amd native core (MI355X / ROCm)";

    // ---- configs ----
    py::class_<ClientConfigC>(m, "ClientConfig")
        .def(py::init<>())
        .def_readwrite("host_addr", &ClientConfigC::host_addr)
        .def_readwrite("service_port", &ClientConfigC::service_port)
        .def_readwrite("connection_type", &ClientConfigC::connection_type)
        .def_readwrite("dev_name", &ClientConfigC::dev_name)
        .def_readwrite("ib_port", &ClientConfigC::ib_port)
        .def_readwrite("link_type", &ClientConfigC::link_type)
        .def_readwrite("log_level", &ClientConfigC::log_level);

    py::class_<ServerConfigPy>(m, "ServerConfig")
        .def(py::init<>())
        .def_readwrite("manage_port", &ServerConfigPy::manage_port)
        .def_readwrite("service_port", &ServerConfigPy::service_port)
        .def_readwrite("log_level", &ServerConfigPy::log_level)
        .def_readwrite("dev_name", &ServerConfigPy::dev_name)
        .def_readwrite("ib_port", &ServerConfigPy::ib_port)
        .def_readwrite("link_type", &ServerConfigPy::link_type)
        .def_readwrite("prealloc_size", &ServerConfigPy::prealloc_size)
        .def_readwrite("minimal_allocate_size", &ServerConfigPy::minimal_allocate_size)
        .def_readwrite("num_stream", &ServerConfigPy::num_stream)
        .def_readwrite("auto_increase", &ServerConfigPy::auto_increase)
        .def_readwrite("devices", &ServerConfigPy::devices)
        .def_readwrite("cpu_only", &ServerConfigPy::cpu_only)
        .def_readwrite("cpu_shards", &ServerConfigPy::cpu_shards)
        .def_readwrite("auto_evict", &ServerConfigPy::auto_evict)
        .def_readwrite("ttl_seconds", &ServerConfigPy::ttl_seconds)
        .def_readwrite("io_threads", &ServerConfigPy::io_threads)
        .def_readwrite("extend_size", &ServerConfigPy::extend_size);

    // ---- client connection ----
    py::class_<ClientConn>(m, "Connection")
        .def(py::init<>())
        .def("init_connection", &ClientConn::init_connection,
             py::call_guard<py::gil_scoped_release>())
        .def("setup_rdma", &ClientConn::setup_rdma, py::call_guard<py::gil_scoped_release>())
        .def("close_conn", &ClientConn::close_conn, py::call_guard<py::gil_scoped_release>())
        .def(
            "rw_local",
            [](ClientConn& c, const std::string& op,
               const std::vector<std::pair<std::string, uint64_t>>& blocks, int block_size,
               uintptr_t ptr, int device) {
                py::gil_scoped_release rel;
                return c.rw_local(op.empty() ? 'W' : op[0], blocks, block_size, ptr, device);
            })
        .def(
            "rw_local_fast",
            [](ClientConn& c, const std::string& op, py::bytes keys_blob, py::bytes offsets,
               size_t n, int block_size, uintptr_t ptr, int device, bool sync_response) {
                char* kb;
                Py_ssize_t kb_len;
                PyBytes_AsStringAndSize(keys_blob.ptr(), &kb, &kb_len);
                char* ob;
                Py_ssize_t ob_len;
                PyBytes_AsStringAndSize(offsets.ptr(), &ob, &ob_len);
                if (static_cast<size_t>(ob_len) != n * 8)
                    throw std::runtime_error("offsets must be n uint64");
                py::gil_scoped_release rel;
                return c.rw_local_packed(op.empty() ? 'W' : op[0], kb,
                                         static_cast<size_t>(kb_len),
                                         reinterpret_cast<const uint64_t*>(ob), n, block_size,
                                         ptr, device, sync_response);
            },
            py::arg("op"), py::arg("keys_blob"), py::arg("offsets"), py::arg("n"),
            py::arg("block_size"), py::arg("ptr"), py::arg("device"),
            py::arg("sync_response") = false)
        .def(
            "rw_local_keys",
            [](ClientConn& c, const std::string& op, py::list keys, py::buffer offsets,
               uint64_t element_size, int block_size, uintptr_t ptr, int device,
               bool sync_response, uint32_t extra_flags, uint32_t n_segments,
               uint64_t segment_stride, const py::object& page_slice) {
                // page_slice: None or (n_pieces, page, offset, piece, stride)
                // in elements; reads only (the client refuses it on 'W').
                const PackedLocalSliceExt sl =
                    slice_to_wire(slice_from_py("rw_local", page_slice, element_size));
                // Build the NUL-joined key blob and byte offsets in C++ —
                // no Python-side join/numpy work on the hot path.
                py::buffer_info ob = offsets.request();
                size_t n = static_cast<size_t>(py::len(keys));
                if (ob.itemsize != 8 || static_cast<size_t>(ob.size) < n)
                    throw std::runtime_error("offsets must be uint64[n]");
                const uint64_t* offs = static_cast<const uint64_t*>(ob.ptr);
                std::string blob;
                blob.reserve(n * 48);
                std::vector<uint64_t> byte_offs(n);
                for (size_t i = 0; i < n; i++) {
                    Py_ssize_t klen = 0;
                    const char* ks =
                        PyUnicode_AsUTF8AndSize(keys[i].ptr(), &klen);
                    if (!ks) throw std::runtime_error("keys must be str");
                    if (i) blob.push_back('\0');
                    blob.append(ks, static_cast<size_t>(klen));
                    byte_offs[i] = offs[i] * element_size;
                }
                py::gil_scoped_release rel;
                return c.rw_local_packed(op.empty() ? 'W' : op[0], blob.data(), blob.size(),
                                         byte_offs.data(), n, block_size, ptr, device,
                                         sync_response, nullptr, extra_flags, n_segments,
                                         segment_stride * element_size, &sl);
            },
            py::arg("op"), py::arg("keys"), py::arg("offsets"), py::arg("element_size"),
            py::arg("block_size"), py::arg("ptr"), py::arg("device"),
            py::arg("sync_response") = false, py::arg("extra_flags") = 0,
            py::arg("n_segments") = 1, py::arg("segment_stride") = 0,
            py::arg("page_slice") = py::none())
        .def(
            "rw_local_blob",
            [](ClientConn& c, const std::string& op, py::buffer blob, py::buffer offsets,
               uint64_t element_size, int block_size, uintptr_t ptr, int device,
               bool sync_response, uint32_t extra_flags, uint32_t n_segments,
               uint64_t segment_stride, const py::object& page_slice) {
                // page_slice: None or (n_pieces, page, offset, piece, stride)
                // in elements; reads only (the client refuses it on 'W').
                const PackedLocalSliceExt sl =
                    slice_to_wire(slice_from_py("rw_local", page_slice, element_size));
                // Zero-pack fast path: keys as one NUL-separated bytes blob
                // (engines cache the serialized page-key chain; re-joining
                // 2k Python strings costs ~30 µs per request otherwise).
                py::buffer_info bb = blob.request();
                py::buffer_info ob = offsets.request();
                if (ob.itemsize != 8) throw std::runtime_error("offsets must be uint64[n]");
                size_t n = static_cast<size_t>(ob.size);
                const uint64_t* offs = static_cast<const uint64_t*>(ob.ptr);
                std::vector<uint64_t> byte_offs(n);
                for (size_t i = 0; i < n; i++) byte_offs[i] = offs[i] * element_size;
                const char* bp = static_cast<const char*>(bb.ptr);
                size_t blen = static_cast<size_t>(bb.size) * bb.itemsize;
                py::gil_scoped_release rel;
                return c.rw_local_packed(op.empty() ? 'W' : op[0], bp, blen, byte_offs.data(),
                                         n, block_size, ptr, device, sync_response, nullptr,
                                         extra_flags, n_segments,
                                         segment_stride * element_size, &sl);
            },
            py::arg("op"), py::arg("blob"), py::arg("offsets"), py::arg("element_size"),
            py::arg("block_size"), py::arg("ptr"), py::arg("device"),
            py::arg("sync_response") = false, py::arg("extra_flags") = 0,
            py::arg("n_segments") = 1, py::arg("segment_stride") = 0,
            py::arg("page_slice") = py::none())
        .def(
            "rw_local_blob_async",
            [](ClientConn& c, const std::string& op, py::buffer blob, py::buffer offsets,
               uint64_t element_size, int block_size, uintptr_t ptr, int device,
               uint32_t n_segments, uint64_t segment_stride, const py::object& page_slice) {
                const PackedLocalSliceExt sl =
                    slice_to_wire(slice_from_py("rw_local", page_slice, element_size));
                // Ticketed form: push the (sync-response) op and return a
                // ticket to pass to wait_local_ticket — the engine overlaps
                // its own work with the copy. Ticket 0 = already complete
                // (op fell back to the blocking socket path).
                py::buffer_info bb = blob.request();
                py::buffer_info ob = offsets.request();
                if (ob.itemsize != 8) throw std::runtime_error("offsets must be uint64[n]");
                size_t n = static_cast<size_t>(ob.size);
                const uint64_t* offs = static_cast<const uint64_t*>(ob.ptr);
                std::vector<uint64_t> byte_offs(n);
                for (size_t i = 0; i < n; i++) byte_offs[i] = offs[i] * element_size;
                const char* bp = static_cast<const char*>(bb.ptr);
                size_t blen = static_cast<size_t>(bb.size) * bb.itemsize;
                uint64_t ticket = 0;
                int ret;
                {
                    py::gil_scoped_release rel;
                    ret = c.rw_local_packed(op.empty() ? 'R' : op[0], bp, blen,
                                            byte_offs.data(), n, block_size, ptr, device,
                                            /*sync_response=*/true, &ticket, 0, n_segments,
                                            segment_stride * element_size, &sl);
                }
                return py::make_tuple(ret, ticket);
            },
            py::arg("op"), py::arg("blob"), py::arg("offsets"), py::arg("element_size"),
            py::arg("block_size"), py::arg("ptr"), py::arg("device"),
            py::arg("n_segments") = 1, py::arg("segment_stride") = 0,
            py::arg("page_slice") = py::none())
        .def(
            "rw_tset_blob",
            [](ClientConn& c, const std::string& op, py::buffer blob, py::buffer offsets,
               uint64_t element_size, int block_size, uint32_t set_id, uint32_t n_tensors,
               int device, bool sync_response, uint32_t extra_flags, uint32_t n_segments,
               uint64_t segment_stride, bool ticketed) {
                // rw_local_blob over a registered tensor set: offsets (in
                // elements) are relative to every tensor of the set and
                // n_segments is the total over all tensors. ticketed: as
                // rw_local_blob_async. Returns (status, ticket).
                py::buffer_info bb = blob.request();
                py::buffer_info ob = offsets.request();
                if (ob.itemsize != 8) throw std::runtime_error("offsets must be uint64[n]");
                size_t n = static_cast<size_t>(ob.size);
                const uint64_t* offs = static_cast<const uint64_t*>(ob.ptr);
                std::vector<uint64_t> byte_offs(n);
                for (size_t i = 0; i < n; i++) byte_offs[i] = offs[i] * element_size;
                const char* bp = static_cast<const char*>(bb.ptr);
                size_t blen = static_cast<size_t>(bb.size) * bb.itemsize;
                const PackedLocalTensorExt ts{set_id, n_tensors, 0};
                uint64_t ticket = 0;
                int ret;
                {
                    py::gil_scoped_release rel;
                    ret = c.rw_local_packed(op.empty() ? 'W' : op[0], bp, blen, byte_offs.data(),
                                            n, block_size, 0, device, sync_response || ticketed,
                                            ticketed ? &ticket : nullptr, extra_flags,
                                            n_segments, segment_stride * element_size, nullptr,
                                            &ts);
                }
                return py::make_tuple(ret, ticket);
            },
            py::arg("op"), py::arg("blob"), py::arg("offsets"), py::arg("element_size"),
            py::arg("block_size"), py::arg("set_id"), py::arg("n_tensors"), py::arg("device"),
            py::arg("sync_response") = false, py::arg("extra_flags") = 0,
            py::arg("n_segments") = 1, py::arg("segment_stride") = 0,
            py::arg("ticketed") = false)
        .def("register_tensor_set", &ClientConn::register_tensor_set, py::arg("ptrs"),
             py::arg("extents"), py::arg("device"), py::call_guard<py::gil_scoped_release>())
        .def("release_tensor_set", &ClientConn::release_tensor_set, py::arg("set_id"),
             py::call_guard<py::gil_scoped_release>())
        .def("wait_local_ticket", &ClientConn::wait_local_ticket,
             py::call_guard<py::gil_scoped_release>())
        .def("sync_local", &ClientConn::sync_local, py::call_guard<py::gil_scoped_release>())
        .def("register_mr", &ClientConn::register_mr, py::call_guard<py::gil_scoped_release>())
        .def(
            "allocate_rdma",
            [](ClientConn& c, const std::vector<std::string>& keys, int block_size) {
                std::vector<RemoteBlockOut> res;
                {
                    py::gil_scoped_release rel;
                    res = c.allocate_rdma(keys, block_size);
                }
                py::list out;
                for (auto& b : res) out.append(py::make_tuple(b.rkey, b.remote_addr));
                return out;
            })
        .def(
            "allocate_rdma_async",
            [](ClientConn& c, const std::vector<std::string>& keys, int block_size,
               py::function cb) {
                auto cbp = hold_callback(std::move(cb));
                auto cb_cpp = [cbp](std::vector<RemoteBlockOut> res) {
                    py::gil_scoped_acquire acq;
                    py::list out;
                    for (auto& b : res) out.append(py::make_tuple(b.rkey, b.remote_addr));
                    (*cbp)(out);
                };
                py::gil_scoped_release rel;
                return c.allocate_rdma_async(keys, block_size, std::move(cb_cpp));
            })
        .def(
            "w_rdma",
            [](ClientConn& c, const std::vector<uint64_t>& offsets, int block_size,
               const std::vector<std::pair<uint32_t, uint64_t>>& remote_blocks, uintptr_t ptr) {
                std::vector<RemoteBlockOut> blks;
                blks.reserve(remote_blocks.size());
                for (auto& rb : remote_blocks) blks.push_back({rb.first, rb.second});
                py::gil_scoped_release rel;
                return c.w_rdma(offsets.data(), offsets.size(), block_size, blks.data(),
                                blks.size(), ptr);
            })
        .def(
            "w_rdma_async",
            [](ClientConn& c, const std::vector<uint64_t>& offsets, int block_size,
               const std::vector<std::pair<uint32_t, uint64_t>>& remote_blocks, uintptr_t ptr,
               py::function cb) {
                std::vector<RemoteBlockOut> blks;
                blks.reserve(remote_blocks.size());
                for (auto& rb : remote_blocks) blks.push_back({rb.first, rb.second});
                auto cbp = hold_callback(std::move(cb));
                auto cb_cpp = [cbp]() {
                    py::gil_scoped_acquire acq;
                    (*cbp)();
                };
                py::gil_scoped_release rel;
                return c.w_rdma_async(offsets.data(), offsets.size(), block_size, blks.data(),
                                      blks.size(), ptr, std::move(cb_cpp));
            })
        .def(
            "r_rdma",
            [](ClientConn& c, const std::vector<std::pair<std::string, uint64_t>>& blocks,
               int block_size, uintptr_t ptr) {
                py::gil_scoped_release rel;
                return c.r_rdma(blocks, block_size, ptr);
            })
        .def(
            "r_rdma_async",
            [](ClientConn& c, const std::vector<std::pair<std::string, uint64_t>>& blocks,
               int block_size, uintptr_t ptr, py::function cb) {
                auto cbp = hold_callback(std::move(cb));
                auto cb_cpp = [cbp]() {
                    py::gil_scoped_acquire acq;
                    (*cbp)();
                };
                py::gil_scoped_release rel;
                return c.r_rdma_async(blocks, block_size, ptr, std::move(cb_cpp));
            })
        .def("sync_rdma", &ClientConn::sync_rdma, py::call_guard<py::gil_scoped_release>())
        .def("check_exist", &ClientConn::check_exist, py::call_guard<py::gil_scoped_release>())
        .def("get_match_last_index", &ClientConn::get_match_last_index,
             py::call_guard<py::gil_scoped_release>())
        .def("delete_keys", &ClientConn::delete_keys, py::call_guard<py::gil_scoped_release>())
        .def("get_stats", &ClientConn::get_stats, py::call_guard<py::gil_scoped_release>())
        .def("shm_active", &ClientConn::shm_active)
        .def("using_verbs", &ClientConn::using_verbs);

    // ---- server ----
    m.def("start_server", &start_server, py::call_guard<py::gil_scoped_release>());
    m.def("stop_server", &stop_server, py::call_guard<py::gil_scoped_release>());
    m.def("purge_kv_map", &purge_kv_map_py);
    m.def("get_kvmap_len", &get_kvmap_len_py);
    m.def("server_stats", &server_stats_py);
    m.def("server_compact", &server_compact_py, py::call_guard<py::gil_scoped_release>());
    m.def("server_snapshot", [](const std::string& path) {
        std::pair<size_t, size_t> r{0, 0};
        bool ok;
        {
            py::gil_scoped_release rel;
            ok = g_server && g_server->snapshot(path, &r);
        }
        return py::make_tuple(ok, r.first, r.second);
    });
    m.def("server_restore", [](const std::string& path) {
        std::pair<size_t, size_t> r{0, 0};
        bool ok;
        {
            py::gil_scoped_release rel;
            ok = g_server && g_server->restore(path, &r);
        }
        return py::make_tuple(ok, r.first, r.second);
    });

    // ---- logging ----
    m.def("set_log_level", [](const std::string& lvl) { set_log_level(lvl.c_str()); });
    m.def("log_msg", [](const std::string& lvl, const std::string& msg) {
        LogLevel l = LogLevel::kInfo;
        if (lvl == "debug") l = LogLevel::kDebug;
        else if (lvl == "warning" || lvl == "warn") l = LogLevel::kWarn;
        else if (lvl == "error") l = LogLevel::kError;
        log_printf(l, "python", 0, "%s", msg.c_str());
    });

    // ---- GPU info / kernels ----
    m.def("gpu_available", [] { return gpu::available(); });
    m.def("gpu_count", [] { return gpu::device_count(); });
    m.def("hash_blocks", &hash_blocks_py, py::call_guard<py::gil_scoped_release>());

    // ---- debug/test surface (kernels, launched directly) ----
    m.def("_dbg_copy_blocks", &copy_blocks_py, py::arg("src_ptrs"), py::arg("dst_ptrs"),
          py::arg("bytes_per_block"), py::arg("device"), py::arg("path"),
          py::call_guard<py::gil_scoped_release>());
    m.def("_dbg_quant_blocks",
          [](const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst,
             size_t elems_per_block, int device) {
              return transform_blocks_py("_dbg_quant_blocks", PageCodec::kFp8, PageDir::kStore,
                                         src, dst, {}, elems_per_block, device);
          },
          py::arg("src_ptrs"), py::arg("dst_ptrs"), py::arg("elems_per_block"),
          py::arg("device"), py::call_guard<py::gil_scoped_release>());
    m.def("_dbg_dequant_blocks",
          [](const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst,
             const std::vector<float>& scales, size_t elems_per_block, int device) {
              transform_blocks_py("_dbg_dequant_blocks", PageCodec::kFp8, PageDir::kLoad, src,
                                  dst, scales, elems_per_block, device);
          },
          py::arg("src_ptrs"), py::arg("dst_ptrs"), py::arg("scales"),
          py::arg("elems_per_block"), py::arg("device"),
          py::call_guard<py::gil_scoped_release>());

    // ---- debug/test surface (segmented kernels, launched directly) ----
    m.def("_dbg_copy_blocks_seg", &copy_blocks_seg_py, py::arg("client_ptrs"),
          py::arg("pool_ptrs"), py::arg("bytes_per_block"), py::arg("n_segments"),
          py::arg("segment_stride"), py::arg("to_pool"), py::arg("device"), py::arg("path"),
          py::call_guard<py::gil_scoped_release>());
    m.def("_dbg_quant_blocks_seg",
          [](int codec, const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst,
             size_t elems_per_block, uint32_t n_segments, uint64_t segment_stride, int device) {
              return transform_blocks_seg_py("_dbg_quant_blocks_seg", codec, PageDir::kStore,
                                             src, dst, {}, elems_per_block, n_segments,
                                             segment_stride, device);
          },
          py::arg("codec"), py::arg("src_ptrs"), py::arg("dst_ptrs"),
          py::arg("elems_per_block"), py::arg("n_segments"), py::arg("segment_stride"),
          py::arg("device"), py::call_guard<py::gil_scoped_release>());
    m.def("_dbg_dequant_blocks_seg",
          [](int codec, const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst,
             const std::vector<float>& scales, size_t elems_per_block, uint32_t n_segments,
             uint64_t segment_stride, int device) {
              transform_blocks_seg_py("_dbg_dequant_blocks_seg", codec, PageDir::kLoad, src,
                                      dst, scales, elems_per_block, n_segments, segment_stride,
                                      device);
          },
          py::arg("codec"), py::arg("src_ptrs"), py::arg("dst_ptrs"), py::arg("scales"),
          py::arg("elems_per_block"), py::arg("n_segments"), py::arg("segment_stride"),
          py::arg("device"), py::call_guard<py::gil_scoped_release>());

    // ---- debug/test surface (the codec table: csrc/core/page_codec.h) ----
    m.def("_dbg_page_codec", &page_codec_py, py::arg("flags"), py::arg("page_bytes"));
    // The read-size predicates, codec by id (0 none, 1 fp8, 2 mxfp4): may a
    // block of `stored` bytes answer a whole-page read of `page` bytes, and
    // does it hold exactly that page (sliced and tensor-set reads).
    m.def("_dbg_stored_serves",
          [](int codec, size_t stored, size_t page) {
              return stored_serves(codec_from_id("_dbg_stored_serves", codec), stored, page);
          },
          py::arg("codec"), py::arg("stored"), py::arg("page"));
    m.def("_dbg_stored_matches",
          [](int codec, size_t stored, size_t page) {
              return stored_matches(codec_from_id("_dbg_stored_matches", codec), stored, page);
          },
          py::arg("codec"), py::arg("stored"), py::arg("page"));
    // The segment-geometry predicate, codec by id (0 none, 1 fp8, 2 mxfp4).
    m.def("_dbg_segments_legal",
          [](int codec, size_t page_bytes, uint64_t n_segments, uint64_t stride_bytes) {
              return segments_legal(codec_from_id("_dbg_segments_legal", codec), page_bytes,
                                    n_segments, stride_bytes);
          },
          py::arg("codec"), py::arg("page_bytes"), py::arg("n_segments"),
          py::arg("stride_bytes"));
    m.attr("_MAX_PAGE_SEGMENTS") = kMaxPageSegments;
    // The tensor-set predicate; n_segments is the total over all tensors.
    m.def("_dbg_tensors_legal",
          [](int codec, size_t page_bytes, uint64_t n_segments, uint64_t stride_bytes,
             uint64_t n_tensors) {
              return tensors_legal(codec_from_id("_dbg_tensors_legal", codec), page_bytes,
                                   n_segments, stride_bytes, n_tensors);
          },
          py::arg("codec"), py::arg("page_bytes"), py::arg("n_segments"),
          py::arg("stride_bytes"), py::arg("n_tensors"));
    m.attr("_MAX_PAGE_TENSORS") = kMaxPageTensors;
    // The tensor-set launchers (gpu.h), called directly: tensor bases, one
    // client byte offset and one pool pointer per block. Return False for
    // what the launcher refuses; the transform form returns (ok, scales).
    m.def("_dbg_copy_blocks_tset", &copy_blocks_tset_py, py::arg("bases"),
          py::arg("client_offsets"), py::arg("pool_ptrs"), py::arg("bytes_per_block"),
          py::arg("n_segments"), py::arg("segment_stride"), py::arg("to_pool"),
          py::arg("device") = 0, py::arg("force_byte") = false);
    m.def("_dbg_transform_blocks_tset", &transform_blocks_tset_py, py::arg("codec"),
          py::arg("to_pool"), py::arg("bases"), py::arg("client_offsets"),
          py::arg("pool_ptrs"), py::arg("scales"), py::arg("elems_per_block"),
          py::arg("n_segments"), py::arg("segment_stride"), py::arg("device") = 0);
    // The slice-geometry predicate; the slice is (n_pieces, page_bytes, offset,
    // piece_bytes, stride) in bytes, the client segments as above.
    m.def("_dbg_slice_legal",
          [](int codec, const py::object& slice, uint32_t n_segments, uint64_t stride_bytes) {
              if (slice.is_none())
                  throw std::invalid_argument("_dbg_slice_legal: a slice is a tuple of 5");
              return slice_legal(codec_from_id("_dbg_slice_legal", codec),
                                 slice_from_py("_dbg_slice_legal", slice, 1),
                                 PageSegments{n_segments, stride_bytes});
          },
          py::arg("codec"), py::arg("slice"), py::arg("n_segments") = 1,
          py::arg("stride_bytes") = 0);
    m.attr("_MAX_SLICE_PIECES") = kMaxSlicePieces;
    m.attr("_SLICE_THREADS") = gpu::kSliceThreads;
    // The sliced-load launcher (gpu.h, launch_load_sliced), called directly:
    // codec id, stored block pointers, client page pointers, one scale per
    // block for fp8 (else ignored), the slice in bytes, the client segments.
    m.def("_dbg_load_sliced", &load_sliced_py, py::arg("codec"), py::arg("stored_ptrs"),
          py::arg("client_ptrs"), py::arg("scales"), py::arg("slice"),
          py::arg("n_segments") = 1, py::arg("segment_stride") = 0, py::arg("device") = 0);
    // _dbg_shard_run's copy jobs, each with a slice (or None) from `slices`.
    m.def("_dbg_shard_run_sliced",
          [](int device, int n_streams, int slots_per_stream, size_t max_descs_per_slot,
             const py::list& copy_jobs, const py::list& slices, int n_threads,
             double timeout_s) -> py::object {
              py::tuple out = shard_run_impl("_dbg_shard_run_sliced", device, n_streams,
                                             slots_per_stream, max_descs_per_slot, copy_jobs,
                                             py::list(), n_threads, timeout_s, &slices);
              return out[0];
          },
          py::arg("device"), py::arg("n_streams"), py::arg("slots_per_stream"),
          py::arg("max_descs_per_slot"), py::arg("copy_jobs"), py::arg("slices"),
          py::arg("n_threads"), py::arg("timeout_s"));
    // _dbg_shard_run's copy jobs, each over a tensor set (or None) from
    // `tsets`: (bases, segs_per_tensor), the client side being offsets.
    // `slices` as for _dbg_shard_run_sliced (a set with a slice is refused).
    m.def("_dbg_shard_run_tset",
          [](int device, int n_streams, int slots_per_stream, size_t max_descs_per_slot,
             const py::list& copy_jobs, const py::list& tsets, int n_threads,
             double timeout_s, const py::object& slices) -> py::object {
              py::list sl;
              if (!slices.is_none()) sl = slices.cast<py::list>();
              py::tuple out = shard_run_impl("_dbg_shard_run_tset", device, n_streams,
                                             slots_per_stream, max_descs_per_slot, copy_jobs,
                                             py::list(), n_threads, timeout_s,
                                             slices.is_none() ? nullptr : &sl, &tsets);
              return out[0];
          },
          py::arg("device"), py::arg("n_streams"), py::arg("slots_per_stream"),
          py::arg("max_descs_per_slot"), py::arg("copy_jobs"), py::arg("tsets"),
          py::arg("n_threads"), py::arg("timeout_s"), py::arg("slices") = py::none());
    // Jobs through a real Shard at small limits. A copy job is (src_ptrs,
    // dst_ptrs, bytes_per_block, codec_id, store, n_segments, segment_stride,
    // scales or None, scales_off), a fabric job (is_put, host buffer,
    // block_ptrs, host_offsets, bytes_per_block). Returns ([{submitted,
    // done_calls, ok, scales}], [(done_calls, ok)]); device -1 is a CPU shard.
    m.def("_dbg_shard_run", &shard_run_py, py::arg("device"), py::arg("n_streams"),
          py::arg("slots_per_stream"), py::arg("max_descs_per_slot"), py::arg("copy_jobs"),
          py::arg("fabric_jobs"), py::arg("n_threads"), py::arg("timeout_s"));
    m.attr("_SHARD_FAN_CHUNK") = Shard::kFanChunk;
    m.attr("_FAB_STAGE_BYTES") = Shard::kFabStageBytes;
    m.attr("_FAB_STAGE_DESCS") = Shard::kFabStageDescs;
    m.def("_dbg_completed_prefix", &completed_prefix_py, py::arg("has_slot"),
          py::arg("fired_at_query"));
    // Packed fast-path framing (core/protocol.h), with and without the
    // segment and slice extensions. op is "w" or "r"; offsets and the slice
    // (n_pieces, page_bytes, offset, piece_bytes, stride) are in bytes.
    m.def("_dbg_build_packed_local",
          [](int device, int pid, uint64_t base_ptr, uint64_t base_offset, uint32_t block_size,
             uint32_t flags, uint32_t alloc_mb, py::bytes ipc,
             const std::vector<uint64_t>& offsets, const std::vector<std::string>& keys,
             uint32_t n_segments, uint64_t segment_stride, const py::object& slice,
             const py::object& tensor_set) {
              const PackedLocalSliceExt sl =
                  slice_to_wire(slice_from_py("_dbg_build_packed_local", slice, 1));
              // None, or (set_id, n_tensors[, rsvd])
              PackedLocalTensorExt ts{};
              if (!tensor_set.is_none()) {
                  py::tuple t = tensor_set.cast<py::tuple>();
                  if (t.size() != 2 && t.size() != 3)
                      throw std::invalid_argument(
                          "_dbg_build_packed_local: a tensor set is (set_id, n_tensors)");
                  ts.set_id = t[0].cast<uint32_t>();
                  ts.n_tensors = t[1].cast<uint32_t>();
                  ts.rsvd = t.size() == 3 ? t[2].cast<uint64_t>() : 0;
              }
              std::string ipc_s = ipc;
              if (ipc_s.size() != 64)
                  throw std::invalid_argument("_dbg_build_packed_local: ipc is 64 bytes");
              if (offsets.size() != keys.size())
                  throw std::invalid_argument("_dbg_build_packed_local: one offset per key");
              PackedLocalHdr h;
              h.device = device;
              h.pid = pid;
              h.base_ptr = base_ptr;
              h.base_offset = base_offset;
              h.block_size = block_size;
              h.n_blocks = static_cast<uint32_t>(keys.size());
              h.flags = flags;
              h.rsvd = alloc_mb;
              memcpy(h.ipc, ipc_s.data(), 64);
              std::string blob;
              for (size_t i = 0; i < keys.size(); i++) {
                  if (i) blob.push_back('\0');
                  blob.append(keys[i]);
              }
              auto v = build_packed_local(h, n_segments, segment_stride, offsets.data(),
                                          blob.data(), blob.size(), &sl,
                                          tensor_set.is_none() ? nullptr : &ts);
              return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
          },
          py::arg("device"), py::arg("pid"), py::arg("base_ptr"), py::arg("base_offset"),
          py::arg("block_size"), py::arg("flags"), py::arg("alloc_mb"), py::arg("ipc"),
          py::arg("offsets"), py::arg("keys"), py::arg("n_segments") = 1,
          py::arg("segment_stride") = 0, py::arg("slice") = py::none(),
          py::arg("tensor_set") = py::none());
    m.def("_dbg_parse_packed_local", [](const std::string& op, py::bytes data) {
        std::string s = data;
        PackedLocalReq r;
        if (op != "w" && op != "r")
            throw std::invalid_argument("_dbg_parse_packed_local: op is \"w\" or \"r\"");
        if (!parse_packed_local(op[0], reinterpret_cast<const uint8_t*>(s.data()), s.size(), &r))
            throw std::invalid_argument("_dbg_parse_packed_local: INVALID_REQ");
        py::dict d;
        d["device"] = r.hdr.device;
        d["pid"] = r.hdr.pid;
        d["base_ptr"] = r.hdr.base_ptr;
        d["base_offset"] = r.hdr.base_offset;
        d["block_size"] = r.hdr.block_size;
        d["flags"] = r.hdr.flags;
        d["alloc_mb"] = r.hdr.rsvd;
        d["n_segments"] = r.n_segments;
        d["segment_stride"] = r.segment_stride;
        // None, or (n_pieces, page_bytes, offset, piece_bytes, stride)
        if (r.slice.n_pieces)
            d["slice"] = py::make_tuple(r.slice.n_pieces, r.slice.page_bytes, r.slice.offset,
                                        r.slice.piece_bytes, r.slice.stride);
        else
            d["slice"] = py::none();
        // None, or (set_id, n_tensors)
        if (r.has_tset)
            d["tensor_set"] = py::make_tuple(r.tset.set_id, r.tset.n_tensors);
        else
            d["tensor_set"] = py::none();
        py::list offs, keys;
        for (auto& [key, off] : r.blocks) {
            offs.append(off);
            keys.append(py::str(std::string(key)));
        }
        d["offsets"] = offs;
        d["keys"] = keys;
        return d;
    });
    // One (name, wire flag, page-size multiple in bf16 elements) per codec.
    m.def("_page_codec_rows", [] {
        std::vector<std::tuple<std::string, uint32_t, size_t>> rows;
        for (const PageCodecInfo& i : kPageCodecs)
            rows.emplace_back(i.name, i.flag,
                              (i.page_multiple + kPageElemBytes - 1) / kPageElemBytes);
        return rows;
    });

    // ---- debug/test surface (fp8 codec on the host: csrc/gpu/fp8_codec.h) ----
    m.def("_dbg_fp8_encode", [](py::buffer f32) {
        py::buffer_info in = f32.request();
        if (in.itemsize != 4 || in.format != py::format_descriptor<float>::format())
            throw std::invalid_argument("_dbg_fp8_encode takes a float32 buffer");
        const float* x = static_cast<const float*>(in.ptr);
        std::string out(static_cast<size_t>(in.size), '\0');
        for (size_t i = 0; i < out.size(); i++)
            out[i] = static_cast<char>(fp8::f32_to_e4m3(x[i]));
        return py::bytes(out);
    });
    m.def("_dbg_fp8_decode", [](py::buffer codes, float scale) {
        py::buffer_info in = codes.request();
        if (in.itemsize != 1) throw std::invalid_argument("_dbg_fp8_decode takes a uint8 buffer");
        const uint8_t* c = static_cast<const uint8_t*>(in.ptr);
        std::vector<uint16_t> out(static_cast<size_t>(in.size));
        for (size_t i = 0; i < out.size(); i++) out[i] = fp8::decode_to_bf16(c[i], scale);
        return py::bytes(reinterpret_cast<const char*>(out.data()), out.size() * 2);
    });
    m.def("_dbg_fp8_scale", [](py::buffer bf16_bits) {
        py::buffer_info in = bf16_bits.request();
        if (in.itemsize != 2)
            throw std::invalid_argument("_dbg_fp8_scale takes the uint16 bits of a bf16 page");
        const uint16_t* h = static_cast<const uint16_t*>(in.ptr);
        uint32_t m = 0;
        for (py::ssize_t i = 0; i < in.size; i++) m = fp8::absmax_step(m, h[i]);
        return fp8::scale_from_absmax_bits(m);
    });

    // ---- debug/test surface (mxfp4 kernels, and the codec on the host:
    // csrc/gpu/mxfp4_codec.h) ----
    m.def("_dbg_mxfp4_quant_blocks",
          [](const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst,
             size_t elems_per_block, int device) {
              transform_blocks_py("_dbg_mxfp4_quant_blocks", PageCodec::kMxfp4, PageDir::kStore,
                                  src, dst, {}, elems_per_block, device);
          },
          py::arg("src_ptrs"), py::arg("dst_ptrs"), py::arg("elems_per_block"),
          py::arg("device"), py::call_guard<py::gil_scoped_release>());
    m.def("_dbg_mxfp4_dequant_blocks",
          [](const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst,
             size_t elems_per_block, int device) {
              transform_blocks_py("_dbg_mxfp4_dequant_blocks", PageCodec::kMxfp4,
                                  PageDir::kLoad, src, dst, {}, elems_per_block, device);
          },
          py::arg("src_ptrs"), py::arg("dst_ptrs"), py::arg("elems_per_block"),
          py::arg("device"), py::call_guard<py::gil_scoped_release>());
    m.attr("_MXFP4_GROUPS_PER_ITER") = gpu::kMxfp4GroupsPerIter;
    // Scale byte E of ONE group: the uint16 bits of its bf16 elements.
    m.def("_dbg_mxfp4_group_exponent", [](py::buffer bf16_bits) {
        py::buffer_info in = bf16_bits.request();
        if (in.itemsize != 2)
            throw std::invalid_argument(
                "_dbg_mxfp4_group_exponent takes the uint16 bits of a bf16 group");
        const uint16_t* h = static_cast<const uint16_t*>(in.ptr);
        uint32_t key = 0;
        for (py::ssize_t i = 0; i < in.size; i++) key = mxfp4::key_step(key, h[i]);
        return static_cast<int>(mxfp4::group_exponent(key));
    });
    // One e2m1 code per byte (not packed) for each bf16 under scale byte E.
    m.def("_dbg_mxfp4_encode", [](py::buffer bf16_bits, int E) {
        py::buffer_info in = bf16_bits.request();
        if (in.itemsize != 2)
            throw std::invalid_argument("_dbg_mxfp4_encode takes a uint16 buffer");
        if (E < 0 || E > 255) throw std::invalid_argument("_dbg_mxfp4_encode: E is a byte");
        const uint16_t* h = static_cast<const uint16_t*>(in.ptr);
        std::string out(static_cast<size_t>(in.size), '\0');
        for (size_t i = 0; i < out.size(); i++)
            out[i] = static_cast<char>(mxfp4::encode(h[i], static_cast<uint8_t>(E)));
        return py::bytes(out);
    });
    // bf16 bits (as bytes) for each code (one per byte) under scale byte E.
    m.def("_dbg_mxfp4_decode", [](py::buffer codes, int E) {
        py::buffer_info in = codes.request();
        if (in.itemsize != 1)
            throw std::invalid_argument("_dbg_mxfp4_decode takes a uint8 buffer");
        if (E < 0 || E > 255) throw std::invalid_argument("_dbg_mxfp4_decode: E is a byte");
        const uint8_t* c = static_cast<const uint8_t*>(in.ptr);
        std::vector<uint16_t> out(static_cast<size_t>(in.size));
        for (size_t i = 0; i < out.size(); i++)
            out[i] = mxfp4::decode(c[i], static_cast<uint8_t>(E));
        return py::bytes(reinterpret_cast<const char*>(out.data()), out.size() * 2);
    });

    // ---- debug/test surface (wire format + mempool) ----
    m.def("_dbg_build_local_meta", [](int device, py::bytes ipc, int block_size,
                                      const std::vector<std::pair<std::string, uint64_t>>& blocks,
                                      uint64_t base_offset) {
        LocalMetaMsg msg;
        msg.device = device;
        std::string s = ipc;
        msg.ipc_handle.assign(s.begin(), s.end());
        msg.block_size = block_size;
        msg.base_offset = base_offset;
        for (auto& b : blocks) msg.blocks.push_back({b.first, b.second});
        auto v = build_local_meta(msg);
        return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
    });
    // Export a device pointer's IPC handle + allocation offset: lets tests
    // hand-craft reference-framed LocalMetaRequest transcripts (the 'W'/'R'
    // flatbuffers ops) without going through this client library.
    m.def("_dbg_ipc_export", [](uintptr_t ptr) {
        ifs::gpu::IpcHandle h;
        uint64_t off = 0;
        if (!ifs::gpu::ipc_export(reinterpret_cast<void*>(ptr), &h, &off))
            throw std::runtime_error("ipc_export failed");
        return py::make_tuple(
            py::bytes(reinterpret_cast<const char*>(h.bytes), sizeof(h.bytes)), off);
    });

    m.def("_dbg_parse_local_meta", [](py::bytes data) {
        std::string s = data;
        LocalMetaMsg msg;
        if (!parse_local_meta(reinterpret_cast<const uint8_t*>(s.data()), s.size(), &msg))
            throw std::runtime_error("parse failed");
        py::list blocks;
        for (auto& b : msg.blocks) blocks.append(py::make_tuple(b.key, b.offset));
        return py::make_tuple(msg.device, py::bytes(reinterpret_cast<char*>(msg.ipc_handle.data()),
                                                    msg.ipc_handle.size()),
                              msg.block_size, blocks, msg.base_offset);
    });
    m.def("_dbg_build_remote_meta",
          [](const std::vector<std::string>& keys, int block_size, uint32_t rkey,
             const std::vector<uint64_t>& addrs, int op) {
              RemoteMetaMsg msg{keys, block_size, rkey, addrs, static_cast<int8_t>(op)};
              auto v = build_remote_meta(msg);
              return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
          });
    m.def("_dbg_parse_remote_meta", [](py::bytes data) {
        std::string s = data;
        RemoteMetaMsg msg;
        if (!parse_remote_meta(reinterpret_cast<const uint8_t*>(s.data()), s.size(), &msg))
            throw std::runtime_error("parse failed");
        return py::make_tuple(msg.keys, msg.block_size, msg.rkey, msg.remote_addrs,
                              static_cast<int>(msg.op));
    });
    m.def("_dbg_build_alloc_resp", [](const std::vector<std::pair<uint32_t, uint64_t>>& blocks) {
        std::vector<RemoteBlockWire> w;
        for (auto& b : blocks) w.push_back({b.first, 0, b.second});
        auto v = build_allocate_response(w);
        return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
    });
    m.def("_dbg_parse_alloc_resp", [](py::bytes data) {
        std::string s = data;
        std::vector<RemoteBlockWire> w;
        if (!parse_allocate_response(reinterpret_cast<const uint8_t*>(s.data()), s.size(), &w))
            throw std::runtime_error("parse failed");
        py::list out;
        for (auto& b : w) out.append(py::make_tuple(b.rkey, b.remote_addr));
        return out;
    });
    m.def("_dbg_build_match_req", [](const std::vector<std::string>& keys) {
        auto v = build_match_request(keys);
        return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
    });
    m.def("_dbg_parse_match_req", [](py::bytes data) {
        std::string s = data;
        std::vector<std::string> keys;
        if (!parse_match_request(reinterpret_cast<const uint8_t*>(s.data()), s.size(), &keys))
            throw std::runtime_error("parse failed");
        return keys;
    });

    // WR flow-control simulation (chain split + outstanding cap + overflow).
    // shm ring framing/wrap test harness: push `msgs` through a tiny ring
    // with an interleaved consumer, return the bodies read back in order.
    m.def("_dbg_shmring_echo", [](const std::vector<py::bytes>& msgs, uint32_t cap,
                                  int drain_every) {
        std::vector<uint8_t> mem(ifs::shmring::Ring::footprint(cap));
        auto* ring = reinterpret_cast<ifs::shmring::Ring*>(mem.data());
        new (&ring->head) std::atomic<uint64_t>(0);
        new (&ring->tail) std::atomic<uint64_t>(0);
        ring->cap = cap;
        std::vector<py::bytes> out;
        uint64_t seq = 0;
        auto drain = [&] {
            for (;;) {
                uint32_t len = 0;
                uint64_t skip = 0;
                const uint8_t* rec = ring->peek(&len, &skip);
                if (!rec) return;
                if (len) {
                    ifs::shmring::RecHdr h;
                    memcpy(&h, rec, sizeof(h));
                    if (h.seq != ++seq) throw std::runtime_error("seq out of order");
                    out.emplace_back(reinterpret_cast<const char*>(rec + sizeof(h)),
                                     h.body_len);
                }
                ring->consume(skip);
            }
        };
        int pushed = 0;
        for (auto& m2 : msgs) {
            std::string body = m2;
            uint32_t need = ifs::shmring::rec_len(body.size());
            uint64_t adv = 0;
            uint8_t* dst = ring->claim(need, &adv);
            for (long spin = 0; !dst; spin++) {  // full: drain like the consumer would
                drain();
                dst = ring->claim(need, &adv);
                if (spin > 1000000) throw std::runtime_error("ring stuck");
            }
            ifs::shmring::RecHdr h{};
            h.len = need;
            h.op = 'T';
            h.body_len = static_cast<uint32_t>(body.size());
            h.seq = static_cast<uint64_t>(pushed + 1);
            memcpy(dst, &h, sizeof(h));
            memcpy(dst + sizeof(h), body.data(), body.size());
            ring->publish(adv);
            if (++pushed % std::max(1, drain_every) == 0) drain();
        }
        drain();
        return out;
    });
    m.def("_dbg_wrflow_sim", [](int n_wrs, int batch, int cap, int complete_after) {
        std::deque<size_t> inflight_chains;
        std::vector<size_t> posted_sizes;
        long peak = 0;
        WrFlow* flow_ptr = nullptr;
        WrFlow flow(
            [&](const WrChain& ch) {
                posted_sizes.push_back(ch.wrs.size());
                inflight_chains.push_back(ch.wrs.size());
                if (flow_ptr && flow_ptr->outstanding() > peak) peak = flow_ptr->outstanding();
                return true;
            },
            batch, cap);
        flow_ptr = &flow;
        (void)complete_after;
        std::vector<WrDesc> wrs(static_cast<size_t>(n_wrs), WrDesc{0, 0, 0, 0, 0});
        flow.submit(std::move(wrs), true, 42, 7);
        size_t parked_peak = flow.parked();
        // Deliver completions FIFO; draining may post more chains.
        while (!inflight_chains.empty()) {
            size_t n = inflight_chains.front();
            inflight_chains.pop_front();
            flow.on_chain_complete(n);
        }
        return py::make_tuple(posted_sizes, peak, flow.outstanding(), parked_peak,
                              flow.parked());
    });

    // KvIndex harness: run (op, keys) steps against one small index through
    // the server's batched sweep; entries carry no block (null shard/ptr).
    // insert -> won flags, find -> present flags, extract/size/clear -> count.
    m.def("_dbg_kvindex_ops",
          [](const std::vector<std::pair<std::string, std::vector<std::string>>>& steps) {
        using L = KvIndex::Lock;
        KvIndex idx(/*ttl_seconds=*/0, /*stripe_slots=*/4);
        idx.reserve(64);  // small: rehash + tombstone reuse run
        py::list out;
        for (auto& [op, keys] : steps) {
            const size_t n = keys.size();
            std::vector<uint64_t> h(n);
            for (size_t i = 0; i < n; i++) h[i] = KvIndex::hash_of(keys[i]);
            std::vector<bool> flags(n);
            std::vector<Ref<BlockEntry>> dropped;  // displaced / extracted refs
            if (op == "insert") {
                SlabBatch slab(n);
                idx.for_each_batched<L::kExclusive>(
                    n, h.data(), KvIndex::rotated_start(h.data(), n), [&](KvMap& m, size_t i) {
                        Ref<BlockEntry> e(slab.make());
                        flags[i] = idx.insert_locked(m, keys[i], h[i], e, true, &dropped);
                        if (!flags[i]) dropped.push_back(std::move(e));  // loser
                        return true;
                    });
                out.append(flags);
            } else if (op == "find") {
                idx.for_each_batched<L::kShared>(n, h.data(), 0, [&](KvMap& m, size_t i) {
                    flags[i] = idx.find_live(m, keys[i], h[i]) != nullptr;
                    return true;
                });
                out.append(flags);
            } else if (op == "extract") {
                idx.for_each_batched<L::kExclusive>(n, h.data(), 0, [&](KvMap& m, size_t i) {
                    Ref<BlockEntry> ref;
                    if (m.extract(keys[i], &ref)) dropped.push_back(std::move(ref));
                    return true;
                });
                out.append(dropped.size());
            } else if (op == "size" || op == "clear") {
                out.append(op == "size" ? idx.size() : idx.clear());
            } else {
                throw std::runtime_error("unknown op " + op);
            }
        }
        return out;
    });

    // Mempool (host-backed) for allocator unit tests.
    py::class_<MemoryPool>(m, "_TestPool")
        .def(py::init([](size_t size, size_t block_size) {
                 void* base = malloc(size);
                 return new MemoryPool(base, size, block_size, 0);
             }),
             py::return_value_policy::take_ownership)
        .def("allocate",
             [](MemoryPool& p, size_t size) { return reinterpret_cast<uintptr_t>(p.allocate(size)); })
        .def("deallocate",
             [](MemoryPool& p, uintptr_t ptr, size_t size) {
                 return p.deallocate(reinterpret_cast<void*>(ptr), size);
             })
        .def("used_blocks", &MemoryPool::used_blocks)
        .def("total_blocks", &MemoryPool::total_blocks)
        .def("base", [](MemoryPool& p) { return reinterpret_cast<uintptr_t>(p.base()); });
}
