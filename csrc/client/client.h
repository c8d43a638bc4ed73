// infinistore-amd client connection.
//
// API parity with the reference's Connection (/root/reference/src/
// libinfinistore.h:34-122): TCP control plane, local-GPU IPC path,
// allocate/write/commit/read with RDMA semantics, async variants with
// callbacks, sync. Data plane here is the TCP fabric (inline payloads) —
// chosen at OP_RDMA_EXCHANGE time, so an ibverbs fabric can be negotiated
// instead when rdma-core + a NIC exist. Unlike the reference, the commit is
// ACKed by the server before the client's write callback fires, closing the
// reference's sync-before-commit race (libinfinistore.cpp:403-410).
#pragma once

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../core/protocol.h"
#include "../core/shm_ring.h"

namespace ifs {

class VerbsClient;  // client_verbs.h

struct ClientConfigC {
    std::string host_addr;
    int service_port = 0;
    std::string connection_type = "RDMA";  // "RDMA" | "LOCAL_GPU"
    std::string dev_name;                  // verbs fabric only
    int ib_port = 1;
    std::string link_type = "Ethernet";
    std::string log_level = "warning";
};

struct RemoteBlockOut {
    uint32_t rkey;
    uint64_t remote_addr;
};

class ClientConn {
   public:
    ClientConn();  // out-of-line: members hold incomplete types (VerbsClient)
    ~ClientConn();
    ClientConn(const ClientConn&) = delete;
    ClientConn& operator=(const ClientConn&) = delete;

    int init_connection(const ClientConfigC& cfg);  // blocking TCP connect
    int setup_rdma(const ClientConfigC& cfg);       // fabric negotiation
    void close_conn();

    // ---- local (IPC) path ----
    // blocks: (key, byte offset into the tensor). op: 'W' or 'R'.
    int rw_local(char op, const std::vector<std::pair<std::string, uint64_t>>& blocks,
                 int block_size, uintptr_t ptr, int device_id);
    // Fast path: keys as one NUL-separated blob + an offsets array — built
    // straight into the packed wire format (OP_W_FAST / OP_R_FAST).
    // n_segments > 1: every page is that many equal pieces of the tensor,
    // segment_stride BYTES apart (segmented pages, core/page_codec.h); with
    // n_segments == 1 the bytes on the wire are exactly the contiguous ones.
    // The shm ring and the socket carry the same body.
    // slice (reads only; null or n_pieces == 0: whole pages): fetch that
    // strided part of every stored page; block_size is then the sliced page,
    // n_pieces * piece_bytes (sliced reads, core/page_codec.h). A slice on
    // op 'W' returns -INVALID_REQ without sending anything.
    int rw_local_packed(char op, const char* keys_blob, size_t blob_len,
                        const uint64_t* offsets, size_t n, int block_size, uintptr_t ptr,
                        int device_id, bool sync_response = false,
                        uint64_t* out_ticket = nullptr, uint32_t extra_flags = 0,
                        uint32_t n_segments = 1, uint64_t segment_stride = 0,
                        const PackedLocalSliceExt* slice = nullptr,
                        const PackedLocalTensorExt* tset = nullptr);
    // Tensor sets (docs/design.md, "tensor sets"): register the tensors at
    // ptrs[g] (extents[g] bytes each, all on device_id) as one ordered set on
    // this connection; returns the set id (> 0) or a negative status. A
    // request that passes `tset` to rw_local_packed addresses the set: ptr is
    // ignored, offsets are relative to each tensor, n_segments is the total
    // over all tensors. With a slice as well it returns -INVALID_REQ without
    // sending anything.
    int register_tensor_set(const std::vector<uintptr_t>& ptrs,
                            const std::vector<uint64_t>& extents, int device_id);
    int release_tensor_set(uint32_t set_id);
    // Wait for a ticketed (async shm) op; ticket 0 = already complete.
    int wait_local_ticket(uint64_t ticket);
    int sync_local();

    // ---- RDMA-semantics path ----
    int register_mr(uintptr_t ptr, size_t size);
    std::vector<RemoteBlockOut> allocate_rdma(const std::vector<std::string>& keys,
                                              int block_size);
    int allocate_rdma_async(const std::vector<std::string>& keys, int block_size,
                            std::function<void(std::vector<RemoteBlockOut>)> cb);
    int w_rdma(const uint64_t* offsets, size_t n_offsets, int block_size,
               const RemoteBlockOut* blocks, size_t n_blocks, uintptr_t base_ptr);
    int w_rdma_async(const uint64_t* offsets, size_t n_offsets, int block_size,
                     const RemoteBlockOut* blocks, size_t n_blocks, uintptr_t base_ptr,
                     std::function<void()> cb);
    int r_rdma(const std::vector<std::pair<std::string, uint64_t>>& blocks, int block_size,
               uintptr_t base_ptr);
    int r_rdma_async(const std::vector<std::pair<std::string, uint64_t>>& blocks, int block_size,
                     uintptr_t base_ptr, std::function<void()> cb);
    int sync_rdma();  // wait for all async ops to drain

    // ---- queries ----
    int check_exist(const std::string& key);
    int get_match_last_index(const std::vector<std::string>& keys);
    // Delete keys; returns the number removed (extension: engine-driven
    // eviction — the reference only offers wholesale purge).
    int delete_keys(const std::vector<std::string>& keys);
    // Server stats JSON over the wire (extension).
    std::string get_stats();

    bool rdma_connected() const { return rdma_connected_; }
    // Which data plane won the OP_RDMA_EXCHANGE negotiation.
    bool using_verbs() const { return verbs_ != nullptr; }
    // Shared-memory ring transport active (same-host fast path for the
    // packed local ops; csrc/core/shm_ring.h).
    bool shm_active() const { return shm_active_; }

   private:
    // synchronous framed request/response (io_mu_ held)
    bool send_req(char op, const uint8_t* body, size_t n);
    bool recv_status(int* code);
    bool recv_payload(std::vector<uint8_t>* out);  // u32 len + bytes

    int do_w_rdma(const uint64_t* offsets, size_t n_offsets, int block_size,
                  const RemoteBlockOut* blocks, size_t n_blocks, uintptr_t base_ptr);
    int do_r_rdma(const std::vector<std::pair<std::string, uint64_t>>& blocks, int block_size,
                  uintptr_t base_ptr);
    std::vector<RemoteBlockOut> do_allocate(const std::vector<std::string>& keys, int block_size);

    // Is [ptr, ptr+n) device memory? (classified at register_mr time; falls
    // back to a hipPointerGetAttributes probe.)
    bool is_device_ptr(uintptr_t ptr);

    void worker_main();
    void enqueue(std::function<void()> fn);

    // ---- shm ring transport ----
    bool try_shm_setup(int port);  // after connect; silent fallback on failure
    // Push one record; want_resp: wait for and return the server status
    // (mapped like the socket path). Returns kShmNoFit when the record does
    // not fit the ring (caller falls back to the socket after a ring sync).
    static constexpr int kShmNoFit = INT32_MIN;
    static constexpr int kShmErr = INT32_MIN + 1;  // transport failure
    int shm_request(char op, const uint8_t* body, size_t n, bool want_resp,
                    uint64_t* out_ticket = nullptr);
    int shm_wait(uint64_t seq);           // drain responses until seq; io_mu_
    int shm_ring_sync();                  // OP_SYNC over the ring; io_mu_
    void shm_drain_responses();           // non-blocking pop; io_mu_
    shmring::Segment shm_;
    bool shm_active_ = false;
    uint64_t shm_seq_ = 0;
    // EWMA of recent shm response waits (µs): sizes the spin budget so a
    // latency-bound client spins through its ~20-300 µs waits while a
    // saturation client stuck behind ms-scale batches backs off to sleeps
    // instead of burning a core (64 concurrent clients x busy-spin was the
    // config-5 concern).
    double shm_ewma_us_ = 50.0;
    uint64_t shm_unacked_ = 0;  // async ring writes since last ring sync
    int shm_async_err_ = 0;     // first error for an unawaited seq (io_mu_)
    std::unordered_map<uint64_t, int> shm_results_;  // ticketed responses (io_mu_)

    int fd_ = -1;
    bool connected_ = false;
    bool rdma_connected_ = false;
    bool local_dirty_ = false;  // writes since last drained sync (io_mu_)
    std::mutex io_mu_;
    std::unique_ptr<VerbsClient> verbs_;  // non-null when the verbs fabric won

    struct Region {
        uintptr_t ptr;
        size_t size;
        bool device;
    };
    std::vector<Region> regions_;
    std::mutex region_mu_;

    // Cache of IPC exports keyed by exact data pointer (KV tensors are
    // long-lived and re-exported every request otherwise).
    struct IpcExport {
        uint8_t handle[64];
        uint64_t base_offset;
        uint64_t alloc_size = 0;
        bool have_handle;
    };
    std::unordered_map<uintptr_t, IpcExport> ipc_export_cache_;
    std::mutex ipc_mu_;

    std::thread worker_;
    std::deque<std::function<void()>> q_;
    std::mutex q_mu_;
    std::condition_variable q_cv_;
    std::condition_variable drain_cv_;
    std::atomic<int> inflight_{0};
    bool worker_stop_ = false;
    bool worker_started_ = false;
};

}  // namespace ifs
