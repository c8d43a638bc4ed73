#include "server.h"

#include "../core/crash.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <future>
#include <unistd.h>

#include "../core/log.h"

namespace ifs {

namespace {

// IFS_SERVER_DEBUG: per-request phase timing on stderr (docs/perf_notes.md).
// Read once, at the first request.
bool debug_on() {
    static const bool on = getenv("IFS_SERVER_DEBUG") != nullptr;
    return on;
}
using Clock = std::chrono::steady_clock;
double us(Clock::time_point a, Clock::time_point b) {
    return std::chrono::duration<double, std::micro>(b - a).count();
}

struct WriteReq {
    uv_write_t req;
    std::vector<uint8_t> data;
    std::shared_ptr<uint8_t[]> raw;  // alternative payload (uninitialized buf)
    size_t raw_len = 0;
};

void send_buf(Server::Conn* c, std::vector<uint8_t> data);

void conn_close(Server::Conn* c) {
    if (c->closed) return;
    c->closed = true;
    uv_close(c->handle(), [](uv_handle_t* h) {
        auto* c = static_cast<Server::Conn*>(h->data);
        c->unref();
    });
}

void send_status(Server::Conn* c, int code) {
    std::vector<uint8_t> v(4);
    memcpy(v.data(), &code, 4);
    send_buf(c, std::move(v));
}

void send_status_payload(Server::Conn* c, int code, const uint8_t* payload, size_t n) {
    std::vector<uint8_t> v(8 + n);
    uint32_t len = static_cast<uint32_t>(n);
    memcpy(v.data(), &code, 4);
    memcpy(v.data() + 4, &len, 4);
    if (n) memcpy(v.data() + 8, payload, n);
    send_buf(c, std::move(v));
}

// Reference-framed response: status + raw payload with NO length prefix
// (the reference's send_resp, infinistore.cpp:1055-1068 — its clients know
// each op's payload size a priori). Used by the query ops for byte-level
// wire compatibility.
void send_status_raw(Server::Conn* c, int code, const void* payload, size_t n) {
    std::vector<uint8_t> v(4 + n);
    memcpy(v.data(), &code, 4);
    if (n) memcpy(v.data() + 4, payload, n);
    send_buf(c, std::move(v));
}

void send_raw(Server::Conn* c, std::shared_ptr<uint8_t[]> buf, size_t len) {
    if (c->closed) return;
    auto* wr = new WriteReq();
    wr->raw = std::move(buf);
    wr->raw_len = len;
    wr->req.data = wr;
    uv_buf_t b = uv_buf_init(reinterpret_cast<char*>(wr->raw.get()),
                             static_cast<unsigned>(len));
    int r = uv_write(&wr->req, c->stream(), &b, 1,
                     [](uv_write_t* req, int status) {
                         auto* wr2 = static_cast<WriteReq*>(req->data);
                         delete wr2;
                         if (status < 0) DEBUG("uv_write status %d", status);
                     });
    if (r != 0) {
        delete wr;
        conn_close(c);
    }
}

void send_buf(Server::Conn* c, std::vector<uint8_t> data) {
    if (c->closed) return;
    auto* wr = new WriteReq();
    wr->data = std::move(data);
    wr->req.data = wr;
    uv_buf_t b = uv_buf_init(reinterpret_cast<char*>(wr->data.data()),
                             static_cast<unsigned>(wr->data.size()));
    int r = uv_write(&wr->req, c->stream(), &b, 1,
                     [](uv_write_t* req, int status) {
                         auto* wr = static_cast<WriteReq*>(req->data);
                         delete wr;
                         if (status < 0) DEBUG("uv_write status %d", status);
                     });
    if (r != 0) {
        delete wr;
        conn_close(c);
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// Server lifecycle
// ---------------------------------------------------------------------------
Server::Server(const ServerOptions& opt) : opt_(opt), index_(opt.ttl_seconds) {
    set_log_level(opt.log_level.c_str());
    if (opt_.devices.empty()) {
        for (int i = 0; i < std::max(1, opt_.cpu_shards); i++) {
            ShardOptions so;
            so.device = -1;
            so.pool_bytes = opt_.prealloc_bytes;
            so.block_granule = opt_.block_granule;
            so.auto_extend = opt_.auto_extend;
            so.extend_bytes = opt_.extend_bytes;
            shards_.emplace_back(new Shard(so));
        }
    } else {
        for (int dev : opt_.devices) {
            ShardOptions so;
            so.device = dev;
            so.pool_bytes = opt_.prealloc_bytes;
            so.block_granule = opt_.block_granule;
            so.n_streams = opt_.n_streams;
            so.auto_extend = opt_.auto_extend;
            so.extend_bytes = opt_.extend_bytes;
            shards_.emplace_back(new Shard(so));
        }
    }
}

Server::~Server() { stop(); }

bool Server::start() {
    if (running_.load()) return true;
    install_crash_handlers();
    for (auto& s : shards_) {
        if (!s->init()) {
            ERROR("shard init failed");
            return false;
        }
    }
    // Enable xGMI peer access between all shard devices up front (cross-GPU
    // reads/writes run the copy kernel on the pool device against peer VAs).
    if (gpu::available()) {
        int n = gpu::device_count();
        for (auto& s : shards_) {
            if (!s->on_gpu()) continue;
            for (int peer = 0; peer < n; peer++) {
                if (peer != s->device()) gpu::enable_peer_access(s->device(), peer);
            }
        }
    }

    // Bring up the main IO loop (listener) and the worker IO loops.
    main_io_.srv = this;
    main_io_.is_main = true;
    uv_loop_init(&main_io_.loop);
    uv_async_init(&main_io_.loop, &main_io_.post_async, &IoLoop::on_post);
    main_io_.post_async.data = &main_io_;
    uv_async_init(&main_io_.loop, &main_io_.stop_async, &IoLoop::on_stop);
    main_io_.stop_async.data = &main_io_;

    uv_tcp_init(&main_io_.loop, &listener_);
    listener_.data = this;
    struct sockaddr_in addr;
    uv_ip4_addr("0.0.0.0", opt_.service_port, &addr);
    int r = uv_tcp_bind(&listener_, reinterpret_cast<const struct sockaddr*>(&addr), 0);
    if (r == 0)
        r = uv_listen(reinterpret_cast<uv_stream_t*>(&listener_), 512,
                      &Server::on_new_connection);
    if (r != 0) {
        ERROR("bind/listen 0.0.0.0:%d failed: %s", opt_.service_port, uv_strerror(r));
        uv_close(reinterpret_cast<uv_handle_t*>(&listener_), nullptr);
        uv_close(reinterpret_cast<uv_handle_t*>(&main_io_.post_async), nullptr);
        uv_close(reinterpret_cast<uv_handle_t*>(&main_io_.stop_async), nullptr);
        uv_run(&main_io_.loop, UV_RUN_NOWAIT);
        uv_loop_close(&main_io_.loop);
        return false;
    }
    // Same-host fast transport: a Unix-domain listener next to the TCP one.
    pipe_path_ = "/tmp/infinistore-amd-" + std::to_string(opt_.service_port) + ".sock";
    unlink(pipe_path_.c_str());
    uv_pipe_init(&main_io_.loop, &pipe_listener_, 0);
    pipe_listener_.data = this;
    if (uv_pipe_bind(&pipe_listener_, pipe_path_.c_str()) == 0 &&
        uv_listen(reinterpret_cast<uv_stream_t*>(&pipe_listener_), 512,
                  &Server::on_new_pipe_connection) == 0) {
        pipe_listening_ = true;
    } else {
        WARN("UDS listener at %s unavailable; same-host clients use TCP",
             pipe_path_.c_str());
        uv_close(reinterpret_cast<uv_handle_t*>(&pipe_listener_), nullptr);
    }

    for (int i = 0; i < std::max(0, opt_.io_threads); i++) {
        auto w = std::make_unique<IoLoop>();
        w->srv = this;
        uv_loop_init(&w->loop);
        uv_async_init(&w->loop, &w->post_async, &IoLoop::on_post);
        w->post_async.data = w.get();
        uv_async_init(&w->loop, &w->stop_async, &IoLoop::on_stop);
        w->stop_async.data = w.get();
        workers_.push_back(std::move(w));
    }
    // Pre-size the index for the pool's block capacity: every block can
    // carry a key, and running the maps near their load limit means rehash
    // + tombstone-compaction cycles under the exclusive stripe locks (a
    // 64-client churn run measured 11 µs per lookup from probe-chain
    // growth). Capped at 16M slots (~1 GB of index).
    // IFS_KV_INITIAL (tests only) shrinks the initial capacity so rehash and
    // tombstone-compaction paths are exercised by small workloads.
    size_t pool_blocks = 0;
    for (auto& s : shards_) pool_blocks += s->total_blocks();
    size_t kv_initial = std::max<size_t>(1u << 20, pool_blocks + pool_blocks / 2);
    kv_initial = std::min<size_t>(kv_initial, 1u << 24);
    if (const char* env = getenv("IFS_KV_INITIAL")) kv_initial = strtoull(env, nullptr, 10);
    index_.reserve(kv_initial);
    running_.store(true);
    stop_requested_.store(false);
    // Fast-op workers (ring write/read handlers): enough to keep every HIP
    // stream fed under a 64-client burst without oversubscribing the box.
    {
        unsigned hw = std::thread::hardware_concurrency();
        unsigned n = std::min(24u, std::max(6u, hw / 8));
        if (const char* e = getenv("IFS_FAST_WORKERS")) {
            unsigned v = static_cast<unsigned>(strtoul(e, nullptr, 10));
            if (v >= 1 && v <= 128) n = v;
        }
        for (unsigned i = 0; i < n; i++)
            fast_workers_.emplace_back([this] { fast_worker_main(); });
    }
    main_io_.start();
    for (auto& w : workers_) w->start();
    if (opt_.ttl_seconds > 0) {
        ttl_thread_ = std::thread([this] {
            // Sweep every ttl/4 (>=1 s): one pass over the index erasing
            // expired idle entries. Lookups already treat expired
            // keys as absent; this just returns their memory early.
            auto period = std::chrono::seconds(std::max(1, opt_.ttl_seconds / 4));
            std::unique_lock<std::mutex> lk(ttl_mu_);
            while (!ttl_cv_.wait_for(lk, period,
                                     [this] { return stop_requested_.load(); })) {
                lk.unlock();
                size_t swept = index_.sweep_expired();
                if (swept) DEBUG("ttl sweep: %zu expired entries erased", swept);
                lk.lock();
            }
        });
    }
    INFO("server listening on 0.0.0.0:%d with %zu shard(s), %zu IO loops",
         opt_.service_port, shards_.size(), workers_.size() + 1);
    return true;
}

void Server::IoLoop::start() {
    thread = std::thread([this] {
        uv_run(&loop, UV_RUN_DEFAULT);
        uv_loop_close(&loop);
    });
}

void Server::stop() {
    if (!running_.load()) return;
    stop_requested_.store(true);
    ttl_cv_.notify_all();
    if (ttl_thread_.joinable()) ttl_thread_.join();
    for (auto& w : workers_) w->request_stop();
    main_io_.request_stop();
    for (auto& w : workers_)
        if (w->thread.joinable()) w->thread.join();
    if (main_io_.thread.joinable()) main_io_.thread.join();
    workers_.clear();
    // After the IO loops (and with them every ring poller) are joined no
    // new fast work can arrive; drain the queue, then join the workers.
    fast_cv_.notify_all();
    for (auto& t : fast_workers_)
        if (t.joinable()) t.join();
    fast_workers_.clear();
    {
        std::lock_guard<std::mutex> jl(extend_mu_);
        if (extend_thread_.joinable()) extend_thread_.join();
    }
    running_.store(false);
    // Drop all stored blocks.
    purge();
}

void Server::IoLoop::on_stop(uv_async_t* h) {
    auto* io = static_cast<IoLoop*>(h->data);
    // Close this loop's connections and handles; the loop exits when none
    // remain.
    for (auto* c : io->conns) {
        io->srv->verbs_teardown(c);
        io->srv->shm_teardown(c);
        conn_close(c);
    }
    io->conns.clear();
    if (io->is_main) {
        uv_close(reinterpret_cast<uv_handle_t*>(&io->srv->listener_), nullptr);
        if (io->srv->pipe_listening_) {
            uv_close(reinterpret_cast<uv_handle_t*>(&io->srv->pipe_listener_), nullptr);
            unlink(io->srv->pipe_path_.c_str());
            io->srv->pipe_listening_ = false;
        }
    }
    uv_close(reinterpret_cast<uv_handle_t*>(&io->post_async), nullptr);
    uv_close(reinterpret_cast<uv_handle_t*>(&io->stop_async), nullptr);
}

void Server::IoLoop::post(std::function<void()> fn) {
    // After stop is requested the async handles are being closed; drop the
    // callback (captured refs release on destruction) instead of touching a
    // dying handle.
    if (srv && srv->stop_requested_.load(std::memory_order_acquire)) return;
    {
        std::lock_guard<std::mutex> lk(post_mu);
        posted.push_back(std::move(fn));
    }
    uv_async_send(&post_async);
}

void Server::IoLoop::on_post(uv_async_t* h) {
    auto* io = static_cast<IoLoop*>(h->data);
    std::vector<std::function<void()>> fns;
    {
        std::lock_guard<std::mutex> lk(io->post_mu);
        fns.swap(io->posted);
    }
    for (auto& f : fns) f();
}

// ---------------------------------------------------------------------------
// Accept + read state machine
// ---------------------------------------------------------------------------
void Server::on_new_connection(uv_stream_t* server, int status) {
    auto* srv = static_cast<Server*>(server->data);
    if (status < 0) {
        WARN("accept error: %s", uv_strerror(status));
        return;
    }
    // Accept on the main loop, then hand the fd to a worker loop (round
    // robin) so request handling scales across IO threads.
    uv_tcp_t* tmp = new uv_tcp_t();
    uv_tcp_init(&srv->main_io_.loop, tmp);
    tmp->data = nullptr;
    if (uv_accept(server, reinterpret_cast<uv_stream_t*>(tmp)) != 0) {
        uv_close(reinterpret_cast<uv_handle_t*>(tmp),
                 [](uv_handle_t* h) { delete reinterpret_cast<uv_tcp_t*>(h); });
        return;
    }
    uv_os_fd_t fd;
    if (uv_fileno(reinterpret_cast<uv_handle_t*>(tmp), &fd) != 0) {
        uv_close(reinterpret_cast<uv_handle_t*>(tmp),
                 [](uv_handle_t* h) { delete reinterpret_cast<uv_tcp_t*>(h); });
        return;
    }
    int fd2 = dup(fd);
    uv_close(reinterpret_cast<uv_handle_t*>(tmp),
             [](uv_handle_t* h) { delete reinterpret_cast<uv_tcp_t*>(h); });
    IoLoop* io = &srv->main_io_;
    if (!srv->workers_.empty()) {
        uint32_t i = srv->next_worker_.fetch_add(1) %
                     static_cast<uint32_t>(srv->workers_.size());
        io = srv->workers_[i].get();
    }
    if (io == &srv->main_io_)
        srv->adopt_fd(io, fd2, false);
    else
        io->post([srv, io, fd2] { srv->adopt_fd(io, fd2, false); });
}

void Server::on_new_pipe_connection(uv_stream_t* server, int status) {
    auto* srv = static_cast<Server*>(server->data);
    if (status < 0) return;
    uv_pipe_t* tmp = new uv_pipe_t();
    uv_pipe_init(&srv->main_io_.loop, tmp, 0);
    tmp->data = nullptr;
    auto close_tmp = [](uv_handle_t* h) { delete reinterpret_cast<uv_pipe_t*>(h); };
    if (uv_accept(server, reinterpret_cast<uv_stream_t*>(tmp)) != 0) {
        uv_close(reinterpret_cast<uv_handle_t*>(tmp), close_tmp);
        return;
    }
    uv_os_fd_t fd;
    if (uv_fileno(reinterpret_cast<uv_handle_t*>(tmp), &fd) != 0) {
        uv_close(reinterpret_cast<uv_handle_t*>(tmp), close_tmp);
        return;
    }
    int fd2 = dup(fd);
    uv_close(reinterpret_cast<uv_handle_t*>(tmp), close_tmp);
    IoLoop* io = &srv->main_io_;
    if (!srv->workers_.empty()) {
        uint32_t i = srv->next_worker_.fetch_add(1) %
                     static_cast<uint32_t>(srv->workers_.size());
        io = srv->workers_[i].get();
    }
    if (io == &srv->main_io_)
        srv->adopt_fd(io, fd2, true);
    else
        io->post([srv, io, fd2] { srv->adopt_fd(io, fd2, true); });
}

void Server::adopt_fd(IoLoop* io, int fd, bool is_pipe) {
    if (stop_requested_.load()) {
        ::close(fd);
        return;
    }
    int bufsz = 4 << 20;  // bulk fabric payloads ride this socket
    setsockopt(fd, SOL_SOCKET, SO_SNDBUF, &bufsz, sizeof(bufsz));
    setsockopt(fd, SOL_SOCKET, SO_RCVBUF, &bufsz, sizeof(bufsz));
    auto* c = new Conn();
    c->srv = this;
    c->owner = io;
    c->is_pipe = is_pipe;
    if (is_pipe) {
        uv_pipe_init(&io->loop, &c->pipe, 0);
        c->pipe.data = c;
        if (uv_pipe_open(&c->pipe, fd) != 0) {
            conn_close(c);
            return;
        }
    } else {
        uv_tcp_init(&io->loop, &c->tcp);
        c->tcp.data = c;
        if (uv_tcp_open(&c->tcp, fd) != 0) {
            conn_close(c);
            return;
        }
        uv_tcp_nodelay(&c->tcp, 1);
    }
    io->conns.push_back(c);
    uv_read_start(
        c->stream(),
        [](uv_handle_t*, size_t suggested, uv_buf_t* buf) {
            buf->base = static_cast<char*>(malloc(suggested));
            buf->len = suggested;
        },
        [](uv_stream_t* stream, ssize_t nread, const uv_buf_t* buf) {
            auto* c = static_cast<Conn*>(stream->data);
            Server* srv = c->srv;
            if (nread < 0) {
                free(buf->base);
                auto& v = c->owner->conns;
                v.erase(std::remove(v.begin(), v.end(), c), v.end());
                srv->verbs_teardown(c);
                srv->shm_teardown(c);
                conn_close(c);
                return;
            }
            if (nread == 0) {
                free(buf->base);
                return;
            }
            c->buf.insert(c->buf.end(), reinterpret_cast<uint8_t*>(buf->base),
                          reinterpret_cast<uint8_t*>(buf->base) + nread);
            free(buf->base);
            // Drain as many complete requests as are buffered.
            size_t consumed = 0;
            for (;;) {
                if (c->state == Conn::kHeader) {
                    if (c->buf.size() - consumed < sizeof(Header)) break;
                    memcpy(&c->hdr, c->buf.data() + consumed, sizeof(Header));
                    consumed += sizeof(Header);
                    if (c->hdr.magic != kMagic) {
                        WARN("bad magic from client; closing");
                        auto& v = c->owner->conns;
                        v.erase(std::remove(v.begin(), v.end(), c), v.end());
                        srv->verbs_teardown(c);
                        srv->shm_teardown(c);
                        conn_close(c);
                        return;
                    }
                    size_t cap = (c->hdr.op == OP_TCP_PUT) ? (256u << 20) : kProtocolBufferSize;
                    if (c->hdr.body_size > cap) {
                        WARN("body too large (%u) for op %c", c->hdr.body_size, c->hdr.op);
                        auto& v = c->owner->conns;
                        v.erase(std::remove(v.begin(), v.end(), c), v.end());
                        srv->verbs_teardown(c);
                        srv->shm_teardown(c);
                        conn_close(c);
                        return;
                    }
                    c->state = Conn::kBody;
                }
                if (c->state == Conn::kBody) {
                    if (c->buf.size() - consumed < c->hdr.body_size) break;
                    std::vector<uint8_t> body(c->buf.data() + consumed,
                                              c->buf.data() + consumed + c->hdr.body_size);
                    consumed += c->hdr.body_size;
                    c->state = Conn::kHeader;
                    srv->handle_request(c, c->hdr.op, std::move(body));
                    if (c->closed) return;
                }
            }
            if (consumed) c->buf.erase(c->buf.begin(), c->buf.begin() + consumed);
        });
}

// ---------------------------------------------------------------------------
// Dispatch
// ---------------------------------------------------------------------------
namespace {

// View over the flatbuffers LocalMetaRequest (msg must outlive the view).
Server::LocalView to_view(const LocalMetaMsg& msg) {
    Server::LocalView v;
    v.device = msg.device;
    v.pid = msg.pid;
    v.base_ptr = msg.base_ptr;
    v.base_offset = msg.base_offset;
    v.block_size = msg.block_size;
    v.ipc = msg.ipc_handle.data();
    v.ipc_len = msg.ipc_handle.size();
    v.blocks.reserve(msg.blocks.size());
    for (auto& b : msg.blocks) v.blocks.push_back({std::string_view(b.key), b.offset});
    return v;
}

// Packed fast-path body (framing and its refusals: core/protocol.h).
bool parse_packed_local(char op, const uint8_t* body, size_t body_len, Server::LocalView* v) {
    PackedLocalReq req;
    if (!ifs::parse_packed_local(op, body, body_len, &req)) return false;
    const PackedLocalHdr& h = req.hdr;
    v->device = h.device;
    v->pid = h.pid;
    v->base_ptr = h.base_ptr;
    v->base_offset = h.base_offset;
    v->block_size = h.block_size;
    v->flags = h.flags;
    v->alloc_mb = h.rsvd;
    v->n_segments = req.n_segments;
    v->segment_stride = req.segment_stride;
    v->slice = slice_from_wire(req.slice);
    v->has_tset = req.has_tset;
    v->tset_id = req.tset.set_id;
    v->tset_n = req.tset.n_tensors;
    v->ipc = body + offsetof(PackedLocalHdr, ipc);
    v->ipc_len = 64;
    v->blocks = std::move(req.blocks);
    return true;
}

}  // namespace

void Server::handle_request(Conn* c, char op, std::vector<uint8_t> body) {
    DEBUG("request op=%s body=%zu", op_name(op).c_str(), body.size());
    struct Timer {
        Server* s;
        char op;
        std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        ~Timer() {
            auto us = std::chrono::duration_cast<std::chrono::microseconds>(
                          std::chrono::steady_clock::now() - t0)
                          .count();
            auto& st = s->op_stats_[static_cast<uint8_t>(op) & 127];
            st.count.fetch_add(1, std::memory_order_relaxed);
            st.total_us.fetch_add(static_cast<uint64_t>(us), std::memory_order_relaxed);
            uint64_t prev = st.max_us.load(std::memory_order_relaxed);
            while (static_cast<uint64_t>(us) > prev &&
                   !st.max_us.compare_exchange_weak(prev, static_cast<uint64_t>(us))) {
            }
        }
    } timer{this, op};
    switch (op) {
        case OP_W: {
            LocalMetaMsg msg;
            if (!parse_local_meta(body.data(), body.size(), &msg)) return send_status(c, INVALID_REQ);
            return op_local_write(c, to_view(msg), ReqCtx{});
        }
        case OP_R: {
            LocalMetaMsg msg;
            if (!parse_local_meta(body.data(), body.size(), &msg)) return send_status(c, INVALID_REQ);
            return op_local_read(c, to_view(msg), ReqCtx{});
        }
        case OP_W_FAST: {
            LocalView v;
            if (!parse_packed_local(op, body.data(), body.size(), &v))
                return send_status(c, INVALID_REQ);
            return op_local_write(c, v, ReqCtx{});
        }
        case OP_R_FAST: {
            LocalView v;
            if (!parse_packed_local(op, body.data(), body.size(), &v))
                return send_status(c, INVALID_REQ);
            return op_local_read(c, v, ReqCtx{});
        }
        case OP_SYNC:
            return op_sync(c, ReqCtx{});
        case OP_SHM_SETUP:
            return op_shm_setup(c, body);
        case OP_TSET_REGISTER:
            return op_tset_register(c, body);
        case OP_TSET_RELEASE:
            return op_tset_release(c, body);
        case OP_RDMA_EXCHANGE:
            return op_exchange(c, body);
        case OP_RDMA_ALLOCATE: {
            RemoteMetaMsg msg;
            if (!parse_remote_meta(body.data(), body.size(), &msg))
                return send_status(c, INVALID_REQ);
            return op_allocate(c, msg);
        }
        case OP_TCP_PUT:
            return op_tcp_put(c, std::move(body));
        case OP_TCP_GET: {
            RemoteMetaMsg msg;
            if (!parse_remote_meta(body.data(), body.size(), &msg))
                return send_status(c, INVALID_REQ);
            return op_tcp_get(c, msg);
        }
        case OP_RDMA_WRITE_COMMIT: {
            RemoteMetaMsg msg;
            if (!parse_remote_meta(body.data(), body.size(), &msg))
                return send_status(c, INVALID_REQ);
            return op_commit(c, msg);
        }
        case OP_CHECK_EXIST:
            return op_check_exist(c, body, ReqCtx{});
        case OP_GET_MATCH_LAST_IDX:
            return op_match_index(c, body, ReqCtx{});
        case OP_DELETE:
            return op_delete(c, body, ReqCtx{});
        case OP_STATS: {
            std::string js = stats_json();
            return send_status_payload(c, FINISH,
                                       reinterpret_cast<const uint8_t*>(js.data()), js.size());
        }
        default:
            WARN("unknown op '%c'", op);
            return send_status(c, INVALID_REQ);
    }
}

Shard* Server::shard_for_device(int device) {
    for (auto& s : shards_)
        if (s->device() == device) return s.get();
    return shards_[static_cast<size_t>(device < 0 ? 0 : device) % shards_.size()].get();
}

Shard* Server::shard_least_used() {
    Shard* best = shards_[0].get();
    size_t best_used = SIZE_MAX;
    for (auto& s : shards_) {
        size_t used = s->used_blocks();
        if (used < best_used) {
            best_used = used;
            best = s.get();
        }
    }
    return best;
}

void Server::maybe_extend(Shard* s) {
    if (!s->need_extend()) return;
    int expect = 0;
    if (!extending_.compare_exchange_strong(expect, 1)) return;
    // Managed (not detached): a detached extender could still be unlocking
    // vdrv_mu_ while ~Server destroys it (TSAN-caught shutdown race).
    std::lock_guard<std::mutex> jl(extend_mu_);
    if (extend_thread_.joinable()) extend_thread_.join();  // prior run done
    extend_thread_ = std::thread([this, s] {
        INFO("extending pool on shard dev=%d", s->device());
        void* arena = nullptr;
        if (s->extend(&arena) && arena) {
            // Verbs fabric live: the new arena must carry an MR or verbs
            // reads from it fail ("pool arena not registered"); the reference
            // registers an MR per pool at pool creation (mempool.cpp:29-44).
            std::lock_guard<std::mutex> lk(vdrv_mu_);
            if (vdrv_ && !vdrv_->reg_region(arena, opt_.extend_bytes, s->on_gpu(), nullptr))
                ERROR("MR registration of extended arena failed; verbs reads from it will error");
        }
        extending_.store(0);
    });
}

// ---- local (IPC) path -----------------------------------------------------
namespace {
// Resolve the client's allocation base: same-process fast path (an IPC
// handle cannot be opened inside the exporting process) or the per-conn
// cached hipIpcOpenMemHandle mapping.
//
// open_mapping_locked is the cached part, shared with tensor-set registration
// (c->ipc_mu held): each distinct handle is opened once per connection.
void* open_mapping_locked(Server::Conn* c, const uint8_t* ipc, int device) {
    std::vector<uint8_t> key(ipc, ipc + gpu::kIpcHandleSize);
    auto it = c->ipc_cache.find(key);
    if (it != c->ipc_cache.end()) return it->second.first;
    // Bound the cache: a client that churns tensors would otherwise pin
    // every old allocation via its stale mapping. Only flush when nothing
    // is in flight (a mapping may be read by a queued kernel). Mappings that
    // a live tensor set uses are neither counted nor closed.
    if (c->ipc_cache.size() >= 64 + c->ipc_set_refs.size() && c->remain.load() == 0 &&
        c->fabric_inflight.load() == 0 && c->ipc_pin.load() == 1) {
        for (auto kv = c->ipc_cache.begin(); kv != c->ipc_cache.end();) {
            if (c->ipc_set_refs.count(kv->second.first)) {
                ++kv;
                continue;
            }
            gpu::ipc_close(kv->second.first);
            kv = c->ipc_cache.erase(kv);
        }
    }
    gpu::IpcHandle h;
    memcpy(h.bytes, ipc, gpu::kIpcHandleSize);
    void* base = gpu::ipc_open(h, device);
    if (base) c->ipc_cache.emplace(std::move(key), std::make_pair(base, device));
    return base;
}

// dmabuf IPC limitation on this ROCm/driver stack: hipIpcOpenMemHandle
// HANGS FOREVER importing allocations >= 2 GiB (bisected by
// scripts/ipc_size_probe.py: 1.5 GiB fine, 2.0 GiB hangs). Refuse
// instead of wedging this conn's poller/worker thread. Clients see a
// clear error and can split tensors (< 2 GiB per allocation, e.g.
// per-layer KV pools) or use the fabric path for the big tensor.
bool import_size_ok(uint32_t alloc_mb) {
    if (alloc_mb < 2048) return true;
    ERROR("refusing IPC import of a %u MB client allocation: "
          "hipIpcOpenMemHandle hangs for >= 2 GiB allocations under "
          "dmabuf IPC; split the tensor or use the fabric path",
          alloc_mb);
    return false;
}

void* resolve_client_base(Server::Conn* c, const Server::LocalView& msg) {
    if (msg.pid != 0 && msg.pid == static_cast<int32_t>(getpid()) && msg.base_ptr != 0)
        return reinterpret_cast<void*>(msg.base_ptr);
    if (!import_size_ok(msg.alloc_mb)) return nullptr;
    std::lock_guard<std::mutex> lk(c->ipc_mu);
    return open_mapping_locked(c, msg.ipc, msg.device);
}

// The registered set a request names, or null (INVALID_REQ) for an unknown or
// released id or a tensor count that is not the registered one.
std::shared_ptr<const Server::Conn::TensorSet> find_tensor_set(Server::Conn* c,
                                                               const Server::LocalView& msg) {
    std::lock_guard<std::mutex> lk(c->ipc_mu);
    auto it = c->tsets.find(msg.tset_id);
    if (it == c->tsets.end() || it->second->bases->size() != msg.tset_n ||
        it->second->device != msg.device)
        return nullptr;
    return it->second;
}

// What a request over a tensor set must satisfy beyond the parser's checks:
// the geometry under `codec`, every page part inside the smallest tensor's
// registered extent, and for a transforming codec aligned bases and offsets.
bool tensor_set_request_ok(const Server::Conn::TensorSet& ts, const Server::LocalView& msg,
                           PageCodec codec) {
    const size_t page = static_cast<size_t>(msg.block_size);
    if (!tensors_legal(codec, page, msg.n_segments, msg.segment_stride, ts.bases->size()))
        return false;
    const uint64_t per = msg.n_segments / ts.bases->size();
    const uint64_t seg = page / msg.n_segments;
    // last byte of a part: offs + (per - 1) * stride + seg, without overflow
    uint64_t span = seg;
    if (per > 1) {
        if (msg.segment_stride > (UINT64_MAX - seg) / (per - 1)) return false;
        span += (per - 1) * msg.segment_stride;
    }
    if (span > ts.min_extent) return false;
    const bool transforms = page_codec_transforms(codec);
    if (transforms && !ts.bases16) return false;
    for (auto& b : msg.blocks) {
        if (b.second > ts.min_extent - span) return false;
        if (transforms && b.second % 16 != 0) return false;
    }
    return true;
}

// Holds Conn::ipc_pin for a handler's resolve→enqueue window so a concurrent
// handler on the other transport cannot flush (ipc_close) a base this one
// resolved but has not yet protected with remain/fabric_inflight.
struct IpcPinGuard {
    Server::Conn* c;
    explicit IpcPinGuard(Server::Conn* conn) : c(conn) { c->ipc_pin.fetch_add(1); }
    ~IpcPinGuard() { c->ipc_pin.fetch_sub(1); }
};
}  // namespace

void Server::op_local_write(Conn* c, const LocalView& msg, const ReqCtx& ctx) {
    const bool dbg = debug_on();
    auto p0 = Clock::now();
    if (!gpu::available()) return reply_local(c, ctx, SYSTEM_ERROR);
    if (msg.ipc_len != gpu::kIpcHandleSize || msg.block_size <= 0)
        return reply_local(c, ctx, INVALID_REQ);
    IpcPinGuard pin(c);
    // Over a tensor set the block offsets are the client descriptors
    // themselves (relative to every tensor's base): there is no single base.
    std::shared_ptr<const Conn::TensorSet> tset;
    uint8_t* client_ptr = nullptr;
    if (msg.has_tset) {
        tset = find_tensor_set(c, msg);
        if (!tset) return reply_local(c, ctx, INVALID_REQ);
    } else {
        void* base = resolve_client_base(c, msg);
        if (!base) return reply_local(c, ctx, INTERNAL_ERROR);
        client_ptr = static_cast<uint8_t*>(base) + msg.base_offset;
    }
    const uintptr_t client_addr = reinterpret_cast<uintptr_t>(client_ptr);

    Shard* shard = shard_for_device(msg.device);
    size_t page = static_cast<size_t>(msg.block_size);
    size_t nb = msg.blocks.size();
    // Ingest compression (extension): the flags pick the stored format, and
    // its page-size rule and stored size come from core/page_codec.h.
    PageCodec codec;
    if (!page_codec_from_flags(msg.flags, &codec)) return reply_local(c, ctx, INVALID_REQ);
    if (!page_legal(codec, page)) return reply_local(c, ctx, INVALID_REQ);
    // Segmented source pages: the geometry rules, the stride's alignment for
    // transforming codecs among them, are segments_legal's.
    if (tset) {
        // tensors_legal, every part inside its tensor, aligned bases and
        // offsets for a transforming codec.
        if (!tensor_set_request_ok(*tset, msg, codec)) return reply_local(c, ctx, INVALID_REQ);
    } else if (!segments_legal(codec, page, msg.n_segments, msg.segment_stride)) {
        return reply_local(c, ctx, INVALID_REQ);
    }
    // The quantize kernels load 16 bytes per lane: every source page must
    // start 16-byte aligned (pool blocks always do), and a 16-byte stride
    // then keeps every segment aligned.
    if (page_codec_transforms(codec) && !tset) {
        for (size_t i = 0; i < nb; i++)
            if ((client_addr + msg.blocks[i].second) % 16 != 0)
                return reply_local(c, ctx, INVALID_REQ);
    }
    const size_t stored = stored_bytes(codec, page);

    // Phase A — dedup check only (shared stripe locks, prefetch-pipelined).
    // The authoritative first-write-wins decision happens at the insert pass
    // (phase D); a key that appears between A and D just wastes one block
    // copy whose memory is released after the kernel completes.
    // An empty request sweeps nothing and replies like an all-duplicates one.
    std::vector<uint64_t> hashes(nb);
    for (size_t i = 0; i < nb; i++) hashes[i] = KvIndex::hash_of(msg.blocks[i].first);
    std::vector<uint32_t> fresh;
    fresh.reserve(nb);
    KvIndex::SweepTimes ta, td;  // lock-wait vs under-lock (dbg)
    index_.for_each_batched<KvIndex::Lock::kShared>(
        nb, hashes.data(), KvIndex::rotated_start(hashes.data(), nb),
        [&](KvMap& m, size_t i) {
            if (!index_.find_live(m, msg.blocks[i].first, hashes[i]))
                fresh.push_back(static_cast<uint32_t>(i));
            return true;
        },
        dbg ? &ta : nullptr);
    if (dbg && nb > 64)
        fprintf(stderr, "[pdbg2] dedup lockwait=%.0f underlock=%.0f\n", ta.lock_wait_us,
                ta.under_lock_us);
    auto p1 = Clock::now();

    n_writes_.fetch_add(1);
    size_t n_fresh = fresh.size();
    bytes_in_.fetch_add(n_fresh * page);
    bool sync_resp = (msg.flags & kLocalFlagSyncResponse) != 0;
    if (n_fresh == 0) {
        // everything was a duplicate — nothing to copy
        if (ctx.shm && !sync_resp) return;  // ring async writes are unacked
        return reply_local(c, ctx, sync_resp ? FINISH : TASK_ACCEPTED);
    }

    // Phase B — batched allocation (shard allocator lock only).
    std::vector<std::pair<void*, int>> slots;
    slots.reserve(n_fresh);
    auto try_alloc = [&] {
        slots.clear();
        return shard->allocate(stored, n_fresh,
                               [&](void* p, int idx) { slots.push_back({p, idx}); });
    };
    bool alloc_ok = try_alloc();
    // Retry loop: with concurrent writers a single evict+retry can lose its
    // freed blocks to a racing allocation; keep evicting until the
    // allocation lands or eviction runs dry.
    for (int attempt = 0; !alloc_ok && opt_.auto_evict && attempt < 4; attempt++) {
        if (index_.evict_lru(shard, page * n_fresh * 2) == 0) break;
        alloc_ok = try_alloc();
    }
    if (!alloc_ok) return reply_local(c, ctx, OUT_OF_MEMORY);
    auto p2 = Clock::now();

    // Phase C — create entries, build the copy job and LAUNCH it; the index
    // insert pass (D) then runs while the kernel is in flight.
    uint64_t t = index_.tick();
    SlabBatch slab_batch(n_fresh);
    auto entries = std::make_shared<std::vector<Ref<BlockEntry>>>();
    entries->reserve(n_fresh);
    Shard::CopyJob job;
    job.bytes_per_block = page;
    job.src.reserve(n_fresh);
    job.dst.reserve(n_fresh);
    auto scales_out = page_codec_info(codec).page_scale
                          ? std::make_shared<std::vector<float>>(n_fresh, 1.f)
                          : nullptr;
    job.codec = codec;
    job.dir = PageDir::kStore;
    job.n_segments = msg.n_segments;
    job.segment_stride = msg.segment_stride;
    if (tset) {
        job.tensor_bases = tset->bases;
        job.segs_per_tensor = msg.n_segments / static_cast<uint32_t>(tset->bases->size());
    }
    job.scales = scales_out;
    for (size_t i = 0; i < n_fresh; i++) {
        auto* e = slab_batch.make();
        e->ptr = slots[i].first;
        e->size = stored;
        e->pool_idx = slots[i].second;
        e->shard = shard;
        e->committed = false;
        e->codec = codec;
        e->born_sec = KvIndex::now_sec();
        e->last_access.store(t, std::memory_order_relaxed);
        entries->emplace_back(e);
        job.src.push_back(client_addr + msg.blocks[fresh[i]].second);
        job.dst.push_back(reinterpret_cast<uint64_t>(slots[i].first));
    }
    maybe_extend(shard);

    c->remain.fetch_add(1);
    c->ref();
    auto t_start = Clock::now();
    // won[i] is written in phase D after the kernel is submitted. The commit
    // must see phase D's result, so it runs on whichever side finishes LAST:
    // both the copy-done callback and the end of phase D bump `arrivals`,
    // and the second arriver performs the commit + reply. Round 1 used a
    // mutex held across submit + phase D instead, which made completion
    // threads BLOCK on handlers that were themselves waiting for copy
    // slots — the only slot-freers waiting on slot-waiters (measured 94 ms
    // slot waits at 64 saturation clients).
    auto won = std::make_shared<std::vector<uint8_t>>(n_fresh, 0);
    auto copy_ok = std::make_shared<std::atomic<bool>>(false);
    auto arrivals = std::make_shared<std::atomic<int>>(0);
    auto fin = [this, c, entries, won, sync_resp, ctx, scales_out, copy_ok] {
        bool ok = copy_ok->load(std::memory_order_acquire);
        if (ok) {
            for (size_t i = 0; i < entries->size(); i++)
                if ((*won)[i]) {
                    if (scales_out) (*entries)[i]->scale = (*scales_out)[i];
                    (*entries)[i]->committed = true;
                }
        } else {
            // Copy failed: drop the keys. Always from the owner loop, never
            // a completion thread (kv_index.h invariants): erase_entries is
            // an O(index) scan under exclusive stripe locks.
            c->ref();
            c->owner->post([this, c, entries, won] {
                std::vector<Ref<BlockEntry>> winners;
                for (size_t i = 0; i < entries->size(); i++)
                    if ((*won)[i]) winners.push_back((*entries)[i]);
                index_.erase_entries(winners);
                c->unref();
            });
        }
        if (sync_resp) reply_local(c, ctx, ok ? FINISH : INTERNAL_ERROR);
        finish_task(c, /*on_owner=*/!ctx.shm);
    };
    job.done = [this, c, entries, fin, ctx, copy_ok, arrivals, t_start, dbg](bool ok) {
        if (dbg && entries->size() > 64)
            fprintf(stderr, "[sdbg] write n=%zu submit->complete=%.0fus\n", entries->size(),
                    us(t_start, Clock::now()));
        copy_ok->store(ok, std::memory_order_release);
        if (ctx.shm) {
            // Never block the completion thread: if phase D has not ended,
            // its own arrival runs fin.
            if (arrivals->fetch_add(1, std::memory_order_acq_rel) == 1) fin();
        } else {
            // Socket path: both arrivals happen on the owner loop thread
            // (this post + the handler itself), preserving reply ordering.
            c->owner->post([fin, arrivals] {
                if (arrivals->fetch_add(1, std::memory_order_acq_rel) == 1) fin();
            });
        }
    };
    // Async write: respond before submitting so the client's next request
    // overlaps the kernel. Sync-response write (flags&1): one round trip,
    // response sent on completion instead. Ring async writes are unacked.
    if (!sync_resp && !ctx.shm) send_status(c, TASK_ACCEPTED);
    bool submitted = shard->submit_copy(std::move(job));
    auto p2b = Clock::now();

    // Phase D — insert pass, overlapped with the in-flight kernel. Losers
    // (a racing writer inserted the key first) keep their block alive until
    // the copy completes, then release it; they are never committed.
    {
        std::vector<uint64_t> fresh_hashes(n_fresh);
        for (size_t p = 0; p < n_fresh; p++) fresh_hashes[p] = hashes[fresh[p]];
        std::vector<Ref<BlockEntry>> displaced;  // expired entries; dropped after the sweep
        index_.for_each_batched<KvIndex::Lock::kExclusive>(
            n_fresh, fresh_hashes.data(), KvIndex::rotated_start(fresh_hashes.data(), n_fresh),
            [&](KvMap& m, size_t p) {
                (*won)[p] = index_.insert_locked(m, msg.blocks[fresh[p]].first, fresh_hashes[p],
                                                 (*entries)[p], /*replace_expired=*/true,
                                                 &displaced);
                return true;
            },
            dbg ? &td : nullptr);
        if (dbg && n_fresh > 64)
            fprintf(stderr, "[pdbg2] insert lockwait=%.0f underlock=%.0f\n", td.lock_wait_us,
                    td.under_lock_us);
    }
    // Phase D done: second arriver commits (the copy may already be done).
    if (submitted && arrivals->fetch_add(1, std::memory_order_acq_rel) == 1) fin();
    auto p3 = Clock::now();
    if (dbg && n_fresh > 64)
        fprintf(stderr, "[pdbg] dedup=%.0f alloc=%.0f submit=%.0f insert=%.0f\n", us(p0, p1),
                us(p1, p2), us(p2, p2b), us(p2b, p3));
    if (!submitted) {
        // The job never launched (e.g. a transform on a CPU shard): the done
        // callback will not fire, so answer sync-response writers here.
        if (sync_resp) reply_local(c, ctx, INTERNAL_ERROR);
        finish_task(c, /*on_owner=*/!ctx.shm);
    }
}

void Server::op_local_read(Conn* c, const LocalView& msg, const ReqCtx& ctx) {
    if (!gpu::available()) return reply_local(c, ctx, SYSTEM_ERROR);
    if (msg.ipc_len != gpu::kIpcHandleSize || msg.block_size <= 0)
        return reply_local(c, ctx, INVALID_REQ);
    IpcPinGuard pin(c);
    // Over a tensor set the block offsets are the client descriptors
    // themselves, as in op_local_write.
    std::shared_ptr<const Conn::TensorSet> tset;
    uint8_t* client_ptr = nullptr;
    if (msg.has_tset) {
        tset = find_tensor_set(c, msg);
        if (!tset || slice_is_set(msg.slice)) return reply_local(c, ctx, INVALID_REQ);
    } else {
        void* base = resolve_client_base(c, msg);
        if (!base) return reply_local(c, ctx, INTERNAL_ERROR);
        client_ptr = static_cast<uint8_t*>(base) + msg.base_offset;
    }
    const uintptr_t client_addr = reinterpret_cast<uintptr_t>(client_ptr);
    size_t page = static_cast<size_t>(msg.block_size);
    // Segmented destination pages. Plain rules here; a compressed entry is
    // checked against its own codec's rules in the sweep, next to
    // stored_matches.
    if (tset) {
        if (!tensor_set_request_ok(*tset, msg, PageCodec::kNone))
            return reply_local(c, ctx, INVALID_REQ);
    } else if (!segments_legal(PageCodec::kNone, page, msg.n_segments, msg.segment_stride)) {
        return reply_local(c, ctx, INVALID_REQ);
    }
    // A request sees entries of at most a few codecs: each is checked once.
    bool tset_codec_ok[kNumPageCodecs] = {true};
    bool tset_codec_seen[kNumPageCodecs] = {true};
    // Sliced read: `page` is the sliced page (what the client receives); the
    // stored pages are slice.page_bytes. Plain rules here too, as in the
    // parser; the sweep checks every entry against its own codec.
    const bool sliced = slice_is_set(msg.slice);
    const PageSegments client_seg{msg.n_segments, msg.segment_stride};
    if (sliced && (!slice_legal(PageCodec::kNone, msg.slice, client_seg) ||
                   page != msg.slice.n * msg.slice.piece_bytes))
        return reply_local(c, ctx, INVALID_REQ);

    auto tr0 = Clock::now();
    // Group blocks by the shard whose GPU EXECUTES the copy. For same-GPU
    // hits that is trivially the owner. For cross-shard hits the choice is
    // deliberate: default OWNER-side (push) — the owner's
    // kernel reads its local HBM and writes the reader's memory over xGMI.
    // xGMI writes are posted (fire-and-forget per link), while remote reads
    // are request/response round trips; and since a multi-shard read groups
    // per owner, N owners push concurrently over N distinct xGMI links into
    // the reader (each GPU has 7 links x ~153 GB/s — per-link bound, so the
    // aggregate scales with the number of pushing GPUs, up to ~1 TB/s into
    // one reader). Reader-side execution (pull) would serialize the same
    // traffic through one GPU's remote-read path and its own CUs.
    // IFS_CROSS_COPY=reader flips to pull for topologies where the owner
    // GPUs are compute-saturated; it requires a shard on the reader's GPU.
    // Compressed entries go into separate dequantizing jobs, one per
    // (executing shard, codec), so one read may mix plain, fp8 and mxfp4 keys.
    static const bool cross_pull = [] {
        const char* v = getenv("IFS_CROSS_COPY");
        return v && std::string(v) == "reader";
    }();
    Shard* reader_shard = nullptr;
    if (cross_pull) {
        Shard* s = shard_for_device(msg.device);
        if (s->device() == msg.device) reader_shard = s;
    }
    auto exec_shard = [&](Shard* owner) {
        return (reader_shard && owner->device() != msg.device) ? reader_shard : owner;
    };
    std::map<std::pair<Shard*, PageCodec>, Shard::CopyJob> jobs;
    std::pair<Shard*, PageCodec> last_key;
    Shard::CopyJob* last_job = nullptr;  // map nodes do not move
    auto held = std::make_shared<std::vector<Ref<BlockEntry>>>();
    held->reserve(msg.blocks.size());
    uint64_t read_tick = index_.tick();
    std::vector<uint64_t> hashes(msg.blocks.size());
    for (size_t i = 0; i < hashes.size(); i++) hashes[i] = KvIndex::hash_of(msg.blocks[i].first);
    int err = 0;  // first failing key ends the sweep
    index_.for_each_batched<KvIndex::Lock::kShared>(
        hashes.size(), hashes.data(), 0, [&](KvMap& m, size_t i) {
            auto& b = msg.blocks[i];
            Ref<BlockEntry>* v = index_.find_live(m, b.first, hashes[i]);
            if (!v || !(*v)->committed) {
                err = KEY_NOT_FOUND;
                return false;
            }
            BlockEntry* e = v->get();
            e->last_access.store(read_tick, std::memory_order_relaxed);
            if (sliced) {
                // Every entry, plain ones included, must hold a page of the
                // size the slice was cut for, and the geometry must be legal
                // for the entry's own codec; a compressed entry needs the
                // 16-byte-aligned client address as below.
                if (!stored_matches(e->codec, e->size, msg.slice.page_bytes) ||
                    !slice_legal(e->codec, msg.slice, client_seg) ||
                    (page_codec_transforms(e->codec) && (client_addr + b.second) % 16 != 0)) {
                    err = INVALID_REQ;
                    return false;
                }
            } else if (tset) {
                // The whole request against the entry's codec (geometry,
                // aligned bases and offsets), once per codec; the page must
                // be the written size, for plain entries too: a smaller
                // stored block would be read past its end.
                const size_t ci = static_cast<size_t>(e->codec);
                if (!tset_codec_seen[ci]) {
                    tset_codec_seen[ci] = true;
                    tset_codec_ok[ci] = tensor_set_request_ok(*tset, msg, e->codec);
                }
                if (!tset_codec_ok[ci] || !stored_matches(e->codec, e->size, page)) {
                    err = INVALID_REQ;
                    return false;
                }
            } else if (!stored_serves(e->codec, e->size, page) ||
                       // A plain entry serves any page up to its own size (one
                       // compare; a larger page would be read past the block's
                       // end). Compressed entries: the page must be the written
                       // size, and the dequantize kernels store 16 bytes per
                       // lane into the client.
                       (page_codec_transforms(e->codec) &&
                        ((client_addr + b.second) % 16 != 0 ||
                         !segments_legal(e->codec, page, msg.n_segments, msg.segment_stride)))) {
                err = INVALID_REQ;
                return false;
            }
            // This runs per block under the stripe lock, where a few ns show
            // in the headline rate: a run of blocks of one (shard, codec)
            // reuses its job, and only a new job reads the codec table.
            const std::pair<Shard*, PageCodec> key{exec_shard(e->shard), e->codec};
            if (!last_job || key != last_key) {
                auto [it, fresh] = jobs.try_emplace(key);
                if (fresh) {
                    it->second.bytes_per_block = page;
                    it->second.codec = e->codec;
                    it->second.dir = PageDir::kLoad;
                    it->second.n_segments = msg.n_segments;
                    it->second.segment_stride = msg.segment_stride;
                    it->second.slice = msg.slice;
                    if (tset) {
                        it->second.tensor_bases = tset->bases;
                        it->second.segs_per_tensor =
                            msg.n_segments / static_cast<uint32_t>(tset->bases->size());
                    }
                    if (page_codec_info(e->codec).page_scale)
                        it->second.scales = std::make_shared<std::vector<float>>();
                }
                last_key = key;
                last_job = &it->second;
            }
            Shard::CopyJob& job = *last_job;
            if (job.scales) job.scales->push_back(e->scale);
            job.src.push_back(reinterpret_cast<uint64_t>(e->ptr));
            job.dst.push_back(client_addr + b.second);
            held->push_back(*v);
            return true;
        });
    if (err) return reply_local(c, ctx, err);
    const bool dbg = debug_on();
    auto tcol = Clock::now();
    n_reads_.fetch_add(1);
    bytes_out_.fetch_add(msg.blocks.size() * page);
    bool sync_resp = (msg.flags & kLocalFlagSyncResponse) != 0;
    if (jobs.empty()) return reply_local(c, ctx, sync_resp ? FINISH : TASK_ACCEPTED);

    c->remain.fetch_add(1);
    c->ref();
    auto pending = std::make_shared<std::atomic<int>>(static_cast<int>(jobs.size()));
    auto all_ok = std::make_shared<std::atomic<bool>>(true);
    auto submit_one = [&](Shard* shard, Shard::CopyJob& job) -> bool {
        Shard::CopyJob j = std::move(job);
        auto t_start2 = Clock::now();
        j.done = [this, c, held, pending, all_ok, sync_resp, ctx, t_start2, dbg](bool ok) {
            if (dbg && held->size() > 64)
                fprintf(stderr, "[sdbg] read n=%zu submit->complete=%.0fus\n", held->size(),
                        us(t_start2, Clock::now()));
            if (!ok) all_ok->store(false);
            if (pending->fetch_sub(1) == 1) {
                if (ctx.shm) {
                    // reply straight from the completion thread: the ring
                    // write needs no loop-thread affinity.
                    if (sync_resp) reply_local(c, ctx, all_ok->load() ? FINISH : INTERNAL_ERROR);
                    finish_task(c, /*on_owner=*/false);
                } else {
                    c->owner->post([this, c, held, all_ok, sync_resp] {
                        if (sync_resp)
                            send_status(c, all_ok->load() ? FINISH : INTERNAL_ERROR);
                        finish_task(c, /*on_owner=*/true);
                    });
                }
            }
        };
        if (!shard->submit_copy(std::move(j))) {
            all_ok->store(false);
            if (pending->fetch_sub(1) == 1) {
                finish_task(c, /*on_owner=*/!ctx.shm);
                reply_local(c, ctx, INTERNAL_ERROR);
                return false;  // error reply sent; stop submitting
            }
        }
        return true;
    };
    for (auto& [key, job] : jobs)
        if (!submit_one(key.first, job)) return;
    if (dbg && msg.blocks.size() > 256)
        fprintf(stderr, "[rdbg] read n=%zu collect=%.0f submit=%.0f\n", msg.blocks.size(),
                us(tr0, tcol), us(tcol, Clock::now()));
    if (!sync_resp && !ctx.shm) send_status(c, TASK_ACCEPTED);
}

// Register a tensor set (socket only; docs/design.md, "tensor sets"). Every
// record is resolved like a request's base: the same-process fast path, or the
// connection's mapping cache, so each distinct handle is opened once. The
// mappings a set uses are counted in ipc_set_refs as they are resolved, which
// keeps a cache flush triggered by a later record from closing them.
void Server::op_tset_register(Conn* c, const std::vector<uint8_t>& body) {
    PackedTensorSetHdr hdr;
    std::vector<PackedTensorRec> recs;
    if (!parse_tensor_set(body.data(), body.size(), &hdr, &recs))
        return send_status(c, INVALID_REQ);
    if (!gpu::available()) return send_status(c, SYSTEM_ERROR);
    const bool same_process = hdr.pid != 0 && hdr.pid == static_cast<int32_t>(getpid());
    for (const PackedTensorRec& r : recs)
        if (r.extent_bytes == 0 || (same_process ? r.base_ptr == 0 : !import_size_ok(r.alloc_mb)))
            return send_status(c, INVALID_REQ);
    IpcPinGuard pin(c);
    auto set = std::make_shared<Conn::TensorSet>();
    auto bases = std::make_shared<std::vector<uint64_t>>();
    set->device = hdr.device;
    set->min_extent = UINT64_MAX;
    set->bases16 = true;
    uint32_t id = 0;
    {
        std::lock_guard<std::mutex> lk(c->ipc_mu);
        if (c->tsets.size() >= kMaxTensorSetsPerConn) return send_status(c, INVALID_REQ);
        bool ok = true;
        for (const PackedTensorRec& r : recs) {
            uint64_t base = r.base_ptr;
            if (!same_process) {
                void* m = open_mapping_locked(c, r.ipc, hdr.device);
                if (!m) {
                    ok = false;
                    break;
                }
                if (std::find(set->mappings.begin(), set->mappings.end(), m) ==
                    set->mappings.end()) {
                    set->mappings.push_back(m);
                    c->ipc_set_refs[m]++;
                }
                base = reinterpret_cast<uint64_t>(m);
            }
            bases->push_back(base + r.base_offset);
            if (bases->back() % 16 != 0) set->bases16 = false;
            set->min_extent = std::min(set->min_extent, r.extent_bytes);
        }
        if (!ok) {
            for (void* m : set->mappings)
                if (--c->ipc_set_refs[m] == 0) c->ipc_set_refs.erase(m);
            return send_status(c, INTERNAL_ERROR);
        }
        set->bases = std::move(bases);
        id = c->next_tset_id++;
        c->tsets.emplace(id, std::move(set));
    }
    send_status_raw(c, FINISH, &id, sizeof(id));
}

// Release a set: its id becomes unknown at once; its mappings stay in the
// cache, open to the next flush. A job in flight keeps the bases it copied.
void Server::op_tset_release(Conn* c, const std::vector<uint8_t>& body) {
    uint32_t id = 0;
    if (body.size() != sizeof(id)) return send_status(c, INVALID_REQ);
    memcpy(&id, body.data(), sizeof(id));
    std::lock_guard<std::mutex> lk(c->ipc_mu);
    auto it = c->tsets.find(id);
    if (it == c->tsets.end()) return send_status(c, INVALID_REQ);
    for (void* m : it->second->mappings)
        if (--c->ipc_set_refs[m] == 0) c->ipc_set_refs.erase(m);
    c->tsets.erase(it);
    send_status(c, FINISH);
}

void Server::op_sync(Conn* c, const ReqCtx& ctx) {
    std::lock_guard<std::mutex> lk(c->sync_mu);
    if (c->remain.load() == 0) {
        reply_query(c, ctx, 0);  // FINISH + remain (infinistore.cpp:1070-1075)
    } else {
        c->sync_waiting = true;  // answered by finish_task when remain drains
        c->sync_ctx = ctx;
    }
}

// Owner loop thread (socket completions) or a completion thread (shm).
void Server::finish_task(Conn* c, bool on_owner) {
    if (c->remain.fetch_sub(1) == 1) {
        ReqCtx ctx;
        bool respond = false;
        {
            std::lock_guard<std::mutex> lk(c->sync_mu);
            if (c->sync_waiting) {
                c->sync_waiting = false;
                respond = true;
                ctx = c->sync_ctx;
            }
        }
        if (respond) {
            if (ctx.shm || on_owner) {
                reply_query(c, ctx, 0);
            } else {
                // socket reply from a completion thread: hop to the owner
                // loop (uv_write is not thread-safe).
                c->ref();
                c->owner->post([this, c, ctx] {
                    reply_query(c, ctx, 0);
                    c->unref();
                });
            }
        }
    }
    c->unref();
}

void Server::reply_local(Conn* c, const ReqCtx& ctx, int code) {
    if (ctx.shm && c->shm) return c->shm->push_resp(ctx.seq, code);
    send_status(c, code);
}

// Query-op responses (check_exist / match / sync): the reference frames
// these as FINISH + 4-byte value on the socket (libinfinistore.cpp:679-694,
// infinistore.cpp:1070-1107); the shm ring carries the value in its
// fixed-size status field instead (ring responses are always 32 bytes).
void Server::reply_query(Conn* c, const ReqCtx& ctx, int value) {
    if (ctx.shm && c->shm) return c->shm->push_resp(ctx.seq, value);
    send_status_raw(c, FINISH, &value, 4);
}

// ---- shared-memory ring transport -----------------------------------------
void Server::ShmPeer::push_resp(uint64_t seq, int status) {
    std::lock_guard<std::mutex> lk(resp_mu);
    shmring::RespRec r{};
    r.h.len = sizeof(r);
    r.h.op = 0;
    r.h.body_len = sizeof(r) - sizeof(r.h);
    r.h.seq = seq;
    r.status = status;
    uint64_t adv = 0;
    uint8_t* dst = seg.resp->claim(sizeof(r), &adv);
    if (!dst) {
        // Client stopped draining (crashed / gone): drop the response; the
        // socket EOF tears the conn down.
        WARN("shm resp ring full; dropping response seq=%llu",
             static_cast<unsigned long long>(seq));
        return;
    }
    memcpy(dst, &r, sizeof(r));
    seg.resp->publish(adv);
}

void Server::op_shm_setup(Conn* c, const std::vector<uint8_t>& body) {
    // Body: shm_open name of a client-created segment. Refuse when already
    // set up, name is implausible, or too many pollers are running.
    if (c->shm || body.empty() || body.size() > 100 || body[0] != '/')
        return send_status(c, INVALID_REQ);
    // Cap on ring pollers: sized for 8 ranks x (4 worker pairs + 1 parent)
    // plus 64 saturation clients with headroom (overflow conns gracefully
    // stay on the socket).
    if (shm_peers_.load() >= 160) return send_status(c, SYSTEM_ERROR);
    std::string name(reinterpret_cast<const char*>(body.data()), body.size());
    auto* p = new ShmPeer();
    p->srv = this;
    p->c = c;
    if (!shmring::open_segment(name, &p->seg)) {
        delete p;
        return send_status(c, INTERNAL_ERROR);
    }
    c->shm = p;
    shm_peers_.fetch_add(1);
    c->ref();  // held by the poller thread; released at poller exit
    p->th = std::thread([this, p] { shm_poll_main(p); });
    INFO("shm ring attached (%zu bytes)", p->seg.len);
    send_status(c, FINISH);
}

void Server::shm_teardown(Conn* c) {
    if (!c->shm) return;
    c->shm->stop.store(true, std::memory_order_release);
    if (c->shm->th.joinable()) c->shm->th.join();
    shm_peers_.fetch_sub(1);
    // The peer + mapping are freed in ~Conn: in-flight completion threads
    // may still write responses into the (now client-less) ring.
}

void Server::fast_worker_main() {
    for (;;) {
        FastWork w;
        {
            std::unique_lock<std::mutex> lk(fast_mu_);
            fast_cv_.wait(lk, [this] { return stop_requested_.load() || !fast_q_.empty(); });
            if (fast_q_.empty()) {
                if (stop_requested_.load()) return;
                continue;
            }
            w = std::move(fast_q_.front());
            fast_q_.pop_front();
        }
        run_fast(w);
    }
}

void Server::run_fast(FastWork& w) {
    ReqCtx ctx{w.seq, true};
    LocalView v;
    if (!parse_packed_local(w.op, w.body.data(), w.body.size(), &v)) {
        reply_local(w.c, ctx, INVALID_REQ);
    } else if (w.op == OP_W_FAST) {
        op_local_write(w.c, v, ctx);
    } else {
        op_local_read(w.c, v, ctx);
    }
    // Balance the poller's enqueue-time remain bump (+ answer a deferred
    // sync if this was the last in-flight unit).
    finish_task(w.c, /*on_owner=*/false);
}

void Server::shm_poll_main(ShmPeer* p) {
    Conn* c = p->c;
    auto last_work = std::chrono::steady_clock::now();
    while (!p->stop.load(std::memory_order_acquire)) {
        uint32_t len = 0;
        uint64_t skip = 0;
        bool corrupt = false;
        const uint8_t* rec = p->seg.req->peek(&len, &skip, &corrupt);
        if (corrupt) {
            // Provably invalid record header (hostile or broken client):
            // following it could read past the mapped segment. Stop polling
            // this ring for good; the conn's socket teardown reclaims it.
            ERROR("shm req ring corrupt (invalid record header); detaching poller");
            break;
        }
        if (!rec) {
            // Adaptive idle: spin while recently hot (sub-µs pickup), back
            // off to 50 µs sleeps when the ring has been quiet.
            if (std::chrono::steady_clock::now() - last_work > std::chrono::milliseconds(2)) {
                usleep(50);
            } else {
#if defined(__x86_64__)
                for (int i = 0; i < 64; i++) __builtin_ia32_pause();
#else
                std::this_thread::yield();
#endif
            }
            continue;
        }
        if (len == 0) {  // wrap marker
            p->seg.req->consume(skip);
            continue;
        }
        shmring::RecHdr h;
        memcpy(&h, rec, sizeof(h));
        const uint8_t* body = rec + sizeof(h);
        ReqCtx ctx{h.seq, true};
        auto t0 = std::chrono::steady_clock::now();
        char op = static_cast<char>(h.op);
        if (debug_on() && h.body_len > 4096)
            fprintf(stderr, "[rdbg] op=%c pickup_wait=%uus\n", op,
                    shmring::mono_us() - h.t_push_us);
        if (h.body_len + sizeof(h) > len) {
            reply_local(c, ctx, INVALID_REQ);
        } else {
            // The record stays in the ring while the handler runs (views
            // point into it); consume() below frees the space.
            switch (op) {
                case OP_W_FAST:
                case OP_R_FAST: {
                    // Hand off to the fast-op pool so this conn's burst of
                    // async requests is handled in parallel (inline handling
                    // serialized each conn behind ~ms handlers). remain is
                    // bumped HERE so a later OP_SYNC on this ring (FIFO)
                    // can never miss the request; the worker balances it.
                    // Hand off only when it pays: many active ring clients
                    // (the pool exists to break per-conn serialization at
                    // saturation — with a handful of pipelined conns the
                    // extra hop just adds latency) and a body big enough
                    // that the handler dwarfs the wakeup (~10 µs vs a
                    // ~20 µs single-page round trip).
                    size_t qlen = 0;
                    bool pool = h.body_len >= 2048 && shm_peers_.load() >= 8 &&
                                !fast_workers_.empty();
                    if (pool) {
                        std::lock_guard<std::mutex> lk(fast_mu_);
                        qlen = fast_q_.size();
                    }
                    if (pool && qlen < 8192) {
                        FastWork w;
                        w.c = c;
                        w.op = op;
                        w.seq = h.seq;
                        w.body.assign(body, body + h.body_len);
                        c->remain.fetch_add(1);
                        c->ref();
                        {
                            std::lock_guard<std::mutex> lk(fast_mu_);
                            fast_q_.push_back(std::move(w));
                        }
                        fast_cv_.notify_one();
                        break;
                    }
                    LocalView v;  // overload fallback: handle inline
                    if (!parse_packed_local(op, body, h.body_len, &v))
                        reply_local(c, ctx, INVALID_REQ);
                    else if (op == OP_W_FAST)
                        op_local_write(c, v, ctx);
                    else
                        op_local_read(c, v, ctx);
                    break;
                }
                case OP_SYNC:
                    op_sync(c, ctx);
                    break;
                case OP_CHECK_EXIST:
                    op_check_exist(c, std::vector<uint8_t>(body, body + h.body_len), ctx);
                    break;
                case OP_GET_MATCH_LAST_IDX:
                    op_match_index(c, std::vector<uint8_t>(body, body + h.body_len), ctx);
                    break;
                case OP_DELETE:
                    op_delete(c, std::vector<uint8_t>(body, body + h.body_len), ctx);
                    break;
                default:
                    reply_local(c, ctx, INVALID_REQ);
            }
        }
        p->seg.req->consume(skip);
        last_work = std::chrono::steady_clock::now();
        auto us = std::chrono::duration_cast<std::chrono::microseconds>(last_work - t0).count();
        auto& st = op_stats_[static_cast<uint8_t>(op) & 127];
        st.count.fetch_add(1, std::memory_order_relaxed);
        st.total_us.fetch_add(static_cast<uint64_t>(us), std::memory_order_relaxed);
        uint64_t prev = st.max_us.load(std::memory_order_relaxed);
        while (static_cast<uint64_t>(us) > prev &&
               !st.max_us.compare_exchange_weak(prev, static_cast<uint64_t>(us))) {
        }
    }
    c->unref();
}

// ---- fabric negotiation + RDMA-semantics ops ------------------------------
void Server::op_exchange(Conn* c, const std::vector<uint8_t>& body) {
    // A body carrying ConnInfo requests the verbs fabric; succeed only when
    // rdma-core + an active NIC are present, else fall back to the TCP data
    // fabric ("TCPF" tag, payloads inline on this socket).
    if (body.size() >= sizeof(vf::ConnInfo)) {
        std::vector<uint8_t> reply;
        if (verbs_handshake(c, body, &reply)) {
            return send_status_payload(c, FINISH, reply.data(), reply.size());
        }
    }
    const char tag[4] = {'T', 'C', 'P', 'F'};
    send_status_payload(c, FINISH, reinterpret_cast<const uint8_t*>(tag), 4);
}

std::vector<RemoteBlockWire> Server::allocate_blocks(Conn* c,
                                                     const std::vector<std::string>& keys,
                                                     size_t page, int* status) {
    *status = FINISH;
    Shard* shard = shard_least_used();
    std::vector<RemoteBlockWire> blocks;
    blocks.reserve(keys.size());
    std::vector<std::tuple<std::string, uint64_t, uint64_t>> created;  // key, hash, ptr
    auto rollback = [&] {
        for (auto& [k, h, p] : created) {
            index_.erase(k, h);
            c->pending_rdma.erase(p);  // drop the ref so the block frees now
        }
    };
    for (auto& key : keys) {
        uint64_t h = KvIndex::hash_of(key);
        if (index_.lookup(key, h)) {
            blocks.push_back({0, 0, 0});  // FAKE block: dup key, client skips
            continue;
        }
        void* ptr = nullptr;
        int pool_idx = -1;
        auto try_alloc = [&] {
            return shard->allocate(page, 1, [&](void* p, int idx) {
                ptr = p;
                pool_idx = idx;
            });
        };
        bool ok = try_alloc();
        for (int attempt = 0; !ok && opt_.auto_evict && attempt < 4; attempt++) {
            if (index_.evict_lru(shard, page * 4) == 0) break;
            ok = try_alloc();
        }
        if (!ok) {
            rollback();
            *status = OUT_OF_MEMORY;
            return {};
        }
        auto* e = new BlockEntry();
        e->ptr = ptr;
        e->size = page;
        e->pool_idx = pool_idx;
        e->shard = shard;
        e->born_sec = KvIndex::now_sec();
        e->last_access.store(index_.tick(), std::memory_order_relaxed);
        Ref<BlockEntry> ref(e);
        if (!index_.insert_if_absent(key, h, ref, /*replace_expired=*/true)) {
            // raced with another writer: first write wins
            blocks.push_back({0, 0, 0});
            continue;  // `ref` releases and frees the block via ~BlockEntry
        }
        // rkey: on the verbs fabric the client posts one-sided RDMA_WRITEs
        // with this key, so it MUST be the registered MR's real rkey for the
        // arena holding the block (reference returns get_rkey(pool_idx) per
        // block, infinistore.cpp:382-396 via mempool.h:56-84). On the TCP
        // fabric the field is unused by the client (addresses key the
        // pending map); an opaque nonzero marker keeps it distinguishable
        // from the FAKE dup sentinel {0,0}.
        uint32_t rkey = static_cast<uint32_t>(shard->device() + 2);
        if (c->verbs) {
            vf::MrInfo mr;
            if (!vdrv_ || !vdrv_->lookup_region(ptr, &mr)) {
                ERROR("allocate: pool arena %p has no MR on the verbs fabric", ptr);
                index_.erase(key, h);
                rollback();
                *status = SYSTEM_ERROR;
                return {};
            }
            rkey = mr.rkey;
        }
        created.push_back({key, h, reinterpret_cast<uint64_t>(ptr)});
        c->pending_rdma.emplace(reinterpret_cast<uint64_t>(ptr), ref);
        blocks.push_back({rkey, 0, reinterpret_cast<uint64_t>(ptr)});
    }
    maybe_extend(shard);
    return blocks;
}

void Server::commit_addrs(Conn* c, const std::vector<uint64_t>& addrs) {
    for (uint64_t addr : addrs) {
        auto it = c->pending_rdma.find(addr);
        if (it == c->pending_rdma.end()) continue;
        it->second->committed = true;
        c->pending_rdma.erase(it);
    }
}

bool Server::collect_read_entries(const std::vector<std::string>& keys,
                                  std::vector<Ref<BlockEntry>>* out) {
    uint64_t t = index_.tick();
    std::vector<uint64_t> hashes(keys.size());
    for (size_t i = 0; i < keys.size(); i++) hashes[i] = KvIndex::hash_of(keys[i]);
    // The sweep visits keys in stripe order; `out` keeps request order.
    out->resize(keys.size());
    return index_.for_each_batched<KvIndex::Lock::kShared>(
        keys.size(), hashes.data(), 0, [&](KvMap& m, size_t i) {
            Ref<BlockEntry>* v = index_.find_live(m, keys[i], hashes[i]);
            // Compressed (fp8, mxfp4) entries are a local-GPU-path feature:
            // the TCP/verbs fabric moves raw bytes and cannot dequantize.
            if (!v || !(*v)->committed || (*v)->codec != PageCodec::kNone) return false;
            (*v)->last_access.store(t, std::memory_order_relaxed);
            (*out)[i] = *v;
            return true;
        });
}

void Server::op_allocate(Conn* c, const RemoteMetaMsg& msg) {
    if (msg.block_size <= 0 || msg.keys.empty()) return send_status(c, INVALID_REQ);
    int status = FINISH;
    auto blocks = allocate_blocks(c, msg.keys, static_cast<size_t>(msg.block_size), &status);
    if (status != FINISH) return send_status(c, status);
    auto payload = build_allocate_response(blocks);
    send_status_payload(c, FINISH, payload.data(), payload.size());
}

void Server::op_tcp_put(Conn* c, std::vector<uint8_t> body) {
    // Layout: [u32 n][u32 block_size][u64 addr x n][payload n*block_size]
    if (body.size() < 8) return send_status(c, INVALID_REQ);
    uint32_t n, bs;
    memcpy(&n, body.data(), 4);
    memcpy(&bs, body.data() + 4, 4);
    size_t need = 8 + static_cast<size_t>(n) * 8 + static_cast<size_t>(n) * bs;
    if (n == 0 || bs == 0 || body.size() < need) return send_status(c, INVALID_REQ);
    const uint64_t* addrs = reinterpret_cast<const uint64_t*>(body.data() + 8);
    size_t payload_off = 8 + static_cast<size_t>(n) * 8;

    // Validate addresses and group by owning shard; copies then run on the
    // shards' fabric worker threads (the IO loop never blocks on memcpy).
    std::map<Shard*, Shard::FabricJob> jobs;
    std::vector<Ref<BlockEntry>> held;
    held.reserve(n);
    for (uint32_t i = 0; i < n; i++) {
        auto it = c->pending_rdma.find(addrs[i]);
        if (it == c->pending_rdma.end()) {
            WARN("tcp_put: unknown addr %llx", (unsigned long long)addrs[i]);
            return send_status(c, INVALID_REQ);
        }
        BlockEntry* e = it->second.get();
        if (e->size < bs) return send_status(c, INVALID_REQ);
        auto& j = jobs[e->shard];
        j.is_put = true;
        j.bytes_per_block = bs;
        j.block_ptrs.push_back(reinterpret_cast<uint64_t>(e->ptr));
        j.host_offsets.push_back(payload_off + static_cast<size_t>(i) * bs);
        held.push_back(it->second);
    }
    n_put_.fetch_add(1);
    bytes_in_.fetch_add(static_cast<size_t>(n) * bs);

    auto shared_body = std::make_shared<std::vector<uint8_t>>(std::move(body));
    auto pending = std::make_shared<std::atomic<int>>(static_cast<int>(jobs.size()));
    auto all_ok = std::make_shared<std::atomic<bool>>(true);
    auto held_sp = std::make_shared<std::vector<Ref<BlockEntry>>>(std::move(held));
    c->fabric_inflight.fetch_add(1);
    c->ref();
    for (auto& [shard, job] : jobs) {
        Shard::FabricJob j = std::move(job);
        j.host = shared_body;
        j.done = [this, c, pending, all_ok, held_sp](bool ok) {
            if (!ok) all_ok->store(false);
            if (pending->fetch_sub(1) == 1) {
                c->owner->post([this, c, all_ok, held_sp] {
                    send_status(c, all_ok->load() ? TASK_ACCEPTED : INTERNAL_ERROR);
                    if (c->fabric_inflight.fetch_sub(1) == 1) {
                        // Drain commits that arrived while copies were in flight.
                        for (auto& addrs2 : c->deferred_commits) {
                            commit_addrs(c, addrs2);
                            send_status(c, FINISH);
                        }
                        c->deferred_commits.clear();
                    }
                    c->unref();
                });
            }
        };
        shard->submit_fabric(std::move(j));
    }
}

void Server::op_commit(Conn* c, const RemoteMetaMsg& msg) {
    if (c->fabric_inflight.load() > 0) {
        // Puts still copying on the fabric workers: commit (and its ACK)
        // must wait so readers never see committed-but-unwritten blocks.
        c->deferred_commits.push_back(msg.remote_addrs);
        return;
    }
    commit_addrs(c, msg.remote_addrs);
    send_status(c, FINISH);
}

void Server::op_tcp_get(Conn* c, const RemoteMetaMsg& msg) {
    if (msg.block_size <= 0 || msg.keys.empty()) return send_status(c, INVALID_REQ);
    size_t page = static_cast<size_t>(msg.block_size);
    std::vector<Ref<BlockEntry>> entries;
    if (!collect_read_entries(msg.keys, &entries)) return send_status(c, KEY_NOT_FOUND);
    // Every entry must hold the page, before a response buffer exists: a
    // streamed response cannot be taken back once its first segment is sent.
    for (const Ref<BlockEntry>& e : entries)
        if (!stored_serves(e->codec, e->size, page)) return send_status(c, INVALID_REQ);
    // The framed response (status + len + blocks) is ONE buffer, filled by
    // the shards' fabric workers; the response is sent on completion.
    // Allocated UNINITIALIZED: value-initializing a 256 MB vector costs
    // ~100 ms before any data moves.
    size_t total = entries.size() * page;
    std::shared_ptr<uint8_t[]> resp(new uint8_t[8 + total]);
    int code = FINISH;
    uint32_t len32 = static_cast<uint32_t>(total);
    memcpy(resp.get(), &code, 4);
    memcpy(resp.get() + 4, &len32, 4);
    std::map<Shard*, Shard::FabricJob> jobs;
    for (size_t i = 0; i < entries.size(); i++) {
        BlockEntry* e = entries[i].get();
        auto& j = jobs[e->shard];
        j.is_put = false;
        j.bytes_per_block = page;
        j.block_ptrs.push_back(reinterpret_cast<uint64_t>(e->ptr));
        j.host_offsets.push_back(8 + i * page);
    }
    n_get_.fetch_add(1);
    bytes_out_.fetch_add(total);
    auto pending = std::make_shared<std::atomic<int>>(static_cast<int>(jobs.size()));
    auto all_ok = std::make_shared<std::atomic<bool>>(true);
    auto held_sp = std::make_shared<std::vector<Ref<BlockEntry>>>(std::move(entries));
    c->ref();
    size_t resp_len = 8 + total;

    // Single-shard big responses STREAM: the job is split into segments and
    // each segment is written to the socket as its copy lands, overlapping
    // the pool→host copy with the send (they were strictly sequential —
    // 256 MB paid copy + send back to back). Payload offsets are ascending
    // within the single job and the fabric worker runs segments FIFO, so
    // in-order streaming holds. Multi-shard responses interleave offsets
    // and keep the single-shot path.
    constexpr size_t kSegBytes = 16u << 20;
    if (jobs.size() == 1 && total > 2 * kSegBytes) {
        auto& [shard, whole] = *jobs.begin();
        size_t nb = whole.block_ptrs.size();
        size_t per_seg = std::max<size_t>(1, kSegBytes / page);
        size_t n_segs = (nb + per_seg - 1) / per_seg;
        auto segs_left = std::make_shared<std::atomic<int>>(static_cast<int>(n_segs));
        for (size_t off = 0; off < nb; off += per_seg) {
            size_t take = std::min(per_seg, nb - off);
            Shard::FabricJob j;
            j.is_put = false;
            j.bytes_per_block = page;
            j.raw_host = resp;
            j.block_ptrs.assign(whole.block_ptrs.begin() + static_cast<long>(off),
                                whole.block_ptrs.begin() + static_cast<long>(off + take));
            j.host_offsets.assign(whole.host_offsets.begin() + static_cast<long>(off),
                                  whole.host_offsets.begin() + static_cast<long>(off + take));
            bool first = off == 0;
            size_t seg_start = first ? 0 : 8 + off * page;  // frame rides seg 0
            size_t seg_len = (first ? 8 : 0) + take * page;
            j.done = [this, c, resp, segs_left, all_ok, held_sp, seg_start,
                      seg_len](bool ok) {
                if (!ok) all_ok->store(false);
                bool last = segs_left->fetch_sub(1) == 1;
                c->ref();
                c->owner->post([this, c, resp, all_ok, seg_start, seg_len, last] {
                    if (all_ok->load()) {
                        std::shared_ptr<uint8_t[]> view(resp, resp.get() + seg_start);
                        send_raw(c, std::move(view), seg_len);
                    } else if (last) {
                        // some earlier segments may already be on the wire;
                        // the client's length-checked read will fail cleanly
                        conn_close(c);
                    }
                    c->unref();
                    if (last) c->unref();  // the op's own ref
                });
            };
            shard->submit_fabric(std::move(j));
        }
        return;
    }

    for (auto& [shard, job] : jobs) {
        Shard::FabricJob j = std::move(job);
        j.raw_host = resp;
        j.done = [this, c, resp, resp_len, pending, all_ok, held_sp](bool ok) {
            if (!ok) all_ok->store(false);
            if (pending->fetch_sub(1) == 1) {
                c->owner->post([this, c, resp, resp_len, all_ok] {
                    if (all_ok->load())
                        send_raw(c, resp, resp_len);
                    else
                        send_status(c, INTERNAL_ERROR);
                    c->unref();
                });
            }
        };
        shard->submit_fabric(std::move(j));
    }
}

// ---- queries ---------------------------------------------------------------
void Server::op_check_exist(Conn* c, const std::vector<uint8_t>& body, const ReqCtx& ctx) {
    // body: raw key bytes (reference framing — body_size IS the key length,
    // libinfinistore.cpp:659-671); response FINISH + int, 0 = exists
    // (infinistore.cpp:1078-1090).
    if (body.empty()) return reply_local(c, ctx, INVALID_REQ);
    std::string key(reinterpret_cast<const char*>(body.data()), body.size());
    Ref<BlockEntry> e = index_.lookup(key, KvIndex::hash_of(key));
    reply_query(c, ctx, e && e->committed ? 0 : 1);
}

void Server::op_match_index(Conn* c, const std::vector<uint8_t>& body, const ReqCtx& ctx) {
    std::vector<std::string> keys;
    if (!parse_match_request(body.data(), body.size(), &keys) || keys.empty())
        return reply_query(c, ctx, -1);
    // Binary search for the last present index, assuming the prefix property
    // (keys[0..i] present iff i <= match). Requires committed entries —
    // divergence from the reference, which counts uncommitted keys as
    // present (infinistore.cpp:1097); an uncommitted key cannot be read, so
    // reporting it as a hit would make the subsequent read_cache fail.
    auto present = [&](size_t i) {
        Ref<BlockEntry> e = index_.lookup(keys[i], KvIndex::hash_of(keys[i]));
        return e && e->committed;
    };
    long left = 0, right = static_cast<long>(keys.size());
    while (left < right) {
        long mid = (left + right) / 2;
        if (present(static_cast<size_t>(mid)))
            left = mid + 1;
        else
            right = mid;
    }
    reply_query(c, ctx, static_cast<int>(left - 1));
}

void Server::op_delete(Conn* c, const std::vector<uint8_t>& body, const ReqCtx& ctx) {
    std::vector<std::string> keys;
    if (!parse_match_request(body.data(), body.size(), &keys))
        return reply_local(c, ctx, INVALID_REQ);
    std::vector<uint64_t> hashes(keys.size());
    for (size_t i = 0; i < keys.size(); i++) hashes[i] = KvIndex::hash_of(keys[i]);
    std::vector<Ref<BlockEntry>> dead;  // one stripe's batch: extracted under its lock
    // Sole-owner entries surrender their block and the blocks free in ONE
    // allocator-lock hold per shard — per-block frees convoyed against
    // concurrent batch allocations (1.3 s per 10k-key delete).
    std::map<Shard*, std::vector<Shard::BlockFree>> by_shard;
    int n = 0;
    index_.for_each_batched<KvIndex::Lock::kExclusive>(
        keys.size(), hashes.data(), 0,
        [&](KvMap& m, size_t i) {
            Ref<BlockEntry> ref;
            if (m.extract(keys[i], &ref)) dead.emplace_back(std::move(ref));
            return true;
        },
        nullptr,
        [&] {
            // Stripe released: drop its batch now, not after the whole sweep.
            // The pause lets a reader that queued on this stripe (reads sweep
            // from stripe 0 too) get ahead instead of trailing us for 64 locks
            // (measured: 2 ms read-handler tails under 12-client delete churn).
            n += static_cast<int>(dead.size());
            for (auto& ref : dead) {
                BlockEntry* e = ref.get();
                if (e->ref_count() == 1 && e->shard && e->ptr) {
                    by_shard[e->shard].push_back({e->ptr, e->size, e->pool_idx});
                    e->shard = nullptr;  // dtor skips the per-block free
                    e->ptr = nullptr;
                }
            }
            dead.clear();
        });
    for (auto& [shard, frees] : by_shard) shard->deallocate_bulk(frees);
    reply_local(c, ctx, n);
}

// ---------------------------------------------------------------------------
// Management plane
// ---------------------------------------------------------------------------
std::pair<size_t, size_t> Server::compact() {
    if (!running_.load()) return {0, 0};
    // Defragmentation in three phases per shard. The index locks are NOT
    // held across the copy wait: the completion threads that fulfil our
    // copy futures also run write handlers' `fin`, and a write handler's
    // phase D takes stripe locks while its kernel is in flight. Holding
    // every stripe while waiting on those threads would park each writer
    // in phase D for the whole copy with its copy slot taken, ahead of our
    // own jobs (the mixed fp8/eviction soak deadlocked on an earlier form).
    //  1. snapshot (all stripe locks, in order): pick committed idle
    //     entries, take a Ref on each so neither delete nor eviction can
    //     free the old block mid-copy.
    //  2. copy (no locks): batched kernel moves into the planned slots.
    //  3. swap (all stripe locks): re-check each entry is still present and
    //     still idle (a reader that started during the copy captured the
    //     OLD pointer and holds a ref — skip those), then flip ptr/pool and
    //     free the old slot. Unapplied moves free their new slot instead.
    size_t moved = 0, bytes = 0;
    for (auto& shard_up : shards_) {
        Shard* shard = shard_up.get();
        std::vector<Ref<BlockEntry>> held;
        std::vector<std::pair<void*, size_t>> movable;
        index_.for_each_all_locked([&](std::string_view, Ref<BlockEntry>& val) {
            BlockEntry* e = val.get();
            if (e->shard == shard && e->committed && e->ref_count() == 1) {
                held.push_back(val);
                movable.push_back({e->ptr, e->size});
            }
        });
        if (movable.empty()) continue;
        auto moves = shard->plan_compaction(movable);
        if (moves.empty()) continue;

        std::map<size_t, Shard::CopyJob> by_size;  // one job per page size
        for (auto& m : moves) {
            auto& j = by_size[m.size];
            j.bytes_per_block = m.size;
            j.src.push_back(reinterpret_cast<uint64_t>(m.old_ptr));
            j.dst.push_back(reinterpret_cast<uint64_t>(m.new_ptr));
        }
        bool copies_ok = true;
        for (auto& [sz, j2] : by_size) {
            std::promise<bool> cp;
            auto cf = cp.get_future();
            Shard::CopyJob jj = std::move(j2);
            jj.done = [&cp](bool ok) { cp.set_value(ok); };
            if (!shard->submit_copy(std::move(jj))) {
                cp.set_value(false);
            }
            if (!cf.get()) copies_ok = false;
        }

        std::map<void*, Shard::Move*> by_old;
        for (auto& m : moves) by_old[m.old_ptr] = &m;
        index_.for_each_all_locked([&](std::string_view, Ref<BlockEntry>& val) {
            BlockEntry* e = val.get();
            auto it = by_old.find(e->ptr);
            if (it == by_old.end() || e->shard != shard) return;
            // map ref + our `held` ref = 2; more means an in-flight
            // read captured the old pointer during the copy.
            if (!copies_ok || e->ref_count() > 2) return;
            Shard::Move* m = it->second;
            e->ptr = m->new_ptr;
            e->pool_idx = m->pool_idx;
            shard->deallocate(m->old_ptr, m->size, m->pool_idx);
            m->old_ptr = nullptr;  // applied
            moved++;
            bytes += m->size;
        });
        for (auto& m : moves)
            if (m.old_ptr != nullptr)  // unapplied: release the planned slot
                shard->deallocate(m.new_ptr, m.size, m.pool_idx);
        // held refs drop here; entries erased during the copy free their
        // (old) blocks now.
    }
    return {moved, bytes};
}

// ---- snapshot / restore ----------------------------------------------------
namespace {
constexpr uint64_t kSnapMagic = 0x53494653504e3150ull;  // "SIFSPN1P"
struct SnapEntryHdr {
    uint32_t key_len;
    uint32_t codec;  // PageCodec value: 0 plain, 1 fp8, 2 mxfp4
    uint64_t size;  // stored bytes
    float scale;
    uint32_t _pad;
};
}  // namespace

bool Server::snapshot(const std::string& path, std::pair<size_t, size_t>* out) {
    *out = {0, 0};
    // Pin a consistent set of committed entries (refs keep blocks alive and
    // make compaction skip them — it requires ref_count()==1), then stream
    // them out without holding any lock.
    std::vector<std::pair<std::string, Ref<BlockEntry>>> pinned;
    index_.for_each_shared([&](std::string_view key, Ref<BlockEntry>& val) {
        if (val->committed && !index_.expired(val.get()))
            pinned.emplace_back(std::string(key), val);
    });
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) {
        ERROR("snapshot: cannot open %s", path.c_str());
        return false;
    }
    uint64_t magic = kSnapMagic, count = pinned.size();
    bool ok = fwrite(&magic, 8, 1, f) == 1 && fwrite(&count, 8, 1, f) == 1;
    std::vector<uint8_t> buf;
    for (auto& [key, ref] : pinned) {
        if (!ok) break;
        BlockEntry* e = ref.get();
        SnapEntryHdr h{static_cast<uint32_t>(key.size()), static_cast<uint32_t>(e->codec),
                       e->size, e->scale, 0};
        buf.resize(e->size);
        if (e->shard->on_gpu()) {
            if (!gpu::memcpy_d2h(buf.data(), e->ptr, e->size)) {
                ok = false;
                break;
            }
        } else {
            memcpy(buf.data(), e->ptr, e->size);
        }
        ok = fwrite(&h, sizeof(h), 1, f) == 1 && fwrite(key.data(), 1, key.size(), f) == key.size() &&
             fwrite(buf.data(), 1, e->size, f) == e->size;
        out->first++;
        out->second += e->size;
    }
    fclose(f);
    if (!ok) ERROR("snapshot: write failed at entry %zu", out->first);
    return ok;
}

bool Server::restore(const std::string& path, std::pair<size_t, size_t>* out) {
    *out = {0, 0};
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) {
        ERROR("restore: cannot open %s", path.c_str());
        return false;
    }
    uint64_t magic = 0, count = 0;
    if (fread(&magic, 8, 1, f) != 1 || magic != kSnapMagic || fread(&count, 8, 1, f) != 1) {
        ERROR("restore: bad snapshot header");
        fclose(f);
        return false;
    }
    std::vector<uint8_t> buf;
    std::string key;
    bool ok = true;
    for (uint64_t i = 0; i < count && ok; i++) {
        SnapEntryHdr h{};
        if (fread(&h, sizeof(h), 1, f) != 1 || h.key_len > 4096 || h.size > (1u << 30) ||
            !page_codec_known(h.codec)) {
            ok = false;
            break;
        }
        key.resize(h.key_len);
        buf.resize(h.size);
        if (fread(key.data(), 1, h.key_len, f) != h.key_len ||
            fread(buf.data(), 1, h.size, f) != h.size) {
            ok = false;
            break;
        }
        Shard* shard = shard_least_used();
        void* ptr = nullptr;
        int pool_idx = -1;
        if (!shard->allocate(h.size, 1, [&](void* p, int idx) {
                ptr = p;
                pool_idx = idx;
            })) {
            WARN("restore: pool full after %zu entries", out->first);
            break;  // partial restore is still useful
        }
        bool copied = shard->on_gpu() ? gpu::memcpy_h2d(ptr, buf.data(), h.size)
                                      : (memcpy(ptr, buf.data(), h.size), true);
        if (!copied) {
            shard->deallocate(ptr, h.size, pool_idx);
            ok = false;
            break;
        }
        auto* e = new BlockEntry();
        e->ptr = ptr;
        e->size = h.size;
        e->pool_idx = pool_idx;
        e->shard = shard;
        e->codec = static_cast<PageCodec>(h.codec);
        e->scale = h.scale;
        e->born_sec = KvIndex::now_sec();
        e->committed = true;
        e->last_access.store(index_.tick(), std::memory_order_relaxed);
        Ref<BlockEntry> ref(e);
        // Plain insert-if-absent: an expired live key still beats the snapshot.
        if (index_.insert_if_absent(key, KvIndex::hash_of(key), ref, /*replace_expired=*/false)) {
            out->first++;
            out->second += h.size;
        }
        // !ins: live key wins over the snapshot; `ref` frees the block.
    }
    fclose(f);
    return ok;
}

std::string Server::stats_json() {
    char buf[1024];
    size_t used = 0, total = 0, frag = 0;
    for (auto& s : shards_) {
        used += s->used_blocks();
        total += s->total_blocks();
        frag = std::max(frag, s->largest_free_run_bytes());
    }
    snprintf(buf, sizeof(buf),
             "{\"kv_len\": %zu, \"shards\": %zu, \"used_blocks\": %zu, \"total_blocks\": %zu, "
             "\"writes\": %llu, \"reads\": %llu, \"puts\": %llu, \"gets\": %llu, "
             "\"bytes_in\": %llu, \"bytes_out\": %llu, \"largest_free_run_bytes\": %zu, "
             "\"op_us\": {",
             kvmap_len(), shards_.size(), used, total,
             (unsigned long long)n_writes_.load(), (unsigned long long)n_reads_.load(),
             (unsigned long long)n_put_.load(), (unsigned long long)n_get_.load(),
             (unsigned long long)bytes_in_.load(), (unsigned long long)bytes_out_.load(), frag);
    std::string out(buf);
    bool first = true;
    for (int i = 0; i < 128; i++) {
        uint64_t cnt = op_stats_[i].count.load();
        if (!cnt) continue;
        char entry[160];
        snprintf(entry, sizeof(entry),
                 "%s\"%s\": {\"count\": %llu, \"avg_us\": %.1f, \"max_us\": %llu}",
                 first ? "" : ", ", op_name(static_cast<char>(i)).c_str(),
                 (unsigned long long)cnt,
                 static_cast<double>(op_stats_[i].total_us.load()) / cnt,
                 (unsigned long long)op_stats_[i].max_us.load());
        out += entry;
        first = false;
    }
    out += "}}";
    return out;
}

}  // namespace ifs
