// Striped key index: string key -> refcounted BlockEntry.
//
// 64 independent open-addressing maps (kvmap.h), each behind its own
// reader-writer lock and selected by the top bits of the wide key hash
// (KvMap uses the low bits for the slot). Lookups take a stripe shared,
// inserts/erases exclusive, so concurrent writers land on different stripes:
// a single exclusive lock measured 334 µs avg / 8.5 ms max handler time under
// 8-client write churn, and 16 stripes still convoyed for ms at 64 writers.
//
// Invariants (the measured lessons of round 2 — keep them when editing):
//  * No BlockEntry destructor, pool free or slab free runs under a stripe
//    lock: refs are moved out under the lock and dropped after it (per-block
//    frees under the lock blocked whole stripes for ms during delete sweeps).
//    clear() is the one exception: a management-plane whole-map teardown.
//  * OP_DELETE surrenders sole-owner blocks and frees them with ONE
//    deallocate_bulk per shard. It drops each stripe's dead refs right after
//    that stripe: a delete that sweeps the 64 locks back to back drags every
//    reader that queued behind it along (reads start at stripe 0 too).
//  * No path holds two stripe locks, except for_each_all_locked() (compact's
//    two all-stripe phases), which takes them in index order.
//  * erase_entries() for a failed copy runs on the conn's owner loop, never
//    on a completion thread.
//  * First write wins; an expired entry counts as absent and is replaced in
//    place; a losing writer keeps its block alive until its copy completes.
//  * The write path's second-arriver commit (arrivals counter, copy_ok
//    release/acquire, socket path posting to the owner loop) lives in
//    Server::op_local_write and never waits on a stripe lock holder.
//  * tick() and BlockEntry::last_access are relaxed atomics, bumped under the
//    SHARED lock by concurrent readers.
#pragma once

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <mutex>
#include <shared_mutex>
#include <string_view>
#include <type_traits>
#include <vector>

#include "../core/page_codec.h"
#include "../core/utils.h"
#include "kvmap.h"
#include "shard.h"

namespace ifs {

// One stored block. Refcounted: the kv map holds one ref; in-flight reads
// hold another so purge cannot free memory under an active copy.
// Slab-allocated: prefill writes create thousands of entries per request,
// so class-level new/delete run on a chunked freelist instead of malloc.
struct BlockEntry : RefCounted {
    void* ptr = nullptr;
    size_t size = 0;
    int pool_idx = -1;
    Shard* shard = nullptr;
    bool committed = false;
    // Compressed page (extension): `size` is the STORED byte size. fp8:
    // half the logical bf16 page, reads dequantize with `scale`. mxfp4:
    // 17/64 of it, the scales are inside the block and `scale` is unused.
    PageCodec codec = PageCodec::kNone;
    float scale = 1.f;
    uint32_t born_sec = 0;  // CLOCK_MONOTONIC seconds at insert (TTL)
    std::atomic<uint64_t> last_access{0};  // LRU tick (auto_evict)
    ~BlockEntry() override {
        if (shard && ptr) shard->deallocate(ptr, size, pool_idx);
    }
    static void* operator new(size_t n);
    static void operator delete(void* p);
    // placement forms (class-level operator new hides the global ones)
    static void* operator new(size_t, void* p) { return p; }
    static void operator delete(void*, void*) {}
};

// One slab lock for a whole burst of entry allocations (hot write path).
struct SlabBatch {
    std::vector<void*> slots;
    size_t next = 0;
    explicit SlabBatch(size_t count);
    ~SlabBatch();  // unused slots go back to the slab
    BlockEntry* make() { return new (slots[next++]) BlockEntry(); }
};

class KvIndex {
   public:
    enum class Lock { kShared, kExclusive };
    struct SweepTimes {  // of one sweep, µs (IFS_SERVER_DEBUG)
        double lock_wait_us = 0, under_lock_us = 0;
    };
    // Every stripe starts with stripe_slots slots (a power of two >= 4; the
    // default is KvMap's own); reserve() only ever grows a stripe.
    explicit KvIndex(int ttl_seconds, size_t stripe_slots = 1 << 20);

    static uint64_t hash_of(std::string_view key) { return KvMap::hash_of(key); }
    // Starting stripe for write sweeps, from the first key's hash: concurrent
    // requests sweeping in the same ascending order convoy on every lock.
    static size_t rotated_start(const uint64_t* hashes, size_t n) {
        return n ? static_cast<size_t>(hashes[0] >> 32) % kStripes : 0;
    }
    static uint32_t now_sec();
    uint64_t tick() { return access_tick_.fetch_add(1, std::memory_order_relaxed); }
    // TTL check (lazy expiry): true when the entry is past its lifetime —
    // lookups treat it as absent; the evictor reclaims it first.
    bool expired(const BlockEntry* e) const {
        return ttl_seconds_ > 0 && now_sec() - e->born_sec > static_cast<uint32_t>(ttl_seconds_);
    }

    // The one batched sweep: bucket indices 0..n-1 by stripe once, then visit
    // the stripes from `start`, holding exactly one stripe lock (mode L) at a
    // time and prefetching slot lines 16 keys ahead of fn(KvMap&, i) -> bool.
    // fn returning false stops the sweep; the result is whether it ran to the
    // end. Total for n == 0. Reads a clock only when `times` is set.
    // after_unlock(), if given, runs after each visited stripe is released.
    template <Lock L, typename Fn, typename After = std::nullptr_t>
    bool for_each_batched(size_t n, const uint64_t* hashes, size_t start, Fn&& fn,
                          SweepTimes* times = nullptr, After&& after_unlock = nullptr);

    // For use inside a sweep's fn (that stripe's lock is held): the slot, or
    // nullptr when the key is absent or expired ...
    Ref<BlockEntry>* find_live(KvMap& m, std::string_view key, uint64_t h) const {
        Ref<BlockEntry>* v = m.find_hashed(key, h);
        return v && !expired(v->get()) ? v : nullptr;
    }
    // ... and insert-if-absent (exclusive lock). With replace_expired an
    // expired entry is replaced in place and its ref moved to `displaced`
    // for the caller to drop after the lock. True when `ref` is in the map.
    bool insert_locked(KvMap& m, std::string_view key, uint64_t h, const Ref<BlockEntry>& ref,
                       bool replace_expired, std::vector<Ref<BlockEntry>>* displaced) const {
        bool inserted = false;
        Ref<BlockEntry>* slot = m.emplace_hashed(key, h, ref, &inserted);
        if (inserted || !replace_expired || !expired(slot->get())) return inserted;
        displaced->push_back(std::move(*slot));
        *slot = ref;
        return true;
    }

    // Single-key entry points (each takes the key's stripe lock itself).
    Ref<BlockEntry> lookup(std::string_view key, uint64_t h);  // live entry or null
    bool insert_if_absent(std::string_view key, uint64_t h, const Ref<BlockEntry>& ref,
                          bool replace_expired);
    bool erase(std::string_view key, uint64_t h);

    // fn(string_view key, Ref<BlockEntry>&) over the whole index under ALL
    // stripe locks, taken exclusively in index order ...
    template <typename Fn>
    void for_each_all_locked(Fn&& fn) {
        std::vector<std::unique_lock<std::shared_mutex>> locks;
        locks.reserve(kStripes);
        for (auto& st : stripes_) locks.emplace_back(st.mu);
        for (auto& st : stripes_) st.map.for_each(fn);
    }
    // ... or one stripe at a time under its shared lock.
    template <typename Fn>
    void for_each_shared(Fn&& fn) {
        for (auto& st : stripes_) {
            std::shared_lock<std::shared_mutex> lk(st.mu);
            st.map.for_each(fn);
        }
    }

    // Remove entries by identity (rare: allocation failure / failed copy).
    void erase_entries(const std::vector<Ref<BlockEntry>>& entries);
    // Evict >= `bytes` of LRU committed idle entries on `shard`; the caller
    // holds no stripe lock. Returns bytes freed.
    size_t evict_lru(Shard* shard, size_t bytes);
    // One TTL pass: erase expired idle entries; returns how many.
    size_t sweep_expired();

    size_t size();
    size_t clear();                // returns the number of entries dropped
    void reserve(size_t n_keys);  // spread evenly over the stripes

   private:
    static constexpr size_t kStripes = 64;
    static constexpr size_t kPrefetch = 16;
    struct Stripe {
        // shared_mutex: dedup/read/query phases take it shared so the
        // pipelined few-connection path keeps its read concurrency.
        std::shared_mutex mu;
        KvMap map{4};  // smallest table KvMap's load limit keeps a free slot in
        size_t evict_hand = 0;  // per-stripe clock cursor (mu held)
    };
    static size_t stripe_of(uint64_t h) { return (h >> 58) & (kStripes - 1); }
    template <typename Pred>  // extract matches under the lock, drop them after
    size_t erase_where(Stripe& st, Pred&& pred);

    // Read on every probe: kept off the cache lines that locks and the
    // per-request counters below dirty.
    alignas(64) const int ttl_seconds_;
    alignas(64) std::array<Stripe, kStripes> stripes_;
    std::atomic<size_t> evict_stripe_rr_{0};
    std::atomic<uint64_t> access_tick_{1};
    std::atomic<uint64_t> n_evicted_{0};
};

template <KvIndex::Lock L, typename Fn, typename After>
bool KvIndex::for_each_batched(size_t n, const uint64_t* hashes, size_t start, Fn&& fn,
                               SweepTimes* times, After&& after_unlock) {
    // Stable counting sort of the indices by stripe (all empty for n == 0).
    std::array<uint32_t, kStripes + 1> first{};
    for (size_t i = 0; i < n; i++) first[stripe_of(hashes[i]) + 1]++;
    for (size_t s = 0; s < kStripes; s++) first[s + 1] += first[s];
    std::vector<uint32_t> order(n);
    {
        auto pos = first;
        for (size_t i = 0; i < n; i++) order[pos[stripe_of(hashes[i])]++] = static_cast<uint32_t>(i);
    }
    using Clock = std::chrono::steady_clock;
    using Guard = std::conditional_t<L == Lock::kShared, std::shared_lock<std::shared_mutex>,
                                     std::unique_lock<std::shared_mutex>>;
    auto us = [](Clock::time_point a, Clock::time_point b) {
        return std::chrono::duration<double, std::micro>(b - a).count();
    };
    for (size_t sk = 0; sk < kStripes; sk++) {
        const size_t si = (start + sk) % kStripes;
        const uint32_t* list = order.data() + first[si];
        const size_t ln = first[si + 1] - first[si];
        if (ln == 0) continue;
        Stripe& st = stripes_[si];
        Clock::time_point t0, t1;
        bool go = true;
        {
            if (times) t0 = Clock::now();
            Guard lk(st.mu);
            if (times) t1 = Clock::now();
            for (size_t i = 0; i < std::min(kPrefetch, ln); i++) st.map.prefetch(hashes[list[i]]);
            for (size_t i = 0; go && i < ln; i++) {
                if (i + kPrefetch < ln) st.map.prefetch(hashes[list[i + kPrefetch]]);
                go = fn(st.map, static_cast<size_t>(list[i]));
            }
            if (times) {
                times->lock_wait_us += us(t0, t1);
                times->under_lock_us += us(t1, Clock::now());
            }
        }
        if constexpr (!std::is_null_pointer_v<std::decay_t<After>>) after_unlock();
        if (!go) return false;
    }
    return true;
}

}  // namespace ifs
