#include "kv_index.h"

#include <ctime>
#include <memory>
#include <string>

#include "../core/log.h"

namespace ifs {

// ---------------------------------------------------------------------------
// BlockEntry slab allocator (entries churn by the thousands per request)
// ---------------------------------------------------------------------------
namespace {
struct EntrySlab {
    std::mutex mu;
    std::vector<void*> free_list;
    std::vector<std::unique_ptr<char[]>> chunks;
    static constexpr size_t kPerChunk = 4096;

    void* take_locked(size_t n) {
        if (free_list.empty()) {
            chunks.emplace_back(new char[n * kPerChunk]);
            char* base = chunks.back().get();
            free_list.reserve(kPerChunk);
            for (size_t i = 0; i < kPerChunk; i++) free_list.push_back(base + i * n);
        }
        void* p = free_list.back();
        free_list.pop_back();
        return p;
    }

    // Thread-local magazines: entry alloc/free happens on every handler,
    // completion and delete path — one global mutex per op (especially
    // give(), which delete churn hit ~6M times per 64-client run) serialized
    // the whole server. Each thread caches up to kMagMax entries and
    // exchanges them with the global list kMagBatch at a time.
    static constexpr size_t kMagBatch = 256;
    static constexpr size_t kMagMax = 512;
    struct Magazine {
        std::vector<void*> items;
        ~Magazine();  // flush to the global list (pollers exit per conn)
    };
    static Magazine& mag() {
        thread_local Magazine m;
        return m;
    }

    void* take(size_t n) {
        auto& m = mag();
        if (m.items.empty()) {
            std::lock_guard<std::mutex> lk(mu);
            m.items.reserve(kMagMax);
            for (size_t i = 0; i < kMagBatch; i++) m.items.push_back(take_locked(n));
        }
        void* p = m.items.back();
        m.items.pop_back();
        return p;
    }
    // Bulk take for a write batch: drain the magazine, top up from the
    // global list under ONE lock.
    void take_bulk(size_t n, size_t count, std::vector<void*>* out) {
        auto& m = mag();
        while (count && !m.items.empty()) {
            out->push_back(m.items.back());
            m.items.pop_back();
            count--;
        }
        if (count) {
            std::lock_guard<std::mutex> lk(mu);
            for (size_t i = 0; i < count; i++) out->push_back(take_locked(n));
        }
    }
    void give(void* p) {
        auto& m = mag();
        m.items.push_back(p);
        if (m.items.size() >= kMagMax) {
            std::lock_guard<std::mutex> lk(mu);
            for (size_t i = 0; i < kMagBatch; i++) {
                free_list.push_back(m.items.back());
                m.items.pop_back();
            }
        }
    }
    void give_bulk(std::vector<void*>& items, size_t from) {
        auto& m = mag();
        for (size_t i = from; i < items.size(); i++) m.items.push_back(items[i]);
        if (m.items.size() >= kMagMax) {
            std::lock_guard<std::mutex> lk(mu);
            while (m.items.size() > kMagBatch) {
                free_list.push_back(m.items.back());
                m.items.pop_back();
            }
        }
    }
};
EntrySlab& entry_slab() {
    // Intentionally leaked: entries may still be freed during interpreter
    // teardown after static destructors would have run.
    static EntrySlab* s = new EntrySlab();
    return *s;
}

EntrySlab::Magazine::~Magazine() {
    if (items.empty()) return;
    auto& s = entry_slab();  // leaked singleton: safe at thread exit
    std::lock_guard<std::mutex> lk(s.mu);
    for (void* p : items) s.free_list.push_back(p);
}
}  // namespace

void* BlockEntry::operator new(size_t n) { return entry_slab().take(n); }
void BlockEntry::operator delete(void* p) { entry_slab().give(p); }

SlabBatch::SlabBatch(size_t count) {
    slots.reserve(count);
    entry_slab().take_bulk(sizeof(BlockEntry), count, &slots);
}
SlabBatch::~SlabBatch() {
    if (next < slots.size()) entry_slab().give_bulk(slots, next);
}

KvIndex::KvIndex(int ttl_seconds, size_t stripe_slots) : ttl_seconds_(ttl_seconds) {
    for (auto& st : stripes_) st.map.reserve(stripe_slots / 2);
}

uint32_t KvIndex::now_sec() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return static_cast<uint32_t>(ts.tv_sec);
}

Ref<BlockEntry> KvIndex::lookup(std::string_view key, uint64_t h) {
    Stripe& st = stripes_[stripe_of(h)];
    std::shared_lock<std::shared_mutex> lk(st.mu);
    Ref<BlockEntry>* v = find_live(st.map, key, h);
    return v ? *v : Ref<BlockEntry>();
}

bool KvIndex::insert_if_absent(std::string_view key, uint64_t h, const Ref<BlockEntry>& ref,
                               bool replace_expired) {
    std::vector<Ref<BlockEntry>> displaced;  // dropped after unlock
    Stripe& st = stripes_[stripe_of(h)];
    std::lock_guard<std::shared_mutex> lk(st.mu);
    return insert_locked(st.map, key, h, ref, replace_expired, &displaced);
}

bool KvIndex::erase(std::string_view key, uint64_t h) {
    Ref<BlockEntry> dead;  // dropped after unlock
    Stripe& st = stripes_[stripe_of(h)];
    std::lock_guard<std::shared_mutex> lk(st.mu);
    return st.map.extract(key, &dead);
}

template <typename Pred>  // pred(const Ref<BlockEntry>&) -> bool
size_t KvIndex::erase_where(Stripe& st, Pred&& pred) {
    std::vector<Ref<BlockEntry>> dead;  // dropped after unlock
    std::lock_guard<std::shared_mutex> lk(st.mu);
    std::vector<std::string> victims;
    st.map.for_each([&](std::string_view key, Ref<BlockEntry>& val) {
        if (pred(val)) victims.emplace_back(key);
    });
    dead.reserve(victims.size());
    for (auto& k : victims) {
        Ref<BlockEntry> ref;
        if (st.map.extract(k, &ref)) dead.emplace_back(std::move(ref));
    }
    return victims.size();
}

void KvIndex::erase_entries(const std::vector<Ref<BlockEntry>>& entries) {
    // O(map) scan, but keys are not kept around on the hot path. One stripe
    // at a time.
    for (auto& st : stripes_)
        erase_where(st, [&](const Ref<BlockEntry>& val) {
            for (auto& e : entries)
                if (val.get() == e.get()) return true;
            return false;
        });
}

size_t KvIndex::sweep_expired() {
    size_t swept = 0;
    for (auto& st : stripes_)
        swept += erase_where(st, [&](const Ref<BlockEntry>& val) {
            return expired(val.get()) && val->ref_count() == 1;
        });
    return swept;
}

size_t KvIndex::evict_lru(Shard* shard, size_t bytes) {
    // Sampled clock-hand eviction: scan bounded slot windows from a
    // persistent per-stripe cursor, evict the least-recently-accessed half
    // of each sample — O(evicted) amortized instead of a full index scan
    // per eviction event (which capped sustained full-pool churn).
    // Candidates: committed, idle (only the map holds a ref), on this shard.
    // Key views stay valid across erase (the arena is append-only).
    // Stripes are visited round-robin (shared cursor) holding one stripe
    // lock at a time.
    size_t freed = 0;
    // NOTE on fresh writes: the sample sort below already evicts oldest
    // first, so recently written keys survive unless a sample is entirely
    // fresh (possible at ~100% occupancy — the pool is then genuinely too
    // small for the working set and evicting fresh data is the honest LRU
    // outcome). An explicit freshness-exemption pass was tried and reverted:
    // at full occupancy it degenerated to an O(map) rescan per allocation
    // (13x soak throughput collapse).
    for (size_t visited = 0; freed < bytes && visited < kStripes; visited++) {
        auto& st = stripes_[evict_stripe_rr_.fetch_add(1) % kStripes];
        std::vector<Ref<BlockEntry>> dead;  // block frees run after unlock
        std::lock_guard<std::shared_mutex> lk(st.mu);
        size_t scanned = 0;
        const size_t scan_cap = st.map.capacity();  // one revolution max
        std::vector<std::pair<uint64_t, std::string_view>> sample;
        sample.reserve(128);
        while (freed < bytes && scanned < scan_cap) {
            size_t window = 4096;
            st.map.scan_from(&st.evict_hand, window,
                             [&](std::string_view key, Ref<BlockEntry>& val) {
                                 BlockEntry* e = val.get();
                                 uint64_t la = e->last_access.load(std::memory_order_relaxed);
                                 if (e->shard == shard && e->committed && e->ref_count() == 1)
                                     sample.push_back({expired(e) ? 0 : la, key});  // expired first
                                 return sample.size() < 128;
                             });
            scanned += window;
            // In a sparse table one window yields few candidates; evicting
            // from a 1-2 entry "sample" degrades LRU to "next key after the
            // cursor". Accumulate across windows until the sample is big
            // enough to rank (or the stripe is fully scanned).
            if (sample.size() < 128 && scanned < scan_cap) continue;
            if (sample.empty()) break;
            std::sort(sample.begin(), sample.end(),
                      [](const auto& a, const auto& b) { return a.first < b.first; });
            size_t take = std::max<size_t>(1, sample.size() / 2);
            for (size_t i = 0; i < take && freed < bytes; i++) {
                Ref<BlockEntry> ref;
                if (!st.map.extract(sample[i].second, &ref)) continue;
                freed += ref->size;
                dead.emplace_back(std::move(ref));
                n_evicted_.fetch_add(1);
            }
            sample.clear();
        }
    }
    if (freed) DEBUG("auto-evicted %zu bytes from shard dev=%d", freed, shard->device());
    return freed;
}

size_t KvIndex::size() {
    size_t n = 0;
    for (auto& st : stripes_) {
        std::shared_lock<std::shared_mutex> lk(st.mu);
        n += st.map.size();
    }
    return n;
}

size_t KvIndex::clear() {
    size_t n = 0;
    for (auto& st : stripes_) {
        std::lock_guard<std::shared_mutex> lk(st.mu);
        n += st.map.size();
        st.map.clear();
    }
    return n;
}

void KvIndex::reserve(size_t n_keys) {
    for (auto& st : stripes_) st.map.reserve(n_keys / kStripes);
}

}  // namespace ifs
