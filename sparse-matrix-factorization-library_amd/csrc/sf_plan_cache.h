// What the struct path's handlers (sf_handlers.hip) know a sparsity pattern by, and where they keep its plans: the key of a
// pattern, the small LRU cache both the single handler and the multi-handler state use, and the host side of the per-panel
// fingerprints a verified resident solve compares (sf_resident.hip).  No HIP here: tools/handlers_host_sanitize.cpp runs all of it
// on a CPU under ASan + UBSan.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "sf_schedule.h"

namespace sf {

struct PlanKey {
    uint64_t h = 0;
    int64_t n = 0, nsuper = 0, isize = 0, xsize = 0, nnz = 0, unz = 0;
    int lu = 0;
    bool operator==(const PlanKey& o) const {
        return h == o.h && n == o.n && nsuper == o.nsuper && isize == o.isize && xsize == o.xsize && nnz == o.nnz && unz == o.unz && lu == o.lu;
    }
};

// 64-bit multiply-xorshift hash over 8-byte words, four independent lanes (memory-bound: ~10 GB/s per thread)
uint64_t hash_words(const int64_t* a, int64_t n, uint64_t seed);

// the arrays a plan depends on: Super, Lsip, Lsxp, Lsi (the symbolic factor) and Lp, Li (Up, Ui) (where the matrix entries go);
// the two long ones (Lsi, Li) are hashed by their own threads
PlanKey make_key(const PlanInput& in);

constexpr size_t MAX_CACHED_PLANS = 2;      // per handler: MATRIX_THREAD_NUM = 2 matrices in flight in the reference's driver

// The plans of the last CAP patterns, least recently used first out.  It owns nothing: whoever evicts, erases or clears destroys
// what the entry's value stands for (on_evict; erase: before the call).  An Entry* holds until the next insert or removal.
template <class V, size_t CAP = MAX_CACHED_PLANS>
struct PlanLru {
    struct Entry { PlanKey key; V value; uint64_t stamp; };
    std::vector<Entry> entries;
    uint64_t clock = 0;

    Entry* find(const PlanKey& key) {           // touches the entry
        for (Entry& e : entries)
            if (e.key == key) { e.stamp = ++clock; return &e; }
        return nullptr;
    }
    template <class F> void make_room(F on_evict) {     // for one more entry
        while (entries.size() >= CAP) {
            size_t lru = 0;
            for (size_t i = 1; i < entries.size(); ++i)
                if (entries[i].stamp < entries[lru].stamp) lru = i;
            on_evict(entries[lru].value);
            entries.erase(entries.begin() + (ptrdiff_t)lru);
        }
    }
    Entry* insert(const PlanKey& key, V value) {
        entries.push_back(Entry{key, std::move(value), ++clock});
        return &entries.back();
    }
    void erase(Entry* e) { entries.erase(entries.begin() + (e - entries.data())); }
    template <class F> void clear(F on_evict) {
        for (Entry& e : entries) on_evict(e.value);
        entries.clear();
    }
    bool empty() const { return entries.empty(); }
    typename std::vector<Entry>::iterator begin() { return entries.begin(); }
    typename std::vector<Entry>::iterator end() { return entries.end(); }
};

// The fingerprint of k_factor_hash over the caller's host array: H[s] = sum of bits(v_e) * (2 e + 1) * K over the values of panel s.
// Worker threads pull chunks of `chunk` values (32 MiB) from a counter and walk them with the supernode of the current value (one
// multiply per word: memory-bound); the per-chunk partial sums are merged under a lock.  Threads: at most 16, at most the
// hardware's, at most one per chunk; SF_VERIFY_THREADS overrides.
void host_panel_hashes(const double* Lsx, const int64_t* Lsxp, int64_t nsuper, std::vector<uint64_t>& out, int64_t chunk = (int64_t)4 << 20);

}  // namespace sf
