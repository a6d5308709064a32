// The hashing loops of sf_plan_cache.h: the key of a sparsity pattern and the host side of the per-panel fingerprints.  Plain C++
// without HIP; the library takes it from hipcc's host compiler, which compiled these loops while they stood in sf_handlers.hip.
#include "sf_plan_cache.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <thread>

namespace sf {

uint64_t hash_words(const int64_t* a, int64_t n, uint64_t seed) {
    const uint64_t M = 0x9E3779B97F4A7C15ull;
    uint64_t h0 = seed ^ 0x1234567ull, h1 = seed + 0x9abcdefull, h2 = ~seed, h3 = seed * M;
    int64_t i = 0;
    for (; i + 4 <= n; i += 4) {
        h0 = (h0 ^ (uint64_t)a[i]) * M;     h0 ^= h0 >> 29;
        h1 = (h1 ^ (uint64_t)a[i + 1]) * M; h1 ^= h1 >> 31;
        h2 = (h2 ^ (uint64_t)a[i + 2]) * M; h2 ^= h2 >> 27;
        h3 = (h3 ^ (uint64_t)a[i + 3]) * M; h3 ^= h3 >> 33;
    }
    for (; i < n; ++i) { h0 = (h0 ^ (uint64_t)a[i]) * M; h0 ^= h0 >> 29; }
    uint64_t h = h0;
    h = (h ^ h1) * M; h ^= h >> 32;
    h = (h ^ h2) * M; h ^= h >> 32;
    h = (h ^ h3) * M; h ^= h >> 32;
    return h;
}

PlanKey make_key(const PlanInput& in) {
    PlanKey k;
    k.lu = in.lu; k.n = in.n; k.nsuper = in.nsuper; k.isize = in.Lsip[in.nsuper]; k.xsize = in.Lsxp[in.nsuper]; k.nnz = in.Lp[in.n];
    k.unz = (in.lu && in.Up) ? in.Up[in.n] : 0;
    uint64_t hl = 0, hi = 0, hu = 0;
    std::thread t1([&] { hl = hash_words(in.Lsi, k.isize, 11); });
    std::thread t2([&] { hi = hash_words(in.Li, k.nnz, 13); });
    std::thread t3([&] { if (k.unz) hu = hash_words(in.Ui, k.unz, 17) ^ hash_words(in.Up, in.n + 1, 19); });
    uint64_t h = hash_words(in.Super, in.nsuper + 1, 1);
    h ^= hash_words(in.Lsip, in.nsuper + 1, 3) * 3;
    h ^= hash_words(in.Lsxp, in.nsuper + 1, 5) * 5;
    h ^= hash_words(in.Lp, in.n + 1, 7) * 7;
    t1.join(); t2.join(); t3.join();
    k.h = h ^ (hl * 11) ^ (hi * 13) ^ (hu * 17);
    return k;
}

void host_panel_hashes(const double* Lsx, const int64_t* Lsxp, int64_t nsuper, std::vector<uint64_t>& out, int64_t chunk) {
    out.assign((size_t)std::max<int64_t>(nsuper, 1), 0);
    const int64_t total = nsuper > 0 ? Lsxp[nsuper] : 0;
    if (total <= 0) return;
    const int64_t nch = (total + chunk - 1) / chunk;
    int T = (int)std::min<int64_t>(nch, std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
    if (const char* e = getenv("SF_VERIFY_THREADS")) T = std::max(1, std::min(64, atoi(e)));
    std::atomic<int64_t> next{0};
    std::mutex mu;
    auto work = [&] {
        std::vector<std::pair<int64_t, uint64_t>> loc;
        const uint64_t K = 0x9E3779B97F4A7C15ull;
        for (int64_t c = next.fetch_add(1); c < nch; c = next.fetch_add(1)) {
            const int64_t b = c * chunk, e_end = std::min(total, b + chunk);
            int64_t s = std::upper_bound(Lsxp, Lsxp + nsuper + 1, b) - Lsxp - 1;
            int64_t e = b;
            while (e < e_end) {
                while (e >= Lsxp[s + 1]) ++s;
                const int64_t stop = std::min(e_end, Lsxp[s + 1]);
                uint64_t acc = 0, m = (2ull * (uint64_t)e + 1ull) * K;
                typedef uint64_t __attribute__((may_alias)) bits64;            // the doubles' bit patterns
                const bits64* w = reinterpret_cast<const bits64*>(Lsx);
                for (; e < stop; ++e, m += 2ull * K) acc += w[e] * m;
                if (acc) loc.emplace_back(s, acc);
            }
        }
        std::lock_guard<std::mutex> g(mu);
        for (auto& pr : loc) out[(size_t)pr.first] += pr.second;
    };
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back(work);
    work();
    for (std::thread& t : th) t.join();
}

}  // namespace sf
