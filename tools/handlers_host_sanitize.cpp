// The host-only parts of the struct path's handlers without a device, under ASan + UBSan (tests/test_handlers_host.py
// builds this file with csrc/sf_plan_cache.cpp, sf_placement.cpp and sf_symbolic.cpp): the pattern key, the LRU plan cache, the
// in-core / out-of-core decision against values derived here from its formula, the retry ladder round plan creation against exact
// call traces of a scripted environment, and the host fingerprints against their definition.  Prints "handlers_host_sanitize: ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "sf_placement.h"
#include "sf_plan_cache.h"
#include "sf_symbolic.h"

using sf::Long;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "handlers_host_sanitize: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

namespace {

// ---- a small pattern: the 5-point stencil on a g x g grid, as the lower triangle or as a whole matrix with entries dropped ----
void analyze(Long g, bool lu, sf::Symbolic& S) {
    std::vector<Long> p{0}, i;
    std::vector<double> x;
    for (Long y = 0; y < g; ++y) for (Long c = 0; c < g; ++c) {
        const Long j = c + g * y;
        auto put = [&](Long r, double v) { i.push_back(r); x.push_back(v); };
        if (lu) {                       // entries above the diagonal, some dropped: the pattern of U differs from L's
            if (y > 0) put(j - g, -1.0);
            if (c > 0 && j % 3 != 0) put(j - 1, -1.0);
        }
        put(j, 4.5);
        if (c + 1 < g) put(j + 1, -1.0);
        if (y + 1 < g) put(j + g, -1.0);
        p.push_back((Long)i.size());
    }
    std::vector<Long> perm((size_t)(g * g));
    int rc = sf::grid_nd_perm(g, g, 1, 3, 1, perm.data());
    if (!rc) rc = lu ? sf::analyze_lu(g * g, p.data(), i.data(), x.data(), perm.data(), (size_t)1 << 30, false, S)
                     : sf::analyze_cholesky(g * g, p.data(), i.data(), x.data(), perm.data(), (size_t)1 << 30, S);
    REQUIRE(rc == 0 && S.nsuper > 1);
}

// the arrays a test may change, and the PlanInput over them
struct Arrays {
    bool lu = false;
    Long n = 0, nsuper = 0;
    std::vector<Long> Super, SuperMap, Lsip, Lsi, Lsxp, Lp, Li, Up, Ui;
    explicit Arrays(const sf::Symbolic& S)
        : lu(S.lu), n(S.n), nsuper(S.nsuper), Super(S.Super), SuperMap(S.SuperMap), Lsip(S.Lsip), Lsi(S.Lsi.begin(), S.Lsi.end()), Lsxp(S.Lsxp),
          Lp(S.Lp), Li(S.Li.begin(), S.Li.end()), Up(S.Up), Ui(S.Ui.begin(), S.Ui.end()) {}
    Arrays() = default;
    PlanInput input() const {
        PlanInput in;
        in.lu = lu; in.n = n; in.nsuper = nsuper;
        in.Super = Super.data(); in.SuperMap = SuperMap.data(); in.Lsip = Lsip.data(); in.Lsi = Lsi.data(); in.Lsxp = Lsxp.data();
        in.Lp = Lp.data(); in.Li = Li.data();
        if (lu && !Up.empty()) { in.Up = Up.data(); in.Ui = Ui.data(); }
        return in;
    }
};

// ---- the key ----
void test_hash_words() {
    for (int64_t len = 0; len <= 9; ++len) {        // the four-lane body and the tail
        std::vector<int64_t> a((size_t)len);
        for (int64_t k = 0; k < len; ++k) a[(size_t)k] = 1000 + 7 * k;
        const uint64_t h = sf::hash_words(a.data(), len, 11);
        REQUIRE(h == sf::hash_words(a.data(), len, 11) && h != sf::hash_words(a.data(), len, 13));
        for (int64_t k = 0; k < len; ++k) {
            std::vector<int64_t> b = a;
            b[(size_t)k] ^= 1;
            REQUIRE(sf::hash_words(b.data(), len, 11) != h);
        }
        if (len > 0) REQUIRE(sf::hash_words(a.data(), len - 1, 11) != h);
    }
}

void test_key(const sf::Symbolic& S) {
    const Arrays A(S);
    const sf::PlanKey k0 = sf::make_key(A.input());
    const Arrays same(S);
    REQUIRE(sf::make_key(same.input()) == k0);
    REQUIRE(k0.n == S.n && k0.nsuper == S.nsuper && k0.isize == S.Lsip[(size_t)S.nsuper] && k0.xsize == S.Lsxp[(size_t)S.nsuper] && k0.nnz == S.Lp[(size_t)S.n]);
    REQUIRE(k0.lu == (S.lu ? 1 : 0) && k0.unz == (S.lu ? S.Up[(size_t)S.n] : 0));
    // one word of one array, one less (a smaller last pointer shortens what is hashed, it never reads past an array)
    std::vector<Long> Arrays::*members[] = {&Arrays::Super, &Arrays::Lsip, &Arrays::Lsxp, &Arrays::Lp, &Arrays::Lsi, &Arrays::Li, &Arrays::Up, &Arrays::Ui};
    for (auto m : members) {
        REQUIRE(S.lu || (A.*m).size() > 0 || m == &Arrays::Up || m == &Arrays::Ui);
        for (size_t w = 0; w < (A.*m).size(); ++w) {
            Arrays B = A;
            (B.*m)[w] -= 1;
            REQUIRE(!(sf::make_key(B.input()) == k0));
        }
    }
    Arrays B = A;           // the same arrays as the other kind of factor (Cholesky: without Up / Ui, as the struct path gives them)
    B.lu = !A.lu;
    REQUIRE(!(sf::make_key(B.input()) == k0));
}

// ---- the LRU cache ----
void test_lru() {
    sf::PlanKey A, B, C;
    A.h = 1; B.h = 2; C.h = 3;
    sf::PlanLru<int, 2> lru;
    std::vector<int> evicted;
    auto on_evict = [&](int v) { evicted.push_back(v); };
    REQUIRE(lru.empty() && !lru.find(A));
    lru.make_room(on_evict);
    REQUIRE(evicted.empty());
    lru.insert(A, 10);
    lru.make_room(on_evict);
    lru.insert(B, 20);
    REQUIRE(evicted.empty() && lru.find(A) && lru.find(A)->value == 10);       // A is now the newer one
    lru.make_room(on_evict);
    REQUIRE(evicted == std::vector<int>{20} && !lru.find(B) && lru.find(A));
    auto* e = lru.insert(C, 30);           // a build that fails afterwards: the entry goes, nobody's callback runs
    REQUIRE(e->value == 30 && lru.find(C) == e);
    lru.erase(e);
    REQUIRE(!lru.find(C) && lru.find(A) && evicted.size() == 1);
    lru.insert(B, 21);
    int seen = 0;
    for (auto& en : lru) seen += en.value;
    REQUIRE(seen == 31);
    evicted.clear();
    lru.clear(on_evict);
    REQUIRE(lru.empty() && evicted.size() == 2 && evicted[0] + evicted[1] == 31 && !lru.find(A));
}

// ---- decide_placement ----
constexpr int64_t MiB = (int64_t)1 << 20, GiB = (int64_t)1 << 30;
struct Sizes { int64_t entries, per_entry, overhead; };
Sizes sizes_of(const PlanInput& in) {          // the formula
    Sizes z{0, in.lu ? 16 : 8, 0};
    for (Long s = 0; s < in.nsuper; ++s) z.entries += (in.Super[s + 1] - in.Super[s]) * (in.Lsip[s + 1] - in.Lsip[s]);
    z.overhead = 12 * in.Lp[in.n] + (in.lu && in.Up ? 12 * in.Up[in.n] : 0) + 24 * in.Lsip[in.nsuper] + 384 * MiB;
    return z;
}
struct FreeMem {        // the device's answer, and how often it was asked
    int64_t bytes = 0;
    bool ok = true;
    int calls = 0;
    std::function<bool(size_t&)> fn() { return [this](size_t& fr) { ++calls; fr = (size_t)bytes; return ok; }; }
};
// what the partition itself says to a budget of panel entries
struct Cut { int rc, ngroups, mode; std::vector<int32_t> group; };
Cut partition(const PlanInput& in, int64_t budget_entries) {
    Cut c{0, 0, 0, std::vector<int32_t>((size_t)in.nsuper, 0)};
    int64_t ge = 0, te = 0, nd = 0;
    c.rc = sf::ooc_partition(in.nsuper, in.Super, in.SuperMap, in.Lsip, in.Lsi, budget_entries, c.group.data(), &c.ngroups, &ge, &te, &nd, &c.mode);
    return c;
}

void test_decide_small(const sf::Symbolic& S) {
    const Arrays A(S);
    const PlanInput in = A.input();
    const Sizes z = sizes_of(in);
    REQUIRE(z.entries > 0 && z.entries * z.per_entry < 64 * MiB && (in.Up != nullptr) == S.lu);
    FreeMem fm;
    sf::Placement pl;
    // small panels, no environment budget: in core without asking (even of a device that would say no)
    fm.ok = false;
    pl.ngroups = 7;
    REQUIRE(sf::decide_placement(in, 1.0, 0, fm.fn(), 0, false, pl) == SF_OK && pl.ngroups == 1 && fm.calls == 0);
    // environment budget: the boundary, exactly
    const int64_t fits = z.entries * z.per_entry + z.overhead;
    REQUIRE(sf::decide_placement(in, 1.0, fits, fm.fn(), 0, false, pl) == SF_OK && pl.ngroups == 1 && fm.calls == 0);
    const int64_t be = (fits - 1 - z.overhead) / z.per_entry;
    REQUIRE(be == z.entries - 1);
    const Cut c = partition(in, be);
    REQUIRE(c.rc == 0 && c.ngroups > 1);
    REQUIRE(sf::decide_placement(in, 1.0, fits - 1, fm.fn(), 0, false, pl) == SF_OK && fm.calls == 0);
    REQUIRE(pl.ngroups == c.ngroups && pl.ngroups > 1 && pl.top_mode == c.mode && pl.group == c.group);
    // shrink scales the environment budget too: 0.5 of twice-what-fits less two bytes is one byte short
    REQUIRE(sf::decide_placement(in, 0.5, 2 * fits, fm.fn(), 0, false, pl) == SF_OK && pl.ngroups == 1);
    REQUIRE(sf::decide_placement(in, 0.5, 2 * fits - 2, fm.fn(), 0, false, pl) == SF_OK && pl.ngroups == c.ngroups);
    // nothing left for panels
    REQUIRE(sf::decide_placement(in, 1.0, z.overhead, fm.fn(), 0, false, pl) == SF_ERR_ALLOC);
    REQUIRE(sf::decide_placement(in, 1.0, z.overhead + z.per_entry - 1, fm.fn(), 0, false, pl) == SF_ERR_ALLOC);
    // room for one panel entry: below the largest single group, the partition's "does not fit" (its line on stderr is expected)
    REQUIRE(partition(in, 1).rc == 2);
    REQUIRE(sf::decide_placement(in, 1.0, z.overhead + z.per_entry, fm.fn(), 0, false, pl) == SF_ERR_ALLOC);
    REQUIRE(fm.calls == 0);
}

// one wide supernode (a dense front of w columns): panels above the 64 MiB shortcut, nothing allocated but the index arrays
Arrays wide_front(Long w, bool lu) {
    Arrays A;
    A.lu = lu; A.n = w; A.nsuper = 1;
    A.Super = {0, w}; A.Lsip = {0, w}; A.Lsxp = {0, lu ? w * w : w * w};
    A.SuperMap.assign((size_t)w, 0);
    A.Lsi.resize((size_t)w);
    for (Long r = 0; r < w; ++r) A.Lsi[(size_t)r] = r;
    A.Lp.assign((size_t)w + 1, 0);
    for (Long j = 0; j <= w; ++j) A.Lp[(size_t)j] = 3 * j;      // (only Lp[n] is read)
    A.Li.assign((size_t)(3 * w), 0);
    if (lu) { A.Up = A.Lp; A.Up[(size_t)w] = 2 * w; A.Ui.assign((size_t)(2 * w), 0); }
    return A;
}

void test_decide_free_memory(bool lu) {
    const Arrays A = wide_front(4096, lu);
    const PlanInput in = A.input();
    const Sizes z = sizes_of(in);
    const int64_t panels = z.entries * z.per_entry, need = panels + 16;
    REQUIRE(z.entries == 4096 * 4096 && panels >= 64 * MiB && z.overhead == 12 * 3 * 4096 + (lu ? 12 * 2 * 4096 : 0) + 24 * 4096 + 384 * MiB);
    FreeMem fm;
    sf::Placement pl;
    // the device is asked; 1 GiB of what it reports is left alone
    fm.bytes = GiB + panels + z.overhead;
    REQUIRE(sf::decide_placement(in, 1.0, 0, fm.fn(), 0, false, pl) == SF_OK && pl.ngroups == 1 && fm.calls == 1);
    // an environment budget answers instead
    REQUIRE(sf::decide_placement(in, 1.0, panels + z.overhead, fm.fn(), 0, false, pl) == SF_OK && pl.ngroups == 1 && fm.calls == 1);
    // a device that does not answer
    fm.ok = false;
    REQUIRE(sf::decide_placement(in, 1.0, 0, fm.fn(), 0, false, pl) == SF_ERR_HIP && fm.calls == 2);
    fm.ok = true;
    // the pool credit, only when the factor fits the idle pool: free - 1 GiB = overhead - 16 is in core, exactly, with the credit
    // of panels + 16, and leaves nothing for panels without it
    fm.bytes = GiB + z.overhead - 16;
    REQUIRE(sf::decide_placement(in, 1.0, 0, fm.fn(), (size_t)need, false, pl) == SF_OK && pl.ngroups == 1);
    REQUIRE(sf::decide_placement(in, 1.0, 0, fm.fn(), (size_t)need - 1, false, pl) == SF_ERR_ALLOC);
    REQUIRE(sf::decide_placement(in, 1.0, 0, fm.fn(), 0, false, pl) == SF_ERR_ALLOC);
    fm.bytes -= 1;
    REQUIRE(sf::decide_placement(in, 1.0, 0, fm.fn(), (size_t)need, false, pl) != SF_OK || pl.ngroups > 1);
    // shrink multiplies AFTER the credit: with base = free - 1 GiB, (base + need) * 0.8 is short of panels + overhead where
    // base * 0.8 + need would not be.  What the partition then makes of (budget - overhead) / per_entry entries is the answer.
    const int64_t base = (int64_t)std::ceil((double)z.overhead / 0.8);
    REQUIRE((int64_t)((double)base * 0.8) + need >= panels + z.overhead);
    const int64_t budget = (int64_t)((double)(base + need) * 0.8);
    REQUIRE(budget < panels + z.overhead && budget > z.overhead);
    fm.bytes = GiB + base;
    const Cut c = partition(in, (budget - z.overhead) / z.per_entry);
    const int want = c.rc == 0 ? SF_OK : (c.rc == 2 ? SF_ERR_ALLOC : SF_ERR_ARG);
    const int got = sf::decide_placement(in, 0.8, 0, fm.fn(), (size_t)need, false, pl);
    REQUIRE(got == want && (got != SF_OK || (pl.ngroups == c.ngroups && pl.ngroups > 1)));
    REQUIRE(sf::decide_placement(in, 1.0, 0, fm.fn(), (size_t)need, false, pl) == SF_OK && pl.ngroups == 1);      // (in core unshrunk)
}

// ---- place_and_create: a scripted environment that records the calls ----
struct Script {
    struct Decision { int rc, ngroups; };
    std::vector<Decision> decisions;        // in the order asked for
    std::vector<int> creations;
    int cached = 0;                         // other plans in the handler's cache
    enum Pool { NONE, IDLE, USED_BY_CACHED } pool = NONE;
    bool budget_set = false;
    std::string trace;
    size_t nd = 0, nc = 0;

    void say(const std::string& w) { trace += (trace.empty() ? "" : " ") + w; }
    int decide(double shrink, sf::Placement& pl) {
        char buf[32];
        snprintf(buf, sizeof buf, "decide(%.2f)", shrink);
        say(buf);
        REQUIRE(nd < decisions.size());
        pl.ngroups = decisions[nd].ngroups;
        return decisions[nd++].rc;
    }
    int create(const sf::Placement&) { say("create"); REQUIRE(nc < creations.size()); return creations[nc++]; }
    bool cache_empty() const { return cached == 0; }
    void drop_cache() { say("drop_cache"); cached = 0; if (pool == USED_BY_CACHED) pool = IDLE; }
    bool pool_idle() const { return pool == IDLE; }
    void release_pool() { say("release_pool"); REQUIRE(pool == IDLE); pool = NONE; }
    bool env_budget_set() const { return budget_set; }
    void device_sync() { say("sync"); }
    void clear_error() { say("clear"); }
};
void expect(const char* name, Script s, int want_rc, const std::string& want_trace) {
    sf::Placement pl;
    const int rc = sf::place_and_create(s, pl);
    if (rc != want_rc || s.trace != want_trace || s.nd != s.decisions.size() || s.nc != s.creations.size()) {
        fprintf(stderr, "handlers_host_sanitize: ladder %s: rc %d (want %d)\n  got  %s\n  want %s\n", name, rc, want_rc, s.trace.c_str(), want_trace.c_str());
        exit(1);
    }
}

void test_ladder() {
    const Script::Decision in_core{SF_OK, 1}, ooc{SF_OK, 3}, no_fit{SF_ERR_ALLOC, 1};
    const int OK = SF_OK, ALLOC = SF_ERR_ALLOC, HIP = SF_ERR_HIP;
    Script s;
    s = Script(); s.decisions = {in_core}; s.creations = {OK};
    expect("a", s, OK, "decide(1.00) create");
    s = Script(); s.decisions = {ooc, in_core}; s.creations = {OK}; s.cached = 1; s.pool = Script::IDLE;
    expect("b", s, OK, "decide(1.00) drop_cache sync decide(1.00) create");
    s.decisions = {ooc, ooc, ooc};
    expect("c", s, OK, "decide(1.00) drop_cache sync decide(1.00) release_pool decide(1.00) create");
    s = Script(); s.decisions = {ooc}; s.creations = {OK}; s.cached = 1; s.pool = Script::IDLE; s.budget_set = true;
    expect("d", s, OK, "decide(1.00) create");
    s = Script(); s.decisions = {in_core, in_core}; s.creations = {ALLOC, OK}; s.cached = 1;
    expect("e", s, OK, "decide(1.00) create drop_cache clear decide(1.00) create");
    s.creations = {HIP, OK};         // (SF_ERR_HIP from a creation is an allocation failure too)
    expect("e, SF_ERR_HIP", s, OK, "decide(1.00) create drop_cache clear decide(1.00) create");
    s = Script(); s.decisions = {in_core, in_core, in_core}; s.creations = {ALLOC, ALLOC, OK}; s.cached = 1; s.pool = Script::USED_BY_CACHED;
    expect("f", s, OK, "decide(1.00) create drop_cache clear decide(1.00) create release_pool clear decide(1.00) create");
    s = Script(); s.decisions = {in_core, in_core, in_core}; s.creations = {ALLOC, ALLOC, ALLOC};
    expect("g", s, ALLOC, "decide(1.00) create clear decide(0.80) create clear decide(0.65) create");
    s.decisions = {in_core, ooc}; s.creations = {ALLOC, OK};
    expect("g, the first cut is enough", s, OK, "decide(1.00) create clear decide(0.80) create");
    s = Script(); s.decisions = {in_core, in_core, in_core}; s.creations = {HIP, HIP, HIP}; s.cached = 1; s.pool = Script::IDLE;
    expect("h", s, HIP, "decide(1.00) create drop_cache clear decide(1.00) create release_pool clear decide(1.00) create");
    s = Script(); s.decisions = {in_core}; s.creations = {HIP};
    expect("h, nothing to give up", s, HIP, "decide(1.00) create");
    s = Script(); s.decisions = {in_core, {SF_ERR_ARG, 1}}; s.creations = {ALLOC};
    expect("i", s, ALLOC, "decide(1.00) create clear decide(0.80)");
    s = Script(); s.decisions = {ooc, ooc, ooc}; s.creations = {OK}; s.cached = 2; s.pool = Script::USED_BY_CACHED;
    expect("j", s, OK, "decide(1.00) drop_cache sync decide(1.00) release_pool decide(1.00) create");
    s.decisions = {ooc, in_core};
    expect("j, in core after the drop", s, OK, "decide(1.00) drop_cache sync decide(1.00) create");
    // a decision that fails is not followed by a creation; SF_ERR_ALLOC from it goes on to the cuts, anything else is returned
    s = Script(); s.decisions = {no_fit, no_fit};
    expect("no decision fits", s, ALLOC, "decide(1.00) clear decide(0.80)");
    s = Script(); s.decisions = {no_fit, in_core}; s.creations = {OK}; s.pool = Script::IDLE;
    expect("the pool goes for the decision", s, OK, "decide(1.00) release_pool decide(1.00) create");
    s = Script(); s.decisions = {{SF_ERR_ARG, 1}}; s.budget_set = true; s.cached = 1;
    expect("a refused structure", s, SF_ERR_ARG, "decide(1.00)");
    s = Script(); s.decisions = {in_core, {HIP, 1}}; s.creations = {ALLOC}; s.cached = 1;
    expect("the second decision fails", s, HIP, "decide(1.00) create drop_cache clear decide(1.00)");
}

// ---- host_panel_hashes ----
double from_bits(uint64_t u) { double d; memcpy(&d, &u, sizeof d); return d; }
void test_panel_hashes() {
    const std::vector<int64_t> lens{1, 6, 7, 8, 20, 0, 3};
    std::vector<int64_t> Lsxp{0};
    for (int64_t l : lens) Lsxp.push_back(Lsxp.back() + l);
    const int64_t total = Lsxp.back(), nsuper = (int64_t)lens.size();
    std::vector<double> v((size_t)total);
    for (int64_t e = 0; e < total; ++e) v[(size_t)e] = 1.0 / (double)(3 + e) - 0.125 * (double)(e % 5);
    v[0] = std::numeric_limits<double>::quiet_NaN();
    v[6] = -0.0;                                                        // the last value of a chunk
    v[7] = std::numeric_limits<double>::denorm_min();                   // the first of the next
    v[13] = from_bits(0x000fffffffffffffull);                           // the largest denormal
    v[21] = from_bits(0xfff8000000000001ull);                           // a NaN with a payload and a sign
    v[(size_t)total - 1] = -std::numeric_limits<double>::infinity();
    std::vector<uint64_t> want((size_t)nsuper, 0);
    const uint64_t K = 0x9E3779B97F4A7C15ull;
    for (int64_t s = 0; s < nsuper; ++s)
        for (int64_t e = Lsxp[(size_t)s]; e < Lsxp[(size_t)s + 1]; ++e) {
            uint64_t bits;
            memcpy(&bits, &v[(size_t)e], sizeof bits);
            want[(size_t)s] += bits * (2 * (uint64_t)e + 1) * K;
        }
    REQUIRE(want[5] == 0 && want[0] != 0);
    for (const char* threads : {"1", "3"}) {
        setenv("SF_VERIFY_THREADS", threads, 1);
        std::vector<uint64_t> got{99};
        sf::host_panel_hashes(v.data(), Lsxp.data(), nsuper, got, 7);
        REQUIRE(got == want);
        sf::host_panel_hashes(v.data(), Lsxp.data(), nsuper, got);      // one chunk of the default length
        REQUIRE(got == want);
    }
    unsetenv("SF_VERIFY_THREADS");
    std::vector<uint64_t> got{99, 98};
    sf::host_panel_hashes(v.data(), Lsxp.data(), nsuper, got, 5);      // the hardware's thread count
    REQUIRE(got == want);
    sf::host_panel_hashes(nullptr, nullptr, 0, got, 7);
    REQUIRE(got == std::vector<uint64_t>{0});
}

}  // namespace

int main() {
    sf::Symbolic chol, lu, chol24, lu24;
    analyze(9, false, chol);
    analyze(9, true, lu);
    analyze(24, false, chol24);     // (9 x 9 is three supernodes: the partition finds no cut; 24 x 24 has 19)
    analyze(24, true, lu24);
    REQUIRE(!chol.lu && lu.lu && !lu.symmetric && !lu.Up.empty() && !lu.Ui.empty());
    test_hash_words();
    test_key(chol);
    test_key(lu);
    test_lru();
    test_decide_small(chol24);
    test_decide_small(lu24);
    test_decide_free_memory(false);
    test_decide_free_memory(true);
    test_ladder();
    test_panel_hashes();
    printf("handlers_host_sanitize: ok\n");
    return 0;
}
