// Sanitizer run of the GPU-free half of the overlapped download (sf_download.h): the gate between the enqueue thread and the
// copy workers, and the unpacking of a staging slot.  On the CPU, without the HIP runtime; built twice:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=thread -static-libtsan
//       -Isparse-matrix-factorization-library_amd/csrc tools/download_sanitize.cpp -o /tmp/dl_tsan && /tmp/dl_tsan
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan
//       -Isparse-matrix-factorization-library_amd/csrc tools/download_sanitize.cpp -o /tmp/dl_asan && /tmp/dl_asan
// The workers here are dl_worker (sf_download.hip) with its HIP calls taken out: claim, drain the piece in hand before blocking,
// wait for the piece's event, take the piece in hand.  Every scenario runs under a watchdog: a lost wake-up ends the program
// with status 3 instead of hanging it.  A data race, a leak or an over-read is the sanitizer's to report; everything else is
// checked here.  Exit status 0: all held.  NOT covered: the HIP half of dl_worker (events, copies, what the copies leave in a slot).
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "sf_download.h"

static std::atomic<int> g_failed{0};
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++g_failed; } \
    } while (0)

// ends the program when a scenario does not finish in time
struct Watchdog {
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    std::thread t;
    explicit Watchdog(const char* what, int workers) {
        t = std::thread([this, what, workers] {
            std::unique_lock<std::mutex> g(mu);
            // (the system clock: its timed wait is one every ThreadSanitizer runtime knows about)
            if (!cv.wait_until(g, std::chrono::system_clock::now() + std::chrono::seconds(10), [this] { return done; })) {
                fprintf(stderr, "download_sanitize: TIMEOUT in '%s' with %d worker(s)\n", what, workers);
                _exit(3);
            }
        });
    }
    ~Watchdog() {
        { std::lock_guard<std::mutex> g(mu); done = true; }
        cv.notify_all();
        t.join();
    }
};

// ---------------------------------------------------------------- the gate ----------------------------------------------------------------
struct Run {
    sf::DlGate& gate;
    std::vector<int> ev;                    // piece -> event
    std::vector<int32_t> group;             // piece -> streamed group (-1: none)
    std::atomic<size_t> recorded{0};        // written by the publisher BEFORE gate.publish: events [0, recorded) exist
    std::unique_ptr<std::atomic<int>[]> claimed, drained;
    std::unique_ptr<std::atomic<int64_t>[]> group_drained;
    std::atomic<int> early{0}, returned_abort{0}, waiting{0};
    Run(sf::DlGate& g, size_t np, size_t ngroups) : gate(g), ev(np, 0), group(np, -1) {
        claimed.reset(new std::atomic<int>[np]);
        drained.reset(new std::atomic<int>[np]);
        for (size_t k = 0; k < np; ++k) { claimed[k].store(0); drained[k].store(0); }
        group_drained.reset(new std::atomic<int64_t>[ngroups + 1]);
        for (size_t k = 0; k <= ngroups; ++k) group_drained[k].store(0);
    }
    // dl_worker without HIP
    void worker() {
        const size_t np = ev.size();
        size_t prev = np;
        auto drain = [&] {
            if (prev == np) return;
            const size_t k = prev;
            prev = np;
            if (group[k] >= 0) ++group_drained[(size_t)group[k]];      // (before the gate hears of it)
            gate.piece_left_device(group[k]);
            ++drained[k];
        };
        for (size_t k = gate.claim(); k < np; k = gate.claim()) {
            if (prev < np && !gate.ready((size_t)ev[k])) drain();
            ++waiting;
            if (!gate.wait_ready((size_t)ev[k])) { ++returned_abort; return; }
            if (recorded.load() <= (size_t)ev[k]) ++early;
            ++claimed[k];
            drain();
            prev = k;
        }
        drain();
    }
    void publish(size_t k) { recorded.store(k); gate.publish(k); }
    void check_complete() {
        for (size_t k = 0; k < ev.size(); ++k) { CHECK(claimed[k].load() == 1); CHECK(drained[k].load() == 1); }
        CHECK(early.load() == 0 && returned_abort.load() == 0 && gate.error() == 0);
    }
};

static void join_all(std::vector<std::thread>& th) { for (std::thread& t : th) t.join(); }

// every piece once, none before its event; `jump`: the publisher records several events at a time
static void scenario_in_core(sf::DlGate& gate, int W, int jump) {
    Watchdog dog(jump > 1 ? "publish jumps" : "claim once", W);
    const size_t np = 240, ne = 80;
    Run r(gate, np, 0);
    for (size_t k = 0; k < np; ++k) r.ev[k] = (int)(k / 3);
    gate.reset({});
    std::vector<std::thread> th;
    for (int w = 0; w < W; ++w) th.emplace_back([&r] { r.worker(); });
    std::thread pub([&] {
        for (size_t k = 0; k < ne;) {
            k = std::min(ne, k + (size_t)jump);
            r.publish(k);
            if (k % 7 == 0) std::this_thread::yield();
        }
    });
    pub.join();
    join_all(th);
    r.check_complete();
}

// out of core: before group g's first launch the enqueue side waits until the pieces of the groups g - 2 .. upto[g] have left the
// device; nothing further is published until then, so a worker that kept a piece in hand while it blocked would stop everything
static void scenario_out_of_core(sf::DlGate& gate, int W) {
    Watchdog dog("out-of-core hand-off", W);
    const int G = 7;
    const std::vector<int64_t> per_group = {5, 1, 4, 6, 2, 5, 3};
    const int upto[G] = {-2, -1, 0, 2, 2, 4, 5};       // (top mode 2: groups 3 and 5 also wait for the group just before them)
    size_t np = 0;
    for (int64_t c : per_group) np += (size_t)c;
    Run r(gate, np, (size_t)G);
    for (size_t k = 0, g = 0, in_g = 0; k < np; ++k) {
        r.ev[k] = (int)g;
        r.group[k] = (int32_t)g;
        if (++in_g == (size_t)per_group[g]) { ++g; in_g = 0; }
    }
    gate.reset(per_group);
    std::vector<std::thread> th;
    for (int w = 0; w < W; ++w) th.emplace_back([&r] { r.worker(); });
    std::thread enq([&] {
        for (int g = 0; g < G; ++g) {
            const int lo = std::max(0, g - 2), hi = std::min(upto[g], g - 1);
            CHECK(gate.wait_groups(lo, hi));
            for (int w = lo; w <= hi; ++w) CHECK(r.group_drained[(size_t)w].load() == per_group[(size_t)w]);
            r.publish((size_t)g + 1);       // group g is computed: its pieces may go
        }
    });
    enq.join();
    join_all(th);
    r.check_complete();
    CHECK(gate.wait_groups(0, G - 1));      // everything has left: no wait
    CHECK(gate.wait_groups(G, G + 2));      // groups reset() was not told of have no pieces
    gate.piece_left_device(G + 1);
}

// fail() while the workers wait in wait_ready and the enqueue side in wait_groups: everyone returns, the first code is kept
static void scenario_fail(sf::DlGate& gate, int W) {
    Watchdog dog("fail", W);
    const size_t np = 64;
    Run r(gate, np, 2);
    for (size_t k = 0; k < np; ++k) { r.ev[k] = (int)(k / 2); r.group[k] = k < np / 2 ? 0 : 1; }
    gate.reset({(int64_t)np / 2, (int64_t)np / 2});
    std::vector<std::thread> th;
    for (int w = 0; w < W; ++w) th.emplace_back([&r] { r.worker(); });
    std::atomic<int> enq_state{0};
    std::thread enq([&] {
        enq_state.store(1);
        const bool ok = gate.wait_groups(0, 1);     // group 1's events are never published
        enq_state.store(ok ? 2 : 3);
    });
    r.publish(3);                                   // six pieces can go, then every worker blocks
    while (r.waiting.load() < 6 + W || enq_state.load() == 0) std::this_thread::yield();     // (np >= 6 + W: one piece each to block on)
    // (announced is not yet asleep, and nothing tells when a thread is: 20 ms for the few instructions in between.  A waiter
    // that is still awake then sees the abort in its predicate -- the scenario passes either way, only the wake-up goes untested)
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
    gate.fail(7);
    gate.fail(9);
    enq.join();
    join_all(th);
    CHECK(enq_state.load() == 3);
    CHECK(r.returned_abort.load() == W);
    CHECK(gate.error() == 7);
    CHECK(!gate.wait_ready(0) && gate.ready(1000));     // an aborted gate lets nobody sleep
    int claimed = 0;
    for (size_t k = 0; k < np; ++k) { CHECK(r.claimed[k].load() <= 1); claimed += r.claimed[k].load(); }
    CHECK(claimed == 6 && r.early.load() == 0);
}

static void test_gate() {
    for (int W : {1, 4, 16}) {
        sf::DlGate gate;        // one gate through every scenario: reset() must bring it back, also after a failed run
        scenario_in_core(gate, W, 1);
        scenario_in_core(gate, W, 5);
        scenario_out_of_core(gate, W);
        scenario_fail(gate, W);
        scenario_out_of_core(gate, W);
        scenario_in_core(gate, W, 1);
    }
}

// ---------------------------------------------------------------- the unpack ----------------------------------------------------------------
// a small LU structure: supernode 1 is square (nscol == nsrow: no U part)
static const int32_t SUPER[] = {0, 2, 5, 9};
static const int64_t LSIP[] = {0, 5, 8, 14};
static const int64_t LSXP[] = {0, 2 * (2 * 5 - 2), 2 * (2 * 5 - 2) + 3 * 3, 2 * (2 * 5 - 2) + 3 * 3 + 4 * (2 * 6 - 4)};

struct Slot {      // an exact-size heap block with distinct values: reading past its end is the sanitizer's to report
    size_t n;
    std::unique_ptr<double[]> v;
    explicit Slot(size_t n_) : n(n_), v(new double[n_]) { for (size_t i = 0; i < n; ++i) v[i] = 1000.0 + (double)i; }
};

static void compare(const DlPiece& pc, const Slot& ring, const std::vector<double>& want, int line) {
    std::vector<double> got(want.size(), std::nan(""));
    sf::dl_unpack(pc, ring.v.get(), got.data(), SUPER, LSIP, LSXP);
    if (memcmp(got.data(), want.data(), want.size() * sizeof(double)) != 0) {
        fprintf(stderr, "line %d: unpacked array differs from the element-by-element reference\n", line);
        ++g_failed;
    }
}

static void test_unpack() {
    const double nan = std::nan("");
    {   // a plain piece in the middle of the array
        DlPiece pc{0, 3, 7, 0, 0};
        Slot ring(7);
        std::vector<double> want(12, nan);
        for (int i = 0; i < 7; ++i) want[(size_t)(3 + i)] = ring.v[(size_t)i];
        compare(pc, ring, want, __LINE__);
    }
    // 2-D Cholesky pieces: rows [skip, ld) of every column travel, the prefixes are zero-filled
    for (int64_t ld : {6, 1})
        for (int64_t skip : {(int64_t)0, (int64_t)1, ld - 1})
            for (int64_t ncols : {1, 3}) {
                if (skip < 0 || skip >= ld) continue;
                const int64_t rows = ld - skip, host_off = 2;
                DlPiece pc{0, host_off, ncols * rows, 0, 0};
                pc.skip = skip; pc.ld = ld; pc.ncols = ncols;
                Slot ring((size_t)(ncols * rows));
                std::vector<double> want((size_t)(host_off + ncols * ld + 3), nan);
                for (int64_t c = 0; c < ncols; ++c)
                    for (int64_t i = 0; i < ld; ++i)
                        want[(size_t)(host_off + c * ld + i)] = i < skip ? 0.0 : ring.v[(size_t)(c * rows + i - skip)];
                compare(pc, ring, want, __LINE__);
            }
    {   // LU direct, whole supernodes 0 and 1: ring = [ L panels | U^T panels ], each as on the device (nsrow x nscol)
        int64_t devL = 0;
        for (int s = 0; s < 2; ++s) devL += (LSIP[s + 1] - LSIP[s]) * (SUPER[s + 1] - SUPER[s]);
        DlPiece pc{0, LSXP[0], LSXP[2] - LSXP[0], 0, 0};
        pc.s0 = 0; pc.s1 = 2; pc.dev_count = devL;
        Slot ring((size_t)(2 * devL));
        std::vector<double> want((size_t)LSXP[3], nan);
        int64_t base = 0;
        for (int s = 0; s < 2; ++s) {
            const int64_t nscol = SUPER[s + 1] - SUPER[s], nsrow = LSIP[s + 1] - LSIP[s], lda = 2 * nsrow - nscol;
            for (int64_t c = 0; c < nscol; ++c)
                for (int64_t i = 0; i < lda; ++i)
                    want[(size_t)(LSXP[s] + c * lda + i)] = i < nsrow ? ring.v[(size_t)(base + c * nsrow + i)]
                                                                      : ring.v[(size_t)(devL + base + c * nsrow + nscol + (i - nsrow))];
            base += nscol * nsrow;
        }
        compare(pc, ring, want, __LINE__);
    }
    {   // LU direct, columns [1, 3) of supernode 2: the L columns whole, of the U^T columns only rows [nscol, nsrow)
        const int s = 2;
        const int64_t nscol = SUPER[s + 1] - SUPER[s], nsrow = LSIP[s + 1] - LSIP[s], nb = nsrow - nscol, lda = nsrow + nb;
        const int64_t j0 = 1, ncols = 2;
        DlPiece pc{j0 * nsrow, LSXP[s] + j0 * lda, ncols * lda, 0, 0};
        pc.s0 = s; pc.s1 = s + 1; pc.j0 = j0; pc.ncols = ncols; pc.ld = nsrow; pc.dev_count = ncols * nsrow;
        Slot ring((size_t)(ncols * nsrow + ncols * nb));
        std::vector<double> want((size_t)LSXP[3], nan);
        for (int64_t c = 0; c < ncols; ++c)
            for (int64_t i = 0; i < lda; ++i)
                want[(size_t)(LSXP[s] + (j0 + c) * lda + i)] = i < nsrow ? ring.v[(size_t)(c * nsrow + i)]
                                                                         : ring.v[(size_t)(ncols * nsrow + c * nb + (i - nsrow))];
        compare(pc, ring, want, __LINE__);
    }
}

int main() {
    test_unpack();
    test_gate();
    if (g_failed.load()) { fprintf(stderr, "download_sanitize: %d check(s) failed\n", g_failed.load()); return 1; }
    printf("download_sanitize: ok\n");
    return 0;
}
