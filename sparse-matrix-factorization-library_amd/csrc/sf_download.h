// The GPU-free half of the overlapped download (sf_chol_plan_factorize_to_host): what a piece is, the gate through
// which the enqueue thread and the copy workers talk, and the unpacking of a staging slot into the caller's array.  No HIP here:
// tools/download_sanitize.cpp builds this header alone with a host compiler, under ThreadSanitizer and under ASan + UBSan.
// The HIP half -- events, copies, the workers themselves -- is sf_download.hip.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

// Overlapped copy-back of the factor (the reference overlaps the D2H of finished blocks with compute on
// s_cudaStream_copyback, C:2888-2895).  A piece is a run of finished panel columns that is contiguous in
// the host layout (and, for Cholesky, in the device layout), at most DL_SLOT doubles; it may be copied once launch
// `ready` - 1 has completed (event `ev`).  Pieces are sorted by `ready`.
constexpr int64_t DL_SLOT_DEFAULT = (int64_t)4 << 20;   // doubles per staging slot (32 MiB)
constexpr int DL_WORKERS_DEFAULT = 4;                   // copy workers: own HIP stream + 2 pinned slots each.  4 = the number of hardware
                                                        // queues the runtime gives the ordinary-priority streams: with 6 two pairs of
                                                        // workers share a queue and the struct call at 128^3 takes 553-603 ms instead of
                                                        // 552-568 (profiles/r02_f_struct_slow_mode.txt, part 5)
constexpr int DL_WORKERS_FRESH = 6;
constexpr int DL_WORKERS_MAX = 16;                      // SF_DL_WORKERS / SF_DL_SLOT_MB (read at plan creation) tune both
struct DlPiece {
    int64_t dev_off, host_off, count;   // doubles; LU: dev_off unused (the piece is packed from the (L, U^T) panels)
    size_t ready;
    int ev;
    // Cholesky block columns right of the first one: the rows above the block's first column are structurally zero (never written on
    // the device either), so only rows [skip, ld) of each of the `ncols` columns cross PCIe (count = ncols * (ld - skip), a 2-D
    // copy) and the host side zero-fills the prefixes.  ld == 0: a plain contiguous piece.
    int64_t skip = 0, ld = 0, ncols = 0;
    // LU (direct form, no pack kernel): the piece is the columns [j0, j0 + ncols) of supernode s0 (s1 == s0 + 1, ld = nsrow: the
    // L part is one contiguous run of the L panel, the U part -- rows [nscol, nsrow) of the same columns of the U^T panel -- a 2-D
    // copy) or the whole supernodes [s0, s1) (ld == 0: both panels' runs copied as they are, dev_count doubles each); the copy
    // worker interleaves the columns into the reference layout (L:2514-2517).  s0 < 0: not an LU-direct piece.
    int32_t s0 = -1, s1 = -1;
    int64_t j0 = 0, dev_count = 0;
    int32_t group = -1;     // out-of-core plans: the streamed group the piece belongs to (-1: a top panel)
};

namespace sf {

// The download's schedule and knobs: what schedule_download (sf_schedule.cpp) builds once per plan.  SfDownload
// (sf_plan_internal.h) derives from it and adds the fill tiles' device copy and the state of a running download.
struct DlSchedule {
    std::vector<DlPiece> pieces;
    std::vector<size_t> ev_ready;               // launch count after which event k is recorded
    std::vector<int64_t> group_pieces;          // out-of-core plans: pieces per streamed group (what the gate counts down)
    // LU direct download: before a piece's event is recorded, the upper triangle (with the diagonal) of its columns' part of the
    // supernode's diagonal block is filled into the L panel from the U^T panel (k_lu_fill_u11), so that the L panel holds the
    // reference's packed L11 \ U11 and the download needs no gather kernel
    bool lu_direct = false;
    std::vector<int64_t> fill_first;            // tiles of event k: [fill_first[k], fill_first[k + 1])
    // ---- the knobs (SF_DL_SLOT_MB, SF_DL_WORKERS, SF_DL_HOST_WAIT; read at plan creation) ----
    int64_t slot = DL_SLOT_DEFAULT;
    int workers = DL_WORKERS_DEFAULT;
    int workers_fresh = DL_WORKERS_FRESH;       // ... when the destination's pages have never been touched (sf_dl_begin)
    bool host_wait = true;                      // copy workers wait for a piece's event on the host (see dl_worker)
};

// The one meeting point of a download's threads: the thread that enqueues the factorization (it records the pieces' events and
// publishes them; in an out-of-core plan it also waits until a group's pieces have left the device before it re-uses the group's
// buffer) and the copy workers (they claim pieces, wait for a piece's event to be published, and count pieces off their groups).
//
// The rule, written once: EVERY field that a waiter's predicate reads -- published, abort, left[] -- is written with `mu` held, and
// every such write that can turn a predicate true is followed by notify_all after the lock is dropped.  A waiter tests its
// predicate under `mu` (condition_variable::wait), so a write either comes before the test and is seen, or after the waiter
// sleeps and its notify wakes it: no wake-up is lost.  (A field written outside `mu`, atomic or not, would break this: the waiter
// may test, the writer write and notify, and the waiter then go to sleep.)  Only `next` is touched outside the mutex: nobody
// waits for it.  One gate serves one download at a time; reset() is called with no worker alive.
class DlGate {
    std::mutex mu;
    std::condition_variable cv;
    size_t published = 0;               // events [0, published) have been recorded
    bool abort = false;
    int err = 0;                        // the first code given to fail()
    std::vector<int64_t> left;          // out-of-core plans: per streamed group, the pieces that are still on the device
    std::atomic<size_t> next{0};        // the shared piece counter

public:
    // a new download: nothing published, no error, every group with all its pieces (none: the plan is in core)
    void reset(const std::vector<int64_t>& pieces_per_group) {
        std::lock_guard<std::mutex> g(mu);
        published = 0;
        abort = false;
        err = 0;
        left = pieces_per_group;
        next.store(0);
    }
    // events [0, k) have been recorded (k only grows during a download)
    void publish(size_t k) {
        {
            std::lock_guard<std::mutex> g(mu);
            published = k;
        }
        cv.notify_all();
    }
    // the download cannot finish: the first code is kept, every waiter returns
    void fail(int code) {
        {
            std::lock_guard<std::mutex> g(mu);
            if (!err) err = code;
            abort = true;
        }
        cv.notify_all();
    }
    int error() {
        std::lock_guard<std::mutex> g(mu);
        return err;
    }
    // the next piece nobody has taken yet (pieces are taken in `ready` order; past the last one: the worker is done)
    size_t claim() { return next.fetch_add(1); }
    // "event ev is published, or the download is aborted", without blocking and blocking.  ready(): wait_ready() would return at
    // once -- a worker with a piece in hand asks first and drains that piece before it blocks.  wait_ready(): false = aborted.
    bool ready(size_t ev) {
        std::lock_guard<std::mutex> g(mu);
        return abort || published > ev;
    }
    bool wait_ready(size_t ev) {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return abort || published > ev; });
        return !abort;
    }
    // a piece of `group` is in the pinned ring (its DMA is complete); the last one of a group wakes the enqueue thread
    void piece_left_device(int32_t group) {
        if (group < 0) return;
        bool last = false;
        {
            std::lock_guard<std::mutex> g(mu);
            if ((size_t)group < left.size()) last = --left[(size_t)group] == 0;
        }
        if (last) cv.notify_all();
    }
    // until no piece of the groups lo .. hi (both included; none when lo > hi) is on the device; false = aborted.  A group that
    // reset() was not told of has no pieces, here as in piece_left_device.
    bool wait_groups(int lo, int hi) {
        std::unique_lock<std::mutex> g(mu);
        for (int w = lo; w <= hi; ++w) {
            cv.wait(g, [&] { return abort || w < 0 || (size_t)w >= left.size() || left[(size_t)w] <= 0; });
            if (abort) return false;
        }
        return true;
    }
};

// A staging slot into the caller's array `host` (the reference layout): `ring` holds what the piece's copies brought, in the order
// they were enqueued (sf_download.hip, dl_enqueue).  Super / Lsip / Lsxp: the structure's pointers (read for LU-direct pieces only).
inline void dl_unpack(const DlPiece& pc, const double* ring, double* host, const int32_t* Super, const int64_t* Lsip,
                      const int64_t* Lsxp) {
    if (pc.s0 >= 0) {
        // LU, direct form: ring = [ L run | U^T run ]; column j of the reference panel = L column (nsrow) followed by rows
        // [nscol, nsrow) of the U^T column
        const double* rl = ring;
        const double* ru = ring + pc.dev_count;
        for (int32_t s = pc.s0; s < pc.s1; ++s) {
            const int64_t nscol = Super[s + 1] - Super[s], nsrow = Lsip[s + 1] - Lsip[s];
            const int64_t nb = nsrow - nscol, lda = nsrow + nb;
            const int64_t j0 = pc.ld > 0 ? pc.j0 : 0, nc = pc.ld > 0 ? pc.ncols : nscol;
            double* dst = host + Lsxp[s] + j0 * lda;
            // 2-D U part (one supernode): nb values per column; whole panels: full columns, the first nscol rows skipped
            const int64_t ustride = pc.ld > 0 ? nb : nsrow, uskip = pc.ld > 0 ? 0 : nscol;
            for (int64_t c = 0; c < nc; ++c) {
                memcpy(dst + c * lda, rl + c * nsrow, (size_t)nsrow * sizeof(double));
                if (nb > 0) memcpy(dst + c * lda + nsrow, ru + c * ustride + uskip, (size_t)nb * sizeof(double));
            }
            rl += nc * nsrow;
            ru += nc * ustride;
        }
    } else if (pc.ld > 0) {
        const int64_t rows = pc.ld - pc.skip;
        for (int64_t c = 0; c < pc.ncols; ++c) {
            double* col = host + pc.host_off + c * pc.ld;
            memset(col, 0, (size_t)pc.skip * sizeof(double));
            memcpy(col + pc.skip, ring + c * rows, (size_t)rows * sizeof(double));
        }
    } else {
        memcpy(host + pc.host_off, ring, (size_t)pc.count * sizeof(double));
    }
}

}   // namespace sf
