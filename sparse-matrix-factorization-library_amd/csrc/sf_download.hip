// Overlapped copy-back (sf_chol_plan_factorize_to_host).  The reference copies finished blocks back on a second stream
// while it computes (s_cudaStream_copyback, C:2888-2895).  Here: a few host threads, each with its own HIP stream and two pinned
// staging slots.  A worker pulls the next piece (pieces are sorted by the launch that finishes them): it
// waits until the main thread has recorded the piece's event on the compute stream, makes its stream wait for that
// event, starts the D2H into one slot and, while that DMA runs, copies the previous slot into the caller's buffer.
// The caller's memory is never pinned or registered: fresh (never touched) pages of a just-malloc'ed Lsx are faulted in
// by the workers in parallel with the factorization (measured: hipHostRegister of fresh memory is a serial 0.06 s/GiB,
// 1.7 s for the 128^3 factor; tools/host_xfer_bench.hip).
// This file is the HIP half: events, copies, threads.  The threads' protocol (sf::DlGate) and the unpacking of a slot
// (sf::dl_unpack) use no GPU and live in sf_download.h, where a stand-alone program tests them under sanitizers.
#include <sparseframe_hip.h>

#include <sched.h>
#include <sys/mman.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "sf_plan_internal.h"

hipError_t sf_dl_publish(sf_chol_plan* p, size_t done) {
    SfDownload& d = p->dl;
    size_t k = d.next_ev;
    while (k < d.ev_ready.size() && d.ev_ready[k] <= done) {
        if (d.lu_direct && d.d_fill && k + 1 < d.fill_first.size()) {
            sf::launch_lu_fill_u11((const sf::FillTile*)d.d_fill + d.fill_first[k], d.fill_first[k + 1] - d.fill_first[k],
                                   p->d_Lsx, p->d_Lsx + p->xC, p->stream);
            const hipError_t ef = hipGetLastError();
            if (ef != hipSuccess) return ef;
        }
        const hipError_t e = hipEventRecord(p->dl_events[k], p->stream);
        if (e != hipSuccess) return e;
        ++k;
    }
    if (k != d.next_ev) {
        d.next_ev = k;
        d.gate.publish(k);
    }
    return hipSuccess;
}

// ... once every piece of group g - 2 has LEFT the device (its DMA into the pinned ring is complete; the copy workers
// count) -- with top mode 2 possibly of a later group, whose top panels' places are taken over here.  Everything those
// pieces wait for has been enqueued and published by now.
int sf_dl_wait_groups(sf_chol_plan* p, int g) {
    const int upto = p->ooc_wait.empty() ? g - 2 : p->ooc_wait[(size_t)g];
    return p->dl.gate.wait_groups(std::max(0, g - 2), std::min(upto, g - 1)) ? SF_OK : SF_ERR_HIP;
}

static double dl_now() {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec / 1e6;
}

// The copy workers move the whole factor (30 GB at 128^3) from the pinned staging ring into the caller's pageable Lsx while the
// factorization runs: ~55 GB/s of memcpy, which on a two-socket host is cheapest from the socket the device hangs on (the ring
// lives there).  SF_DL_PIN=1 confines the workers to the CPUs of the device's NUMA node (hipDeviceAttributeHostNumaId or the PCI
// device's sysfs entry), intersected with the affinity mask the process was given.  OFF by default: measured neutral on the
// two-socket box of this project (profiles/r02_f_struct_slow_mode.txt, part 3 -- the slow calls seen there had another cause, see
// the stream priorities in plan_create), and a library should not move its caller's threads around without being asked.
static void dl_lookup_cpus(sf_chol_plan* p) {
    p->dl.cpus_known = -1;
    const char* pin_env = sf_exp_env("SF_DL_PIN");
    if (!pin_env || atoi(pin_env) == 0) return;
    int node = -1;
    if (hipDeviceGetAttribute(&node, hipDeviceAttributeHostNumaId, p->device) != hipSuccess) { (void)hipGetLastError(); node = -1; }
    if (node < 0) {                                              // older runtimes: the PCI device's own sysfs entry
        char bdf[32] = {0}, path0[96];
        if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, p->device) == hipSuccess) {
            for (char* q = bdf; *q; ++q) *q = (char)tolower((unsigned char)*q);
            snprintf(path0, sizeof path0, "/sys/bus/pci/devices/%s/numa_node", bdf);
            if (FILE* f0 = fopen(path0, "r")) {
                if (fscanf(f0, "%d", &node) != 1) node = -1;
                fclose(f0);
            }
        } else (void)hipGetLastError();
    }
    if (getenv("SF_TRACE")) fprintf(stderr, "[sparseframe-hip]   device %d hangs on NUMA node %d\n", p->device, node);
    if (node < 0) return;
    char path[96];
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    FILE* f = fopen(path, "r");
    if (!f) return;
    char buf[4096];
    const bool got = fgets(buf, sizeof buf, f) != nullptr;
    fclose(f);
    if (!got) return;
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return;
    for (char* q = buf; *q;) {                                   // "0-63,128-191"
        char* e = nullptr;
        const long a = strtol(q, &e, 10);
        if (e == q) break;
        long b = a;
        if (*e == '-') { q = e + 1; b = strtol(q, &e, 10); if (e == q) break; }
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c)
            if (c >= 0 && CPU_ISSET((int)c, &allowed)) p->dl.cpus.push_back((int)c);
        q = (*e == ',') ? e + 1 : e;
        if (*e != ',') break;
    }
    if (!p->dl.cpus.empty()) p->dl.cpus_known = 1;
}

// ---- the copies of one piece into the pinned slot `hslot`, on the worker's stream: one helper per piece form.  What they
// leave in the slot, in this order, is what sf::dl_unpack reads ----
static bool dl_copy_plain(const DlPiece& pc, const double* src, double* hslot, hipStream_t ws) {
    return hipMemcpyAsync(hslot, src, (size_t)pc.count * sizeof(double), hipMemcpyDeviceToHost, ws) == hipSuccess;
}
// Cholesky block columns right of a panel's first: rows [skip, ld) of every column, the zero prefixes stay off the link
static bool dl_copy_2d(const DlPiece& pc, const double* src, double* hslot, hipStream_t ws) {
    const size_t rb = (size_t)(pc.ld - pc.skip) * sizeof(double);
    return hipMemcpy2DAsync(hslot, rb, src + pc.skip, (size_t)pc.ld * sizeof(double), rb, (size_t)pc.ncols, hipMemcpyDeviceToHost, ws) == hipSuccess;
}
// LU, direct form: the L run as it is; the U^T run as it is (whole supernodes) or rows [nscol, nsrow) of its columns
static bool dl_copy_lu_direct(const sf_chol_plan* p, const DlPiece& pc, const double* src, double* hslot, hipStream_t ws) {
    const double* usrc = src + p->xC;
    if (hipMemcpyAsync(hslot, src, (size_t)pc.dev_count * sizeof(double), hipMemcpyDeviceToHost, ws) != hipSuccess) return false;
    if (pc.ld == 0)
        return hipMemcpyAsync(hslot + pc.dev_count, usrc, (size_t)pc.dev_count * sizeof(double), hipMemcpyDeviceToHost, ws) == hipSuccess;
    const int64_t nscol = p->h_Super[pc.s0 + 1] - p->h_Super[pc.s0], nb = pc.ld - nscol;
    return nb <= 0 || hipMemcpy2DAsync(hslot + pc.dev_count, (size_t)nb * sizeof(double), usrc + nscol, (size_t)pc.ld * sizeof(double),
                                       (size_t)nb * sizeof(double), (size_t)pc.ncols, hipMemcpyDeviceToHost, ws) == hipSuccess;
}
// LU through the pack kernel: the piece's stretch of the reference layout is gathered into the device slot, then copied like a
// Cholesky piece
static bool dl_copy_lu_pack(const sf_chol_plan* p, const DlPiece& pc, double* dslot, double* hslot, hipStream_t ws) {
    sf::launch_pack_lu(p->d_Super, p->d_Lsip, p->d_Xp, p->d_Lsxp, (int32_t)p->nsuper, p->d_Lsx, p->d_Lsx + p->xC,
                       dslot, pc.host_off, pc.host_off + pc.count, ws);
    if (hipGetLastError() != hipSuccess) return false;
    return pc.ld > 0 ? dl_copy_2d(pc, dslot, hslot, ws) : dl_copy_plain(pc, dslot, hslot, ws);
}
static bool dl_enqueue(const sf_chol_plan* p, const DlPiece& pc, int64_t ring_off, hipStream_t ws) {
    double* hslot = p->h_ring + ring_off;
    const double* src = p->d_Lsx + pc.dev_off;
    if (pc.s0 >= 0) return dl_copy_lu_direct(p, pc, src, hslot, ws);
    if (p->lu) return dl_copy_lu_pack(p, pc, p->d_ring + ring_off, hslot, ws);
    return pc.ld > 0 ? dl_copy_2d(pc, src, hslot, ws) : dl_copy_plain(pc, src, hslot, ws);
}

static void dl_worker(sf_chol_plan* p, int w) {
    SfDownload& d = p->dl;
    if (d.cpus_known == 1) {
        cpu_set_t set;
        CPU_ZERO(&set);
        for (int c : d.cpus) CPU_SET(c, &set);
        (void)sched_setaffinity(0, sizeof set, &set);            // this thread only; a failure leaves it where it was
    }
    struct CpuNote { SfDownload& d; int w; ~CpuNote() { d.last_cpu[w] = sched_getcpu(); } } note{d, w};
    if (hipSetDevice(p->device) != hipSuccess) { d.gate.fail(SF_ERR_HIP); return; }
    hipStream_t ws = p->dl_streams[w];
    const size_t np = d.pieces.size();
    auto ring_off = [&](int sl) { return ((int64_t)w * 2 + sl) * d.slot; };
    auto stamp = [&](size_t k, int what) { if (!d.trace.empty()) d.trace[3 * k + what] = dl_now() - d.t0; };
    size_t prev = np;           // the piece in hand (np: none): its copies are enqueued into slot prev_slot, nothing more
    int prev_slot = 0, slot = 0;
    // the piece in hand, if any, out of the ring: wait for its DMA, count it off its group, unpack it
    auto drain = [&]() -> bool {
        if (prev == np) return true;
        const size_t k = prev;
        prev = np;
        const DlPiece& pc = d.pieces[k];
        if (hipEventSynchronize(p->dl_done[w][prev_slot]) != hipSuccess) return false;
        d.gate.piece_left_device(pc.group);     // out of core: this piece has left the device
        stamp(k, 1);
        sf::dl_unpack(pc, p->h_ring + ring_off(prev_slot), d.host, p->h_Super.data(), p->h_Lsip.data(), p->h_Lsxp.data());
        stamp(k, 2);
        return true;
    };
    // pieces are pulled from one shared counter, in ready order: streams do not all get the same share of the SDMA
    // engines (measured: with a static round-robin split one worker of three finished at 570 ms, the others at 940 and
    // 1070 ms), so the split has to be dynamic
    for (size_t k = d.gate.claim(); k < np; k = d.gate.claim()) {
        const DlPiece& pc = d.pieces[k];
        // nothing to fetch yet: finish the piece in hand first (an out-of-core plan's enqueue thread may be waiting for
        // exactly that piece before it publishes anything further)
        if (prev < np && !d.gate.ready((size_t)pc.ev) && !drain()) { d.gate.fail(SF_ERR_HIP); return; }
        if (!d.gate.wait_ready((size_t)pc.ev)) return;
        stamp(k, 0);
        // The piece's event is waited for on the HOST, by this thread, and the copy is enqueued with nothing in front of it.  A
        // device-side wait (hipStreamWaitEvent, SF_DL_HOST_WAIT=0) sits in the hardware queue the runtime has put this stream on
        // and holds up whatever else shares that queue -- another worker's copy of a piece that has long been ready, or a stream
        // of the caller's (the runtime multiplexes all streams of one priority over 4 hardware queues; plan_create has the story).
        // While the event is still in the future, the previous piece is copied out of the ring first.
        bool ok = true;
        if (d.host_wait) {
            if (prev < np && hipEventQuery(p->dl_events[pc.ev]) != hipSuccess) {
                (void)hipGetLastError();            // hipErrorNotReady is not an error
                ok = drain();
            }
            ok = ok && hipEventSynchronize(p->dl_events[pc.ev]) == hipSuccess;
        } else {
            ok = hipStreamWaitEvent(ws, p->dl_events[pc.ev], 0) == hipSuccess;
        }
        ok = ok && dl_enqueue(p, pc, ring_off(slot), ws) && hipEventRecord(p->dl_done[w][slot], ws) == hipSuccess;
        ok = ok && drain();     // (the previous piece, while this one's DMA runs)
        if (!ok) { d.gate.fail(SF_ERR_HIP); return; }
        prev = k;
        prev_slot = slot;
        slot ^= 1;
    }
    if (!drain()) d.gate.fail(SF_ERR_HIP);
}

int sf_dl_begin(sf_chol_plan* p, double* host_out) {
    if (!p || !host_out || p->dl.active) return SF_ERR_ARG;
    if (p->dry) return SF_ERR_ARG;        // a schedule-only plan has no device side
    HIP_TRY(hipSetDevice(p->device));
    SfDownload& d = p->dl;
    if (d.cpus_known == 0) dl_lookup_cpus(p);
    if (!p->h_ring) {
        const size_t rb = (size_t)std::max(d.workers, d.workers_fresh) * 2 * d.slot * sizeof(double);
        if (p->h_ring.alloc(rb / sizeof(double))) return SF_ERR_HIP;
        if (p->lu && !d.lu_direct) {
            if (p->d_ring.alloc(rb / sizeof(double))) return SF_ERR_HIP;
            p->bytes_device += rb;
        }
        for (int w = 0; w < std::max(d.workers, d.workers_fresh); ++w) {
            HIP_TRY(hipStreamCreateWithFlags(p->dl_streams[w].put(), hipStreamNonBlocking));
            for (int k = 0; k < 2; ++k) HIP_TRY(hipEventCreateWithFlags(p->dl_done[w][k].put(), hipEventDisableTiming));
        }
    }
    // transparent huge pages for the destination (this box: THP = madvise): 512x fewer first-touch faults when the
    // caller hands over a just-malloc'ed Lsx, harmless otherwise
    if (p->xsize > 0) {
        const uintptr_t pg = (uintptr_t)2 << 20;
        const uintptr_t a = ((uintptr_t)host_out + pg - 1) & ~(pg - 1), b = ((uintptr_t)(host_out + p->xsize)) & ~(pg - 1);
        if (b > a) (void)madvise((void*)a, b - a, MADV_HUGEPAGE);
    }
    d.host = host_out;
    d.next_ev = 0;
    d.gate.reset(d.group_pieces);
    d.active = true;
    d.threads.clear();
    // SF_DL_TRACE=path: per piece, the times (ms since the start of the download) at which its event was published, its DMA
    // finished and its copy into the caller's buffer finished
    d.trace.clear();
    if (getenv("SF_DL_TRACE")) d.trace.assign(3 * d.pieces.size(), 0.0);
    d.t0 = dl_now();
    // A destination whose pages have never been touched (the first call after SparseFrame_analyze malloc'ed Lsx) makes every worker's
    // memcpy fault its pages in as it goes, and 4 workers no longer keep up with the factorization: 6 bring the first struct call at
    // 128^3 from 714 to 662 ms; on touched pages 4 are enough and 6 only share hardware queues (sf_download.h).  mincore() on a
    // sample of the destination's pages tells the two apart.
    int nw_call = d.workers;
    if (d.workers_fresh > nw_call && p->xsize > (int64_t)(64 << 20)) {
        const long pg = sysconf(_SC_PAGESIZE);
        int resident = 0, probed = 0;
        for (int k = 0; k < 16 && pg > 0; ++k) {
            const uintptr_t a = ((uintptr_t)(host_out + (p->xsize / 16) * k + p->xsize / 32)) & ~((uintptr_t)pg - 1);
            unsigned char vec = 0;
            if (mincore((void*)a, (size_t)pg, &vec) == 0) { ++probed; resident += vec & 1; }
        }
        if (probed > 0 && 2 * resident < probed) nw_call = d.workers_fresh;
    }
    d.workers_last = nw_call;
    const int nw = (int)std::min<size_t>(nw_call, d.pieces.size());
    for (int w = 0; w < nw; ++w) d.threads.emplace_back(dl_worker, p, w);
    // (First touch of a just-malloc'ed destination is left to the copy workers.  Helper threads that populate the page tables ahead
    // of them -- MADV_POPULATE_WRITE over the array in address order -- were measured and make the first call SLOWER: 637 ms of
    // copy-back with none, 857 ms with 2, 1100 ms with 8 or 16 at 128^3 (profiles/r03_d_first_call_touch_threads.txt): the page
    // allocator serialises them with the workers' own faults.)
    return SF_OK;
}

int sf_dl_end(sf_chol_plan* p) {
    if (!p || !p->dl.active) return SF_ERR_ARG;
    SfDownload& d = p->dl;
    // a factorization that stopped early (an error in the enqueue path) must still release the workers
    if (d.next_ev < d.ev_ready.size()) {
        // (everything: an owner-computes block at the very end of the plan is ready "one launch after" its chain, see plan_create)
        if (hipSetDevice(p->device) != hipSuccess || sf_dl_publish(p, (size_t)-1) != hipSuccess) d.gate.fail(SF_ERR_HIP);
        if (d.next_ev < d.ev_ready.size()) d.gate.fail(SF_ERR_HIP);
    }
    for (std::thread& t : d.threads) t.join();
    d.threads.clear();
    d.active = false;
    d.host = nullptr;
    if (!d.trace.empty()) {
        if (FILE* f = fopen(getenv("SF_DL_TRACE") ? getenv("SF_DL_TRACE") : "/dev/null", "w")) {
            fprintf(f, "piece,ready_launch,doubles,t_published_ms,t_dma_done_ms,t_copied_ms\n");
            for (size_t k = 0; k < d.pieces.size(); ++k)
                fprintf(f, "%zu,%zu,%lld,%.3f,%.3f,%.3f\n", k, d.pieces[k].ready, (long long)d.pieces[k].count,
                        d.trace[3 * k], d.trace[3 * k + 1], d.trace[3 * k + 2]);
            fclose(f);
        }
    }
    return d.gate.error();
}

extern "C" {

// values H2D + numeric factorization + factor D2H into `host_out` (reference layout, xsize doubles), the download
// overlapped with the computation.  What one SparseFrame_factorize call does once its plan exists.
int sf_chol_plan_factorize_to_host(sf_chol_plan* p, const sf_float* Lx, const sf_float* Ux, sf_float* host_out) {
    if (!p || (!host_out && p->xsize > 0) || p->nranks > 1) return SF_ERR_ARG;
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    int rc = p->lu ? sf_lu_plan_set_values(p, Lx, Ux) : sf_chol_plan_set_values(p, Lx);
    if (rc) return rc;
    if (p->xsize <= 0) return sf_chol_plan_factorize(p, 1);
    if ((rc = sf_dl_begin(p, host_out))) return rc;
    rc = sf_chol_plan_factorize(p, 0);
    const int rc_dl = sf_dl_end(p);
    const int rc_sync = sf_chol_plan_sync(p);
    clock_gettime(CLOCK_MONOTONIC, &t1);
    p->last_to_host_ms = (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) / 1e6;
    return rc ? rc : (rc_sync ? rc_sync : rc_dl);
}

}   // extern "C"
