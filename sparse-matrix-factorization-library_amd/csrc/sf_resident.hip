// The registry of resident factors and SparseFrame_solve_supernodal's fast path on them (see sparseframe_flat.h): a factorization
// through the handlers (sf_handlers.hip) registers the host array it filled; a solve that finds its Lsx here runs on the device(s),
// after every panel's fingerprint over the caller's array has been compared with the device's.  Lock order: sf_resident.h.
#include "sf_resident.h"

#include <atomic>
#include <chrono>
#include <cstring>
#include <mutex>
#include <unordered_map>

#include "sf_plan_cache.h"

namespace {

// host copies of factors that are still on the device(s): in a single handler's cached plan (plan), or distributed over the
// per-rank plans of a multi-handler factorization (parts), see sf_handlers_solve_resident
struct Resident {
    sf_chol_plan* plan = nullptr;
    int plan_epoch = 0;                 // the factorization of `plan` the host copy belongs to
    std::vector<sf_chol_plan*> parts;
    std::vector<int> part_epochs;
    std::shared_ptr<SolverSlot> slot;
    std::vector<sf_comm*> comms;        // the ranks' communicators (owned by the handler list), for the distributed solve
    int device = 0;
};
using Registry = std::unordered_map<const void*, Resident>;
// (leaked on purpose: a process that exits with entries still registered -- no SparseFrame_free_gpu -- must not run plan destructors,
// i.e. HIP calls, from a static destructor after the runtime has been torn down)
std::mutex& g_res_mu = *new std::mutex();
Registry& g_resident = *new Registry();
int64_t g_resident_solves = 0;      // solves served from a resident factor (tests)
std::atomic<int64_t> g_fingerprint_fallbacks{0};   // verified solves that fell back to the host sweep because a fingerprint differed (sf_handlers_fingerprint_fallbacks)
// resident-solve policy (sf_handlers_set_resident_solve): 0 never, 1 after a FULL comparison of fingerprints (default), 2 trusted
std::atomic<int> g_resident_mode{1};

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// ---- step 1: the plan(s) that answer ----
struct Chosen {
    sf_chol_plan* plan = nullptr;       // single or gathered
    bool distributed = false;           // the ranks' plans solve together, in place
    bool stale = false;                 // refused because the device holds a later factorization: the entry goes
};
// Distributed factor, gathered: once per factorization into a whole plan on the first handler's device -- panels travel device to
// device, the solve then runs there.  Needs the symbolic arrays (to build that plan) and room for the whole factor on one device;
// otherwise the caller solves on the host.
const char* gather_parts(Resident& R, const PlanInput& in, Chosen& c) {
    SolverSlot& S = *R.slot;
    if (!S.plan) {
        if (!in.Super || !in.SuperMap || !in.Lsip || !in.Lsi || !in.Lsxp || !in.Lp || !in.Li || in.nsuper <= 0) return "distributed factor and no symbolic arrays";
        size_t free_b = 0, total_b = 0;
        if (hipSetDevice(R.device) != hipSuccess || hipMemGetInfo(&free_b, &total_b) != hipSuccess) return "hipMemGetInfo failed";
        const double need = (double)in.Lsxp[in.nsuper] * 8.0 * (in.lu ? 2.0 : 1.0) * 1.15 + 2e9;
        if ((double)free_b < need) return "the first handler's device has no room for the whole factor";
        PlanInput whole = in;
        whole.device = R.device;
        if (sf_resident::create_plan(&S.plan, whole, sf_resident::CREATE_PLAIN)) { S.plan = nullptr; (void)hipGetLastError(); return "the whole plan could not be built"; }
        S.imported.clear();
    }
    if (S.imported != R.part_epochs) {
        if (sf_plan_import_from(S.plan, R.parts.data(), (int)R.parts.size()) != SF_OK) { S.imported.clear(); return "gathering the panels failed"; }
        S.imported = R.part_epochs;
    }
    c.plan = S.plan;
    return nullptr;
}
// nullptr, or why the resident factor cannot be used
const char* choose_plan(Resident& R, const PlanInput& in, Chosen& c) {
    if (R.parts.empty()) {
        c.plan = R.plan;
        c.stale = R.plan->fs.factor_epoch() != R.plan_epoch || R.plan->partial;
        return c.stale ? "the plan holds a later factorization" : nullptr;
    }
    for (size_t r = 0; r < R.parts.size(); ++r)
        if (R.parts[r]->fs.factor_epoch() != R.part_epochs[r]) { c.stale = true; return "a rank's plan holds a later factorization"; }
    // The factor stays where it is and the ranks solve together (sf_chol_plan_solve_distributed), one host thread per rank as in
    // the factorization.  SF_SOLVE=gather: gather the panels into a whole plan on the first handler's device instead.
    c.distributed = R.comms.size() == R.parts.size();
    if (const char* e = getenv("SF_SOLVE")) c.distributed = c.distributed && strcmp(e, "gather") != 0;
    return c.distributed ? nullptr : gather_parts(R, in, c);
}

// ---- step 2: the host copy must still be what the device holds (it came from there bit by bit) ----
// The fingerprints of the caller's array against the plan's (k_factor_hash; cached per factorization; Cholesky and LU).
// stored_only: a rank's part -- only the panels it stores.  0 equal, 1 different, -1 the device's could not be computed.
int fingerprints_differ(sf_chol_plan* plan, const std::vector<uint64_t>& host, bool stored_only) {
    const uint64_t* dh = nullptr;
    if (sf_plan_panel_hashes(plan, &dh) != SF_OK) return -1;
    for (int64_t sn = 0; sn < plan->nsuper; ++sn)
        if (!(stored_only && plan->h_XP[sn] < 0) && dh[sn] != host[(size_t)sn]) return 1;
    return 0;
}
// EVERY panel, one pass over the host array (threaded), against every plan that stores the panel.  nullptr, or why not;
// *changed: a fingerprint differed.
const char* verify_fingerprints(const Resident& R, const Chosen& c, const sf_float* Lsx_host, bool trace, bool* changed) {
    const auto t0 = std::chrono::steady_clock::now();
    const std::vector<sf_chol_plan*> plans = c.distributed ? R.parts : std::vector<sf_chol_plan*>{c.plan};
    std::vector<uint64_t> hh;
    sf::host_panel_hashes(Lsx_host, plans[0]->h_Lsxp.data(), plans[0]->nsuper, hh);
    if (trace && c.distributed) fprintf(stderr, "[sparseframe-hip] resident solve: host fingerprints %.1f ms\n", ms_since(t0));
    for (sf_chol_plan* p : plans) {
        const int d = fingerprints_differ(p, hh, c.distributed);
        if (d < 0) return c.distributed ? "a rank's fingerprints could not be computed" : "the device fingerprints could not be computed";
        *changed = d > 0;
        if (d > 0) return c.distributed ? "the host copy differs from a rank's panel (fingerprint)" : "the host copy differs from the device's (fingerprint)";
    }
    return nullptr;
}

// ---- step 3 ----
int solve_distributed(const Resident& R, const sf_float* b, sf_float* x) {
    const size_t N = R.parts.size();
    std::vector<int> rcs(N, SF_OK);
    std::vector<std::thread> th;
    for (size_t r = 0; r < N; ++r)
        th.emplace_back([&, r] { rcs[r] = sf_chol_plan_solve_distributed(R.parts[r], R.comms[r], b, x); });
    for (std::thread& t : th) t.join();
    for (size_t r = 0; r < N; ++r)
        if (rcs[r]) return rcs[r];
    return SF_OK;
}

}  // namespace

namespace sf_resident {

void register_plan(const void* Lsx, sf_chol_plan* plan) {
    std::lock_guard<std::mutex> g(g_res_mu);
    if (plan->ooc_groups > 1) { g_resident.erase(Lsx); return; }
    Resident R;
    R.plan = plan;
    R.plan_epoch = plan->fs.factor_epoch();
    g_resident[Lsx] = std::move(R);
}

void register_parts(const void* Lsx, const std::vector<sf_chol_plan*>& parts, const std::shared_ptr<SolverSlot>& slot,
                    const std::vector<sf_comm*>& comms, int device) {
    Resident R;
    R.parts = parts;
    for (sf_chol_plan* q : parts) R.part_epochs.push_back(q->fs.factor_epoch());
    R.slot = slot;
    R.comms = comms;
    R.device = device;
    std::lock_guard<std::mutex> g(g_res_mu);
    g_resident[Lsx] = std::move(R);
}

void erase(const void* Lsx) {
    std::lock_guard<std::mutex> g(g_res_mu);
    g_resident.erase(Lsx);
}

void forget_plan(sf_chol_plan* plan) {
    std::lock_guard<std::mutex> g(g_res_mu);
    for (auto it = g_resident.begin(); it != g_resident.end();) {
        bool hit = it->second.plan == plan;
        for (sf_chol_plan* q : it->second.parts) hit = hit || q == plan;
        if (hit) it = g_resident.erase(it); else ++it;
    }
}

void destroy_plan(sf_chol_plan* plan) {
    if (!plan) return;
    forget_plan(plan);
    sf_chol_plan_destroy(plan);
}

int create_plan(sf_chol_plan** plan, const PlanInput& in, CreateKind kind, const int32_t* owner) {
#define SF_SYMBOLIC_ARGS in.n, in.nsuper, in.Super, in.SuperMap, in.Lsip, in.Lsi, in.Lsxp, in.Lp, in.Li
    switch (kind) {
        case CREATE_OOC:
            return in.lu ? sf_lu_plan_create_ooc(plan, in.device, SF_SYMBOLIC_ARGS, in.Up, in.Ui, in.ooc_group, in.ooc_ngroups, in.ooc_top_mode)
                         : sf_chol_plan_create_ooc(plan, in.device, SF_SYMBOLIC_ARGS, in.ooc_group, in.ooc_ngroups, in.ooc_top_mode);
        case CREATE_MAPPED:     // proportional mapping: own subtrees + the top supernodes above them
            return in.lu ? sf_lu_plan_create_mapped(plan, in.device, SF_SYMBOLIC_ARGS, in.Up, in.Ui, owner, in.rank, in.nranks)
                         : sf_chol_plan_create_mapped(plan, in.device, SF_SYMBOLIC_ARGS, owner, in.rank, in.nranks);
        default:
            return in.lu ? sf_lu_plan_create(plan, in.device, SF_SYMBOLIC_ARGS, in.Up, in.Ui) : sf_chol_plan_create(plan, in.device, SF_SYMBOLIC_ARGS);
    }
#undef SF_SYMBOLIC_ARGS
}

}  // namespace sf_resident

extern "C" {

int sf_handlers_solve_resident_sym(const sf_float* Lsx_host, const sf_float* b, sf_float* x, int lu, sf_long n, sf_long nsuper,
                                   const sf_long* Super, const sf_long* SuperMap, const sf_long* Lsip, const sf_long* Lsi,
                                   const sf_long* Lsxp, const sf_long* Lp, const sf_long* Li, const sf_long* Up, const sf_long* Ui) {
    if (!Lsx_host || !b || !x) return SF_ERR_ARG;
    PlanInput in;
    in.lu = lu != 0; in.n = n; in.nsuper = nsuper;
    in.Super = Super; in.SuperMap = SuperMap; in.Lsip = Lsip; in.Lsi = Lsi; in.Lsxp = Lsxp; in.Lp = Lp; in.Li = Li; in.Up = Up; in.Ui = Ui;
    const bool trace = getenv("SF_TRACE") != nullptr;
    auto why = [&](const char* m) { if (trace) fprintf(stderr, "[sparseframe-hip] resident solve not used: %s\n", m); return SF_ERR_ARG; };
    if (const char* e = getenv("SF_SOLVE"))
        if (!strcmp(e, "host")) return SF_ERR_ARG;
    const int mode = g_resident_mode.load();
    if (mode == 0) return SF_ERR_ARG;
    std::lock_guard<std::mutex> g(g_res_mu);
    auto it = g_resident.find((const void*)Lsx_host);
    if (it == g_resident.end()) return why("no resident factor is registered for this Lsx");
    Resident& R = it->second;
    Chosen c;
    if (const char* no = choose_plan(R, in, c)) {
        if (c.stale) g_resident.erase(it);
        return why(no);
    }
    const auto tv0 = std::chrono::steady_clock::now();
    bool changed = false;
    if (mode == 1)
        if (const char* no = verify_fingerprints(R, c, Lsx_host, trace, &changed)) {
            if (changed) { g_resident.erase(it); ++g_fingerprint_fallbacks; }
            return why(no);
        }
    int rc;
    if (c.distributed) {
        const double verify_ms = ms_since(tv0);
        const auto tv1 = std::chrono::steady_clock::now();
        rc = solve_distributed(R, b, x);
        if (trace) fprintf(stderr, "[sparseframe-hip] resident solve: verification %.1f ms, distributed solve %.1f ms\n", verify_ms, ms_since(tv1));
        if (rc) return why("the distributed solve failed");
    } else {
        rc = c.plan->lu ? sf_lu_plan_solve(c.plan, b, x) : sf_chol_plan_solve(c.plan, b, x);
    }
    if (!rc) ++g_resident_solves;
    return rc;
}

int sf_handlers_solve_resident(const sf_float* Lsx_host, const sf_float* b, sf_float* x) {
    return sf_handlers_solve_resident_sym(Lsx_host, b, x, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// how often a verified resident solve found the caller's array different from the device's factor and left the solve to the host sweep:
// expected only after the caller changed Lsx; anything else (e.g. replicas of a shared panel that are no longer bit-identical) shows
// up here instead of as a silently slower solve (bench.py reports it, the tests assert on it)
int64_t sf_handlers_fingerprint_fallbacks(void) { return g_fingerprint_fallbacks.load(); }

int64_t sf_handlers_resident_solves(void) {
    std::lock_guard<std::mutex> g(g_res_mu);
    return g_resident_solves;
}

int sf_handlers_set_resident_solve(int mode) {
    if (mode < 0 || mode > 2) return SF_ERR_ARG;
    g_resident_mode.store(mode);
    return SF_OK;
}

// Test hook: how many values of the panels that several ranks store (the shared top supernodes of a multi-handler factorization)
// differ BITWISE between a rank's copy and the first holder's.  0 is the invariant the LU pivot decisions rest on (plan_create);
// -1: no multi-handler factor is registered for this host array.
int64_t sf_handlers_replica_mismatches(const sf_float* Lsx_host) {
    std::lock_guard<std::mutex> g(g_res_mu);
    auto it = g_resident.find((const void*)Lsx_host);
    if (it == g_resident.end() || it->second.parts.size() < 2) return -1;
    const std::vector<sf_chol_plan*>& parts = it->second.parts;
    const sf_chol_plan* P0 = parts[0];
    int64_t bad = 0;
    std::vector<double> a, b;
    for (int64_t s = 0; s < P0->nsuper; ++s) {
        const size_t len = (size_t)(P0->h_Lsip[s + 1] - P0->h_Lsip[s]) * (size_t)(P0->h_Super[s + 1] - P0->h_Super[s]);
        const sf_chol_plan* first = nullptr;
        for (sf_chol_plan* P : parts) {
            if (P->h_XP[s] < 0) continue;
            std::vector<double>& dst = first ? b : a;
            dst.resize(len * (P->lu ? 2 : 1));
            if (hipSetDevice(P->device) != hipSuccess ||
                hipMemcpy(dst.data(), P->d_Lsx + P->h_XP[s], len * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -1;
            if (P->lu && !P->u_alias &&
                hipMemcpy(dst.data() + len, P->d_Lsx + P->xC + P->h_XP[s], len * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return -1;
            if (P->lu && P->u_alias) dst.resize(len);
            if (!first) { first = P; continue; }
            // (LU: the upper triangle of an L panel's diagonal block is not factor data -- it is scratch for the download, filled
            // with U11 on the ranks that copy that block column back, see k_lu_fill_u11)
            const size_t nsr = (size_t)(P0->h_Lsip[s + 1] - P0->h_Lsip[s]), nsc = (size_t)(P0->h_Super[s + 1] - P0->h_Super[s]);
            for (size_t i = 0; i < a.size(); ++i) {
                if (P->lu && i < len && (i % nsr) <= (i / nsr) && (i % nsr) < nsc) continue;
                bad += memcmp(&a[i], &b[i], sizeof(double)) != 0;
            }
        }
    }
    return bad;
}

}  // extern "C"
