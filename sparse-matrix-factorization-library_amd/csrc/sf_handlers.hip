// Device handlers behind the reference's struct entry points (SparseFrame_allocate_gpu C:16-285, _free_gpu C:287-366,
// _factorize_supernodal C:2150-3017, _factorize C:3019-3034; the LU library forwards here too).
//
// The reference builds, per device handler, eight equal device slots plus pinned mirrors and streams, and stages every
// panel through them.  Here a handler owns
//   * a lock (the reference's gpuLock, C:2287: MATRIX_THREAD_NUM callers share the handler list),
//   * a small cache of device plans keyed by a hash of the symbolic pattern (sf_plan_cache.h): the task tables, the relative maps
//     and the resident factor are built once per pattern and re-used by every later factorization of that pattern,
//   * a device pool it lends to one plan's factor,
// and a factorization is: values H2D, the level-scheduled numeric phase, and the factor copied back into
// matrix_info->Lsx WHILE the upper levels still compute (sf_chol_plan_factorize_to_host; reference C:2888-2895).
// This file: the handler list, the pool, the LU pivot policy of the struct calls and the two factorize drivers.  Where a new
// pattern's factor goes and what is given up for it: sf_placement.h; the factors that stay resident and their solves: sf_resident.hip.
#include <sparseframe_hip.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "sf_kernels.h"
#include "sf_placement.h"
#include "sf_plan_cache.h"
#include "sf_plan_internal.h"
#include "sf_resident.h"
#include "sf_symbolic.h"

int sf_comm_create_all(sf_comm** comms, int nranks, const int* devices);     // sf_multi.hip

namespace {

using sf_resident::destroy_plan;
using sf_resident::forget_plan;

// ---- LU pivoting policy of the struct entry points ----
// (sf_handlers_set_lu_pivoting): unset = whatever the plans were created with (the reference's behaviour, no pivoting, unless
// SF_LU_PIVOT_TOL said otherwise); g_perturbed: perturbed pivots of the factorization that filled a given host array
// (leaked on purpose, as the registry of sf_resident.hip: nothing runs from a static destructor)
std::mutex& g_piv_mu = *new std::mutex();
bool g_piv_set = false;
double g_piv_tol = 0.0, g_piv_perturb = 0.0;
std::unordered_map<const void*, int64_t>& g_perturbed = *new std::unordered_map<const void*, int64_t>();
// the policy of ONE call (sf_handlers_set_lu_pivoting_next_call: the struct library passes a matrix_info's own setting this way);
// read by the thread that calls sf_handlers_factorize, before it hands the plans to the handlers' threads
thread_local bool t_piv_set = false;
thread_local double t_piv_tol = 0.0, t_piv_perturb = 0.0;
// Every LU factorization through the handlers states its policy: the call's own, else the process-wide one, else what the plan was
// created with -- a cached plan must not carry the previous matrix's setting into the next one's factorization.
int apply_pivot_policy(sf_chol_plan* plan) {
    if (!plan || !plan->lu) return SF_OK;
    if (t_piv_set) return sf_lu_plan_set_pivoting(plan, t_piv_tol, t_piv_perturb);
    std::lock_guard<std::mutex> g(g_piv_mu);
    return g_piv_set ? sf_lu_plan_set_pivoting(plan, g_piv_tol, g_piv_perturb)
                     : sf_lu_plan_set_pivoting(plan, plan->piv_tol0, plan->piv_perturb0);
}
void note_perturbed(const void* Lsx, int64_t count) {
    std::lock_guard<std::mutex> g(g_piv_mu);
    if (g_perturbed.size() > 4096) g_perturbed.clear();
    g_perturbed[Lsx] = count;
}

// ---- the handlers ----
// all handlers of a list working on ONE matrix (the reference runs numGPU + numCPU workers inside
// SparseFrame_factorize_supernodal, C:2267): communicators and the per-rank distributed plans, hung off handler 0
struct MultiState {
    std::mutex mu;
    std::vector<sf_comm*> comms;
    struct RankPlans { std::vector<sf_chol_plan*> plans; std::shared_ptr<SolverSlot> slot; };
    sf::PlanLru<RankPlans> cache;
    uint64_t builds = 0;        // sets of per-rank plans built (cache misses)
    static void drop(RankPlans& v) {
        for (sf_chol_plan*& p : v.plans) { destroy_plan(p); p = nullptr; }
    }
    ~MultiState() {
        cache.clear(drop);
        for (sf_comm* c : comms) sf_comm_destroy(c);
    }
};

struct HandlerState {
    std::mutex mu;
    sf::PlanLru<sf_chol_plan*> cache;
    uint64_t builds = 0;                // plans built by this handler (cache misses)
    MultiState* multi = nullptr;        // handler 0 only
    // Device pool: ONE buffer allocated in SparseFrame_allocate_gpu (where the reference allocates its eight slots, C:92-283) that
    // the handler lends to the plan of one pattern at a time for its factor -- so that the first SparseFrame_factorize of a pattern
    // does not start with a hipMalloc of tens of GB (12 - 790 ms, depending on what the box did before).  A factor that does not
    // fit the pool, or a second cached pattern, allocates as before; a multi-handler factorization gives the pools back first.
    int device = 0;
    double* pool = nullptr;
    size_t pool_bytes = 0;
    sf_chol_plan* pool_user = nullptr;
    bool pool_idle() const { return pool && !pool_user; }
    void release_pool() {
        if (pool_idle()) { (void)hipSetDevice(device); (void)hipFree(pool); pool = nullptr; pool_bytes = 0; }
    }
    void drop(sf_chol_plan* q) {        // a cached plan goes; the pool's user leaves the pool idle
        if (pool_user == q) pool_user = nullptr;
        destroy_plan(q);
    }
    void drop_cache() { cache.clear([this](sf_chol_plan* q) { drop(q); }); }
    ~HandlerState() {
        drop_cache();
        pool_user = nullptr;
        release_pool();
        delete multi;
    }
};

// what sf::place_and_create (sf_placement.h) asks of one handler while it builds the plan of a new pattern into `plan`
struct HandlerEnv {
    HandlerState& S;
    const PlanInput& in;
    bool trace;
    sf_chol_plan*& plan;
    int decide(double shrink, sf::Placement& pl) {
        int64_t budget = 0;
        if (const char* env = getenv("SF_DEVICE_BUDGET_MB")) budget = (int64_t)strtoll(env, nullptr, 10) << 20;
        auto free_bytes = [&](size_t& fr) { size_t tot = 0; return hipSetDevice(in.device) == hipSuccess && hipMemGetInfo(&fr, &tot) == hipSuccess; };
        return sf::decide_placement(in, shrink, budget, free_bytes, S.pool_idle() ? S.pool_bytes : 0, trace, pl);
    }
    int create(const sf::Placement& pl) {
        const bool offered = S.pool_idle();
        if (offered) sf_plan_offer_factor_buffer(S.pool, S.pool_bytes);
        struct Claim {      // whoever got the buffer is its user until it is dropped
            HandlerState& S; sf_chol_plan*& plan; bool offered;
            ~Claim() { sf_plan_offer_factor_buffer(nullptr, 0); if (offered && plan && sf_plan_factor_borrowed(plan)) S.pool_user = plan; }
        } claim{S, plan, offered};
        if (pl.ngroups <= 1) return sf_resident::create_plan(&plan, in, sf_resident::CREATE_PLAIN);
        PlanInput ooc = in;
        ooc.ooc_group = pl.group.data(); ooc.ooc_ngroups = pl.ngroups; ooc.ooc_top_mode = pl.top_mode;
        return sf_resident::create_plan(&plan, ooc, sf_resident::CREATE_OOC);
    }
    bool cache_empty() const { return S.cache.empty(); }
    void drop_cache() { S.drop_cache(); }
    bool pool_idle() const { return S.pool_idle(); }
    void release_pool() { S.release_pool(); }
    bool env_budget_set() const { return getenv("SF_DEVICE_BUDGET_MB") != nullptr; }
    void device_sync() { (void)hipDeviceSynchronize(); }
    void clear_error() { (void)hipGetLastError(); }
};

}  // namespace

struct gpu_info_struct {
    int gpuIndex_physical;
    size_t devMemSize;
    HandlerState* st;
};

// every rank thread builds its distributed plan where the entry has none yet, and uploads the values.  A rank without a usable
// plan cannot take part in the collectives; the others would wait for it, so all ranks are checked before any of them starts
static int load_rank_plans(MultiState::RankPlans& v, const struct gpu_info_struct* list, const PlanInput& in, const std::vector<int32_t>& owner,
                           const sf_float* Lx, const sf_float* Ux) {
    const int N = (int)v.plans.size();
    std::vector<int> rcs((size_t)N, SF_OK);
    std::vector<std::thread> th;
    for (int r = 0; r < N; ++r)
        th.emplace_back([&, r] {
            int rc = SF_OK;
            sf_chol_plan*& plan = v.plans[r];
            if (!plan) {
                PlanInput mine = in;
                mine.device = list[r].gpuIndex_physical; mine.rank = r; mine.nranks = N;
                rc = sf_resident::create_plan(&plan, mine, sf_resident::CREATE_MAPPED, owner.data());
            }
            if (!rc) rc = in.lu ? sf_lu_plan_set_values(plan, Lx, Ux) : sf_chol_plan_set_values(plan, Lx);
            rcs[r] = rc;
        });
    for (std::thread& t : th) t.join();
    for (int r = 0; r < N; ++r)
        if (rcs[r]) return rcs[r];
    return SF_OK;
}

// ONE factorization over all handlers of the list: rank r = handler r.  Every rank thread builds (or finds) its
// distributed plan, uploads the values and runs sf_chol_plan_factorize_distributed with the overlapped copy-back of its
// own pieces into Lsx_out (owned subtree panels; the top panels' pieces are dealt out over the ranks).
static int factorize_all_handlers(struct common_info_struct* common, struct gpu_info_struct* list, const PlanInput& in,
                                  const sf_float* Lx, const sf_float* Ux, sf_float* Lsx_out, sf_long* PivOut) {
    const int N = common->numGPU;
    MultiState& M = *list[0].st->multi;
    sf::PlanKey key = sf::make_key(in);
    key.h ^= 0x5bd1e995ull * (uint64_t)N;
    std::lock_guard<std::mutex> guard(M.mu);
    if (M.comms.empty()) {
        std::vector<int> devs(N);
        for (int r = 0; r < N; ++r) devs[r] = list[r].gpuIndex_physical;
        M.comms.assign(N, nullptr);
        const int rc = sf_comm_create_all(M.comms.data(), N, devs.data());
        if (rc) { M.comms.clear(); return rc; }
    }
    auto* entry = M.cache.find(key);
    std::vector<int32_t> owner;
    if (!entry) {
        M.cache.make_room(MultiState::drop);
        owner.assign(in.nsuper, 0);
        // cost of a top flop relative to a subtree flop: its 1/N share plus the replicated chain and the all-reduce
        if (sf::subtree_partition(in.nsuper, in.Super, in.SuperMap, in.Lsip, in.Lsi, N, owner.data(), nullptr, nullptr, 1.0 / N + 0.25)) return SF_ERR_ARG;
        entry = M.cache.insert(key, MultiState::RankPlans{std::vector<sf_chol_plan*>(N, nullptr), std::make_shared<SolverSlot>()});
        ++M.builds;
    }
    std::vector<sf_chol_plan*>& plans = entry->value.plans;
    if (int rc = load_rank_plans(entry->value, list, in, owner, Lx, Ux)) {
        MultiState::drop(entry->value);
        M.cache.erase(entry);
        return rc;
    }
    for (int r = 0; r < N; ++r) forget_plan(plans[r]);       // the host copies these plans' factors stood for are history
    for (int r = 0; r < N; ++r)
        if (int rc = apply_pivot_policy(plans[r])) return rc;
    std::vector<int> rcs(N, SF_OK);
    std::vector<std::thread> th;
    for (int r = 0; r < N; ++r)
        th.emplace_back([&, r] { rcs[r] = sf_chol_plan_factorize_distributed(plans[r], M.comms[r], Lsx_out, 1); });
    for (std::thread& t : th) t.join();
    for (int r = 0; r < N; ++r)
        if (rcs[r]) return rcs[r];
    if (in.lu && PivOut)   // every rank reports the blocks of the panels it stores (the top panels' records agree on all ranks)
        for (int r = 0; r < N; ++r)
            if (int rc = sf_lu_plan_get_pivots(plans[r], PivOut)) return rc;
    if (in.lu) {           // (a shared top panel's perturbations are counted by every rank of its group: an upper bound, 0 is exact)
        int64_t per = 0;
        for (int r = 0; r < N; ++r) per += plans[r]->last_perturbed;
        note_perturbed(Lsx_out, per);
    }
    // the factor is now spread over the ranks' plans; a solve of the struct path runs there, or gathers it into a whole plan on the
    // first handler's device (sf_handlers_solve_resident)
    sf_resident::register_parts(Lsx_out, plans, entry->value.slot, M.comms, list[0].gpuIndex_physical);
    return SF_OK;
}

extern "C" {

int sf_handlers_allocate(struct common_info_struct* common, struct gpu_info_struct** list) {
    if (!common || !list) return 1;
    const auto t0 = std::chrono::steady_clock::now();
    const int nphys = sf_device_count();
    int ndev = nphys;
    // SF_EMULATE_HANDLERS=N on a one-GPU box: N handlers that share device 0 (the multi-handler code path end to end,
    // with the all-reduce done by a kernel on that device instead of RCCL) -- tests and rehearsals only
    if (nphys == 1)
        if (const char* env = getenv("SF_EMULATE_HANDLERS")) ndev = std::max(1, std::min(16, atoi(env)));
    common->numGPU_physical = nphys;
    common->numGPU = ndev;       // one handler per device; no virtual-GPU splitting (reference C:36-41)
    common->numCPU = 0;          // the numeric phase has no CPU worker
    common->minDevMemSize = 0;
    common->minHostMemSize = 0;
    *list = (struct gpu_info_struct*)calloc(ndev > 0 ? ndev : 1, sizeof(struct gpu_info_struct));
    if (!*list) return 1;
    size_t min_mem = (size_t)-1;
    for (int d = 0; d < ndev; ++d) {
        hipDeviceProp_t prop;
        const int phys = nphys == 1 ? 0 : d;
        if (hipGetDeviceProperties(&prop, phys) != hipSuccess) continue;
        (*list)[d].gpuIndex_physical = phys;
        (*list)[d].devMemSize = prop.totalGlobalMem;
        (*list)[d].st = new (std::nothrow) HandlerState();
        min_mem = std::min(min_mem, (size_t)prop.totalGlobalMem);
        // pay the per-process, per-device one-time costs here (the reference creates its streams and cuBLAS / cuSOLVER handles in
        // this call, C:92-283) instead of inside the first SparseFrame_factorize: runtime and code-object initialisation, the first
        // device and pinned allocations
        if (d == phys && hipSetDevice(phys) == hipSuccess) {
            void* dp = nullptr;
            void* hp = nullptr;
            if (hipMalloc(&dp, 1 << 20) == hipSuccess) (void)hipFree(dp);
            if (hipHostMalloc(&hp, 1 << 20, hipHostMallocDefault) == hipSuccess) (void)hipHostFree(hp);
            sf::launch_noop(nullptr);
            (void)hipDeviceSynchronize();
            (void)hipGetLastError();
        }
    }
    if (ndev > 0 && (*list)[0].st) (*list)[0].st->multi = new (std::nothrow) MultiState();
    if (ndev > 0 && min_mem != (size_t)-1) {
        common->devSlotSize = sf_reference_slot_size(ndev, min_mem);
        common->minDevMemSize = common->devSlotSize * 8;
        // the pool: what the reference's eight slots would take (at most a quarter of the device); SF_DEVICE_POOL_MB overrides, 0 = none.
        // One handler per physical device only (not for emulated handlers sharing a device), and only where one handler = one matrix:
        // with several handlers the default is ONE matrix over all of them, whose per-rank plans need the memory themselves.
        size_t want = std::min(common->devSlotSize * 8, min_mem / 4);
        if (const char* env = getenv("SF_DEVICE_POOL_MB")) want = (size_t)strtoull(env, nullptr, 10) << 20;
        const char* mode = getenv("SF_MULTI");
        const bool per_matrix = ndev == 1 || (mode && strcmp(mode, "matrix") == 0);
        for (int d = 0; d < ndev && want > 0 && ndev == nphys && per_matrix; ++d) {
            HandlerState* st = (*list)[d].st;
            if (!st) continue;
            st->device = (*list)[d].gpuIndex_physical;
            void* q = nullptr;
            if (hipSetDevice(st->device) == hipSuccess && hipMalloc(&q, want) == hipSuccess) { st->pool = (double*)q; st->pool_bytes = want; }
            else (void)hipGetLastError();
        }
    } else {
        const char* env = getenv("SF_DEVSLOT");
        common->devSlotSize = env ? (size_t)strtoull(env, nullptr, 10) : ((size_t)1 << 30);
    }
    common->allocateTime = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

// number of device plans (sets of per-rank plans for a multi-handler factorization) the handlers of a list have built so far:
// a repeated sparsity pattern must not add to it (tests; SF_TRACE prints the same per call)
int64_t sf_handlers_plan_builds(struct gpu_info_struct* list, int n_handlers) {
    int64_t total = 0;
    if (!list) return 0;
    for (int d = 0; d < n_handlers; ++d) {
        if (!list[d].st) continue;
        std::lock_guard<std::mutex> guard(list[d].st->mu);
        total += (int64_t)list[d].st->builds;
        if (list[d].st->multi) total += (int64_t)list[d].st->multi->builds;
    }
    return total;
}

// the device pool of handler d: out[0] = bytes (0: none), out[1] = 1 while a plan's factor lives in it, out[2] = that plan's n
int sf_handlers_pool_info(struct gpu_info_struct* list, int d, sf_long* out) {
    if (!list || d < 0 || !out || !list[d].st) return SF_ERR_ARG;
    std::lock_guard<std::mutex> guard(list[d].st->mu);
    out[0] = (sf_long)list[d].st->pool_bytes;
    out[1] = list[d].st->pool_user ? 1 : 0;
    out[2] = list[d].st->pool_user ? list[d].st->pool_user->n : 0;
    return SF_OK;
}

int sf_handlers_free(struct common_info_struct* common, struct gpu_info_struct** list) {
    if (!list || !*list) return 1;
    const auto t0 = std::chrono::steady_clock::now();
    const int nh = common ? std::max(common->numGPU, 0) : 0;
    for (int d = 0; d < nh; ++d) {
        delete (*list)[d].st;           // destroys the cached plans (device memory, pinned rings)
        (*list)[d].st = nullptr;
    }
    free(*list);
    *list = nullptr;
    if (common) {
        common->numGPU = 0;
        common->freeTime = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    return 0;
}

// One numeric factorization through the handler list.  Returns SF_OK or an SF_ERR_* code; Lsx_out receives the factor in
// the reference layout.
int sf_handlers_factorize(struct common_info_struct* common, struct gpu_info_struct* list, int lu, int serial,
                          sf_long n, sf_long nsuper, const sf_long* Super, const sf_long* SuperMap,
                          const sf_long* Lsip, const sf_long* Lsi, const sf_long* Lsxp,
                          const sf_long* Lp, const sf_long* Li, const sf_long* Up, const sf_long* Ui,
                          const sf_float* Lx, const sf_float* Ux, sf_float* Lsx_out, sf_long* PivOut) {
    struct OneCallPolicy { ~OneCallPolicy() { t_piv_set = false; } } one_call_policy;      // sf_handlers_set_lu_pivoting_next_call holds for THIS call only
    if (!common || !Lsx_out || !Super || !Lsip || !Lsxp || !Lp || n < 0 || nsuper < 0) return SF_ERR_ARG;
    if (common->numGPU <= 0 || !list) {
        fprintf(stderr, "[sparseframe-hip] SparseFrame_factorize: no GPU handler (numGPU = %d); no CPU fallback\n", common->numGPU);
        return SF_ERR_NO_DEVICE;
    }
    if (n > 0 && (!SuperMap || !Lsi || !Li)) return SF_ERR_ARG;
    PlanInput in;
    in.lu = lu != 0; in.n = n; in.nsuper = nsuper;
    in.Super = Super; in.SuperMap = SuperMap; in.Lsip = Lsip; in.Lsi = Lsi; in.Lsxp = Lsxp; in.Lp = Lp; in.Li = Li; in.Up = Up; in.Ui = Ui;
    // Several handlers: all of them factorize this matrix together, as in the reference (C:2267) -- elimination-tree
    // subtrees per handler, RCCL for the parent-front merge.  SF_MULTI=matrix keeps one matrix per handler instead.
    if (common->numGPU > 1 && nsuper > 0 && list[0].st && list[0].st->multi) {
        const char* mode = getenv("SF_MULTI");
        if (!mode || strcmp(mode, "matrix") != 0) return factorize_all_handlers(common, list, in, Lx, Ux, Lsx_out, PivOut);
    }
    // one matrix = one handler; the caller's matrix threads (MATRIX_THREAD_NUM, C:3375) are spread over the devices
    struct gpu_info_struct& H = list[(serial >= 0 ? serial : 0) % common->numGPU];
    if (!H.st) return SF_ERR_NO_DEVICE;
    in.device = H.gpuIndex_physical;
    const bool trace = getenv("SF_TRACE") != nullptr;      // stderr: where the time of this call goes
    const auto tk0 = std::chrono::steady_clock::now();
    const sf::PlanKey key = sf::make_key(in);
    const auto tk1 = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> guard(H.st->mu);
    HandlerState& S = *H.st;
    auto* entry = S.cache.find(key);
    sf_chol_plan* plan = entry ? entry->value : nullptr;
    if (!plan) {        // make room first when the cache is full, then decide where the factor goes and build the plan
        S.cache.make_room([&](sf_chol_plan* q) { S.drop(q); });
        sf::Placement pl;
        HandlerEnv env{S, in, trace, plan};
        if (int rc = sf::place_and_create(env, pl)) return rc;
        S.cache.insert(key, plan);
        ++S.builds;
    }
    const auto tk2 = std::chrono::steady_clock::now();
    forget_plan(plan);              // whatever host copy this plan's factor stood for is about to be overwritten on the device
    int rc = apply_pivot_policy(plan);
    if (!rc) rc = sf_chol_plan_factorize_to_host(plan, Lx, Ux, Lsx_out);
    if (!rc && lu && PivOut) rc = sf_lu_plan_get_pivots(plan, PivOut);
    if (!rc && lu) note_perturbed(Lsx_out, plan->last_perturbed);
    if (!rc) sf_resident::register_plan(Lsx_out, plan);
    if (trace) {
        const auto tk3 = std::chrono::steady_clock::now();
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "[sparseframe-hip] factorize: pattern hash %.1f ms, plan lookup/build %.1f ms, H2D + numeric + overlapped D2H %.1f ms\n",
                ms(tk0, tk1), ms(tk1, tk2), ms(tk2, tk3));
        fprintf(stderr, "[sparseframe-hip]   copy workers %s, last on CPUs", plan->dl.cpus_known == 1 ? "confined to the device's NUMA node" : "not confined");
        for (int w = 0; w < plan->dl.workers_last; ++w) fprintf(stderr, " %d", plan->dl.last_cpu[w]);
        fprintf(stderr, "\n");
    }
    return rc;
}

void sf_handlers_forget(const sf_float* Lsx_host) {
    if (!Lsx_host) return;
    sf_resident::erase((const void*)Lsx_host);
    std::lock_guard<std::mutex> g(g_piv_mu);
    g_perturbed.erase((const void*)Lsx_host);
}

// 1 when the library was built with the A/B switches of finished experiments (make EXP=1), 0 for a release build
int sf_build_experiments(void) {
#ifdef SF_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

int sf_handlers_set_lu_pivoting(double tol, double perturb) {
    if (!(tol >= 0.0) || tol > 1.0 || !(perturb >= 0.0)) return SF_ERR_ARG;
    std::lock_guard<std::mutex> g(g_piv_mu);
    g_piv_set = true;
    g_piv_tol = tol;
    g_piv_perturb = perturb;
    return SF_OK;
}

int sf_handlers_set_lu_pivoting_next_call(double tol, double perturb) {
    if (!(tol >= 0.0) || tol > 1.0 || !(perturb >= 0.0)) return SF_ERR_ARG;
    t_piv_set = true;
    t_piv_tol = tol;
    t_piv_perturb = perturb;
    return SF_OK;
}

int64_t sf_handlers_perturbed_pivots(const sf_float* Lsx_host) {
    std::lock_guard<std::mutex> g(g_piv_mu);
    auto it = g_perturbed.find((const void*)Lsx_host);
    return it == g_perturbed.end() ? -1 : it->second;
}

}  // extern "C"
