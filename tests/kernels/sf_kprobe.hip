// Test-only probe: thin extern "C" wrappers around the sf::launch_* entry points of libsparseframe_hip.so, so that the
// tests can run ONE kernel launch on task lists they build themselves.  Each wrapper copies a host image of a double arena
// (and the task arrays, maps, flags, pivot records) to the device, launches once, synchronises, and copies the arena and
// the outputs back.  No numerical logic lives here; tests/kernel_ref.py and tests/test_kernels.py do the rest.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <vector>

#include "sf_kernels.h"

#ifdef KP_EIGHT_SOLVE_LAUNCHERS
// The solve launchers as they were before they took the block width (one set per kernel family): with this defined the probe
// builds against that sf_kernels.h, so the one-launch solve tests can be run on the kernels as they were before csrc/sf_solve.hip.
namespace sf {
inline void launch_solve_small_fwd(const SolveTask* t, int nt, int width, const double* Lsx, const int32_t* Lsi, double* x, int unit,
                                   const int32_t* pivpos, hipStream_t st) {
    if (width == 1) launch_solve_small_fwd(t, nt, Lsx, Lsi, x, unit, pivpos, st);
    else launch_solve_many_small_fwd(t, nt, Lsx, Lsi, x, unit, pivpos, st);
}
inline void launch_solve_small_bwd(const SolveTask* t, int nt, int width, const double* Lsx, const int32_t* Lsi, double* x, hipStream_t st) {
    if (width == 1) launch_solve_small_bwd(t, nt, Lsx, Lsi, x, st);
    else launch_solve_many_small_bwd(t, nt, Lsx, Lsi, x, st);
}
inline void launch_solve_fwd(const SolveTask* t, int nt, int width, int big, const double* Lsx, const int32_t* Lsi, double* x, int unit,
                             const int32_t* pivpos, int* sync, int* ticket, int* info, hipStream_t st) {
    if (width == 1) launch_solve_fwd(t, nt, big, Lsx, Lsi, x, unit, pivpos, sync, ticket, info, st);
    else launch_solve_many_fwd(t, nt, big, Lsx, Lsi, x, unit, pivpos, sync, ticket, info, st);
}
inline void launch_solve_bwd(const SolveTask* t, int nt, int width, int big, const double* Lsx, const int32_t* Lsi, double* x, int* sync,
                             int* ticket, int* info, hipStream_t st, const double* Tbase) {
    if (width == 1) launch_solve_bwd(t, nt, big, Lsx, Lsi, x, sync, ticket, info, st, Tbase);
    else launch_solve_many_bwd(t, nt, big, Lsx, Lsi, x, sync, ticket, info, st, Tbase);
}
}  // namespace sf
#endif

namespace {

// device copies of host arrays, freed on scope exit; the first failing HIP call is kept in `rc`
struct Dev {
    std::vector<void*> ptrs;
    hipError_t rc = hipSuccess;
    ~Dev() { for (void* p : ptrs) (void)hipFree(p); }
    template <class T> T* in(const T* h, int64_t count) {
        if (rc != hipSuccess || count <= 0) return nullptr;
        void* d = nullptr;
        if ((rc = hipMalloc(&d, (size_t)count * sizeof(T))) != hipSuccess) return nullptr;
        ptrs.push_back(d);
        if (h) rc = hipMemcpy(d, h, (size_t)count * sizeof(T), hipMemcpyHostToDevice);
        else rc = hipMemset(d, 0, (size_t)count * sizeof(T));
        return (T*)d;
    }
    template <class T> void out(T* h, const T* d, int64_t count) {
        if (rc == hipSuccess && h && d && count > 0) rc = hipMemcpy(h, d, (size_t)count * sizeof(T), hipMemcpyDeviceToHost);
    }
    void finish() {
        if (rc != hipSuccess) return;
        rc = hipGetLastError();
        if (rc == hipSuccess) rc = hipDeviceSynchronize();
    }
};

}  // namespace

// host images of the structure arrays of the selected inversion (sf::SelStruct) with their lengths
struct KpSel {
    const int32_t *Super, *SuperMap;
    const int64_t* Lsip;
    const int32_t* Lsi;
    const int64_t* Xp;
    const sf::SelPair* pairs;
    const int32_t* relmap;
    int64_t nsuper, n, nLsi, npair, nrel;
};

namespace {

sf::SelStruct sel_in(Dev& d, const KpSel* h) {
    sf::SelStruct t;
    t.Super = d.in(h->Super, h->nsuper + 1);
    t.SuperMap = d.in(h->SuperMap, h->n);
    t.Lsip = d.in(h->Lsip, h->nsuper + 1);
    t.Lsi = d.in(h->Lsi, h->nLsi);
    t.Xp = d.in(h->Xp, h->nsuper + 1);
    t.pairs = d.in(h->pairs, h->npair);
    t.relmap = d.in(h->relmap, h->nrel);
    return t;
}

}  // namespace

extern "C" {

int kp_sizeof(const char* name) {
    if (!strcmp(name, "GemmProb")) return (int)sizeof(sf::GemmProb);
    if (!strcmp(name, "GemmTask")) return (int)sizeof(sf::GemmTask);
    if (!strcmp(name, "PotrfTask")) return (int)sizeof(sf::PotrfTask);
    if (!strcmp(name, "TrsmTask")) return (int)sizeof(sf::TrsmTask);
    if (!strcmp(name, "StepTask")) return (int)sizeof(sf::StepTask);
    if (!strcmp(name, "SolveTask")) return (int)sizeof(sf::SolveTask);
    if (!strcmp(name, "FillTile")) return (int)sizeof(sf::FillTile);
    if (!strcmp(name, "CondScalars")) return (int)sizeof(sf::CondScalars);
    if (!strcmp(name, "SelUnit")) return (int)sizeof(sf::SelUnit);
    if (!strcmp(name, "SelPair")) return (int)sizeof(sf::SelPair);
    return -1;
}

int kp_free_mem(int64_t* free_bytes) {
    size_t f = 0, t = 0;
    const hipError_t rc = hipMemGetInfo(&f, &t);
    *free_bytes = (int64_t)f;
    return (int)rc;
}

int kp_gemm(double* arena, int64_t narena, const sf::GemmProb* probs, int nprobs, const sf::GemmTask* tasks, int ntasks,
            const uint32_t* kt_prefix, uint32_t u_lo, uint32_t u_hi, int mode, const int32_t* relmap, int64_t nrel,
            int use_ticket, int whole_tiles, int grid_cap) {
    Dev d;
    double* A = d.in(arena, narena);
    const sf::GemmProb* P = d.in(probs, nprobs);
    const sf::GemmTask* T = d.in(tasks, ntasks);
    const uint32_t* K = d.in(kt_prefix, (int64_t)ntasks + 1);
    const int32_t* R = d.in(relmap, nrel);
    int* tk = use_ticket ? d.in<int>(nullptr, 8) : nullptr;
    if (d.rc == hipSuccess) sf::launch_gemm(P, T, K, ntasks, u_lo, u_hi, mode, A, R, tk, 0, whole_tiles, grid_cap);
    d.finish();
    d.out(arena, A, narena);
    return (int)d.rc;
}

int kp_update_small(double* arena, int64_t narena, const sf::GemmProb* probs, int nprobs, const sf::GemmTask* tasks, int ntasks,
                    const int32_t* relmap, int64_t nrel) {
    Dev d;
    double* A = d.in(arena, narena);
    const sf::GemmProb* P = d.in(probs, nprobs);
    const sf::GemmTask* T = d.in(tasks, ntasks);
    const int32_t* R = d.in(relmap, nrel);
    if (d.rc == hipSuccess) sf::launch_update_small(P, T, ntasks, A, R, 0);
    d.finish();
    d.out(arena, A, narena);
    return (int)d.rc;
}

int kp_build_relmaps(const sf::GemmProb* probs, int nprobs, const int32_t* Lsi, int64_t nLsi, int32_t* relmap, int64_t nrel) {
    Dev d;
    const sf::GemmProb* P = d.in(probs, nprobs);
    const int32_t* L = d.in(Lsi, nLsi);
    int32_t* R = d.in(relmap, nrel);
    if (d.rc == hipSuccess) sf::launch_build_relmaps(P, nprobs, L, R, 0);
    d.finish();
    d.out(relmap, R, nrel);
    return (int)d.rc;
}

int kp_potrf(double* arena, int64_t narena, const sf::PotrfTask* tasks, int ntasks, int* info) {
    Dev d;
    double* A = d.in(arena, narena);
    const sf::PotrfTask* T = d.in(tasks, ntasks);
    int* I = d.in(info, 1);
    if (d.rc == hipSuccess) sf::launch_potrf(T, ntasks, A, I, 0);
    d.finish();
    d.out(arena, A, narena);
    d.out(info, I, 1);
    return (int)d.rc;
}

// pivpos / pivinv: npiv entries each, or null (tol == 0: no record); nperturb: one counter
int kp_getrf(double* arena, int64_t narena, const sf::PotrfTask* tasks, int ntasks, int64_t u_shift, int* info, double tol, double eps,
             int32_t* pivpos, int32_t* pivinv, int64_t npiv, int* nperturb) {
    Dev d;
    double* A = d.in(arena, narena);
    const sf::PotrfTask* T = d.in(tasks, ntasks);
    int* I = d.in(info, 1);
    int32_t* pp = pivpos ? d.in(pivpos, npiv) : nullptr;
    int32_t* pi = pivinv ? d.in(pivinv, npiv) : nullptr;
    int* np = d.in(nperturb, 1);
    if (d.rc == hipSuccess) sf::launch_getrf(T, ntasks, A, u_shift, I, sf::PivotCtl{tol, eps, pp, pi, np}, 0);
    d.finish();
    d.out(arena, A, narena);
    d.out(info, I, 1);
    d.out(pivpos, pp, npiv);
    d.out(pivinv, pi, npiv);
    d.out(nperturb, np, 1);
    return (int)d.rc;
}

int kp_trsm(double* arena, int64_t narena, const sf::TrsmTask* tasks, int ntasks, const int32_t* pivinv, int64_t npiv) {
    Dev d;
    double* A = d.in(arena, narena);
    const sf::TrsmTask* T = d.in(tasks, ntasks);
    const int32_t* pi = pivinv ? d.in(pivinv, npiv) : nullptr;
    if (d.rc == hipSuccess) sf::launch_trsm(T, ntasks, A, pi, 0);
    d.finish();
    d.out(arena, A, narena);
    return (int)d.rc;
}

// flags: nflags words, in and out (a second launch with epoch + 1 re-uses them); tinv: ntinv doubles of scratch
int kp_step(double* arena, int64_t narena, const sf::StepTask* tasks, int ntasks, int lu, int* flags, int nflags, int epoch, int* info,
            int64_t ntinv, double tol, double eps, int32_t* pivpos, int32_t* pivinv, int64_t npiv, int* nperturb) {
    Dev d;
    double* A = d.in(arena, narena);
    const sf::StepTask* T = d.in(tasks, ntasks);
    int* F = d.in(flags, nflags);
    int* I = d.in(info, 1);
    double* tinv = d.in<double>(nullptr, ntinv);
    int* tk = d.in<int>(nullptr, 1);
    int32_t* pp = pivpos ? d.in(pivpos, npiv) : nullptr;
    int32_t* pi = pivinv ? d.in(pivinv, npiv) : nullptr;
    int* np = d.in(nperturb, 1);
    if (d.rc == hipSuccess) sf::launch_step(T, ntasks, lu, A, F, epoch, I, tinv, tk, sf::PivotCtl{tol, eps, pp, pi, np}, 0);
    d.finish();
    d.out(arena, A, narena);
    d.out(flags, F, nflags);
    d.out(info, I, 1);
    d.out(pivpos, pp, npiv);
    d.out(pivinv, pi, npiv);
    d.out(nperturb, np, 1);
    return (int)d.rc;
}

// The LU layout kernels: the L panels at arena + Xp[s], the U^T panels at arena + u_shift + Xp[s].
// out: nout values, in and out (the launch writes the first e_end - e_begin of them)
int kp_pack_lu(const double* arena, int64_t narena, int64_t u_shift, const int32_t* Super, const int64_t* Lsip, const int64_t* Xp,
               const int64_t* RefXp, int32_t nsuper, double* out, int64_t nout, int64_t e_begin, int64_t e_end) {
    Dev d;
    const double* A = d.in(arena, narena);
    const int32_t* S = d.in(Super, (int64_t)nsuper + 1);
    const int64_t* Lp = d.in(Lsip, (int64_t)nsuper + 1);
    const int64_t* X = d.in(Xp, nsuper);
    const int64_t* RX = d.in(RefXp, (int64_t)nsuper + 1);
    double* O = d.in(out, nout);
    if (d.rc == hipSuccess) sf::launch_pack_lu(S, Lp, X, RX, nsuper, A, A + u_shift, O, e_begin, e_end, 0);
    d.finish();
    d.out(out, O, nout);
    return (int)d.rc;
}

int kp_lu_fill_u11(double* arena, int64_t narena, int64_t u_shift, const sf::FillTile* tiles, int64_t ntiles) {
    Dev d;
    double* A = d.in(arena, narena);
    const sf::FillTile* T = d.in(tiles, ntiles);
    if (d.rc == hipSuccess) sf::launch_lu_fill_u11(T, ntiles, A, A + u_shift, 0);
    d.finish();
    d.out(arena, A, narena);
    return (int)d.rc;
}

// H: nsuper words, in and out (the launch adds to them)
int kp_factor_hash(const double* arena, int64_t narena, int64_t u_shift, const int32_t* Super, const int64_t* Lsip, const int64_t* Xp,
                   const int64_t* RefXp, int32_t nsuper, int lu, int64_t total, unsigned long long* H) {
    Dev d;
    const double* A = d.in(arena, narena);
    const int32_t* S = d.in(Super, (int64_t)nsuper + 1);
    const int64_t* Lp = d.in(Lsip, (int64_t)nsuper + 1);
    const int64_t* X = d.in(Xp, nsuper);
    const int64_t* RX = d.in(RefXp, (int64_t)nsuper + 1);
    unsigned long long* dH = d.in(H, nsuper);
    if (d.rc == hipSuccess) sf::launch_factor_hash(S, Lp, X, RX, nsuper, A, A + u_shift, lu, total, dH, 0);
    d.finish();
    d.out(H, dH, nsuper);
    return (int)d.rc;
}

// One step of the device solve: the forward launch on `tasks` (diagonal tasks first, then their row tiles; small != 0: the
// narrow kernel, diagonal tasks only).  x: nx entries (width 1) or the row-major nx x SVM_W block (width SVM_W), in and out.
// The probe owns the solve's words -- info, nsync sync words, one ticket -- zeroed before the launch; *info comes back.
int kp_solve_fwd(double* arena, int64_t narena, const int32_t* Lsi, int64_t nLsi, double* x, int64_t nx, const sf::SolveTask* tasks,
                 int ntasks, int width, int big, int small, int unit, const int32_t* pivpos, int64_t npiv, int nsync, int* info) {
    Dev d;
    double* A = d.in(arena, narena);
    const int32_t* L = d.in(Lsi, nLsi);
    double* X = d.in(x, nx * width);
    const sf::SolveTask* T = d.in(tasks, ntasks);
    const int32_t* pp = pivpos ? d.in(pivpos, npiv) : nullptr;
    int* W = d.in<int>(nullptr, 2 + (int64_t)nsync);
    if (d.rc == hipSuccess) {
        int *sync = W + 1, *ticket = W + 1 + nsync;
        if (small) sf::launch_solve_small_fwd(T, ntasks, width, A, L, X, unit, pp, 0);
        else sf::launch_solve_fwd(T, ntasks, width, big, A, L, X, unit, pp, sync, ticket, W, 0);
    }
    d.finish();
    d.out(arena, A, narena);
    d.out(x, X, nx * width);
    d.out(info, W, 1);
    return (int)d.rc;
}

// The backward launch (row tiles first, then the diagonal tasks).  nT > 0: a scratch of nT doubles for the row-major copies of
// the diagonal blocks of the tasks that carry a tdiag, made by launch_solve_transpose_diag in front of the launch.
int kp_solve_bwd(double* arena, int64_t narena, const int32_t* Lsi, int64_t nLsi, double* x, int64_t nx, const sf::SolveTask* tasks,
                 int ntasks, int width, int big, int small, int64_t nT, int nsync, int* info) {
    Dev d;
    double* A = d.in(arena, narena);
    const int32_t* L = d.in(Lsi, nLsi);
    double* X = d.in(x, nx * width);
    const sf::SolveTask* T = d.in(tasks, ntasks);
    int* W = d.in<int>(nullptr, 2 + (int64_t)nsync);
    double* Tb = nT > 0 ? d.in<double>(nullptr, nT) : nullptr;
    std::vector<int64_t> list;
    for (int i = 0; Tb && i < ntasks; ++i)
        if (tasks[i].nrows == 0 && tasks[i].tdiag) list.push_back(i);
    const int64_t* dl = d.in(list.data(), (int64_t)list.size());
    if (d.rc == hipSuccess) {
        int *sync = W + 1, *ticket = W + 1 + nsync;
        sf::launch_solve_transpose_diag(T, dl, (int64_t)list.size(), A, Tb, 0);
        if (small) sf::launch_solve_small_bwd(T, ntasks, width, A, L, X, 0);
        else sf::launch_solve_bwd(T, ntasks, width, big, A, L, X, sync, ticket, W, 0, Tb);
    }
    d.finish();
    d.out(arena, A, narena);
    d.out(x, X, nx * width);
    d.out(info, W, 1);
    return (int)d.rc;
}

// The transposed backward launch over the same task lists (csrc/sf_solve_t.hip): arena = the L panels (diagonal implied), pivpos:
// npiv entries or null.  nT > 0: the row-major copies are made from the same arena first, as the transposed sweep does.
int kp_tsolve_bwd(double* arena, int64_t narena, const int32_t* Lsi, int64_t nLsi, double* x, int64_t nx, const sf::SolveTask* tasks,
                  int ntasks, int width, int big, int small, const int32_t* pivpos, int64_t npiv, int64_t nT, int nsync, int* info) {
    Dev d;
    double* A = d.in(arena, narena);
    const int32_t* L = d.in(Lsi, nLsi);
    double* X = d.in(x, nx * width);
    const sf::SolveTask* T = d.in(tasks, ntasks);
    const int32_t* pp = pivpos ? d.in(pivpos, npiv) : nullptr;
    int* W = d.in<int>(nullptr, 2 + (int64_t)nsync);
    double* Tb = nT > 0 ? d.in<double>(nullptr, nT) : nullptr;
    std::vector<int64_t> list;
    for (int i = 0; Tb && i < ntasks; ++i)
        if (tasks[i].nrows == 0 && tasks[i].tdiag) list.push_back(i);
    const int64_t* dl = d.in(list.data(), (int64_t)list.size());
    if (d.rc == hipSuccess) {
        int *sync = W + 1, *ticket = W + 1 + nsync;
        sf::launch_solve_transpose_diag(T, dl, (int64_t)list.size(), A, Tb, 0);
        if (small) sf::launch_tsolve_small_bwd(T, ntasks, width, A, L, X, pp, 0);
        else sf::launch_tsolve_bwd(T, ntasks, width, big, A, L, X, pp, sync, ticket, W, 0, Tb);
    }
    d.finish();
    d.out(arena, A, narena);
    d.out(x, X, nx * width);
    d.out(info, W, 1);
    return (int)d.rc;
}

// The condition estimate's kernels.  x / y / xi: `len` doubles each, in and out (len >= n: the tail is the test's sentinel);
// scalars: the 16-byte CondScalars, in and out
int kp_condest_fill(double* x, int64_t len, int64_t n, int mode) {
    Dev d;
    double* X = d.in(x, len);
    if (d.rc == hipSuccess) sf::launch_condest_fill(X, n, mode, 0);
    d.finish();
    d.out(x, X, len);
    return (int)d.rc;
}

int kp_condest_sign_norm(double* y, double* xi, int64_t len, int64_t n, int solve_info_value, sf::CondScalars* scalars) {
    Dev d;
    double* Y = d.in(y, len);
    double* Xi = d.in(xi, len);
    const int* I = d.in(&solve_info_value, 1);
    sf::CondScalars* S = d.in(scalars, 1);
    if (d.rc == hipSuccess) sf::launch_condest_sign_norm(Y, Xi, n, I, S, 0);
    d.finish();
    d.out(y, Y, len);
    d.out(xi, Xi, len);
    d.out(scalars, S, 1);
    return (int)d.rc;
}

int kp_condest_argmax_next(double* x, int64_t len, int64_t n, sf::CondScalars* scalars, int first, int last) {
    Dev d;
    double* X = d.in(x, len);
    sf::CondScalars* S = d.in(scalars, 1);
    if (d.rc == hipSuccess) sf::launch_condest_argmax_next(X, n, S, first, last, 0);
    d.finish();
    d.out(x, X, len);
    d.out(scalars, S, 1);
    return (int)d.rc;
}

// Bc: nBc doubles (column-major n x cw in front), X: nX doubles (row-major n x SVM_W in front); the destination in and out
int kp_solve_many_pack(const double* Bc, int64_t nBc, int64_t n, int cw, double* X, int64_t nX) {
    Dev d;
    const double* B = d.in(Bc, nBc);
    double* Xd = d.in(X, nX);
    if (d.rc == hipSuccess) sf::launch_solve_many_pack(B, n, cw, Xd, 0);
    d.finish();
    d.out(X, Xd, nX);
    return (int)d.rc;
}

int kp_solve_many_unpack(const double* X, int64_t nX, int64_t n, int cw, double* Bc, int64_t nBc) {
    Dev d;
    const double* Xd = d.in(X, nX);
    double* B = d.in(Bc, nBc);
    if (d.rc == hipSuccess) sf::launch_solve_many_unpack(Xd, n, cw, B, 0);
    d.finish();
    d.out(Bc, B, nBc);
    return (int)d.rc;
}

int kp_build_loadmap(const int64_t* Lp, const int32_t* Li, int32_t n, const int32_t* Super, const int32_t* SuperMap, int32_t nsuper,
                     const int64_t* Lsip, const int32_t* Lsi, const int64_t* Lsxp, int64_t base, int skip_diag, int64_t* map) {
    Dev d;
    const int64_t nnz = Lp[n];
    const int64_t* dLp = d.in(Lp, (int64_t)n + 1);
    const int32_t* dLi = d.in(Li, nnz);
    const int32_t* dS = d.in(Super, (int64_t)nsuper + 1);
    const int32_t* dSM = d.in(SuperMap, n);
    const int64_t* dLsip = d.in(Lsip, (int64_t)nsuper + 1);
    const int32_t* dLsi = d.in(Lsi, Lsip[nsuper]);
    const int64_t* dLsxp = d.in(Lsxp, (int64_t)nsuper + 1);
    int64_t* dmap = d.in(map, nnz);
    if (d.rc == hipSuccess) sf::launch_build_loadmap(dLp, dLi, n, dS, dSM, dLsip, dLsi, dLsxp, base, skip_diag, dmap, 0);
    d.finish();
    d.out(map, dmap, nnz);
    return (int)d.rc;
}

int kp_load_mapped(double* arena, int64_t narena, const double* Lx, const int64_t* map, int64_t nnz) {
    Dev d;
    double* A = d.in(arena, narena);
    const double* dLx = d.in(Lx, nnz);
    const int64_t* dmap = d.in(map, nnz);
    if (d.rc == hipSuccess) sf::launch_load_mapped(dLx, dmap, nnz, A, 0);
    d.finish();
    d.out(arena, A, narena);
    return (int)d.rc;
}

// load_mask: nsuper bytes, or null
int kp_load_panels(double* arena, int64_t narena, const int64_t* Lp, const int32_t* Li, const double* Lx, int32_t n,
                   const int32_t* Super, const int32_t* SuperMap, int32_t nsuper, const int64_t* Lsip, const int32_t* Lsi,
                   const int64_t* Lsxp, int skip_diag, const int8_t* load_mask) {
    Dev d;
    const int64_t nnz = Lp[n];
    double* A = d.in(arena, narena);
    const int64_t* dLp = d.in(Lp, (int64_t)n + 1);
    const int32_t* dLi = d.in(Li, nnz);
    const double* dLx = d.in(Lx, nnz);
    const int32_t* dS = d.in(Super, (int64_t)nsuper + 1);
    const int32_t* dSM = d.in(SuperMap, n);
    const int64_t* dLsip = d.in(Lsip, (int64_t)nsuper + 1);
    const int32_t* dLsi = d.in(Lsi, Lsip[nsuper]);
    const int64_t* dLsxp = d.in(Lsxp, (int64_t)nsuper + 1);
    const int8_t* dmask = load_mask ? d.in(load_mask, nsuper) : nullptr;
    if (d.rc == hipSuccess) sf::launch_load_panels(dLp, dLi, dLx, n, dS, dSM, dLsip, dLsi, dLsxp, A, skip_diag, dmask, 0);
    d.finish();
    d.out(arena, A, narena);
    return (int)d.rc;
}

// ---- the selected inversion (csrc/sf_selinv.hip, csrc/sf_selinv_lu.hip): tests/test_kernels_selinv.py ----
// The factor (L, or PL / PU) and the arenas of Sigma (S, or SL / SU) are separate images with the same panel offsets; Sigma in and out.
int kp_selinv_small(const double* L, double* S, int64_t narena, const sf::SelUnit* units, int nunits, const KpSel* sel) {
    Dev d;
    const double* dL = d.in(L, narena);
    double* dS = d.in(S, narena);
    const sf::SelUnit* U = d.in(units, nunits);
    const sf::SelStruct t = sel_in(d, sel);
    if (d.rc == hipSuccess) sf::launch_selinv_small(U, nunits, dL, dS, t, 0);
    d.finish();
    d.out(S, dS, narena);
    return (int)d.rc;
}

int kp_lu_selinv_small(const double* PL, const double* PU, double* SL, double* SU, int64_t narena, const sf::SelUnit* units, int nunits,
                       const KpSel* sel) {
    Dev d;
    const double* dPL = d.in(PL, narena);
    const double* dPU = d.in(PU, narena);
    double* dSL = d.in(SL, narena);
    double* dSU = d.in(SU, narena);
    const sf::SelUnit* U = d.in(units, nunits);
    const sf::SelStruct t = sel_in(d, sel);
    if (d.rc == hipSuccess) sf::launch_lu_selinv_small(U, nunits, dPL, dPU, dSL, dSU, t, 0);
    d.finish();
    d.out(SL, dSL, narena);
    d.out(SU, dSU, narena);
    return (int)d.rc;
}

// lu == 0: k_selinv_trinv; otherwise k_lu_selinv_trinv with `unit`.  out: nout doubles, in and out (the launch writes the first w * w)
int kp_selinv_trinv(const double* P, int64_t narena, const sf::SelUnit* u, int lu, int unit, double* out, int64_t nout) {
    Dev d;
    const double* dP = d.in(P, narena);
    double* O = d.in(out, nout);
    if (d.rc == hipSuccess) {
        if (lu) sf::launch_lu_selinv_trinv(*u, dP, unit, O, 0);
        else sf::launch_selinv_trinv(*u, dP, O, 0);
    }
    d.finish();
    d.out(out, O, nout);
    return (int)d.rc;
}

// A, B and C at offsets of one scratch image `buf` (in and out); a_off < 0: no A (am == 2).  S / S2: the arenas of the gathered
// operand (am == 2; S2 null: S2 = S), sel: the structure arrays, or null when am != 2
int kp_selinv_gemm(int am, int M, int N, int K, double* buf, int64_t nbuf, int64_t a_off, int64_t lda, int64_t b_off, int64_t ldb,
                   int64_t c_off, int64_t ldc, int slabs, int64_t cstride, int acc_in, const sf::SelUnit* u, const double* S, const double* S2,
                   int64_t narena, const KpSel* sel) {
    Dev d;
    double* W = d.in(buf, nbuf);
    const double* dS = S ? d.in(S, narena) : nullptr;
    const double* dS2 = S2 ? d.in(S2, narena) : dS;
    sf::SelStruct t{};
    if (sel) t = sel_in(d, sel);
    if (d.rc == hipSuccess)
        sf::launch_selinv_gemm(am, M, N, K, a_off < 0 ? nullptr : W + a_off, lda, W + b_off, ldb, W + c_off, ldc, slabs, cstride, acc_in, *u, dS,
                               dS2, t, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

int kp_selinv_sum(double* buf, int64_t nbuf, int64_t src_off, int nslab, int64_t stride, int64_t count, int64_t dst_off, int acc_in) {
    Dev d;
    double* W = d.in(buf, nbuf);
    if (d.rc == hipSuccess) sf::launch_selinv_sum(W + src_off, nslab, stride, count, W + dst_off, acc_in, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

// Zu null: k_selinv_finish on S; otherwise k_lu_selinv_finish on (S, SU)
int kp_selinv_finish(const sf::SelUnit* u, const double* Z, const double* Zu, int64_t nZ, const double* Sc, int64_t nSc, double* S, double* SU,
                     int64_t narena) {
    Dev d;
    const double* dZ = d.in(Z, nZ);
    const double* dZu = Zu ? d.in(Zu, nZ) : nullptr;
    const double* dSc = d.in(Sc, nSc);
    double* dS = d.in(S, narena);
    double* dSU = Zu ? d.in(SU, narena) : nullptr;
    if (d.rc == hipSuccess) {
        if (Zu) sf::launch_lu_selinv_finish(*u, dZ, dZu, dSc, dS, dSU, 0);
        else sf::launch_selinv_finish(*u, dZ, dSc, dS, 0);
    }
    d.finish();
    d.out(S, dS, narena);
    if (Zu) d.out(SU, dSU, narena);
    return (int)d.rc;
}

// dg: nd doubles, in and out (the launch writes the first n)
int kp_selinv_diag(int64_t n, const double* S, int64_t narena, const KpSel* sel, int lu, double* dg, int64_t nd) {
    Dev d;
    const double* dS = d.in(S, narena);
    const sf::SelStruct t = sel_in(d, sel);
    double* D = d.in(dg, nd);
    if (d.rc == hipSuccess) {
        if (lu) sf::launch_lu_selinv_diag(n, dS, t, D, 0);
        else sf::launch_selinv_diag(n, dS, t, D, 0);
    }
    d.finish();
    d.out(dg, D, nd);
    return (int)d.rc;
}

// buf: nbuf doubles, in and out: ceil(n / 256) partial sums, then the result (one double; lu: two); neg: the counts (lu only)
int kp_logdet(int64_t n, const double* P, int64_t narena, const KpSel* sel, int lu, double* buf, int64_t nbuf, int32_t* neg, int64_t nneg) {
    Dev d;
    const double* dP = d.in(P, narena);
    const sf::SelStruct t = sel_in(d, sel);
    double* B = d.in(buf, nbuf);
    int32_t* G = lu ? d.in(neg, nneg) : nullptr;
    if (d.rc == hipSuccess) {
        if (lu) sf::launch_lu_logdet(n, dP, t, B, G, 0);
        else sf::launch_logdet(n, dP, t, B, 0);
    }
    d.finish();
    d.out(buf, B, nbuf);
    if (lu) d.out(neg, G, nneg);
    return (int)d.rc;
}

// out: nout doubles, in and out (the launch writes the first e_end - e_begin)
int kp_lu_selinv_pack(const KpSel* sel, const int64_t* RefXp, const double* SL, const double* SU, int64_t narena, double* out, int64_t nout,
                      int64_t e_begin, int64_t e_end) {
    Dev d;
    const sf::SelStruct t = sel_in(d, sel);
    const int64_t* RX = d.in(RefXp, sel->nsuper + 1);
    const double* dSL = d.in(SL, narena);
    const double* dSU = d.in(SU, narena);
    double* O = d.in(out, nout);
    if (d.rc == hipSuccess) sf::launch_lu_selinv_pack(t, RX, (int32_t)sel->nsuper, dSL, dSU, O, e_begin, e_end, 0);
    d.finish();
    d.out(out, O, nout);
    return (int)d.rc;
}

// ---- residual, refinement, reductions, sampling and transfers (sf_kernels.hip, sf_refine.hip, sf_gram.hip, sf_gram_lu.hip,
// sf_sample.hip, sf_device_io.hip): tests/test_kernels_apply.py ----
// Every double operand lies at an offset of ONE image `buf` (in and out), so that a test sees everything a launch wrote.

// Up null: (Lp, Li) is one triangle used symmetrically.  Values at buf + lx_off / ux_off; r, colsum, b: n doubles each, norms: 4
int kp_residual(const int64_t* Lp, const int32_t* Li, int64_t nnzL, const int64_t* Up, const int32_t* Ui, int64_t nnzU, int32_t n, double* buf,
                int64_t nbuf, int64_t lx_off, int64_t ux_off, int64_t x_off, int64_t r_off, int64_t c_off, int64_t b_off, int64_t norms_off) {
    Dev d;
    double* W = d.in(buf, nbuf);
    const int64_t* dLp = d.in(Lp, (int64_t)n + 1);
    const int32_t* dLi = d.in(Li, nnzL);
    const int64_t* dUp = Up ? d.in(Up, (int64_t)n + 1) : nullptr;
    const int32_t* dUi = Up ? d.in(Ui, nnzU) : nullptr;
    if (d.rc == hipSuccess)
        sf::launch_residual(dLp, dLi, W + lx_off, dUp, dUi, Up ? W + ux_off : nullptr, n, W + x_off, W + r_off, W + c_off, W + b_off,
                            W + norms_off, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

int kp_loadmap_drop(const int64_t* drop, int64_t count, int64_t* map, int64_t nmap) {
    Dev d;
    const int64_t* D = d.in(drop, count);
    int64_t* M = d.in(map, nmap);
    if (d.rc == hipSuccess) sf::launch_loadmap_drop(D, count, M, 0);
    d.finish();
    d.out(map, M, nmap);
    return (int)d.rc;
}

// the form's arrays: n + 1 pointers, nent entries; Vd / Vt at buf + vd_off / vt_off.  sums == 0: launch_refine_resid (x, b, r, w);
// otherwise launch_refine_abs_sums into the word at buf + amax_off
int kp_refine_resid(const int64_t* ptr, const int32_t* col, const int64_t* pos, int64_t nent, int64_t n, double* buf, int64_t nbuf,
                    int64_t vd_off, int64_t vt_off, int64_t x_off, int64_t b_off, int64_t r_off, int64_t w_off, int sums, int64_t amax_off) {
    Dev d;
    double* W = d.in(buf, nbuf);
    sf::RefineForm f;
    f.ptr = d.in(ptr, n + 1);
    f.col = d.in(col, nent);
    f.pos = d.in(pos, nent);
    f.Vd = W + vd_off;
    f.Vt = W + vt_off;
    if (d.rc == hipSuccess) {
        if (sums) sf::launch_refine_abs_sums(f, n, W + amax_off, 0);
        else sf::launch_refine_resid(f, n, W + x_off, W + b_off, W + r_off, W + w_off, 0);
    }
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

// use_info == 0: no info word (null)
int kp_refine_norms(int64_t n, double* buf, int64_t nbuf, int64_t r_off, int64_t w_off, int64_t x_off, int64_t b_off, int64_t s_off,
                    int use_info, int solve_info_value) {
    Dev d;
    double* W = d.in(buf, nbuf);
    const int* I = use_info ? d.in(&solve_info_value, 1) : nullptr;
    if (d.rc == hipSuccess) sf::launch_refine_norms(n, W + r_off, W + w_off, W + x_off, W + b_off, I, W + s_off, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

int kp_refine_update(int64_t n, double* buf, int64_t nbuf, int64_t x_off, int64_t d_off, int64_t best_off, int save) {
    Dev d;
    double* W = d.in(buf, nbuf);
    if (d.rc == hipSuccess) sf::launch_refine_update(n, W + x_off, W + d_off, W + best_off, save, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

int kp_gram_slabs(int64_t n, int64_t* slab_rows) { return sf::gram_slabs(n, slab_rows); }

int kp_gram_row(double* buf, int64_t nbuf, int64_t y_off, int64_t n, int a, int64_t k, int64_t part_off, int64_t g_off, int64_t ldg) {
    Dev d;
    double* W = d.in(buf, nbuf);
    if (d.rc == hipSuccess) sf::launch_gram_row(W + y_off, n, a, k, W + part_off, W + g_off, ldg, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

int kp_gram2_col(double* buf, int64_t nbuf, int64_t z_off, int64_t yb_off, int64_t n, int nza, int b, int64_t m, int64_t k, int64_t part_off,
                 int64_t g_off, int64_t ldg) {
    Dev d;
    double* W = d.in(buf, nbuf);
    if (d.rc == hipSuccess) sf::launch_gram2_col(W + z_off, W + yb_off, n, nza, b, m, k, W + part_off, W + g_off, ldg, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

int kp_dot(double* buf, int64_t nbuf, int64_t x_off, int64_t y_off, int64_t n, int64_t scratch_off, int64_t out_off) {
    Dev d;
    double* W = d.in(buf, nbuf);
    if (d.rc == hipSuccess) sf::launch_dot(W + x_off, W + y_off, n, W + scratch_off, W + out_off, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

int kp_quadform(double* buf, int64_t nbuf, int64_t x_off, int64_t n, int width, int64_t scratch_off) {
    Dev d;
    double* W = d.in(buf, nbuf);
    if (d.rc == hipSuccess) sf::launch_quadform(W + x_off, n, width, W + scratch_off, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

int kp_sample_fill(double* buf, int64_t nbuf, int64_t x_off, int64_t n, int cw, uint64_t seed, uint64_t s0) {
    Dev d;
    double* W = d.in(buf, nbuf);
    if (d.rc == hipSuccess) sf::launch_sample_fill(W + x_off, n, cw, seed, s0, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

// perm: n entries, or null
int kp_dev_load1(double* buf, int64_t nbuf, int64_t b_off, const int32_t* perm, int64_t n, int64_t x_off) {
    Dev d;
    double* W = d.in(buf, nbuf);
    const int32_t* P = perm ? d.in(perm, n) : nullptr;
    if (d.rc == hipSuccess) sf::launch_dev_load1(W + b_off, P, n, W + x_off, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

int kp_dev_store1(double* buf, int64_t nbuf, int64_t x_off, const int32_t* perm, int64_t n, int64_t out_off) {
    Dev d;
    double* W = d.in(buf, nbuf);
    const int32_t* P = perm ? d.in(perm, n) : nullptr;
    if (d.rc == hipSuccess) sf::launch_dev_store1(W + x_off, P, n, W + out_off, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

int kp_dev_pack(double* buf, int64_t nbuf, int64_t b_off, int64_t ldb, const int32_t* perm, int64_t n, int cw, int64_t x_off) {
    Dev d;
    double* W = d.in(buf, nbuf);
    const int32_t* P = perm ? d.in(perm, n) : nullptr;
    if (d.rc == hipSuccess) sf::launch_dev_pack(W + b_off, ldb, P, n, cw, W + x_off, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

int kp_dev_unpack(double* buf, int64_t nbuf, int64_t x_off, const int32_t* perm, int64_t n, int cw, int64_t d_off, int64_t ldx) {
    Dev d;
    double* W = d.in(buf, nbuf);
    const int32_t* P = perm ? d.in(perm, n) : nullptr;
    if (d.rc == hipSuccess) sf::launch_dev_unpack(W + x_off, P, n, cw, W + d_off, ldx, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

int kp_dev_gather_values(double* buf, int64_t nbuf, int64_t ax_off, const int64_t* map, int64_t count, int64_t out_off) {
    Dev d;
    double* W = d.in(buf, nbuf);
    const int64_t* M = d.in(map, count);
    if (d.rc == hipSuccess) sf::launch_dev_gather_values(W + ax_off, M, count, W + out_off, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

// *nparts = the launcher's return value: the parts written at buf + part_off
int kp_dev_absmax(double* buf, int64_t nbuf, int64_t v_off, int64_t count, int64_t part_off, int* nparts) {
    Dev d;
    double* W = d.in(buf, nbuf);
    if (d.rc == hipSuccess) *nparts = sf::launch_dev_absmax(W + v_off, count, W + part_off, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

// ---- Sigma on the pattern of A (csrc/sf_selinv_pattern.hip): tests/test_kernels_selpat.py ----
// No double arena: the launch computes offsets and dereferences none.  pos: npos words, offd: npos bytes or null, both in and out
int kp_selpat_build(const int64_t* Lp, const int32_t* Li, int32_t n, const int32_t* Super, const int32_t* SuperMap, int32_t nsuper,
                    const int64_t* Lsip, const int32_t* Lsi, const int64_t* Xp, int64_t* pos, uint8_t* offd, int64_t npos) {
    Dev d;
    const int64_t* dLp = d.in(Lp, (int64_t)n + 1);
    const int32_t* dLi = d.in(Li, Lp[n]);
    const int32_t* dS = d.in(Super, (int64_t)nsuper + 1);
    const int32_t* dSM = d.in(SuperMap, n);
    const int64_t* dLsip = d.in(Lsip, (int64_t)nsuper + 1);
    const int32_t* dLsi = d.in(Lsi, Lsip[nsuper]);
    const int64_t* dXp = d.in(Xp, (int64_t)nsuper + 1);
    int64_t* dpos = d.in(pos, npos);
    uint8_t* doffd = offd ? d.in(offd, npos) : nullptr;
    if (d.rc == hipSuccess) sf::launch_selpat_build(dLp, dLi, n, dS, dSM, dLsip, dLsi, dXp, dpos, doffd, 0);
    d.finish();
    d.out(pos, dpos, npos);
    if (offd) d.out(offd, doffd, npos);
    return (int)d.rc;
}

// pos: count entries
int kp_selpat_gather(double* buf, int64_t nbuf, int64_t s_off, const int64_t* pos, int64_t count, int64_t out_off) {
    Dev d;
    double* W = d.in(buf, nbuf);
    const int64_t* dpos = d.in(pos, count);
    if (d.rc == hipSuccess) sf::launch_selpat_gather(dpos, count, W + s_off, W + out_off, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

// map, offd (or null), vmap (or null): nmap entries each (nmap >= count: what lies past count is the test's); *launched = the
// launcher's return value
int kp_selpat_part(int mapped, const int64_t* map, const uint8_t* offd, const int64_t* vmap, int64_t nmap, int64_t count, double* buf,
                   int64_t nbuf, int64_t s_off, int64_t shift, int64_t v_off, int64_t ldv, int m, int64_t part_off, int64_t part0,
                   int64_t nparts, int64_t* launched) {
    Dev d;
    double* W = d.in(buf, nbuf);
    const int64_t* dmap = d.in(map, nmap);
    const uint8_t* doffd = offd ? d.in(offd, nmap) : nullptr;
    const int64_t* dvmap = vmap ? d.in(vmap, nmap) : nullptr;
    if (d.rc == hipSuccess)
        *launched = sf::launch_selpat_part(mapped != 0, dmap, doffd, count, W + s_off, shift, W + v_off, ldv, dvmap, m, W + part_off, part0,
                                           nparts, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

int kp_selpat_final(double* buf, int64_t nbuf, int64_t part_off, int64_t nparts, int m, int64_t out_off) {
    Dev d;
    double* W = d.in(buf, nbuf);
    if (d.rc == hipSuccess) sf::launch_selpat_final(W + part_off, nparts, m, W + out_off, 0);
    d.finish();
    d.out(buf, W, nbuf);
    return (int)d.rc;
}

// rows, cols: count entries; the arena(s) at buf + s_off (lu: the second one xC doubles behind); *outside in and out
int kp_selpat_entries(const int64_t* rows, const int64_t* cols, int64_t count, int lu, int64_t xC, double* buf, int64_t nbuf, int64_t s_off,
                      const KpSel* sel, int64_t out_off, unsigned long long* outside) {
    Dev d;
    double* W = d.in(buf, nbuf);
    const int64_t* R = d.in(rows, count);
    const int64_t* Cc = d.in(cols, count);
    const sf::SelStruct t = sel_in(d, sel);
    unsigned long long* O = d.in(outside, 1);
    if (d.rc == hipSuccess) sf::launch_selpat_entries(R, Cc, count, lu, xC, W + s_off, t, W + out_off, O, 0);
    d.finish();
    d.out(buf, W, nbuf);
    d.out(outside, O, 1);
    return (int)d.rc;
}

}  // extern "C"
