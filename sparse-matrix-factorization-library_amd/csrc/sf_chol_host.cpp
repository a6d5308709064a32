// libsparseframe_hip.so: the reference's struct-based entry points over the Cholesky layout of matrix_info_struct
// (Cholesky/Include/info.h, "I:"), as sf_lu_host.cpp has them over the LU layout.  What both libraries do alike is in
// sf_struct_path.inc; here are the export of the symbolic arrays and the factorization.
// Reference file: Cholesky/Source/SparseFrame.c ("C:").
#include "sf_host_solve.h"
#include "sf_struct_common.h"
#include <sparseframe_hip.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <mutex>
#include <string>

#include "sf_symbolic.h"

using sf::Long;

namespace {

template <class T, class A>
T* dup_array(const std::vector<T, A>& v, size_t min_elems = 1) {
    const size_t n = v.size() > min_elems ? v.size() : min_elems;
    T* p = (T*)malloc(n * sizeof(T));
    // (one thread: splitting the copy of the big arrays -- 16 - 80 MB each, first touch of fresh pages -- over four threads made
    // SparseFrame_analyze 0.45 s SLOWER at 128^3, 1.41 - 1.49 s against 1.10: concurrent first-touch faults of one process serialise on
    // its address-space lock, the effect that also ruled out page-populating helpers for Lsx)
    if (p && !v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

// hand a RawVec's buffer to the caller as it is (malloc'ed: sf_symbolic.h); the vector keeps pointing at it until it is destroyed, its
// deallocate then skips the stolen pointer.  Empty vectors get the one-element block the reference's callers may index.
template <class T>
T* steal_array(sf::RawVec<T>& v) {
    if (v.empty()) return (T*)malloc(sizeof(T));
    sf::raw_mark_stolen(v.data());
    return v.data();
}

// what sf_struct_path.inc asks of its library: no U, no interchanges, no fields or side table beyond the common ones
const enum FactorizeType kFactorizeType = TYPE_CHOLESKY;
const bool kLU = false;
sf_struct::Upper upper_of(const struct matrix_info_struct*) { return {nullptr, nullptr, nullptr, nullptr}; }
void free_lu_fields(struct matrix_info_struct*, bool) {}
void drop_matrix_pivoting(const struct matrix_info_struct*) {}

}  // namespace

extern "C" {

long sf_abi_layout(const char* name) {
    if (!name) return -1;
    const std::string k(name);
    if (k == "sizeof_common") return (long)sizeof(struct common_info_struct);
    if (k == "sizeof_matrix") return (long)sizeof(struct matrix_info_struct);
    if (k == "offsetof_Lsx") return (long)offsetof(struct matrix_info_struct, Lsx);
    if (k == "offsetof_workspace") return (long)offsetof(struct matrix_info_struct, workspace);
    if (k == "offsetof_residual") return (long)offsetof(struct matrix_info_struct, residual);
    if (k == "offsetof_devSlotSize") return (long)offsetof(struct common_info_struct, devSlotSize);
    return -1;
}

#include "sf_struct_path.inc"

// the handler list is sf_handlers.hip's: one handler per device, plan cache, overlapped copy-back
int SparseFrame_allocate_gpu(struct common_info_struct* common, struct gpu_info_struct** list) { return sf_handlers_allocate(common, list); }   // C:16-285
int SparseFrame_free_gpu(struct common_info_struct* common, struct gpu_info_struct** list) { return sf_handlers_free(common, list); }       // C:287-366

// The symbolic arrays go from sf::Symbolic to the struct directly, the large ones without a copy (steal_array): the by-name copies
// of the flat ABI that the LU library takes would first-touch every one of them a second time.
int SparseFrame_analyze(struct common_info_struct* common, struct matrix_info_struct* mi) {  // C:1916-1978
    if (!common || !mi || !mi->Cp) return 1;
    const double t0 = sf_struct::wall_seconds();
    sf::Symbolic S;
    const sf_long* perm = nullptr;
    std::vector<sf_long> builtin;
    if (analysis_perm(mi, builtin, &perm)) return 1;
    int rc = sf::analyze_cholesky(mi->nrow, mi->Cp, mi->Ci, mi->Cx, perm, common->devSlotSize, S);
    if (rc) return rc;

    free_analysis(mi, false);
    SF_FREE(Lsx);

    mi->Lp = dup_array(S.Lp);   mi->Li = steal_array(S.Li);   mi->Lx = steal_array(S.Lx);
    mi->LTp = dup_array(S.LTp); mi->LTi = steal_array(S.LTi); mi->LTx = steal_array(S.LTx);
    mi->Perm = dup_array(S.Perm);
    mi->Parent = dup_array(S.Parent);
    mi->Post = dup_array(S.Post);
    mi->ColCount = dup_array(S.ColCount);
    mi->nsuper = S.nsuper;
    // the reference allocates Super with nrow+1 entries, SuperMap/Sparent with nrow (C:1969-1971)
    mi->Super = (sf_long*)calloc(mi->nrow + 1, sizeof(sf_long));
    mi->Sparent = (sf_long*)calloc(mi->nrow > 0 ? mi->nrow : 1, sizeof(sf_long));
    if (mi->Super) memcpy(mi->Super, S.Super.data(), S.Super.size() * sizeof(sf_long));
    if (mi->Sparent && S.nsuper) memcpy(mi->Sparent, S.Sparent.data(), S.nsuper * sizeof(sf_long));
    mi->SuperMap = dup_array(S.SuperMap);
    mi->nsleaf = S.nsleaf;
    mi->LeafQueue = dup_array(S.LeafQueue);
    mi->isize = S.isize;
    mi->xsize = S.xsize;
    mi->Lsip = dup_array(S.Lsip);
    mi->Lsxp = dup_array(S.Lsxp);
    mi->Lsi = steal_array(S.Lsi);
    mi->Lsx = (sf_float*)malloc((S.xsize > 0 ? S.xsize : 1) * sizeof(sf_float));  // output, C:1647-1651
    mi->csize = S.csize;
    mi->nstage = S.nstage;
    mi->ST_Map = dup_array(S.ST_Map);
    mi->ST_Pointer = dup_array(S.ST_Pointer);
    mi->ST_Index = dup_array(S.ST_Index);
    mi->ST_Parent = nullptr;
    mi->Aoffset = (size_t*)malloc((S.nsuper > 0 ? S.nsuper : 1) * sizeof(size_t));
    mi->Moffset = (size_t*)malloc((S.nsuper > 0 ? S.nsuper : 1) * sizeof(size_t));
    if (!mi->Lsx || !mi->Aoffset || !mi->Moffset || !mi->Super || !mi->Sparent) return 1;
    for (Long s = 0; s < S.nsuper; ++s) {
        mi->Aoffset[s] = (size_t)S.Aoffset[s];
        mi->Moffset[s] = (size_t)S.Moffset[s];
    }
    mi->analyzeTime = sf_struct::wall_seconds() - t0;
    return 0;
}

int SparseFrame_factorize_supernodal(struct common_info_struct* common, struct gpu_info_struct* list,
                                     struct matrix_info_struct* mi) {   // C:2150-3017
    if (!common || !mi || !mi->Lsx) return SF_ERR_ARG;
    return sf_handlers_factorize(common, list, 0, mi->serial, mi->nrow, mi->nsuper, mi->Super, mi->SuperMap, mi->Lsip, mi->Lsi,
                                 mi->Lsxp, mi->Lp, mi->Li, nullptr, nullptr, mi->Lx, nullptr, mi->Lsx, nullptr);
}

int SparseFrame_factorize(struct common_info_struct* common, struct gpu_info_struct* list, struct matrix_info_struct* mi) {   // C:3019-3034
    const double t0 = sf_struct::wall_seconds();
    const int rc = SparseFrame_factorize_supernodal(common, list, mi);
    if (mi) mi->factorizeTime = sf_struct::wall_seconds() - t0;
    return rc;
}

#include "sf_driver.inc"

}  // extern "C"
