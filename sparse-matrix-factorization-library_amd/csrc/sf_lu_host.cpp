// libsparseframe_lu_hip.so: the reference's struct-based entry points over the LU layout of matrix_info_struct
// (LU/Include/info.h), forwarding to the flat ABI of libsparseframe_hip.so (sf_symbolic_create_lu, sf_lu_plan_*).  What both
// libraries do alike is in sf_struct_path.inc; here are the export of the symbolic arrays, the factorization and the pivoting controls.
// Reference file: LU/Source/SparseFrame.c ("L:").
#include "sf_host_solve.h"
#include "sf_struct_common.h"
#include <sparseframe_lu_hip.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>

namespace {

sf_long* dup_long(const sf_symbolic* S, const char* name, sf_long min_len = 1) {
    sf_long len = 0;
    const sf_long* src = sf_symbolic_long_array(S, name, &len);
    sf_long* p = (sf_long*)calloc((size_t)(len > min_len ? len : min_len), sizeof(sf_long));
    if (p && src && len > 0) memcpy(p, src, (size_t)len * sizeof(sf_long));
    return p;
}
sf_float* dup_float(const sf_symbolic* S, const char* name) {
    sf_long len = 0;
    const sf_float* src = sf_symbolic_float_array(S, name, &len);
    sf_float* p = (sf_float*)calloc((size_t)(len > 1 ? len : 1), sizeof(sf_float));
    if (p && src && len > 0) memcpy(p, src, (size_t)len * sizeof(sf_float));
    return p;
}

// per-matrix_info pivoting policy (SparseFrame_set_matrix_pivoting): side table keyed by the struct's address
std::mutex g_mi_piv_mu;
std::unordered_map<const void*, std::pair<double, double>> g_mi_piv;

// what sf_struct_path.inc asks of its library
const enum FactorizeType kFactorizeType = TYPE_LU;
const bool kLU = true;
sf_struct::Upper upper_of(const struct matrix_info_struct* mi) {
    if (mi->isSymmetric) return {nullptr, nullptr, nullptr, mi->PivInv};       // U aliases L
    return {mi->Up, mi->Ui, mi->Ux, mi->PivInv};
}
void free_lu_fields(struct matrix_info_struct* mi, bool cleanup) {
    SF_FREE(Up); SF_FREE(Ui); SF_FREE(Ux); SF_FREE(UTp); SF_FREE(UTi); SF_FREE(UTx);
    SF_FREE(PivInv);            // sized by nrow at the next factorization (a re-analysis may follow a read of a larger matrix)
    if (cleanup) { SF_FREE(CPCTp); SF_FREE(CPCTi); }        // never produced here (sparseframe_lu_hip.h): a re-analysis leaves them
}
void drop_matrix_pivoting(const struct matrix_info_struct* mi) {
    std::lock_guard<std::mutex> g(g_mi_piv_mu);
    g_mi_piv.erase((const void*)mi);
}

}  // namespace

extern "C" {

long sf_lu_abi_layout(const char* name) {
    if (!name) return -1;
    const std::string k(name);
    if (k == "sizeof_common") return (long)sizeof(struct common_info_struct);
    if (k == "sizeof_matrix") return (long)sizeof(struct matrix_info_struct);
    if (k == "offsetof_Lsx") return (long)offsetof(struct matrix_info_struct, Lsx);
    if (k == "offsetof_Up") return (long)offsetof(struct matrix_info_struct, Up);
    if (k == "offsetof_workspace") return (long)offsetof(struct matrix_info_struct, workspace);
    if (k == "offsetof_residual") return (long)offsetof(struct matrix_info_struct, residual);
    return -1;
}

#include "sf_struct_path.inc"

// the handler list is the main library's (sf_handlers.hip): one handler per device, plan cache, overlapped copy-back
int SparseFrame_allocate_gpu(struct common_info_struct* common, struct gpu_info_struct** list) { return sf_handlers_allocate(common, list); }   // L:16-285
int SparseFrame_free_gpu(struct common_info_struct* common, struct gpu_info_struct** list) { return sf_handlers_free(common, list); }       // L:287-366

int SparseFrame_analyze(struct common_info_struct* common, struct matrix_info_struct* mi) {   // L:2233-2458
    if (!common || !mi || !mi->Cp) return 1;
    const double t0 = sf_struct::wall_seconds();
    sf_symbolic* S = nullptr;
    const sf_long* perm = nullptr;
    std::vector<sf_long> builtin;
    if (analysis_perm(mi, builtin, &perm)) return 1;
    if (sf_symbolic_create_lu(&S, mi->nrow, mi->Cp, mi->Ci, mi->Cx, perm, common->devSlotSize, mi->isSymmetric)) return 1;

    free_analysis(mi, false);
    SF_FREE(Lsx);

    mi->Lp = dup_long(S, "Lp"); mi->Li = dup_long(S, "Li"); mi->Lx = dup_float(S, "Lx");
    mi->LTp = dup_long(S, "LTp"); mi->LTi = dup_long(S, "LTi"); mi->LTx = dup_float(S, "LTx");
    if (!mi->isSymmetric) {
        mi->Up = dup_long(S, "Up"); mi->Ui = dup_long(S, "Ui"); mi->Ux = dup_float(S, "Ux");
        mi->UTp = dup_long(S, "UTp"); mi->UTi = dup_long(S, "UTi"); mi->UTx = dup_float(S, "UTx");
    }
    mi->Perm = dup_long(S, "Perm");
    mi->Parent = dup_long(S, "Parent");
    mi->Post = dup_long(S, "Post");
    mi->ColCount = dup_long(S, "ColCount");
    mi->nsuper = sf_symbolic_scalar(S, "nsuper");
    mi->Super = dup_long(S, "Super", mi->nrow + 1);      // the reference allocates nrow+1 / nrow entries (L:2449-2451)
    mi->SuperMap = dup_long(S, "SuperMap");
    mi->Sparent = dup_long(S, "Sparent", mi->nrow);
    mi->nsleaf = sf_symbolic_scalar(S, "nsleaf");
    mi->LeafQueue = dup_long(S, "LeafQueue");
    mi->isize = sf_symbolic_scalar(S, "isize");
    mi->xsize = sf_symbolic_scalar(S, "xsize");
    mi->Lsip = dup_long(S, "Lsip"); mi->Lsxp = dup_long(S, "Lsxp"); mi->Lsi = dup_long(S, "Lsi");
    mi->Lsx = (sf_float*)malloc((size_t)(mi->xsize > 0 ? mi->xsize : 1) * sizeof(sf_float));
    mi->csize = sf_symbolic_scalar(S, "csize");
    mi->nstage = sf_symbolic_scalar(S, "nstage");
    mi->ST_Map = dup_long(S, "ST_Map"); mi->ST_Pointer = dup_long(S, "ST_Pointer"); mi->ST_Index = dup_long(S, "ST_Index");
    mi->ST_Parent = nullptr;
    mi->Aoffset = (size_t*)dup_long(S, "Aoffset");      // size_t and int64_t have the same size and non-negative values
    mi->Moffset = (size_t*)dup_long(S, "Moffset");
    sf_symbolic_destroy(S);
    mi->analyzeTime = sf_struct::wall_seconds() - t0;
    return mi->Lsx ? 0 : 1;
}

int SparseFrame_factorize_supernodal(struct common_info_struct* common, struct gpu_info_struct* list,
                                     struct matrix_info_struct* mi) {   // L:2668-3573
    if (!common || !mi || !mi->Lsx) return SF_ERR_ARG;
    // PivInv (LU/Include/info.h: the field of the reference's disabled static pre-pivot, L:589-673) carries the record of the
    // in-block interchanges: PivInv[g] = row position of original row g (same 64-column block); identity when nothing moved
    if (!mi->PivInv) mi->PivInv = (sf_long*)malloc((size_t)(mi->nrow > 0 ? mi->nrow : 1) * sizeof(sf_long));
    if (!mi->PivInv) return SF_ERR_ALLOC;
    for (sf_long j = 0; j < mi->nrow; ++j) mi->PivInv[j] = j;
    {
        std::lock_guard<std::mutex> g(g_mi_piv_mu);
        auto it = g_mi_piv.find((const void*)mi);
        if (it != g_mi_piv.end()) (void)sf_handlers_set_lu_pivoting_next_call(it->second.first, it->second.second);
    }
    return sf_handlers_factorize(common, list, 1, mi->serial, mi->nrow, mi->nsuper, mi->Super, mi->SuperMap, mi->Lsip, mi->Lsi,
                                 mi->Lsxp, mi->Lp, mi->Li, mi->isSymmetric ? nullptr : mi->Up, mi->isSymmetric ? nullptr : mi->Ui,
                                 mi->Lx, mi->isSymmetric ? nullptr : mi->Ux, mi->Lsx, mi->PivInv);
}

// Pivoting is opt-in: by default the factor is the reference's (no interchanges, PivInv = identity, nothing perturbed).
// SparseFrame_set_pivoting: the process-wide default of the struct path.  SparseFrame_set_matrix_pivoting: ONE matrix_info's own
// setting (the reference's driver runs MATRIX_THREAD_NUM matrices at a time over one handler list, L:3375: two matrices may want
// different policies).  matrix_info_struct is the reference's layout and has no field for it, so the setting lives in a side table
// keyed by the struct's address; SparseFrame_initialize_matrix / _cleanup_matrix drop it.
int SparseFrame_set_pivoting(double tol, double perturb) { return sf_handlers_set_lu_pivoting(tol, perturb); }
int SparseFrame_set_matrix_pivoting(struct matrix_info_struct* mi, double tol, double perturb) {
    if (!mi || !(tol >= 0.0) || tol > 1.0 || !(perturb >= 0.0)) return SF_ERR_ARG;
    std::lock_guard<std::mutex> g(g_mi_piv_mu);
    g_mi_piv[(const void*)mi] = {tol, perturb};
    return SF_OK;
}
int SparseFrame_clear_matrix_pivoting(struct matrix_info_struct* mi) {
    drop_matrix_pivoting(mi);
    return SF_OK;
}
sf_long SparseFrame_perturbed_pivots(const struct matrix_info_struct* mi) {
    return (mi && mi->Lsx) ? (sf_long)sf_handlers_perturbed_pivots(mi->Lsx) : -1;
}

int SparseFrame_factorize(struct common_info_struct* common, struct gpu_info_struct* list, struct matrix_info_struct* mi) {
    const double t0 = sf_struct::wall_seconds();
    const int rc = SparseFrame_factorize_supernodal(common, list, mi);
    if (mi) mi->factorizeTime = sf_struct::wall_seconds() - t0;
    return rc;
}

#include "sf_driver.inc"

}  // extern "C"
