// The struct entry points that are the same in both libraries, written over the fields of matrix_info_struct: matrix set-up, the
// MatrixMarket reader, the ordering, the triangular solve, validation and clean-up (Cholesky/Source/SparseFrame.c "C:", and the same
// functions of LU/Source/SparseFrame.c).  Included by sf_chol_host.cpp and sf_lu_host.cpp inside extern "C", as sf_driver.inc is and
// for the same reason: each library has its own struct layout behind the same names, so no translation unit can see both.  What
// needs no struct is in sf_struct_common.h and sf_host_solve.h.  The including file says what differs, before this point:
//   const FactorizeType kFactorizeType                               TYPE_CHOLESKY / TYPE_LU
//   const bool kLU                                              the panel layout and sweeps of sf_host_solve.h
//   sf_struct::Upper upper_of(const matrix_info_struct*)        the U arrays and PivInv for the solve and the residual, or nulls
//   void free_lu_fields(matrix_info_struct*, bool cleanup)      the pointers only the LU layout has (free_analysis below)
//   void drop_matrix_pivoting(const matrix_info_struct*)        the LU library's per-matrix pivoting policy

int SparseFrame_initialize_matrix(struct matrix_info_struct* mi) {  // C:589-650
    if (!mi) return 1;
    drop_matrix_pivoting(mi);
    const int serial = mi->serial;
    const char* path = mi->path;
    memset(mi, 0, sizeof(*mi));
    mi->serial = serial;
    mi->path = path;
    mi->factorizeType = kFactorizeType;
    // the reference's analyze always orders with METIS (C:1937); here PERM_METIS with no Perm supplied selects the
    // built-in nested dissection, and natural order is an explicit opt-in: SparseFrame_set_perm(mi, NULL)
    mi->permMethod = PERM_METIS;
    return 0;
}

int SparseFrame_set_matrix_csc(struct matrix_info_struct* mi, sf_long nrow, sf_long nz,
                               const sf_long* Cp, const sf_long* Ci, const sf_float* Cx, int isSymmetric) {
    if (!mi || nrow < 0 || nz < 0 || !Cp || (nz > 0 && (!Ci || !Cx))) return 1;
    if (Cp[0] != 0 || Cp[nrow] != nz) return 1;
    SF_FREE(Cp); SF_FREE(Ci); SF_FREE(Cx); SF_FREE(workspace);
    if (nrow != mi->nrow) SF_FREE(Perm);     // an ordering (the caller's, or the last analysis') of another size: analyze would read past it
    mi->isSymmetric = isSymmetric;
    mi->isComplex = 0;
    mi->nrow = mi->ncol = nrow;
    mi->nzmax = nz;
    mi->Cp = (sf_long*)malloc((nrow + 1) * sizeof(sf_long));
    mi->Ci = (sf_long*)malloc((nz > 0 ? nz : 1) * sizeof(sf_long));
    mi->Cx = (sf_float*)malloc((nz > 0 ? nz : 1) * sizeof(sf_float));
    // workspace sized as C:679-684 (the idx_t term is the same size with 64-bit idx_t), its second term kept from going negative;
    // factorize carves 8*nsuper Longs out of it (C:2221-2228); nsuper <= nrow so 10*nrow covers it
    mi->workSize = (size_t)(10 * nrow + (2 * nz - nrow > 0 ? 2 * nz - nrow : 0) + 1) * sizeof(sf_long);
    mi->workspace = malloc(mi->workSize);
    if (!mi->Cp || !mi->Ci || !mi->Cx || !mi->workspace) return 1;
    memcpy(mi->Cp, Cp, (nrow + 1) * sizeof(sf_long));
    if (nz > 0) {
        memcpy(mi->Ci, Ci, nz * sizeof(sf_long));
        memcpy(mi->Cx, Cx, nz * sizeof(sf_float));
    }
    return 0;
}

int SparseFrame_read_matrix(struct matrix_info_struct* mi) {
    if (!mi || !mi->path) return 1;
    const double t0 = sf_struct::wall_seconds();
    sf_long n = 0;
    int symmetric = 0;
    std::vector<sf_long> Cp, Ci;
    std::vector<sf_float> Cx;
    if (sf_struct::read_matrix_market(mi->path, &n, Cp, Ci, Cx, &symmetric)) return 1;
    const int rc = SparseFrame_set_matrix_csc(mi, n, (sf_long)Cx.size(), Cp.data(), Ci.data(), Cx.data(), symmetric);
    mi->readTime = sf_struct::wall_seconds() - t0;
    return rc;
}

int SparseFrame_set_perm(struct matrix_info_struct* mi, const sf_long* perm) {
    if (!mi || mi->nrow <= 0) return 1;
    SF_FREE(Perm);
    if (!perm) { mi->permMethod = PERM_IDENTITY; return 0; }
    mi->Perm = (sf_long*)malloc(mi->nrow * sizeof(sf_long));
    if (!mi->Perm) return 1;
    memcpy(mi->Perm, perm, mi->nrow * sizeof(sf_long));
    mi->permMethod = PERM_METIS;  // "externally ordered"
    return 0;
}

// The ordering SparseFrame_analyze hands on: none (identity by opt-in), the caller's (SparseFrame_set_perm), or the built-in BFS
// nested dissection of the pattern of A + A^T, kept in `builtin` (the reference orders with METIS_NodeND here, C:1937 / L:2271).
static int analysis_perm(const struct matrix_info_struct* mi, std::vector<sf_long>& builtin, const sf_long** perm) {
    *perm = nullptr;
    if (mi->permMethod == PERM_IDENTITY) return 0;
    if (!(*perm = mi->Perm)) {
        builtin.resize(mi->nrow > 0 ? mi->nrow : 1);
        if (sf_graph_nd_perm(mi->nrow, mi->Cp, mi->Ci, 64, builtin.data())) return 1;
        *perm = builtin.data();
    }
    return 0;
}

// what SparseFrame_analyze and _factorize allocate, except Lsx (a re-analysis and the clean-up release that one differently);
// `cleanup`: also the LU layout's fields that only a caller can have set
static void free_analysis(struct matrix_info_struct* mi, bool cleanup) {
    SF_FREE(Lp); SF_FREE(Li); SF_FREE(Lx); SF_FREE(LTp); SF_FREE(LTi); SF_FREE(LTx);
    SF_FREE(Perm); SF_FREE(Post); SF_FREE(Parent); SF_FREE(ColCount);
    SF_FREE(Super); SF_FREE(SuperMap); SF_FREE(Sparent); SF_FREE(LeafQueue);
    SF_FREE(Lsip); SF_FREE(Lsxp); SF_FREE(Lsi);
    SF_FREE(ST_Map); SF_FREE(ST_Pointer); SF_FREE(ST_Index); SF_FREE(Aoffset); SF_FREE(Moffset);
    free_lu_fields(mi, cleanup);
}

// Forward and backward supernodal substitution, permuted space (C:3036-3139, L:3592-3700).
int SparseFrame_solve_supernodal(struct matrix_info_struct* mi) {
    if (!mi || !mi->Lsx || !mi->Bx || !mi->Xx) return 1;
    const double t0 = sf_struct::wall_seconds();
    const sf_struct::Upper U = upper_of(mi);
    // the factor SparseFrame_factorize copied into Lsx is normally still resident in the handler's plan: solve there (two sweeps
    // over the factor in HBM instead of host memory).  Falls through to the reference's host solve when it is not (several
    // handlers, plan evicted or re-used, Lsx changed by the caller, SF_SOLVE=host).
    if (sf_handlers_solve_resident_sym(mi->Lsx, mi->Bx, mi->Xx, kLU, mi->nrow, mi->nsuper, mi->Super, mi->SuperMap, mi->Lsip, mi->Lsi,
                                       mi->Lsxp, mi->Lp, mi->Li, U.p, U.i) != SF_OK) {
        memcpy(mi->Xx, mi->Bx, mi->nrow * sizeof(double));
        // a large factor: the two sweeps on several threads; otherwise, or with no partition to be had, the reference's scalar sweep
        // (the top is shared by all threads: a top flop costs 1 / T of a subtree flop, plus the barriers)
        const int T = sf_host_solve::threads_for(mi->xsize);
        std::vector<int32_t> owner(T > 1 ? (size_t)(mi->nsuper > 0 ? mi->nsuper : 1) : 0, 0);
        if (T > 1 && sf_subtree_partition_weighted(mi->nsuper, mi->Super, mi->SuperMap, mi->Lsip, mi->Lsi, T, 1.0 / T + 0.05, owner.data(),
                                                   nullptr, nullptr) == SF_OK)
            sf_host_solve::solve_parallel<kLU>(mi->nrow, mi->nsuper, mi->Super, mi->SuperMap, mi->Lsip, mi->Lsi, mi->Lsxp, mi->Lsx,
                                               U.PivInv, owner.data(), T, mi->Xx);
        else
            sf_host_solve::solve_scalar<kLU>(mi->nsuper, mi->Super, mi->Lsip, mi->Lsi, mi->Lsxp, mi->Lsx, U.PivInv, mi->Xx);
    }
    mi->solveTime = sf_struct::wall_seconds() - t0;
    return 0;
}

// b_i = 1 + i/n, solve, r = A x - b, residual = |r|_inf / (|A|_1 |x|_inf + |b|_inf)   (C:3141-3266, L:3702-3858)
int SparseFrame_validate(struct matrix_info_struct* mi) {
    if (!mi || !mi->Lp || !mi->Lsx) return 1;
    const sf_long n = mi->nrow;
    SF_FREE(Bx); SF_FREE(Xx); SF_FREE(Rx);
    mi->Bx = (double*)malloc((n > 0 ? n : 1) * sizeof(double));
    mi->Xx = (double*)malloc((n > 0 ? n : 1) * sizeof(double));
    mi->Rx = (double*)malloc((n > 0 ? n : 1) * sizeof(double));
    if (!mi->Bx || !mi->Xx || !mi->Rx) return 1;
    sf_struct::fill_rhs(n, mi->Bx);
    if (SparseFrame_solve_supernodal(mi)) return 1;
    const sf_struct::Upper U = upper_of(mi);
    mi->residual = sf_struct::residual(n, mi->Lp, mi->Li, mi->Lx, U.p, U.i, U.x, mi->Xx, mi->Bx, mi->Rx);
    return 0;
}

int SparseFrame_cleanup_matrix(struct matrix_info_struct* mi) {  // C:3268-3321
    if (!mi) return 1;
    sf_handlers_forget(mi->Lsx);
    SF_FREE(Tj); SF_FREE(Ti); SF_FREE(Tx);
    SF_FREE(Cp); SF_FREE(Ci); SF_FREE(Cx);
    free_analysis(mi, true);
    SF_FREE(workspace);
    SF_FREE(Bx); SF_FREE(Xx); SF_FREE(Rx);
    // Lsx LAST: a concurrent munmap of tens of GB makes every other munmap wait
    sf_struct::free_big_async(mi->Lsx, (size_t)(mi->xsize > 0 ? mi->xsize : 0) * sizeof(sf_float));
    // keep the timers and the residual readable after clean-up, as the reference's driver
    // prints them after calling this (C:3423-3433)
    const double rt = mi->readTime, at = mi->analyzeTime, ft = mi->factorizeTime, st = mi->solveTime;
    const double res = mi->residual;
    SparseFrame_initialize_matrix(mi);
    mi->readTime = rt; mi->analyzeTime = at; mi->factorizeTime = ft; mi->solveTime = st;
    mi->residual = res;
    return 0;
}
