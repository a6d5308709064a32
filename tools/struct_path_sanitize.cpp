// The struct entry points (csrc/sf_struct_path.inc, sf_struct_common.h, sf_host_solve.h under csrc/sf_chol_host.cpp or
// csrc/sf_lu_host.cpp) on a CPU: initialize -> read -> analyze -> validate -> cleanup on small MatrixMarket files this program
// writes, with a factor it makes itself by dense elimination of the permuted matrix and places by the layout sf_host_solve.h
// documents; a re-read of a larger matrix into the same struct, the ill-formed files of tests/test_abi.py, clean-up twice.  No GPU,
// no HIP: the few sf_handlers_* functions the entry points call are stubs below (no device, no resident factor).
// tests/test_struct_path_host.py builds this file twice under ASan + UBSan -- with sf_chol_host.cpp, and with -DSF_STRUCT_LU and
// sf_lu_host.cpp (the two public headers define different layouts under one struct name) -- each time with sf_host.cpp and
// sf_symbolic.cpp.  argv[1]: a directory to write to.  Prints "struct_path_sanitize: ok" and returns 0.
#ifdef SF_STRUCT_LU
#include <sparseframe_lu_hip.h>
static const bool kLU = true;
#else
#include <sparseframe_hip.h>
static const bool kLU = false;
#endif

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" {
int sf_handlers_allocate(struct common_info_struct*, struct gpu_info_struct** list) { if (list) *list = nullptr; return SF_ERR_NO_DEVICE; }
int sf_handlers_free(struct common_info_struct*, struct gpu_info_struct**) { return SF_OK; }
int sf_handlers_factorize(struct common_info_struct*, struct gpu_info_struct*, int, int, sf_long, sf_long, const sf_long*, const sf_long*,
                          const sf_long*, const sf_long*, const sf_long*, const sf_long*, const sf_long*, const sf_long*, const sf_long*,
                          const sf_float*, const sf_float*, sf_float*, sf_long*) { return SF_ERR_NO_DEVICE; }
int sf_handlers_solve_resident_sym(const sf_float*, const sf_float*, sf_float*, int, sf_long, sf_long, const sf_long*, const sf_long*,
                                   const sf_long*, const sf_long*, const sf_long*, const sf_long*, const sf_long*, const sf_long*,
                                   const sf_long*) { return SF_ERR_ARG; }       // not resident
void sf_handlers_forget(const sf_float*) {}
int sf_handlers_set_lu_pivoting(double, double) { return SF_OK; }
int sf_handlers_set_lu_pivoting_next_call(double, double) { return SF_OK; }
int64_t sf_handlers_perturbed_pivots(const sf_float*) { return -1; }
}

static int g_fail = 0;
static std::string g_case;
#define CHECK(cond)                                                                                           \
    do {                                                                                                      \
        if (!(cond) && ++g_fail <= 20) printf("FAIL %s: %s (line %d)\n", g_case.c_str(), #cond, __LINE__);     \
    } while (0)

typedef std::vector<std::vector<double>> Dense;

static unsigned long long g_seed = 20240229;
static double rnd() { g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull; return (double)(g_seed >> 40) / (double)(1 << 24) - 0.5; }

// the 5-point stencil on a gx x gy grid; unsymmetric: other values above the diagonal, some entries dropped, a few diagonals small
static Dense grid(int gx, int gy, bool unsymmetric) {
    const int n = gx * gy;
    Dense A(n, std::vector<double>(n, 0.0));
    for (int y = 0; y < gy; ++y) for (int x = 0; x < gx; ++x) {
        const int j = x + gx * y;
        A[j][j] = (unsymmetric && j % 7 == 3) ? 0.25 : 4.0;
        if (x + 1 < gx) { A[j + 1][j] = -1.0; A[j][j + 1] = unsymmetric ? (j % 4 ? -1.5 : 0.0) : -1.0; }
        if (y + 1 < gy) { A[j + gx][j] = -1.0; A[j][j + gx] = unsymmetric ? -0.5 : -1.0; }
    }
    return A;
}
// a full matrix: one supernode of n columns.  Symmetric positive definite, or unsymmetric with no dominant diagonal (rows move)
static Dense full(int n, bool unsymmetric) {
    Dense B(n, std::vector<double>(n)), A(n, std::vector<double>(n, 0.0));
    for (auto& row : B) for (double& v : row) v = 2 * rnd();
    if (unsymmetric) return B;
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { for (int k = 0; k < n; ++k) A[i][j] += B[i][k] * B[j][k]; if (i == j) A[i][j] += n; }
    return A;
}

static std::string write_mm(const std::string& dir, const char* name, const Dense& A, bool symmetric) {
    const std::string path = dir + "/" + name + ".mtx";
    const int n = (int)A.size();
    long nz = 0;
    for (int j = 0; j < n; ++j) for (int i = symmetric ? j : 0; i < n; ++i) nz += A[i][j] != 0;
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { printf("FAIL cannot write %s\n", path.c_str()); exit(2); }
    fprintf(f, "%%%%MatrixMarket matrix coordinate real %s\n%% struct_path_sanitize\n%d %d %ld\n", symmetric ? "symmetric" : "general", n, n, nz);
    for (int j = 0; j < n; ++j) for (int i = symmetric ? j : 0; i < n; ++i) if (A[i][j] != 0) fprintf(f, "%d %d %.17g\n", i + 1, j + 1, A[i][j]);
    fclose(f);
    return path;
}
static std::string write_text(const std::string& dir, const char* name, const char* text) {
    const std::string path = dir + "/" + name + ".mtx";
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { printf("FAIL cannot write %s\n", path.c_str()); exit(2); }
    fputs(text, f);
    fclose(f);
    return path;
}

// the permuted matrix the analysis left in the struct: L by columns, U (LU library, unsymmetric) by rows or the mirror of L
static Dense permuted_matrix(const struct matrix_info_struct* mi) {
    const sf_long n = mi->nrow;
    Dense A(n, std::vector<double>(n, 0.0));
    const sf_long *Up = nullptr, *Ui = nullptr;
    const sf_float* Ux = nullptr;
#ifdef SF_STRUCT_LU
    if (!mi->isSymmetric) { Up = mi->Up; Ui = mi->Ui; Ux = mi->Ux; }
#endif
    for (sf_long j = 0; j < n; ++j) {
        for (sf_long p = mi->Lp[j]; p < mi->Lp[j + 1]; ++p) { A[mi->Li[p]][j] = mi->Lx[p]; if (!Up) A[j][mi->Li[p]] = mi->Lx[p]; }
        if (Up) for (sf_long p = Up[j]; p < Up[j + 1]; ++p) if (Ui[p] != j) A[j][Ui[p]] = Ux[p];
    }
    return A;
}

// Dense elimination of M in place, placed into Lsx.  Cholesky: M = L L^T.  LU: M = L U, unit L, with partial pivoting among the rows
// of each 64-column block of a supernode (pivinv[g] = position of original row g, as the library's PivInv); a moved row takes its
// entries from the block's first column on with it, the L entries to the left stay at the row's original place.
static void factor_into_lsx(const struct matrix_info_struct* mi, Dense M, std::vector<sf_long>& pivinv, sf_long* max_width) {
    const sf_long n = mi->nrow;
    pivinv.resize(n);
    for (sf_long g = 0; g < n; ++g) pivinv[g] = g;
    *max_width = 0;
    for (sf_long s = 0; s < mi->nsuper; ++s) {
        const sf_long nscol = mi->Super[s + 1] - mi->Super[s], nsrow = mi->Lsip[s + 1] - mi->Lsip[s], lda = kLU ? 2 * nsrow - nscol : nsrow;
        const sf_long* rows = mi->Lsi + mi->Lsip[s];
        *max_width = std::max(*max_width, nscol);
        for (sf_long c = 0; c < nscol; ++c) {
            const sf_long k = mi->Super[s] + c, c0 = mi->Super[s] + c / 64 * 64, c1 = std::min(c0 + 64, mi->Super[s + 1]);
            CHECK(rows[c] == k);
            if (kLU) {
                sf_long best = k;
                for (sf_long r = k + 1; r < c1; ++r) if (std::fabs(M[r][k]) > std::fabs(M[best][k])) best = r;
                if (best != k) {
                    for (sf_long j = c0; j < n; ++j) std::swap(M[k][j], M[best][j]);
                    for (sf_long g = c0; g < c1; ++g) if (pivinv[g] == k || pivinv[g] == best) pivinv[g] = pivinv[g] == k ? best : k;
                }
                for (sf_long r = k + 1; r < n; ++r) {
                    if (M[r][k] == 0) continue;
                    const double l = (M[r][k] /= M[k][k]);
                    for (sf_long j = k + 1; j < n; ++j) M[r][j] -= l * M[k][j];
                }
            } else {
                CHECK(M[k][k] > 0);
                const double d = M[k][k] = std::sqrt(M[k][k]);
                for (sf_long r = k + 1; r < n; ++r) M[r][k] /= d;
                for (sf_long j = k + 1; j < n; ++j) for (sf_long r = j; r < n; ++r) M[r][j] -= M[r][k] * M[j][k];
            }
        }
        double* P = mi->Lsx + mi->Lsxp[s];
        CHECK(mi->Lsxp[s] + nscol * lda <= mi->xsize);
        std::vector<char> in_rows(n, 0);
        for (sf_long r = 0; r < nsrow; ++r) in_rows[rows[r]] = 1;
        for (sf_long c = 0; c < nscol; ++c) {
            const sf_long k = mi->Super[s] + c;
            for (sf_long r = 0; r < nsrow; ++r) P[c * lda + r] = (kLU || r >= c) ? M[rows[r]][k] : 0.0;     // L, and U11 above the diagonal
            if (kLU) for (sf_long r = nscol; r < nsrow; ++r) P[(nsrow - nscol) + c * lda + r] = M[k][rows[r]];   // U12^T
            for (sf_long r = k; r < n; ++r) if (!in_rows[r]) CHECK(M[r][k] == 0 && (!kLU || M[k][r] == 0));      // no fill outside the panel
        }
    }
}

// validate with T host threads; the library's residual and solution against this program's dense ones
static void validate(struct matrix_info_struct* mi, const Dense& A, int T, double tol) {
    setenv("SF_HOST_SOLVE_THREADS", std::to_string(T).c_str(), 1);
    CHECK(SparseFrame_validate(mi) == 0);
    const sf_long n = mi->nrow;
    Dense M = A;                                    // x_ref by Gaussian elimination with partial pivoting over all rows
    std::vector<double> x(n), b(n);
    for (sf_long i = 0; i < n; ++i) x[i] = b[i] = 1 + i / (double)n;
    for (sf_long k = 0; k < n; ++k) {
        sf_long best = k;
        for (sf_long r = k + 1; r < n; ++r) if (std::fabs(M[r][k]) > std::fabs(M[best][k])) best = r;
        std::swap(M[k], M[best]); std::swap(x[k], x[best]);
        for (sf_long r = k + 1; r < n; ++r) {
            const double l = M[r][k] / M[k][k];
            if (l == 0) continue;
            for (sf_long j = k; j < n; ++j) M[r][j] -= l * M[k][j];
            x[r] -= l * x[k];
        }
    }
    for (sf_long k = n - 1; k >= 0; --k) { for (sf_long j = k + 1; j < n; ++j) x[k] -= M[k][j] * x[j]; x[k] /= M[k][k]; }
    double anorm = 0, bnorm = 0, xnorm = 0, rnorm = 0, xerr = 0;
    for (sf_long j = 0; j < n; ++j) { double c = 0; for (sf_long i = 0; i < n; ++i) c += std::fabs(A[i][j]); anorm = std::max(anorm, c); }
    for (sf_long i = 0; i < n; ++i) {
        double r = -b[i];
        for (sf_long j = 0; j < n; ++j) r += A[i][j] * mi->Xx[j];
        CHECK(mi->Bx[i] == b[i]);
        rnorm = std::max(rnorm, std::fabs(r)); bnorm = std::max(bnorm, std::fabs(b[i])); xnorm = std::max(xnorm, std::fabs(mi->Xx[i]));
        xerr = std::max(xerr, std::fabs(mi->Xx[i] - x[i]));
    }
    const double own = rnorm / (anorm * xnorm + bnorm);
    printf("  %-22s T=%d residual %.2e (dense: %.2e)  max|x - x_dense| / max|x| = %.2e\n", g_case.c_str(), T, (double)mi->residual, own, xerr / xnorm);
    // both residuals are rounding errors of the same r, summed in different orders: each within tol, and the solutions agree
    CHECK(mi->residual <= tol && own <= tol && xerr <= 1e4 * tol * xnorm);
}

// analyze, make the factor, validate with 1 and 3 threads.  want_wide: a supernode of more than 64 columns; want_moved: some row moved
static void analyze_and_validate(struct common_info_struct* common, struct matrix_info_struct* mi, bool want_wide, bool want_moved, double tol) {
    CHECK(SparseFrame_analyze(common, mi) == 0);
    CHECK(SparseFrame_factorize(common, nullptr, mi) == SF_ERR_NO_DEVICE);      // the stub; the LU library sizes PivInv on the way
    const Dense A = permuted_matrix(mi);
    std::vector<sf_long> pivinv;
    sf_long width = 0, moved = 0;
    factor_into_lsx(mi, A, pivinv, &width);
    for (sf_long g = 0; g < mi->nrow; ++g) moved += pivinv[g] != g;
#ifdef SF_STRUCT_LU
    CHECK(mi->PivInv != nullptr);
    if (mi->PivInv) memcpy(mi->PivInv, pivinv.data(), mi->nrow * sizeof(sf_long));
    CHECK(!want_moved || moved > 0);
#endif
    CHECK(!want_wide || width > 64);
    printf("  %-22s n=%ld nsuper=%ld widest supernode %ld, rows moved %ld\n", g_case.c_str(), (long)mi->nrow, (long)mi->nsuper, (long)width, (long)moved);
    for (int T : {1, 3}) validate(mi, A, T, tol);
    (void)want_moved;
}

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    setenv("SF_HOST_SOLVE_MIN", "0", 1);             // the threaded sweeps whatever the size
    struct common_info_struct common;
    memset(&common, 0, sizeof common);
    common.devSlotSize = (size_t)1 << 30;
    struct gpu_info_struct* gpus = nullptr;
    CHECK(SparseFrame_allocate_gpu(&common, &gpus) == SF_ERR_NO_DEVICE);

    struct matrix_info_struct* mi = nullptr;
    common.matrixThreadNum = 1;
    CHECK(SparseFrame_allocate_matrix(&common, &mi) == 0 && mi);
    if (!mi) return 2;

    // ---- the whole path on each matrix: built-in ordering, then a supplied one; the second matrix re-read into the same struct
    struct Case { const char* name; Dense A; bool symmetric, wide; };
    std::vector<Case> cases;
    cases.push_back({"grid_6x7_symmetric", grid(6, 7, false), true, false});
    cases.push_back({"full_70_symmetric", full(70, false), true, true});
    if (kLU) {
        cases.push_back({"grid_7x6_general", grid(7, 6, true), false, false});
        cases.push_back({"full_70_general", full(70, true), false, true});
    }
    for (const Case& c : cases) {
        g_case = c.name;
        common.devSlotSize = c.wide ? (size_t)1 << 30 : 6000;          // a small slot caps the supernodes: several of them, subtrees and a top
        const std::string path = write_mm(dir, c.name, c.A, c.symmetric);
        CHECK(SparseFrame_initialize_matrix(mi) == 0);
        CHECK(mi->factorizeType == (kLU ? TYPE_LU : TYPE_CHOLESKY) && mi->permMethod == PERM_METIS);
        mi->path = path.c_str();
        CHECK(SparseFrame_read_matrix(mi) == 0);
        const sf_long n = (sf_long)c.A.size();
        CHECK(mi->nrow == n && mi->isSymmetric == (c.symmetric ? 1 : 0) && mi->Cp[n] == mi->nzmax);
#ifdef SF_STRUCT_LU
        CHECK(SparseFrame_set_matrix_pivoting(mi, 0.5, 0.0) == SF_OK);          // the side table: dropped by the clean-up below
#endif
        const double tol = c.symmetric ? 1e-13 : 1e-11;
        analyze_and_validate(&common, mi, c.wide, !c.symmetric, tol);              // built-in nested dissection
        std::vector<sf_long> perm(n);
        for (sf_long i = 0; i < n; ++i) perm[i] = (i * 11 + 3) % n;                // 11 is prime to 42 and 70
        CHECK(SparseFrame_set_perm(mi, perm.data()) == 0);
        analyze_and_validate(&common, mi, c.wide, !c.symmetric, tol);
        CHECK(SparseFrame_set_perm(mi, nullptr) == 0 && mi->permMethod == PERM_IDENTITY);
        analyze_and_validate(&common, mi, c.wide, !c.symmetric, tol);

        // a larger matrix into the same struct, analysed twice (the second time with the first's ordering still in place)
        g_case = std::string(c.name) + " -> grid_9x9";
        const Dense big = grid(9, 9, !c.symmetric);
        const std::string path2 = write_mm(dir, "grid_9x9", big, c.symmetric);
        mi->path = path2.c_str();
        mi->permMethod = PERM_METIS;
        CHECK(SparseFrame_read_matrix(mi) == 0 && mi->nrow == 81);
        CHECK(SparseFrame_analyze(&common, mi) == 0);
        analyze_and_validate(&common, mi, false, false, tol);
        CHECK(SparseFrame_cleanup_matrix(mi) == 0);
        CHECK(!mi->Lsx && !mi->Cp && !mi->Perm && !mi->Xx && mi->nsuper == 0 && mi->residual <= tol);
        CHECK(SparseFrame_cleanup_matrix(mi) == 0);
    }

    // ---- the reader: the files of tests/test_abi.py, and a size line that announces more entries than any machine holds
    struct Text { const char* name; const char* text; int rc; long nz; };
    const Text texts[] = {
        {"zeros", "%%MatrixMarket matrix coordinate real symmetric\n% comment\n3 3 5\n1 1 2.0\n2 1 0.0\n2 2 3.0\n3 2 -1.0\n3 3 4.0\n", 0, 4},
        {"integer-upper-blank", "%%MatrixMarket matrix coordinate integer symmetric\n% a\n%b\n\n3 3 4\n1 1 2\n1 2 -1\n\n2 2 3\n3 3 4\n", 0, 4},
        {"general", "%%MatrixMarket matrix coordinate real general\n2 2 3\n1 1 1.5\n2 1 -0.5\n2 2 2.5\n", 0, 3},
        {"oversize", "%%MatrixMarket matrix coordinate real symmetric\n2 2 4000000000000000000\n1 1 1.0\n", 0, 1},
        {"empty", "%%MatrixMarket matrix coordinate real symmetric\n0 0 0\n", 0, 0},
        {"complex", "%%MatrixMarket matrix coordinate complex general\n1 1 1\n1 1 1.0 0.0\n", 1, 0},
        {"no-banner", "3 3 1\n1 1 1.0\n", 1, 0},
        {"short-size-line", "%%MatrixMarket matrix coordinate real symmetric\n3 3\n1 1 1.0\n", 1, 0},
        {"short-entry", "%%MatrixMarket matrix coordinate real symmetric\n2 2 2\n1 1 1.0\n2 2\n", 1, 0},
        {"too-many", "%%MatrixMarket matrix coordinate real symmetric\n2 2 1\n1 1 1.0\n2 2 1.0\n", 1, 0},
        {"out-of-range", "%%MatrixMarket matrix coordinate real symmetric\n2 2 1\n3 1 1.0\n", 1, 0},
        {"rectangular", "%%MatrixMarket matrix coordinate real general\n2 3 1\n1 1 1.0\n", 1, 0},
        {"oversize-order", "%%MatrixMarket matrix coordinate real general\n4000000000000000000 4000000000000000000 1\n1 1 1.0\n", 1, 0},
    };
    CHECK(SparseFrame_initialize_matrix(mi) == 0);
    for (const Text& t : texts) {
        g_case = t.name;
        const std::string path = write_text(dir, t.name, t.text);
        mi->path = path.c_str();
        CHECK(SparseFrame_read_matrix(mi) == t.rc);
        if (t.rc == 0) CHECK(mi->nzmax == t.nz && mi->Cp[0] == 0 && mi->Cp[mi->nrow] == t.nz && mi->workSize >= (size_t)(10 * mi->nrow + 1) * sizeof(sf_long));
    }
    g_case = "missing file";
    const std::string nowhere = dir + "/does_not_exist.mtx";
    mi->path = nowhere.c_str();
    CHECK(SparseFrame_read_matrix(mi) == 1);
    CHECK(mi->Cp != nullptr);                       // a failed read leaves the last matrix in place
    CHECK(SparseFrame_cleanup_matrix(mi) == 0 && SparseFrame_cleanup_matrix(mi) == 0 && !mi->Cp && !mi->workspace);

    CHECK(SparseFrame_free_matrix(&common, &mi) == 0 && !mi);
    CHECK(SparseFrame_free_gpu(&common, &gpus) == SF_OK);
    if (g_fail) { printf("struct_path_sanitize (%s): %d checks FAILED\n", kLU ? "LU" : "Cholesky", g_fail); return 1; }
    printf("struct_path_sanitize: ok (%s)\n", kLU ? "LU" : "Cholesky");
    return 0;
}
