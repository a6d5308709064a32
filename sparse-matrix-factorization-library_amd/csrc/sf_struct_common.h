// What the struct entry points of both libraries (sf_chol_host.cpp, sf_lu_host.cpp, through sf_struct_path.inc) do on plain
// pointers and sizes: the MatrixMarket reader, validate's right-hand side and residual, the timer and the release of big blocks.
// No HIP and neither public struct header: the two headers define different layouts under one struct name.
// Reference files: Cholesky/Source/SparseFrame.c (C:), LU/Source/SparseFrame.c (L:).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <sys/stat.h>
#include <thread>
#include <time.h>
#include <vector>

namespace sf_struct {

typedef int64_t Long;

// the U arrays and the interchange record a library hands to the solve and the residual: Cholesky none, LU p = nullptr when U aliases L
struct Upper {
    const Long *p, *i;
    const double* x;
    const Long* PivInv;
};

inline double wall_seconds() {
    struct timespec tp;
    clock_gettime(CLOCK_REALTIME, &tp);
    return tp.tv_sec + (double)tp.tv_nsec / 1.0e9;
}

template <class T>
void free_and_null(T*& p) {
    free(p);
    p = nullptr;
}
// the one macro of the struct path, for the free lists of the files that see a matrix_info_struct `mi`
#define SF_FREE(field) sf_struct::free_and_null(mi->field)

// Returning a factor of tens of GB to the system (free -> munmap: the kernel tears down millions of page-table entries) takes 0.85 s for
// the 30 GB of 128^3 -- as long as the factorization.  Nobody waits for it: big blocks are released by a detached thread.
inline void free_big_async(void* q, size_t bytes) {
    if (!q) return;
    if (bytes < ((size_t)1 << 30)) { free(q); return; }
    try { std::thread([q] { free(q); }).detach(); } catch (...) { free(q); }
}

// validate's right-hand side (C:3141-3266)
inline void fill_rhs(Long n, double* b) {
    for (Long i = 0; i < n; ++i) b[i] = 1 + i / (double)n;
}

// MatrixMarket "coordinate {real|integer} {symmetric|general}" reader: drops explicit zeros (C:496) and compresses the triplets to
// CSC with a counting sort (C:526-587).  0, or 1 for a file that is missing, ill-formed or too large to hold; nothing is thrown.
inline int read_matrix_market(const char* path, Long* n, std::vector<Long>& Cp, std::vector<Long>& Ci, std::vector<double>& Cx,
                              int* symmetric) try {
    struct Open {       // closed and freed on every way out, a throwing push_back included
        FILE* f;
        char* line = nullptr;
        ~Open() { free(line); if (f) fclose(f); }
    } file{fopen(path, "r")};
    FILE* const f = file.f;
    if (!f) return 1;
    char*& line = file.line;
    size_t cap = 0;
    int rc = 1;
    std::vector<Long> Ti, Tj;
    std::vector<double> Tx;
    long nrow = 0, ncol = 0, nzmax = 0;
    do {
        ssize_t got;
        while ((got = getline(&line, &cap, f)) != -1 && line[0] == '\n') {}
        if (got == -1 || strncmp(line, "%%MatrixMarket", 14) != 0) break;
        char s0[64], s1[64], s2[64], s3[64], s4[64];
        s3[0] = s4[0] = 0;
        sscanf(line, "%63s %63s %63s %63s %63s", s0, s1, s2, s3, s4);
        *symmetric = strcmp(s4, "symmetric") == 0;
        if (strcmp(s3, "real") != 0 && strcmp(s3, "integer") != 0) break;  // complex: unsupported (reference solve is TODO)
        while ((got = getline(&line, &cap, f)) != -1 && (line[0] == '%' || line[0] == '\n')) {}
        if (got == -1 || sscanf(line, "%ld %ld %ld", &nrow, &ncol, &nzmax) != 3) break;
        if (nrow != ncol || nrow < 0 || nzmax < 0) break;
        struct stat st;     // the size line is the file's word only: reserve no more than the file could hold ("1 1 1\n" is six bytes)
        const long room = fstat(fileno(f), &st) == 0 ? (long)(st.st_size / 6) : 0;
        Ti.reserve(std::min(nzmax, room)); Tj.reserve(std::min(nzmax, room)); Tx.reserve(std::min(nzmax, room));
        bool bad = false;
        while (getline(&line, &cap, f) != -1) {
            if (line[0] == '\n' || line[0] == 0) continue;
            long i, j; double x;
            {   // "%ld %ld %lg" by hand: strtol / strtod are several times faster than sscanf on files of 10^7 lines
                char *e1, *e2, *e3;
                i = strtol(line, &e1, 10);
                j = strtol(e1, &e2, 10);
                x = strtod(e2, &e3);
                if (e1 == line || e2 == e1 || e3 == e2) { bad = true; break; }
            }
            if (x != 0) {
                if ((long)Tx.size() >= nzmax || i < 1 || j < 1 || i > nrow || j > ncol) { bad = true; break; }
                Ti.push_back(i - 1); Tj.push_back(j - 1); Tx.push_back(x);
            }
        }
        if (!bad) rc = 0;
    } while (0);
    if (rc) return rc;

    const Long nz = (Long)Tx.size();
    *n = nrow;
    Cp.assign((size_t)ncol + 1, 0);
    Ci.resize((size_t)nz);
    Cx.resize((size_t)nz);
    for (Long k = 0; k < nz; ++k) Cp[Tj[k] + 1]++;
    for (Long j = 0; j < ncol; ++j) Cp[j + 1] += Cp[j];
    std::vector<Long> fill(Cp.begin(), Cp.end() - 1);
    for (Long k = 0; k < nz; ++k) {
        const Long p = fill[Tj[k]]++;
        Ci[p] = Ti[k];
        Cx[p] = Tx[k];
    }
    return 0;
} catch (...) {     // an allocation that the size line asked for and the machine does not have
    return 1;
}

// r = A x - b and |r|_inf / (|A|_1 |x|_inf + |b|_inf) (C:3141-3266, L:3702-3858).  A = L + U^T without U's diagonal, both by columns:
// the LU library's two triangles, or (Up == nullptr) the stored triangle used symmetrically.  Every r_i and every column sum
// receives its terms in the order of the reference's loops, in either form: the result is theirs to the bit.
inline double residual(Long n, const Long* Lp, const Long* Li, const double* Lx, const Long* Up, const Long* Ui, const double* Ux,
                       const double* x, const double* b, double* r) {
    if (!Up) { Up = Lp; Ui = Li; Ux = Lx; }
    std::vector<double> colsum((size_t)n, 0.0);
    for (Long i = 0; i < n; ++i) r[i] = -b[i];
    for (Long j = 0; j < n; ++j) {
        for (Long p = Lp[j]; p < Lp[j + 1]; ++p) {
            r[Li[p]] += Lx[p] * x[j];
            colsum[j] += std::fabs(Lx[p]);
        }
        for (Long p = Up[j]; p < Up[j + 1]; ++p) {
            const Long i = Ui[p];
            if (i != j) {
                r[j] += Ux[p] * x[i];
                colsum[i] += std::fabs(Ux[p]);
            }
        }
    }
    double anorm = 0, bnorm = 0, xnorm = 0, rnorm = 0;
    bool finite = true;     // fmax returns its non-NaN operand: a non-finite r_i or x_i is kept apart, as k_refine_norms' flag word does
    for (Long i = 0; i < n; ++i) {
        anorm = std::fmax(anorm, colsum[i]);
        bnorm = std::fmax(bnorm, std::fabs(b[i]));
        xnorm = std::fmax(xnorm, std::fabs(x[i]));
        rnorm = std::fmax(rnorm, std::fabs(r[i]));
        if (!std::isfinite(r[i]) || !std::isfinite(x[i])) finite = false;
    }
    // a non-finite solution is no solve at all: NaN fails every `residual <= tol` (the return code stays 0)
    return finite ? rnorm / (anorm * xnorm + bnorm) : std::numeric_limits<double>::quiet_NaN();
}

}  // namespace sf_struct
