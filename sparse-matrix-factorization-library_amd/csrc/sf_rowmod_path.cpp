// The row tasks, the sweep list and the update path of a row deletion / addition (sf_rowmod_path.h).  No HIP.
#include "sf_rowmod_path.h"

#include <algorithm>

namespace sf {

namespace {

// the position of row j among the rows below p (ascending), as an index into the whole row list of p; -1: not there
int64_t find_below(const UpdownStruct& S, int64_t p, int64_t j) {
    const int32_t* b0 = S.Lsi + S.Lsip[p] + S.nscol(p);
    const int32_t* b1 = S.Lsi + S.Lsip[p + 1];
    const int32_t* q = std::lower_bound(b0, b1, (int32_t)j);
    return q != b1 && *q == j ? (int64_t)(q - (S.Lsi + S.Lsip[p])) : -1;
}

}  // namespace

int rowmod_path(const UpdownStruct& S, int64_t row, int64_t nz, const int64_t* Ai, const int32_t* iperm, RowmodPath& out, int64_t* bad) {
    out = RowmodPath();
    if (bad) *bad = -1;
    if (S.n <= 0 || S.nsuper <= 0 || !S.Super || !S.Lsip || !S.Lsi) return UPDOWN_BAD_ARG;
    if (row < 0 || row >= S.n || nz < 0 || (nz > 0 && !Ai)) return UPDOWN_BAD_ARG;
    const int64_t j = iperm ? iperm[row] : row;
    const int64_t s = S.super_of(j), c = j - S.Super[s];
    out.j = j;
    out.s = s;
    out.c = c;
    out.mapped.reserve((size_t)nz);
    for (int64_t q = 0; q < nz; ++q) {
        if (Ai[q] < 0 || Ai[q] >= S.n) return UPDOWN_BAD_ARG;
        out.mapped.push_back((int32_t)(iperm ? iperm[Ai[q]] : Ai[q]));
    }
    {
        std::vector<int32_t> sorted(out.mapped);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return UPDOWN_BAD_ARG;
    }
    // admissibility, and the supernodes the chains start in
    std::vector<int64_t> starts;
    for (int64_t q = 0; q < nz; ++q) {
        const int64_t i = out.mapped[(size_t)q];
        bool ok = true;
        if (i < j) {
            const int64_t si = S.super_of(i);
            if (si != s) {
                ok = find_below(S, si, j) >= 0;
                if (ok) starts.push_back(si);
            }
        } else if (i > j) {
            ok = i < S.Super[s + 1] || find_below(S, s, i) >= 0;
        }
        if (!ok) {
            if (bad) *bad = q;
            out.mapped.clear();
            return UPDOWN_INADMISSIBLE;
        }
    }
    // row j of L: every p < s with j among its rows below
    for (int64_t p = 0; p < s; ++p) {
        const int64_t pos = find_below(S, p, j);
        if (pos < 0) continue;
        out.rows_supers.push_back(p);
        out.rows_pos.push_back(pos);
    }
    // The chains: a supernode with j below it has a parent that is s or has j below it too (containment), so every chain reaches
    // s; the bounds on p only keep a malformed structure from walking off.
    std::vector<char> seen((size_t)S.nsuper, 0);
    for (int64_t s0 : starts)
        for (int64_t p = s0; p >= 0 && p < s && !seen[(size_t)p]; p = S.parent(p)) {
            seen[(size_t)p] = 1;
            out.sweep.push_back(p);
        }
    std::sort(out.sweep.begin(), out.sweep.end());
    // w = L(j + 1:, j)
    for (int64_t q = S.Lsip[s] + c + 1; q < S.Lsip[s + 1]; ++q) out.w_rows.push_back(S.Lsi[q]);
    if (!out.w_rows.empty()) {
        const int64_t Wp[2] = {0, (int64_t)out.w_rows.size()};
        int64_t bad_column = -1;
        const int rc = updown_path(S, 1, Wp, out.w_rows.data(), nullptr, out.update, &bad_column);
        if (rc != UPDOWN_OK) return UPDOWN_BAD_ARG;         // (containment does not hold: not a structure of this library)
    }
    return UPDOWN_OK;
}

}  // namespace sf
