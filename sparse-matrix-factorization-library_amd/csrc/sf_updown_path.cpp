// The path of a rank-k update through the supernodal forest and the admissibility rule (sf_updown_path.h).  No HIP.
#include "sf_updown_path.h"

#include <algorithm>

namespace sf {

int64_t UpdownStruct::super_of(int64_t j) const {
    // Super is strictly ascending with Super[0] = 0 and Super[nsuper] = n: the last s with Super[s] <= j
    const int32_t* e = std::upper_bound(Super, Super + nsuper + 1, (int32_t)j);
    return (int64_t)(e - Super) - 1;
}

int updown_path(const UpdownStruct& S, int64_t k, const int64_t* Wp, const int64_t* Wi, const int32_t* iperm,
                std::vector<int64_t>& supers, int64_t* bad_column, std::vector<int32_t>* rows) {
    supers.clear();
    if (rows) rows->clear();
    if (bad_column) *bad_column = -1;
    if (k < 0 || !Wp || S.n < 0 || S.nsuper < 0) return UPDOWN_BAD_ARG;
    if (Wp[0] < 0) return UPDOWN_BAD_ARG;
    for (int64_t t = 0; t < k; ++t)
        if (Wp[t + 1] < Wp[t]) return UPDOWN_BAD_ARG;
    if (Wp[k] > Wp[0] && !Wi) return UPDOWN_BAD_ARG;
    if (Wp[k] > Wp[0] && (S.nsuper <= 0 || !S.Super || !S.Lsip || !S.Lsi)) return UPDOWN_BAD_ARG;     // (no row can be in range)
    if (rows) rows->reserve((size_t)(Wp[k] - Wp[0]));

    std::vector<int64_t> col;               // the rows of one column, mapped and sorted
    std::vector<int64_t> starts;            // s0 of every non-empty column
    int64_t bad = -1;
    for (int64_t t = 0; t < k; ++t) {
        col.clear();
        for (int64_t q = Wp[t]; q < Wp[t + 1]; ++q) {
            int64_t i = Wi[q];
            if (i < 0 || i >= S.n) return UPDOWN_BAD_ARG;
            if (iperm) i = iperm[i];
            col.push_back(i);
            if (rows) rows->push_back((int32_t)i);
        }
        if (col.empty()) continue;
        std::sort(col.begin(), col.end());
        if (std::adjacent_find(col.begin(), col.end()) != col.end()) return UPDOWN_BAD_ARG;
        const int64_t s0 = S.super_of(col[0]);
        const int64_t cend = S.Super[s0 + 1];
        const int32_t* below = S.Lsi + S.Lsip[s0] + S.nscol(s0);
        const int32_t* bend = S.Lsi + S.Lsip[s0 + 1];
        bool ok = true;
        for (size_t q = 1; q < col.size() && ok; ++q) {
            if (col[q] < cend) continue;                                    // a column of s0
            // the rows below are ascending and so is col: `below` only moves forward
            below = std::lower_bound(below, bend, (int32_t)col[q]);
            ok = below != bend && *below == col[q];
        }
        if (!ok) {
            if (bad < 0) bad = t;           // (the columns after it are still checked for their arguments)
            continue;
        }
        starts.push_back(s0);
    }
    if (bad >= 0) {
        if (bad_column) *bad_column = bad;
        if (rows) rows->clear();
        return UPDOWN_INADMISSIBLE;
    }
    std::vector<char> seen((size_t)S.nsuper, 0);
    for (int64_t s0 : starts)
        for (int64_t s = s0; s >= 0 && !seen[(size_t)s]; s = S.parent(s)) {     // (an ancestor seen before has its whole chain in)
            seen[(size_t)s] = 1;
            supers.push_back(s);
        }
    std::sort(supers.begin(), supers.end());
    return UPDOWN_OK;
}

}  // namespace sf
