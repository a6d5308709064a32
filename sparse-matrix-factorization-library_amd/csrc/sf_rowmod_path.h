// What deleting or adding row and column j of a Cholesky factor with a static pattern touches: the panels that hold
// row j, the supernodes of rowadd's forward sweep, the rows of the rank-1 vector that follows and its path.  Plain C++ without HIP,
// as sf_updown_path.h: built by the host compiler, run under the sanitizers by tools/rowmod_path_sanitize.cpp, and it works on
// schedule-only plans.
#pragma once
#include <cstdint>
#include <vector>

#include "sf_updown_path.h"

namespace sf {

struct RowmodPath {
    int64_t j = -1, s = -1, c = -1;         // the row in the plan's numbering, its supernode, its local column j - Super[s]
    // the supernodes p < s, ascending, that hold row j below their own columns, and its position in their row list
    // Lsi[Lsip[p] ..): row j of L lies in row rows_pos of the panel of p, and in local row c of s, columns [0, c)
    std::vector<int64_t> rows_supers, rows_pos;
    // rowadd: the supernodes p < s of the forward sweep, ascending: the union of the chains SuperMap[i] -> parent -> ... that
    // stop before s, over the indices i < j outside s
    std::vector<int64_t> sweep;
    // the rows of L(j + 1:, j): the columns of s behind c, then the rows below s; the path of a rank-1 update with these rows
    std::vector<int64_t> w_rows, update;
    std::vector<int32_t> mapped;            // Ai in the plan's numbering, aligned with Ai
};

// row (and Ai) in the plan's numbering, or with iperm in the caller's: j = iperm[row].  Ai[nz]: the indices of the new column of
// rowadd (nz = 0: rowdel).  An index i < j is ADMISSIBLE when j is in the row list of the supernode of i or that supernode is s;
// an index i > j when it is a column of s or one of the rows below s; j itself always is.
//   UPDOWN_BAD_ARG       row or an index outside [0, n), nz < 0, a missing array, an index twice
//   UPDOWN_INADMISSIBLE  *bad = the first position in Ai whose index is not admissible; out holds j, s, c only
//   UPDOWN_OK            *bad = -1
int rowmod_path(const UpdownStruct& S, int64_t row, int64_t nz, const int64_t* Ai, const int32_t* iperm, RowmodPath& out, int64_t* bad);

}  // namespace sf
