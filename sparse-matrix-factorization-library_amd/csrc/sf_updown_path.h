// Which supernodes a rank-k update A' = A +- W W^T of a Cholesky factor with a static pattern changes, and whether the pattern can
// stay as it is.  Plain C++ without HIP: sf_updown_path.cpp is built by the host compiler, tools/updown_path_sanitize.cpp
// runs it under the sanitizers on a CPU, and it works on schedule-only plans.
#pragma once
#include <cstdint>
#include <vector>

namespace sf {

// the supernodal structure as the schedule keeps it (SfSchedule::h_Super, h_Lsip, h_Lsi): supernode s has the columns
// [Super[s], Super[s + 1]) and the rows Lsi[Lsip[s] .. Lsip[s + 1]), its own columns first, then the rows below in ascending order
struct UpdownStruct {
    int64_t n = 0, nsuper = 0;
    const int32_t* Super = nullptr;
    const int64_t* Lsip = nullptr;
    const int32_t* Lsi = nullptr;

    int64_t nscol(int64_t s) const { return Super[s + 1] - Super[s]; }
    int64_t nsrow(int64_t s) const { return Lsip[s + 1] - Lsip[s]; }
    // the supernode of column j (0 <= j < n)
    int64_t super_of(int64_t j) const;
    // the parent of s in the supernodal forest: the supernode of its first row below, -1 for a root
    int64_t parent(int64_t s) const { return nsrow(s) > nscol(s) ? super_of(Lsi[Lsip[s] + nscol(s)]) : -1; }
};

enum : int { UPDOWN_OK = 0, UPDOWN_BAD_ARG = 1, UPDOWN_INADMISSIBLE = 2 };

// W = k sparse columns (Wp[k + 1], Wi), row indices in any order inside a column; iperm (or null): Wi is in the caller's numbering,
// row i of the plan is iperm[Wi].  A column is ADMISSIBLE when, with j0 its smallest row and s0 the supernode of j0, every other row
// is a column of s0 or one of the rows below s0.  An empty column is admissible and adds nothing.
//   UPDOWN_BAD_ARG       k < 0, a missing array, Wp not ascending from a value >= 0, a row outside [0, n), a row twice in a column
//   UPDOWN_INADMISSIBLE  *bad_column = the first column that is not admissible
//   UPDOWN_OK            *bad_column = -1; supers = the union of the chains s0 -> parent -> ... -> root over the columns, ascending
//                        (ascending supernode numbers are a topological order of the forest)
// rows (optional): the mapped row indices, aligned with Wi from Wp[0] on.  Every column is checked before anything is reported.
int updown_path(const UpdownStruct& S, int64_t k, const int64_t* Wp, const int64_t* Wi, const int32_t* iperm,
                std::vector<int64_t>& supers, int64_t* bad_column, std::vector<int32_t>* rows = nullptr);

}  // namespace sf
