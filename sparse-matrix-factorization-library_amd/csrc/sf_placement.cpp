// decide_placement (sf_placement.h): arithmetic over the pattern plus one question to the device.  Plain C++ without HIP.
#include "sf_placement.h"

#include <algorithm>
#include <cstdio>

#include "sf_symbolic.h"

namespace sf {

int decide_placement(const PlanInput& in, double shrink, int64_t env_budget, const std::function<bool(size_t& free_now)>& free_bytes,
                     size_t idle_pool, bool trace, Placement& pl) {
    int64_t entries = 0;
    for (sf_long s = 0; s < in.nsuper; ++s) entries += in.nscol(s) * in.nsrow(s);
    const int64_t per_entry = in.lu ? 16 : 8;
    // everything a plan keeps on the device besides the panels, generously: values, structure, relative maps, task tables, rings
    const int64_t overhead = 12 * (int64_t)in.Lp[in.n] + (in.lu && in.Up ? 12 * (int64_t)in.Up[in.n] : 0) + 24 * (int64_t)in.Lsip[in.nsuper] +
                             ((int64_t)384 << 20);
    pl.ngroups = 1;
    int64_t budget = env_budget;
    if (budget <= 0) {
        // (a small factor is not worth the question: the estimate of everything else a plan needs is generous, and a device that
        //  is nearly full should still take a matrix of a few MB -- the allocation itself will tell)
        if (entries * per_entry < ((int64_t)64 << 20)) return SF_OK;
        size_t fr = 0;
        if (!free_bytes(fr)) return SF_ERR_HIP;
        budget = (int64_t)fr - ((int64_t)1 << 30);
        // (the factor of an in-core plan goes into the handler's idle pool if it fits there: counted as free for exactly that)
        if (idle_pool && (size_t)(entries * per_entry + 16) <= idle_pool) budget += entries * per_entry + 16;
    }
    budget = (int64_t)((double)budget * shrink);
    if (entries * per_entry + overhead <= budget) return SF_OK;           // in core
    const int64_t budget_entries = (budget - overhead) / per_entry;
    if (budget_entries <= 0) return SF_ERR_ALLOC;
    pl.group.assign((size_t)std::max<sf_long>(in.nsuper, 1), 0);
    int64_t ge = 0, te = 0, nd = 0;
    const int rc = ooc_partition(in.nsuper, in.Super, in.SuperMap, in.Lsip, in.Lsi, budget_entries, pl.group.data(), &pl.ngroups, &ge, &te, &nd, &pl.top_mode);
    if (trace || rc)
        fprintf(stderr, "[sparseframe-hip] factorize: %.2f GB of panels against a device budget of %.2f GB -> out of core: %d groups, "
                        "top %.2f GB %s + 2 buffers of %.2f GB%s\n", entries * per_entry / 1e9, budget / 1e9, pl.ngroups,
                te * per_entry / 1e9, pl.top_mode == 0 ? "resident (top mode 0)" : (pl.top_mode == 1 ? "for the active top panels (top mode 1)" : "for the active top panels (top mode 2)"), ge * per_entry / 1e9, rc == 2 ? " -- DOES NOT FIT" : "");
    return rc == 0 ? SF_OK : (rc == 2 ? SF_ERR_ALLOC : SF_ERR_ARG);
}

}  // namespace sf
