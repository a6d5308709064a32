// Where the factor of a new pattern goes -- in core, or out of core in how many groups -- and what the struct path's handler gives
// up to get its plan built.  A factor that does not fit the device (or SF_DEVICE_BUDGET_MB, for tests and shared devices) is
// factorized OUT OF CORE: top panels resident, subtree groups streamed through two buffers while the finished ones travel to the
// host -- the role the reference gives its slot-sized stages (C:1721-1846, C:2421-2467).  Decided per pattern, before the plan is
// built.  No HIP here: the handler (sf_handlers.hip) supplies the device's answers, tools/handlers_host_sanitize.cpp a script
// (DESIGN 8t).
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#include "sf_schedule.h"

namespace sf {

struct Placement {
    int ngroups = 1, top_mode = 0;      // ngroups > 1: out of core (sf::ooc_partition)
    std::vector<int32_t> group;         // per supernode, filled when out of core
};

// in: the symbolic arrays and lu.  env_budget: SF_DEVICE_BUDGET_MB in bytes, <= 0 = unset: the budget is then what free_bytes
// reports (false: SF_ERR_HIP) less 1 GiB, plus the factor's own bytes when it fits idle_pool (the bytes of the handler's pool
// while nobody uses it, else 0: an in-core factor goes there).  shrink scales the budget.
// SF_OK (pl set), SF_ERR_ALLOC (nothing fits), SF_ERR_ARG (the partition refused the structure), SF_ERR_HIP.
int decide_placement(const PlanInput& in, double shrink, int64_t env_budget, const std::function<bool(size_t& free_now)>& free_bytes,
                     size_t idle_pool, bool trace, Placement& pl);

// The plan of a new pattern: decide, give up what stands in the way, create, and on an allocation failure give up more and cut the
// budget.  DESIGN 8t has the steps as a numbered list.  Env (all of them called from here only):
//   int decide(double shrink, Placement&)   decide_placement with the device's answers as they are NOW
//   int create(const Placement&)            plan creation; SF_ERR_ALLOC / SF_ERR_HIP: no memory
//   bool cache_empty(), void drop_cache()   the handler's other cached plans (dropping the pool's user makes the pool idle)
//   bool pool_idle(), void release_pool()   the handler's device pool exists and no plan lives in it; give it back for good
//   bool env_budget_set()                   SF_DEVICE_BUDGET_MB is set: the free memory is not what decides, so nothing is given up for the decision
//   void device_sync(), void clear_error()
template <class Env>
int place_and_create(Env& e, Placement& pl) {
    auto wants_more = [&](int rc) { return rc != SF_OK || pl.ngroups > 1; };
    auto no_memory = [](int rc) { return rc == SF_ERR_ALLOC || rc == SF_ERR_HIP; };
    auto again = [&](double shrink) {
        e.clear_error();
        const int rc = e.decide(shrink, pl);
        return rc == SF_OK ? e.create(pl) : rc;
    };
    int rc = e.decide(1.0, pl);
    if (wants_more(rc) && !e.cache_empty() && !e.env_budget_set()) {
        // the free memory the decision saw did not count what the cached plans hold: they go first, then the decision is taken again
        e.drop_cache();
        e.device_sync();
        rc = e.decide(1.0, pl);
    }
    if (wants_more(rc) && e.pool_idle() && !e.env_budget_set()) {
        // ... and so does the idle pool when the factor is too large for it: the memory serves the plan better directly
        e.release_pool();
        rc = e.decide(1.0, pl);
    }
    if (rc == SF_OK) rc = e.create(pl);
    // when the device is out of memory, drop everything cached and retry once
    if (no_memory(rc) && !e.cache_empty()) { e.drop_cache(); rc = again(1.0); }
    // the pool itself is in the way (a factor larger than the pool, on a device that holds little else): give it back for good
    if (no_memory(rc) && e.pool_idle()) { e.release_pool(); rc = again(1.0); }
    // the estimate of what else lives on the device was too low (or somebody else took memory meanwhile): cut deeper, twice
    for (double shrink = 0.8; rc == SF_ERR_ALLOC && shrink > 0.6; shrink -= 0.15) {
        e.clear_error();
        if (e.decide(shrink, pl) != SF_OK) break;       // (the last create's SF_ERR_ALLOC is what the caller gets)
        rc = e.create(pl);
    }
    return rc;
}

}  // namespace sf
