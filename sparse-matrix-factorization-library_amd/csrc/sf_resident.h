// What the handlers (sf_handlers.hip) need of the registry of resident factors (sf_resident.hip): host arrays whose factor is still
// on the device(s), by the address of Lsx, for SparseFrame_solve_supernodal's fast path.  Internal to the library.
//
// LOCK ORDER.  A handler's lock (HandlerState::mu, or MultiState::mu) is taken first, the registry's lock second: every function
// below takes the registry's lock itself and may be called with a handler's lock held.  The solve takes the registry's lock ALONE
// and holds it for the whole solve: a factorization or a destruction of the same plan waits in forget_plan until it is over, so
// nobody else touches the plan meanwhile.
#pragma once
#include <memory>
#include <vector>

#include "sf_plan_internal.h"

// whole plan a distributed factor is gathered into for the struct path's solve (owned by a MultiState cache entry and by the
// registry entries that point at it)
struct SolverSlot {
    sf_chol_plan* plan = nullptr;
    std::vector<int> imported;          // epochs of the parts the plan currently holds
    ~SolverSlot() { if (plan) sf_chol_plan_destroy(plan); }
};

namespace sf_resident {

// Lsx holds the factor `plan` has just computed (an out-of-core factor exists on the host only: its entry is erased, its solves
// take the host sweep)
void register_plan(const void* Lsx, sf_chol_plan* plan);
// ... the factor spread over the ranks' plans `parts`; a solve runs there with comms, or gathers it into slot's plan on `device`
void register_parts(const void* Lsx, const std::vector<sf_chol_plan*>& parts, const std::shared_ptr<SolverSlot>& slot,
                    const std::vector<sf_comm*>& comms, int device);
void erase(const void* Lsx);
// whatever host copies this plan's factor stood for are history: before it is factorized again, and before it is destroyed
void forget_plan(sf_chol_plan* plan);
void destroy_plan(sf_chol_plan* plan);

// The public creators by kind.  in: the symbolic arrays, lu, device; OOC: in.ooc_group, ooc_ngroups, ooc_top_mode; MAPPED: owner,
// in.rank, in.nranks.
enum CreateKind { CREATE_PLAIN, CREATE_OOC, CREATE_MAPPED };
int create_plan(sf_chol_plan** plan, const PlanInput& in, CreateKind kind, const int32_t* owner = nullptr);

}  // namespace sf_resident
