// Host side of the Brownian-bridge barrier pricer (include/mcgpu.h: mcg_barrier_survival, mcg_price_barriers_bridge): what
// the entry points reject of a level and of the step variance, and the plan of a book -- its distinct levels, their groups of
// BRIDGE_L_MAX, and the order in which the book kernel walks the contracts.  Plain C++ (no HIP header): host/barrier_bridge.cpp
// builds and runs without the runtime (tests/cpp/barrier_bridge_host_main.cpp, under the sanitizers).
#pragma once
#include <vector>

#include "../../include/mcgpu.h"

namespace mcg {

constexpr int BRIDGE_L_MAX = MCG_BRIDGE_L_MAX;  // levels one pass of k_bridge_survival keeps in registers

// A book of barrier contracts as the kernels walk it.  A level is (barrier, up), compared bitwise; the distinct levels stand in
// the order of their first appearance, level l belongs to group l / l_max and has slot l % l_max there.  `order` lists the
// contracts by group (within a group in book order): order[s] is the book index of the s-th contract the book kernel sees,
// and group g's contracts are order[group_begin[g] .. group_begin[g + 1]).
struct BridgePlan {
    std::vector<double> barrier;   // [n_levels]
    std::vector<int> up;           // [n_levels] 1: an up level
    std::vector<int> level_of;     // [n_contracts] book index -> level
    std::vector<int> order;        // [n_contracts]
    std::vector<int> group_begin;  // [n_groups + 1]
    int n_levels() const { return (int)barrier.size(); }
    int n_groups() const { return (int)group_begin.size() - 1; }
};
// book: n_contracts >= 1 contracts of kinds MCG_X_BARRIER_UP_OUT .. MCG_X_BARRIER_DOWN_IN (checked by the caller); l_max >= 1
void bridge_plan(const mcg_exotic* book, int n_contracts, int l_max, BridgePlan& plan);

// MCG_ERR_INVALID with a message unless B is finite and positive (`what` and `index` name it in the message)
int bridge_check_level(double barrier, const char* what, int index);
// ... unless dt is finite and positive and, on the scalar route (have_var false), sigma is finite and non-negative
int bridge_check_variance(bool have_var, double sigma, double dt);
// ... unless the kind is one of the four barrier kinds
int bridge_check_kind(const mcg_exotic& x, int index);

}  // namespace mcg
