// Host side of the Brownian-bridge barrier pricer: see barrier_bridge.hpp.  Plain C++: no HIP header, so that it builds and
// runs (tests/cpp/barrier_bridge_host_main.cpp, under the sanitizers) without the runtime; the error channel is the
// library's mcg::fail, which that program supplies itself.
#include "barrier_bridge.hpp"

#include <cmath>
#include <cstdint>
#include <cstring>

namespace mcg {
int fail(int status, const char* fmt, ...);

namespace {
uint64_t bits_of(double x) {
    uint64_t u;
    std::memcpy(&u, &x, sizeof(u));
    return u;
}
}  // namespace

void bridge_plan(const mcg_exotic* book, int n_contracts, int l_max, BridgePlan& plan) {
    plan = BridgePlan{};
    plan.level_of.resize((size_t)n_contracts);
    for (int c = 0; c < n_contracts; ++c) {
        const int up = (book[c].kind == MCG_X_BARRIER_UP_OUT || book[c].kind == MCG_X_BARRIER_UP_IN) ? 1 : 0;
        const uint64_t b = bits_of(book[c].barrier);
        int l = 0;
        // (a book holds at most 1024 contracts: the quadratic search is at most half a million comparisons)
        for (; l < plan.n_levels(); ++l)
            if (plan.up[(size_t)l] == up && bits_of(plan.barrier[(size_t)l]) == b) break;
        if (l == plan.n_levels()) {
            plan.barrier.push_back(book[c].barrier);
            plan.up.push_back(up);
        }
        plan.level_of[(size_t)c] = l;
    }
    const int n_groups = (plan.n_levels() + l_max - 1) / l_max;
    plan.group_begin.assign((size_t)n_groups + 1, 0);
    for (int c = 0; c < n_contracts; ++c) ++plan.group_begin[(size_t)(plan.level_of[(size_t)c] / l_max) + 1];
    for (int g = 0; g < n_groups; ++g) plan.group_begin[(size_t)g + 1] += plan.group_begin[(size_t)g];
    plan.order.resize((size_t)n_contracts);
    std::vector<int> at(plan.group_begin.begin(), plan.group_begin.end() - 1);
    for (int c = 0; c < n_contracts; ++c) plan.order[(size_t)at[(size_t)(plan.level_of[(size_t)c] / l_max)]++] = c;
}

int bridge_check_level(double barrier, const char* what, int index) {
    if (!std::isfinite(barrier)) return fail(MCG_ERR_INVALID, "%s %d: barrier must be finite", what, index);
    if (!(barrier > 0.0)) return fail(MCG_ERR_INVALID, "%s %d: barrier must be positive (got %g)", what, index, barrier);
    return MCG_OK;
}

int bridge_check_variance(bool have_var, double sigma, double dt) {
    if (!have_var && !(std::isfinite(sigma) && sigma >= 0.0))
        return fail(MCG_ERR_INVALID, "sigma must be finite and non-negative (got %g)", sigma);
    if (!(std::isfinite(dt) && dt > 0.0)) return fail(MCG_ERR_INVALID, "dt must be finite and positive (got %g)", dt);
    return MCG_OK;
}

int bridge_check_kind(const mcg_exotic& x, int index) {
    if (x.kind < MCG_X_BARRIER_UP_OUT || x.kind > MCG_X_BARRIER_DOWN_IN)
        return fail(MCG_ERR_INVALID, "contract %d: kind must be a barrier kind in [6, 9] (got %d)", index, x.kind);
    return MCG_OK;
}

}  // namespace mcg
