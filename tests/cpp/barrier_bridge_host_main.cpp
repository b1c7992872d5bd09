// Stand-alone driver of the host part of the Brownian-bridge barrier pricer (montecarlooptionspricer_amd/host/barrier_bridge.cpp:
// bridge_plan and the checks), meant to be compiled together with that file under -fsanitize=address,undefined and run directly
// (tests/test_barrier_bridge_reference.py does).  It supplies the library's error channel itself, walks through the books named
// in that test and exits 0 when every check holds.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../montecarlooptionspricer_amd/host/barrier_bridge.hpp"

static char g_error[512];

namespace mcg {
int fail(int status, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return status;
}
}  // namespace mcg

static int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);     \
            ++g_failed;                                                      \
        }                                                                    \
    } while (0)

using mcg::BridgePlan;
constexpr int LM = mcg::BRIDGE_L_MAX;

static mcg_exotic contract(int kind, double barrier, double rebate = 0.0) { return mcg_exotic{kind, 1, 100.0, barrier, rebate}; }
static bool is_up(const mcg_exotic& x) { return x.kind == MCG_X_BARRIER_UP_OUT || x.kind == MCG_X_BARRIER_UP_IN; }
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

// What every plan must satisfy, whatever the book: the map points at the contract's own level, the levels are distinct and in
// the order of first appearance, `order` is a permutation sorted by group that keeps the book order inside a group, and
// group_begin counts the groups' contracts.  n_levels: what the caller expects.
static void check_plan(const std::vector<mcg_exotic>& book, int l_max, int n_levels) {
    BridgePlan p;
    mcg::bridge_plan(book.data(), (int)book.size(), l_max, p);
    const int nc = (int)book.size();
    CHECK(p.n_levels() == n_levels);
    CHECK((int)p.up.size() == p.n_levels() && (int)p.level_of.size() == nc && (int)p.order.size() == nc);
    CHECK(p.n_groups() == (n_levels + l_max - 1) / l_max);
    if (g_failed) return;
    int seen = 0;
    for (int c = 0; c < nc; ++c) {
        const int l = p.level_of[c];
        CHECK(l >= 0 && l < p.n_levels());
        CHECK(same_bits(p.barrier[l], book[c].barrier) && (p.up[l] != 0) == is_up(book[c]));
        CHECK(l <= seen);                       // first appearance numbers the levels
        if (l == seen) ++seen;
    }
    CHECK(seen == p.n_levels());
    for (int a = 0; a < p.n_levels(); ++a)
        for (int b = a + 1; b < p.n_levels(); ++b) CHECK(!(same_bits(p.barrier[a], p.barrier[b]) && p.up[a] == p.up[b]));
    std::vector<int> hits(nc, 0);
    CHECK(p.group_begin.front() == 0 && p.group_begin.back() == nc);
    for (int g = 0; g < p.n_groups(); ++g) {
        CHECK(p.group_begin[g] < p.group_begin[g + 1]);   // every group holds a contract
        for (int s = p.group_begin[g]; s < p.group_begin[g + 1]; ++s) {
            const int c = p.order[s];
            CHECK(c >= 0 && c < nc);
            if (c < 0 || c >= nc) continue;
            ++hits[c];
            CHECK(p.level_of[c] / l_max == g);
            if (s > p.group_begin[g]) CHECK(p.order[s - 1] < c);
        }
    }
    for (int c = 0; c < nc; ++c) CHECK(hits[c] == 1);
}

int main() {
    // one contract; 1024 contracts on one level; 1024 distinct levels
    check_plan({contract(MCG_X_BARRIER_DOWN_OUT, 90.0)}, LM, 1);
    {
        std::vector<mcg_exotic> same, distinct;
        for (int c = 0; c < 1024; ++c) {
            same.push_back(contract(c % 2 ? MCG_X_BARRIER_UP_OUT : MCG_X_BARRIER_UP_IN, 120.0, (double)c));
            distinct.push_back(contract(MCG_X_BARRIER_DOWN_OUT + c % 2, 50.0 + 0.01 * c));
        }
        check_plan(same, LM, 1);
        check_plan(distinct, LM, 1024);
        check_plan(distinct, 1, 1024);
    }
    // L_MAX - 1, L_MAX, L_MAX + 1 and 2 L_MAX + 3 distinct levels, each level used by three contracts that stand apart in the book
    for (int nl : {LM - 1, LM, LM + 1, 2 * LM + 3}) {
        std::vector<mcg_exotic> book;
        for (int rep = 0; rep < 3; ++rep)
            for (int l = 0; l < nl; ++l) {
                const int q = rep == 1 ? nl - 1 - l : l;   // the second round walks the levels backwards
                book.push_back(contract(q % 2 ? MCG_X_BARRIER_UP_OUT + rep % 2 : MCG_X_BARRIER_DOWN_OUT + rep % 2, 80.0 + q, 0.5 * rep));
            }
        check_plan(book, LM, nl);
        BridgePlan p;
        mcg::bridge_plan(book.data(), (int)book.size(), LM, p);
        for (int l = 0; l < nl; ++l) {
            CHECK(p.barrier[l] == 80.0 + l && p.up[l] == l % 2);
            CHECK(p.level_of[l] == l && p.level_of[nl + (nl - 1 - l)] == l && p.level_of[2 * nl + l] == l);
        }
        const int n_groups = (nl + LM - 1) / LM;
        CHECK(p.n_groups() == n_groups);
        for (int g = 0; g < n_groups; ++g) CHECK(p.group_begin[g + 1] - p.group_begin[g] == 3 * (std::min(nl, (g + 1) * LM) - g * LM));
    }
    // +0.0 and -0.0 rebates share a level (only the barrier and the direction make one); one barrier in both directions is two
    {
        std::vector<mcg_exotic> book = {contract(MCG_X_BARRIER_UP_OUT, 110.0, 0.0), contract(MCG_X_BARRIER_UP_IN, 110.0, -0.0),
                                        contract(MCG_X_BARRIER_DOWN_OUT, 110.0, 0.0), contract(MCG_X_BARRIER_DOWN_IN, 110.0, -0.0),
                                        contract(MCG_X_BARRIER_UP_OUT, std::nextafter(110.0, 111.0), 0.0)};
        check_plan(book, LM, 3);
        BridgePlan p;
        mcg::bridge_plan(book.data(), 5, LM, p);
        CHECK(p.level_of[0] == 0 && p.level_of[1] == 0 && p.level_of[2] == 1 && p.level_of[3] == 1 && p.level_of[4] == 2);
        CHECK(p.up[0] == 1 && p.up[1] == 0 && p.up[2] == 1);
    }
    // the checks
    CHECK(mcg::bridge_check_level(90.0, "level", 0) == MCG_OK);
    for (double bad : {0.0, -0.0, -1.0, std::numeric_limits<double>::infinity(), std::nan("")}) {
        g_error[0] = 0;
        CHECK(mcg::bridge_check_level(bad, "level", 3) == MCG_ERR_INVALID && std::strstr(g_error, "level 3: barrier must be") != nullptr);
    }
    CHECK(mcg::bridge_check_variance(false, 0.0, 0.01) == MCG_OK && mcg::bridge_check_variance(true, std::nan(""), 0.01) == MCG_OK);
    for (double bad : {-0.1, std::numeric_limits<double>::infinity(), std::nan("")})
        CHECK(mcg::bridge_check_variance(false, bad, 0.01) == MCG_ERR_INVALID && std::strstr(g_error, "sigma must be") != nullptr);
    for (double bad : {0.0, -0.01, std::numeric_limits<double>::infinity(), std::nan("")})
        CHECK(mcg::bridge_check_variance(true, 0.2, bad) == MCG_ERR_INVALID && std::strstr(g_error, "dt must be") != nullptr);
    for (int kind = -1; kind <= 10; ++kind)
        CHECK((mcg::bridge_check_kind(contract(kind, 90.0), 7) == MCG_OK) == (kind >= MCG_X_BARRIER_UP_OUT && kind <= MCG_X_BARRIER_DOWN_IN));
    CHECK(std::strstr(g_error, "contract 7: kind must be a barrier kind") != nullptr);
    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
