// Stand-alone driver of the host side of mcg_mlmc_localvol_level_ex (montecarlooptionspricer_amd/host/mlmc.cpp: mlmc_check_scheme,
// mlmc_bridge_plan, mcg_mlmc_bridge_levels), meant to be compiled together with that file under -fsanitize=address,undefined and
// run directly (tests/test_mlmc_bridge_reference.py does).  It supplies the library's error channel itself, walks through books
// of every size with buffers of exactly the size the interface asks for -- a write past the four levels or past the slots is
// reported -- and through the invalid arguments, and exits 0 when every check holds.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mlmc.hpp"

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

static mcg_exotic contract(int kind, double barrier) {
    mcg_exotic x;
    std::memset(&x, 0, sizeof(x));
    x.kind = kind;
    x.is_call = 0;
    x.K = 100.0;
    x.barrier = barrier;
    x.rebate = 0.0;
    return x;
}

int main() {
    // ---- books of 1 .. 1024 contracts on at most four levels: heap buffers of the exact sizes ------------------------------
    const double B[4] = {85.0, 120.0, 85.0, 97.5};
    const int kinds[4] = {MCG_X_BARRIER_DOWN_OUT, MCG_X_BARRIER_UP_IN, MCG_X_BARRIER_UP_OUT, MCG_X_BARRIER_DOWN_IN};
    for (int nc = 1; nc <= 1024; nc = nc < 12 ? nc + 1 : nc * 2) {
        std::vector<mcg_exotic> book((size_t)nc);
        for (int c = 0; c < nc; ++c) {
            if (c % 7 == 5) book[(size_t)c] = contract(MCG_X_LOOKBACK_FLOAT, 0.0);
            else if (c % 7 == 6) book[(size_t)c] = contract(MCG_X_BARRIER_DOWN_OUT, c % 2 ? 0.0 : -0.0);
            else book[(size_t)c] = contract(kinds[c % 4], B[c % 4]);
        }
        std::vector<double> barriers(MCG_MLMC_BRIDGE_L_MAX);
        std::vector<int> up(MCG_MLMC_BRIDGE_L_MAX), slot((size_t)nc);
        int n = -1;
        CHECK(mcg::mlmc_bridge_plan(book.data(), nc, barriers.data(), up.data(), slot.data(), &n) == MCG_OK);
        CHECK(n == (nc < 4 ? nc : 4));
        for (int c = 0; c < nc; ++c) {
            const int s = slot[(size_t)c];
            if (c % 7 == 5) CHECK(s == mcg::MLMC_SLOT_NONE);
            else if (c % 7 == 6) CHECK(s == mcg::MLMC_SLOT_UNTOUCHED);
            else CHECK(s >= 0 && s < n && barriers[(size_t)s] == B[c % 4] && up[(size_t)s] == (c % 4 == 1 || c % 4 == 2));
        }
        int n2 = -1;
        std::vector<double> b2(MCG_MLMC_BRIDGE_L_MAX);
        std::vector<int> up2(MCG_MLMC_BRIDGE_L_MAX);
        CHECK(mcg_mlmc_bridge_levels(book.data(), nc, b2.data(), up2.data(), &n2) == MCG_OK && n2 == n);
        for (int l = 0; l < n; ++l) CHECK(b2[(size_t)l] == barriers[(size_t)l] && up2[(size_t)l] == up[(size_t)l]);
    }
    // ---- the first appearance decides the order; +0 and -0 are the same "never touched" ------------------------------------
    {
        mcg_exotic book[5] = {contract(MCG_X_BARRIER_UP_OUT, 120.0), contract(MCG_X_BARRIER_DOWN_OUT, 120.0), contract(MCG_X_BARRIER_UP_IN, 120.0),
                              contract(MCG_X_BARRIER_DOWN_OUT, 0.0), contract(MCG_X_ASIAN_GEO_FIXED, -5.0)};
        double barriers[MCG_MLMC_BRIDGE_L_MAX];
        int up[MCG_MLMC_BRIDGE_L_MAX], slot[5], n = -1;
        CHECK(mcg::mlmc_bridge_plan(book, 5, barriers, up, slot, &n) == MCG_OK && n == 2);
        CHECK(barriers[0] == 120.0 && up[0] == 1 && barriers[1] == 120.0 && up[1] == 0);
        CHECK(slot[0] == 0 && slot[1] == 1 && slot[2] == 0 && slot[3] == mcg::MLMC_SLOT_UNTOUCHED && slot[4] == mcg::MLMC_SLOT_NONE);
    }
    // ---- rejections -----------------------------------------------------------------------------------------------------
    {
        double barriers[MCG_MLMC_BRIDGE_L_MAX];
        int up[MCG_MLMC_BRIDGE_L_MAX], n = -1;
        mcg_exotic five[5];
        for (int c = 0; c < 5; ++c) five[c] = contract(MCG_X_BARRIER_DOWN_OUT, 80.0 + c);
        CHECK(mcg_mlmc_bridge_levels(five, 5, barriers, up, &n) == MCG_ERR_INVALID && std::strstr(g_error, "more than 4"));
        CHECK(mcg_mlmc_bridge_levels(five, 4, barriers, up, &n) == MCG_OK && n == 4);
        mcg_exotic x = contract(MCG_X_BARRIER_DOWN_OUT, -1.0);
        CHECK(mcg_mlmc_bridge_levels(&x, 1, barriers, up, &n) == MCG_ERR_INVALID && std::strstr(g_error, "bridge level"));
        x = contract(MCG_X_BARRIER_UP_OUT, 0.0);
        CHECK(mcg_mlmc_bridge_levels(&x, 1, barriers, up, &n) == MCG_ERR_INVALID && std::strstr(g_error, "bridge level"));
        x = contract(MCG_X_BARRIER_UP_IN, NAN);
        CHECK(mcg_mlmc_bridge_levels(&x, 1, barriers, up, &n) == MCG_ERR_INVALID && std::strstr(g_error, "finite"));
        x = contract(MCG_X_BARRIER_DOWN_IN, INFINITY);
        CHECK(mcg_mlmc_bridge_levels(&x, 1, barriers, up, &n) == MCG_ERR_INVALID && std::strstr(g_error, "finite"));
        x = contract(10, 85.0);
        CHECK(mcg_mlmc_bridge_levels(&x, 1, barriers, up, &n) == MCG_ERR_INVALID && std::strstr(g_error, "kind"));
        x = contract(MCG_X_BARRIER_DOWN_OUT, 85.0);
        CHECK(mcg_mlmc_bridge_levels(&x, 0, barriers, up, &n) == MCG_ERR_INVALID && mcg_mlmc_bridge_levels(&x, 1025, barriers, up, &n) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_bridge_levels(nullptr, 1, barriers, up, &n) == MCG_ERR_INVALID && mcg_mlmc_bridge_levels(&x, 1, nullptr, up, &n) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_bridge_levels(&x, 1, barriers, nullptr, &n) == MCG_ERR_INVALID && mcg_mlmc_bridge_levels(&x, 1, barriers, up, nullptr) == MCG_ERR_INVALID);
        for (int scheme = -2; scheme <= 3; ++scheme)
            for (int bridge = -2; bridge <= 3; ++bridge)
                CHECK((mcg::mlmc_check_scheme(scheme, bridge) == MCG_OK) == ((scheme == 0 || scheme == 1) && (bridge == 0 || bridge == 1)));
    }
    if (g_failed) return 1;
    std::printf("ok\n");
    return 0;
}
