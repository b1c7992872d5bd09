// Stand-alone driver of the host side of multilevel Monte Carlo (montecarlooptionspricer_amd/host/mlmc.cpp: mcg_mlmc_combine,
// mcg_mlmc_plan, and what mcg_mlmc_localvol_level rejects of a level's shape), meant to be compiled together with that file under
// -fsanitize=address,undefined and run directly (tests/test_mlmc_reference.py does).  It supplies the library's error channel
// itself, walks through every level count with buffers of exactly the size the interface asks for -- a write past n_opt's end
// is reported -- and through the invalid arguments, and exits 0 when every check holds.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <vector>

#include "mcgpu.h"

static char g_error[512];

namespace mcg {
int fail(int status, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return status;
}
int mlmc_check_level(const mcg_mlmc_level* lv, double T);
}  // namespace mcg

static int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);     \
            ++g_failed;                                                      \
        }                                                                    \
    } while (0)

int main() {
    // ---- every level count: geometric tables as the theory gives them -----------------------------------------------------
    for (int L = 1; L <= MCG_MLMC_MAX_LEVELS; ++L) {
        std::vector<double> n((size_t)L), mean((size_t)L), var((size_t)L), cost((size_t)L), n_opt((size_t)L), sy((size_t)L), sy2((size_t)L);
        for (int l = 0; l < L; ++l) {
            n[(size_t)l] = 1000.0;
            mean[(size_t)l] = l ? 0.8 * std::ldexp(1.0, -l) : 10.0;
            var[(size_t)l] = l ? 0.3 * std::ldexp(1.0, -l) : 185.0;
            cost[(size_t)l] = l ? 6.0 * std::ldexp(1.0, l) : 4.0;
            sy[(size_t)l] = mean[(size_t)l] * n[(size_t)l];
            sy2[(size_t)l] = (var[(size_t)l] + mean[(size_t)l] * mean[(size_t)l]) * n[(size_t)l];
        }
        double alpha = -1.0, bias = -1.0, price = -1.0, se = -1.0;
        int conv = -1;
        CHECK(mcg_mlmc_plan(n.data(), mean.data(), var.data(), cost.data(), L, 0.01, n_opt.data(), &alpha, &bias, &conv) == MCG_OK);
        for (int l = 0; l < L; ++l) CHECK(n_opt[(size_t)l] >= 1.0 && n_opt[(size_t)l] == std::floor(n_opt[(size_t)l]));
        for (int l = 2; l < L; ++l) CHECK(n_opt[(size_t)l] <= n_opt[(size_t)l - 1]);  // V falls, C rises
        CHECK(alpha >= 0.5 && alpha <= 2.0 && (conv == 0 || conv == 1));
        if (L == 1) CHECK(std::isinf(bias) && conv == 0);
        if (L >= 3) CHECK(std::fabs(alpha - 1.0) <= 1e-12 && std::fabs(bias - mean[(size_t)L - 1]) <= 1e-12);  // the last two terms tie
        if (L >= 10) CHECK(conv == 1);
        CHECK(mcg_mlmc_combine(sy.data(), sy2.data(), n.data(), L, 0.04, 1.0, &price, &se) == MCG_OK);
        CHECK(price > 0.0 && se > 0.0 && std::isfinite(price) && std::isfinite(se));
        CHECK(mcg_mlmc_combine(sy.data(), sy2.data(), n.data(), L, 0.04, 1.0, &price, nullptr) == MCG_OK);
        CHECK(mcg_mlmc_plan(n.data(), mean.data(), var.data(), cost.data(), L, 0.01, n_opt.data(), nullptr, nullptr, nullptr) == MCG_OK);
    }
    {   // the formulas on numbers one can do by hand
        const double sy[2] = {3.0, 1.0}, sy2[2] = {9.0, 5.0}, n[2] = {1.0, 2.0};
        double price = -1.0, se = -1.0;
        CHECK(mcg_mlmc_combine(sy, sy2, n, 2, 0.0, 1.0, &price, &se) == MCG_OK && price == 3.5 && se == 1.5);  // V_0 = 0 at one path
        const double m[3] = {9.0, 0.0, 0.0}, v[3] = {4.0, 0.0, 0.0}, c[3] = {4.0, 12.0, 24.0}, nn[3] = {5.0, 5.0, 5.0};
        double n_opt[3], alpha = -1.0, bias = -1.0;
        int conv = -1;
        CHECK(mcg_mlmc_plan(nn, m, v, c, 3, 1.0, n_opt, &alpha, &bias, &conv) == MCG_OK);
        CHECK(n_opt[0] == 8.0 && n_opt[1] == 0.0 && n_opt[2] == 0.0 && alpha == 1.0 && bias == 0.0 && conv == 1);
    }
    {   // what the two reject
        const double one[2] = {1.0, 1.0}, zero[2] = {1.0, 0.0}, neg[2] = {1.0, -1.0}, nan[2] = {1.0, std::nan("")};
        double out[2], x = 0.0;
        std::vector<double> big((size_t)MCG_MLMC_MAX_LEVELS + 1, 1.0), big_out((size_t)MCG_MLMC_MAX_LEVELS + 1);
        CHECK(mcg_mlmc_combine(nullptr, one, one, 2, 0.0, 1.0, &x, &x) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_combine(one, nullptr, one, 2, 0.0, 1.0, &x, &x) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_combine(one, one, nullptr, 2, 0.0, 1.0, &x, &x) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_combine(one, one, one, 2, 0.0, 1.0, nullptr, &x) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_combine(one, one, one, 0, 0.0, 1.0, &x, &x) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_combine(big.data(), big.data(), big.data(), MCG_MLMC_MAX_LEVELS + 1, 0.0, 1.0, &x, &x) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_combine(one, one, zero, 2, 0.0, 1.0, &x, &x) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_combine(one, one, nan, 2, 0.0, 1.0, &x, &x) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_combine(one, one, one, 2, std::nan(""), 1.0, &x, &x) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_combine(one, one, one, 2, 0.0, INFINITY, &x, &x) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(nullptr, one, one, one, 2, 0.1, out, &x, &x, nullptr) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(one, nullptr, one, one, 2, 0.1, out, &x, &x, nullptr) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(one, one, nullptr, one, 2, 0.1, out, &x, &x, nullptr) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(one, one, one, nullptr, 2, 0.1, out, &x, &x, nullptr) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(one, one, one, one, 2, 0.1, nullptr, &x, &x, nullptr) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(one, one, one, one, 0, 0.1, out, &x, &x, nullptr) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(big.data(), big.data(), big.data(), big.data(), MCG_MLMC_MAX_LEVELS + 1, 0.1, big_out.data(), &x, &x, nullptr) ==
              MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(zero, one, one, one, 2, 0.1, out, &x, &x, nullptr) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(one, nan, one, one, 2, 0.1, out, &x, &x, nullptr) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(one, one, neg, one, 2, 0.1, out, &x, &x, nullptr) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(one, one, nan, one, 2, 0.1, out, &x, &x, nullptr) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(one, one, one, zero, 2, 0.1, out, &x, &x, nullptr) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(one, one, one, neg, 2, 0.1, out, &x, &x, nullptr) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(one, one, one, one, 2, 0.0, out, &x, &x, nullptr) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(one, one, one, one, 2, -0.1, out, &x, &x, nullptr) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(one, one, one, one, 2, std::nan(""), out, &x, &x, nullptr) == MCG_ERR_INVALID);
        CHECK(mcg_mlmc_plan(one, one, one, one, 2, 0.1, out, &x, &x, nullptr) == MCG_OK);
    }
    {   // the shape of a level
        const mcg_mlmc_level ok{7ull, 8, 1, 2, 1, 1, 0ull, 100};
        CHECK(mcg::mlmc_check_level(&ok, 1.0) == MCG_OK);
        CHECK(mcg::mlmc_check_level(nullptr, 1.0) == MCG_ERR_INVALID);
        for (double T : {0.0, -1.0, (double)INFINITY, (double)NAN}) CHECK(mcg::mlmc_check_level(&ok, T) == MCG_ERR_INVALID);
        auto with = [&](int n_fine, int coarse, int sf, int sc, int first) {
            const mcg_mlmc_level lv{7ull, n_fine, coarse, sf, sc, first, ~0ull, 1};
            return mcg::mlmc_check_level(&lv, 0.5);
        };
        CHECK(with(1, 0, 1, 0, 0) == MCG_OK);        // (stride_coarse is not read without a coarse path)
        CHECK(with(7, 0, 7, -3, 1) == MCG_OK);
        CHECK(with(2, 1, 2, 1, 1) == MCG_OK);
        CHECK(with(252, 1, 126, 63, 0) == MCG_OK);
        CHECK(with(0, 0, 1, 1, 1) == MCG_ERR_INVALID);
        CHECK(with(-2, 1, 1, 1, 1) == MCG_ERR_INVALID);
        CHECK(with(7, 1, 1, 1, 1) == MCG_ERR_INVALID);
        CHECK(with(8, 1, 0, 1, 1) == MCG_ERR_INVALID);
        CHECK(with(8, 1, -1, 1, 1) == MCG_ERR_INVALID);
        CHECK(with(8, 1, 3, 1, 1) == MCG_ERR_INVALID);
        CHECK(with(8, 1, 16, 1, 1) == MCG_ERR_INVALID);
        CHECK(with(8, 1, 1, 0, 1) == MCG_ERR_INVALID);
        CHECK(with(8, 1, 1, 3, 1) == MCG_ERR_INVALID);
        CHECK(with(8, 1, 1, 8, 1) == MCG_ERR_INVALID);
        CHECK(with(8, 1, 1, 1, 2) == MCG_ERR_INVALID);
        CHECK(with(8, 1, 1, 1, -1) == MCG_ERR_INVALID);
    }
    if (g_failed) {
        std::printf("%d check(s) failed (last message: %s)\n", g_failed, g_error);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
