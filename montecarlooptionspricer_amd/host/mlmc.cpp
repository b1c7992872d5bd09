// The host side of multilevel Monte Carlo (include/mcgpu.h: mcg_mlmc_combine, mcg_mlmc_plan, mcg_mlmc_bridge_levels) and what
// mcg_mlmc_localvol_level and mcg_mlmc_localvol_level_ex reject of a level's shape, the scheme and the book's bridge levels
// (host/mlmc.hpp).  A host translation unit: no FMA contraction here, so the formulas below, written in any
// language's binary64 in the same order, give the same bits.
#include <cmath>
#include <cstring>

#include "mlmc.hpp"

namespace mcg {
int fail(int status, const char* fmt, ...);

int mlmc_check_level(const mcg_mlmc_level* lv, double T) {
    if (!lv) return fail(MCG_ERR_INVALID, "mlmc: lv is NULL");
    if (!std::isfinite(T)) return fail(MCG_ERR_INVALID, "mlmc: T must be finite");
    if (!(T > 0.0)) return fail(MCG_ERR_INVALID, "mlmc: T must be > 0 (got %g)", T);
    if (lv->n_fine < 1) return fail(MCG_ERR_INVALID, "mlmc: n_fine must be >= 1 (got %d)", lv->n_fine);
    if (lv->has_coarse && (lv->n_fine & 1)) return fail(MCG_ERR_INVALID, "mlmc: a coarse path needs an even n_fine (got %d)", lv->n_fine);
    if (lv->stride_fine < 1 || lv->n_fine % lv->stride_fine != 0)
        return fail(MCG_ERR_INVALID, "mlmc: stride_fine must be >= 1 and divide n_fine = %d (got %d)", lv->n_fine, lv->stride_fine);
    if (lv->has_coarse && (lv->stride_coarse < 1 || (lv->n_fine / 2) % lv->stride_coarse != 0))
        return fail(MCG_ERR_INVALID, "mlmc: stride_coarse must be >= 1 and divide n_coarse = %d (got %d)", lv->n_fine / 2, lv->stride_coarse);
    if (lv->first_obs != 0 && lv->first_obs != 1) return fail(MCG_ERR_INVALID, "mlmc: first_obs must be 0 or 1 (got %d)", lv->first_obs);
    return MCG_OK;
}

int mlmc_check_scheme(int scheme, int bridge) {
    if (scheme != MCG_MLMC_LOG_EULER && scheme != MCG_MLMC_MILSTEIN)
        return fail(MCG_ERR_INVALID, "mlmc: scheme must be 0 (log-Euler) or 1 (Milstein) (got %d)", scheme);
    if (bridge != 0 && bridge != 1) return fail(MCG_ERR_INVALID, "mlmc: bridge must be 0 or 1 (got %d)", bridge);
    return MCG_OK;
}

// The bridge levels of a book: (barrier, up) of its barrier contracts, compared bitwise, in the order of first appearance.
// slot (may be null) [n_contracts]: the level of a barrier contract, MLMC_SLOT_UNTOUCHED for a down barrier at zero,
// MLMC_SLOT_NONE for a contract of another kind.
int mlmc_bridge_plan(const mcg_exotic* book, int n_contracts, double* barriers, int* is_up, int* slot, int* n_levels) {
    int n = 0;
    for (int c = 0; c < n_contracts; ++c) {
        const mcg_exotic& x = book[c];
        if (x.kind < MCG_X_ASIAN_ARITH_FIXED || x.kind > MCG_X_BARRIER_DOWN_IN)
            return fail(MCG_ERR_INVALID, "contract %d: kind must be in [0, 9] (got %d)", c, x.kind);
        int s = MLMC_SLOT_NONE;
        if (x.kind >= MCG_X_BARRIER_UP_OUT) {
            const int up = x.kind == MCG_X_BARRIER_UP_OUT || x.kind == MCG_X_BARRIER_UP_IN;
            if (!std::isfinite(x.barrier)) return fail(MCG_ERR_INVALID, "contract %d: barrier must be finite", c);
            if (!up && x.barrier == 0.0) {
                s = MLMC_SLOT_UNTOUCHED;
            } else if (!(x.barrier > 0.0)) {
                return fail(MCG_ERR_INVALID, "contract %d: a bridge level needs a barrier > 0, or a down barrier at 0 (got %s %g)", c,
                            up ? "up" : "down", x.barrier);
            } else {
                for (s = 0; s < n; ++s)
                    if (std::memcmp(&barriers[s], &x.barrier, sizeof(double)) == 0 && is_up[s] == up) break;
                if (s == n) {
                    if (n == MCG_MLMC_BRIDGE_L_MAX)
                        return fail(MCG_ERR_INVALID, "contract %d: more than %d distinct bridge levels in one call", c, MCG_MLMC_BRIDGE_L_MAX);
                    barriers[n] = x.barrier;
                    is_up[n] = up;
                    ++n;
                }
            }
        }
        if (slot) slot[c] = s;
    }
    *n_levels = n;
    return MCG_OK;
}

// what both host entry points reject of a table of levels
static int mlmc_check_levels(const char* who, int n_levels, const double* n) {
    if (n_levels < 1 || n_levels > MCG_MLMC_MAX_LEVELS)
        return fail(MCG_ERR_INVALID, "%s: n_levels must be in [1, %d] (got %d)", who, MCG_MLMC_MAX_LEVELS, n_levels);
    for (int l = 0; l < n_levels; ++l)
        if (!(n[l] >= 1.0) || !std::isfinite(n[l])) return fail(MCG_ERR_INVALID, "%s: level %d holds no paths (n = %g)", who, l, n[l]);
    return MCG_OK;
}

}  // namespace mcg

using namespace mcg;

extern "C" int mcg_mlmc_bridge_levels(const mcg_exotic* book, int n_contracts, double* barriers, int* is_up, int* n_levels) {
    if (!book || !barriers || !is_up || !n_levels) return fail(MCG_ERR_INVALID, "mlmc bridge levels: book/barriers/is_up/n_levels is NULL");
    if (n_contracts < 1 || n_contracts > 1024) return fail(MCG_ERR_INVALID, "n_contracts must be in [1, 1024] (got %d)", n_contracts);
    return mlmc_bridge_plan(book, n_contracts, barriers, is_up, nullptr, n_levels);
}

extern "C" int mcg_mlmc_combine(const double* sum_y, const double* sum_y2, const double* n, int n_levels, double r, double T,
                                double* price, double* std_err) {
    if (!sum_y || !sum_y2 || !n || !price) return fail(MCG_ERR_INVALID, "mlmc combine: sum_y/sum_y2/n/price is NULL");
    int rc = mlmc_check_levels("mlmc combine", n_levels, n);
    if (rc) return rc;
    if (!std::isfinite(r) || !std::isfinite(T)) return fail(MCG_ERR_INVALID, "mlmc combine: r and T must be finite");
    double mean = 0.0, var = 0.0;
    for (int l = 0; l < n_levels; ++l) {
        const double m = sum_y[l] / n[l];
        double v = 0.0;
        if (n[l] > 1.0) {
            v = (sum_y2[l] - n[l] * m * m) / (n[l] - 1.0);
            if (!(v > 0.0)) v = 0.0;
        }
        mean = mean + m;
        var = var + v / n[l];
    }
    const double disc = std::exp(-r * T);
    *price = disc * mean;
    if (std_err) *std_err = disc * std::sqrt(var);
    return MCG_OK;
}

extern "C" int mcg_mlmc_plan(const double* n, const double* mean, const double* var, const double* cost, int n_levels, double eps,
                             double* n_opt, double* alpha_out, double* bias, int* converged) {
    if (!n || !mean || !var || !cost || !n_opt) return fail(MCG_ERR_INVALID, "mlmc plan: n/mean/var/cost/n_opt is NULL");
    int rc = mlmc_check_levels("mlmc plan", n_levels, n);
    if (rc) return rc;
    if (!std::isfinite(eps) || !(eps > 0.0)) return fail(MCG_ERR_INVALID, "mlmc plan: eps must be finite and > 0");
    for (int l = 0; l < n_levels; ++l) {
        if (!std::isfinite(mean[l])) return fail(MCG_ERR_INVALID, "mlmc plan: mean[%d] is not finite", l);
        if (!std::isfinite(var[l]) || var[l] < 0.0) return fail(MCG_ERR_INVALID, "mlmc plan: var[%d] must be finite and >= 0", l);
        if (!std::isfinite(cost[l]) || !(cost[l] > 0.0)) return fail(MCG_ERR_INVALID, "mlmc plan: cost[%d] must be finite and > 0", l);
    }
    // Giles' rule
    double total = 0.0;
    for (int l = 0; l < n_levels; ++l) total = total + std::sqrt(var[l] * cost[l]);
    const double scale = 2.0 / (eps * eps);
    for (int l = 0; l < n_levels; ++l) n_opt[l] = std::ceil(scale * std::sqrt(var[l] / cost[l]) * total);
    // the weak rate: least squares of log2 |mean_l| on l over the levels l >= 1 with a mean other than zero
    const int L = n_levels - 1;
    double sl = 0.0, sy = 0.0, sll = 0.0, sly = 0.0, cnt = 0.0;
    for (int l = 1; l <= L; ++l) {
        const double m = std::fabs(mean[l]);
        if (m > 0.0) {
            const double y = std::log2(m), x = (double)l;
            cnt = cnt + 1.0;
            sl = sl + x;
            sy = sy + y;
            sll = sll + x * x;
            sly = sly + x * y;
        }
    }
    double alpha = 1.0;
    if (cnt >= 2.0) {
        const double den = cnt * sll - sl * sl;
        if (den > 0.0) alpha = -(cnt * sly - sl * sy) / den;
    }
    if (!(alpha >= 0.5)) alpha = 0.5;  // (a NaN slope too)
    if (alpha > 2.0) alpha = 2.0;
    const double two_a = std::pow(2.0, alpha);
    double b = INFINITY;  // one level: nothing to extrapolate from
    if (L >= 1) {
        b = std::fabs(mean[L]);
        if (L >= 2) {
            const double prev = std::fabs(mean[L - 1]) / two_a;
            if (prev > b) b = prev;
        }
        b = b / (two_a - 1.0);
    }
    if (alpha_out) *alpha_out = alpha;
    if (bias) *bias = b;
    if (converged) *converged = b < eps / std::sqrt(2.0) ? 1 : 0;
    return MCG_OK;
}
