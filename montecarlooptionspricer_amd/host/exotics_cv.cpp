// Host arithmetic of the control-variate estimator (include/mcgpu.h: mcg_exotics_cv_from_sums, mcg_gbm_expectation).
// Plain C++: no HIP header, so that it builds and runs (tests/cpp/exotics_cv_host_main.cpp, under the sanitizers) without
// the runtime; the error channel is the library's mcg::fail, which that program supplies itself.
#include <algorithm>
#include <cmath>

#include "../../include/mcgpu.h"

namespace mcg {
int fail(int status, const char* fmt, ...);
}

namespace {

// sums_to_mean_stderr of mcg_internal.hpp on {sum Y, sum Y^2, n}, discounted
void plain_estimate(double sum, double sum2, double n, double disc, double* price, double* se) {
    const double m = sum / n;
    const double var = n > 1.0 ? std::max(0.0, (sum2 - n * m * m) / (n - 1.0)) : 0.0;
    *price = disc * m;
    *se = disc * std::sqrt(var / n);
}

double norm_cdf(double x) { return 0.5 * std::erfc(-x * 0.70710678118654752440); }

// E max(X - K, 0) / E max(K - X, 0) for ln X ~ N(mu, var): Black's formula on the forward e^{mu + var/2}, undiscounted.
// var = 0 or K <= 0 (X > 0 always): the deterministic payoff of the forward.
double black_lognormal(double mu, double var, double K, bool call) {
    const double F = std::exp(mu + 0.5 * var);
    if (!(var > 0.0) || !(K > 0.0)) return call ? std::max(F - K, 0.0) : std::max(K - F, 0.0);
    const double sd = std::sqrt(var);
    const double d2 = (mu - std::log(K)) / sd, d1 = d2 + sd;
    return call ? F * norm_cdf(d1) - K * norm_cdf(d2) : K * norm_cdf(-d2) - F * norm_cdf(-d1);
}

}  // namespace

int mcg_exotics_cv_from_sums(const double* sums, int n_contracts, const int* ctrl, double r, double T, double* price, double* std_err,
                             double* beta, double* plain_price, double* plain_se) {
    if (!sums || !ctrl || !price) return mcg::fail(MCG_ERR_INVALID, "sums/ctrl/price is NULL");
    if (n_contracts < 1 || n_contracts > 1024) return mcg::fail(MCG_ERR_INVALID, "n_contracts must be in [1, 1024] (got %d)", n_contracts);
    for (int c = 0; c < n_contracts; ++c)
        if (ctrl[2 * c + 1] >= 0 && ctrl[2 * c] < 0)
            return mcg::fail(MCG_ERR_INVALID, "contract %d: a second control needs a first one", c);
    const double n = sums[9 * (size_t)n_contracts];
    if (!(n >= 1.0)) return mcg::fail(MCG_ERR_EMPTY_PATHS, "no paths to price");
    const double disc = std::exp(-r * T);
    for (int c = 0; c < n_contracts; ++c) {
        const double* s = sums + 9 * (size_t)c;
        double pp, ps;
        plain_estimate(s[0], s[1], n, disc, &pp, &ps);
        if (plain_price) plain_price[c] = pp;
        if (plain_se) plain_se[c] = ps;
        const double yb = s[0] / n;
        const double Syy = s[1] - n * yb * yb;
        // slot 0: a, slot 1: b
        double db[2] = {0.0, 0.0}, Sdd[2] = {0.0, 0.0}, Syd[2] = {0.0, 0.0};
        bool kept[2] = {false, false};
        for (int k = 0; k < 2; ++k) {
            if (ctrl[2 * c + k] < 0) continue;
            const double *t = s + 2 + 3 * k;  // {sum d, sum d^2, sum Y d}
            db[k] = t[0] / n;
            Sdd[k] = t[1] - n * db[k] * db[k];
            Syd[k] = t[2] - n * yb * db[k];
            kept[k] = Sdd[k] > 1e-12 * t[1];
        }
        double rho = 0.0;
        if (kept[0] && kept[1]) {
            const double Sab = s[8] - n * db[0] * db[1];
            rho = Sab / std::sqrt(Sdd[0] * Sdd[1]);
            if (1.0 - rho * rho <= 1e-8) kept[1] = false;
        }
        int n_kept = (kept[0] ? 1 : 0) + (kept[1] ? 1 : 0);
        if (n - 1.0 - n_kept < 1.0) {
            kept[0] = kept[1] = false;
            n_kept = 0;
        }
        double g[2] = {0.0, 0.0}, u[2] = {0.0, 0.0}, b[2] = {0.0, 0.0};
        for (int k = 0; k < 2; ++k)
            if (kept[k]) u[k] = Syd[k] / std::sqrt(Sdd[k]);
        if (n_kept == 2) {
            g[1] = (u[1] - rho * u[0]) / (1.0 - rho * rho);
            g[0] = u[0] - rho * g[1];
            b[0] = g[0] / std::sqrt(Sdd[0]);
            b[1] = g[1] / std::sqrt(Sdd[1]);
        } else if (n_kept == 1) {
            const int k = kept[0] ? 0 : 1;
            g[k] = u[k];
            b[k] = Syd[k] / Sdd[k];
        }
        const double rss = std::max(Syy - (g[0] * u[0] + g[1] * u[1]), 0.0);
        const double dof = n - 1.0 - n_kept;
        price[c] = disc * (yb - (b[0] * db[0] + b[1] * db[1]));
        if (std_err) std_err[c] = dof >= 1.0 ? disc * std::sqrt(rss / dof / n) : 0.0;
        if (beta) {
            beta[2 * c] = b[0];
            beta[2 * c + 1] = b[1];
        }
    }
    return MCG_OK;
}

int mcg_gbm_expectation(const mcg_control* c, double S0, double r, double q, double sigma, double dt, int n_steps, int first_row,
                        double* mean) {
    if (!c || !mean) return mcg::fail(MCG_ERR_INVALID, "control/mean is NULL");
    if (!(std::isfinite(S0) && std::isfinite(r) && std::isfinite(q) && std::isfinite(dt)) || !(S0 > 0.0) || !(dt > 0.0))
        return mcg::fail(MCG_ERR_INVALID, "gbm expectation: S0 and dt must be positive, r and q finite");
    if (n_steps < 1 || first_row < 0 || first_row > n_steps)
        return mcg::fail(MCG_ERR_INVALID, "gbm expectation: n_steps must be >= 1 and first_row in [0, n_steps] (got %d, %d)", n_steps, first_row);
    const int N = n_steps - first_row + 1;
    const double g = r - q;
    if (c->form == MCG_CV_ST) {
        *mean = S0 * std::exp(g * ((double)n_steps * dt));
        return MCG_OK;
    }
    if (c->form == MCG_CV_A) {
        double s = 0.0;
        for (int j = first_row; j <= n_steps; ++j) s += std::exp(g * ((double)j * dt));
        *mean = S0 / (double)N * s;
        return MCG_OK;
    }
    const bool geo = c->form == MCG_CV_G || (c->form == MCG_CV_PAYOFF && c->x.kind == MCG_X_ASIAN_GEO_FIXED);
    if (!geo && c->form != MCG_CV_VANILLA) {
        if (c->form < MCG_CV_PAYOFF || c->form > MCG_CV_G) return mcg::fail(MCG_ERR_INVALID, "control form must be in [0, 4] (got %d)", c->form);
        return mcg::fail(MCG_ERR_INVALID, "gbm expectation: no closed form for a payoff of kind %d", c->x.kind);
    }
    if (!std::isfinite(sigma) || sigma < 0.0) return mcg::fail(MCG_ERR_INVALID, "gbm expectation: sigma must be finite and >= 0");
    const double drift = g - 0.5 * sigma * sigma;
    double mu, var;
    if (geo) {
        // sum_{j,k} min(t_j, t_k) over the N sorted dates: t_i counts for the 2 (N - 1 - i) + 1 pairs whose smaller member it is
        double tsum = 0.0, msum = 0.0;
        for (int i = 0; i < N; ++i) {
            const double t = (double)(first_row + i) * dt;
            tsum += t;
            msum += t * (double)(2 * (N - 1 - i) + 1);
        }
        mu = std::log(S0) + drift * (tsum / (double)N);
        var = sigma * sigma * msum / ((double)N * (double)N);
    } else {
        const double T = (double)n_steps * dt;
        mu = std::log(S0) + drift * T;
        var = sigma * sigma * T;
    }
    if (c->form == MCG_CV_G) {
        *mean = std::exp(mu + 0.5 * var);
        return MCG_OK;
    }
    if (!std::isfinite(c->x.K)) return mcg::fail(MCG_ERR_INVALID, "gbm expectation: K must be finite");
    *mean = black_lognormal(mu, var, c->x.K, c->x.is_call != 0);
    return MCG_OK;
}
