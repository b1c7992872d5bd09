// mcg_localvol_table (include/mcgpu.h): the per-step slices of a local-volatility surface as the path kernel gathers them, and
// the validation and scalar constants mcg_paths_localvol* shares with it.  A host translation unit: no FMA contraction here, so
// the loops below, written in any language's binary64, give the same bits.
#include <cmath>

#include "../csrc/mcg_internal.hpp"

namespace mcg {

int localvol_check_surface(const double* times, int n_t, int n_x, const double* sigma, double dt, int n_steps) {
    if (!times || !sigma) return fail(MCG_ERR_INVALID, "local vol: times/sigma is NULL");
    if (n_t < 1 || n_t > LOCALVOL_MAX_NT) return fail(MCG_ERR_INVALID, "local vol: n_t must be in [1, %d] (got %d)", LOCALVOL_MAX_NT, n_t);
    if (n_x < 2 || n_x > LOCALVOL_MAX_NX) return fail(MCG_ERR_INVALID, "local vol: n_x must be in [2, %d] (got %d)", LOCALVOL_MAX_NX, n_x);
    for (int i = 0; i < n_t; ++i) {
        if (!std::isfinite(times[i])) return fail(MCG_ERR_INVALID, "local vol: times[%d] is not finite", i);
        if (i > 0 && !(times[i] > times[i - 1]))
            return fail(MCG_ERR_INVALID, "local vol: times must be strictly increasing (times[%d] = %.17g, times[%d] = %.17g)", i - 1,
                        times[i - 1], i, times[i]);
    }
    for (int k = 0; k < n_t * n_x; ++k) {
        if (!std::isfinite(sigma[k])) return fail(MCG_ERR_INVALID, "local vol: sigma[%d][%d] is not finite", k / n_x, k % n_x);
        if (!(sigma[k] >= 0.0)) return fail(MCG_ERR_INVALID, "local vol: sigma[%d][%d] must be >= 0 (got %g)", k / n_x, k % n_x, sigma[k]);
    }
    if (!std::isfinite(dt)) return fail(MCG_ERR_INVALID, "local vol: dt must be finite");
    if (!(dt > 0.0)) return fail(MCG_ERR_INVALID, "local vol: dt must be > 0");
    if (n_steps < 1) return fail(MCG_ERR_INVALID, "local vol: n_steps must be >= 1 (got %d)", n_steps);
    return MCG_OK;
}

// The table of the header; the surface has passed localvol_check_surface.
void localvol_fill_table(const double* times, int n_t, int n_x, const double* sigma, double dt, int n_steps, double* table) {
    const int n_slices = n_t == 1 ? 1 : n_steps;
    const double sq = std::sqrt(dt);
    double a[LOCALVOL_MAX_NX];
    for (int n = 0; n < n_slices; ++n) {
        const double t = (double)n * dt;
        if (t <= times[0] || t >= times[n_t - 1]) {  // flat beyond the first and the last knot
            const double* row = sigma + (size_t)(t <= times[0] ? 0 : n_t - 1) * n_x;
            for (int j = 0; j < n_x; ++j) a[j] = row[j] * sq;
        } else {
            int i = 0;
            while (!(t < times[i + 1])) ++i;  // times[i] <= t < times[i + 1]
            const double g = (t - times[i]) / (times[i + 1] - times[i]);
            const double* lo = sigma + (size_t)i * n_x;
            for (int j = 0; j < n_x; ++j) a[j] = (lo[j] + g * (lo[n_x + j] - lo[j])) * sq;
        }
        double* row = table + (size_t)n * (n_x - 1) * 2;
        for (int j = 0; j < n_x - 1; ++j) {
            row[2 * j] = a[j];
            row[2 * j + 1] = a[j + 1] - a[j];
        }
    }
}

int localvol_check_model(double S0, double r, double q, double x_min, double x_max, bool payoff, double K) {
    const double args[] = {S0, r, q, x_min, x_max};
    const char* names[] = {"S0", "r", "q", "x_min", "x_max"};
    for (int i = 0; i < 5; ++i)
        if (!std::isfinite(args[i])) return fail(MCG_ERR_INVALID, "local vol: %s must be finite", names[i]);
    if (payoff && !std::isfinite(K)) return fail(MCG_ERR_INVALID, "local vol: K must be finite");
    if (!(S0 > 0.0)) return fail(MCG_ERR_INVALID, "local vol: S0 must be > 0");
    if (!(x_min < x_max)) return fail(MCG_ERR_INVALID, "local vol: x_min must be < x_max (got %g, %g)", x_min, x_max);
    return MCG_OK;
}

LocalVolScalars localvol_scalars(double r, double q, double x_min, double x_max, int n_x, double dt) {
    LocalVolScalars c;
    c.inv_dx = (double)(n_x - 1) / (x_max - x_min);
    c.u0 = -x_min * c.inv_dx;
    c.m = (r - q) * dt;
    return c;
}

}  // namespace mcg

extern "C" int mcg_localvol_table(const double* times, int n_t, int n_x, const double* sigma, double dt, int n_steps,
                                  double* table_out) {
    if (!table_out) return mcg::fail(MCG_ERR_INVALID, "local vol: table_out is NULL");
    int rc = mcg::localvol_check_surface(times, n_t, n_x, sigma, dt, n_steps);
    if (rc) return rc;
    mcg::localvol_fill_table(times, n_t, n_x, sigma, dt, n_steps, table_out);
    return MCG_OK;
}
