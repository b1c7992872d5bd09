// Host side of the LSM exercise policies (include/mcgpu.h: mcg_lsm_fit, mcg_lsm_apply, mcg_lsm_policy_continuation): what
// a policy must look like, the rows a fit's exported coefficient blocks become, the discount table the apply kernel reads,
// and the continuation curve of a date.  Plain C++ in binary64 with explicit fma, no HIP header: it builds and runs without
// the runtime (tests/cpp/lsm_policy_host_main.cpp, under the sanitizers); the error channel is the library's mcg::fail, which
// that program supplies itself.
#include <cmath>
#include <limits>

#include "../../include/mcgpu.h"

namespace mcg {
int fail(int status, const char* fmt, ...);

// The header alone: what mcg_lsm_fit checks of its arguments and every reader of a policy checks first.
int lsm_policy_check_header(int n_steps, int poly_order, double r, double K, double maturity, double dt) {
    if (n_steps < 0) return fail(MCG_ERR_INVALID, "policy: n_steps must be >= 0 (got %d)", n_steps);
    if (poly_order < 0 || poly_order > 15) return fail(MCG_ERR_INVALID, "poly_order must be in [0,15] (got %d)", poly_order);
    if (!std::isfinite(r) || !std::isfinite(K) || !std::isfinite(maturity) || !std::isfinite(dt))
        return fail(MCG_ERR_INVALID, "r, K, maturity and dt must be finite");
    if (!(K > 0.0)) return fail(MCG_ERR_INVALID, "K must be > 0 (got %g)", K);
    if (!(dt > 0.0)) return fail(MCG_ERR_INVALID, "dt must be > 0 (got %g)", dt);
    return MCG_OK;
}

// A whole policy: the header, then every row's kind and the numbers an EXERCISE_RULE row is evaluated with.
int lsm_policy_check(const mcg_lsm_policy_hdr* hdr, const double* coef) {
    if (!hdr || !coef) return fail(MCG_ERR_INVALID, "policy header/coef is NULL");
    int rc = lsm_policy_check_header(hdr->n_steps, hdr->poly_order, hdr->r, hdr->K, hdr->maturity, hdr->dt);
    if (rc) return rc;
    for (int j = 0; j <= hdr->n_steps; ++j) {
        const double* row = coef + (size_t)j * MCG_LSM_POLICY_STRIDE;
        const double kind = row[18];
        if (!(kind == (double)MCG_POL_CONTINUE || kind == (double)MCG_POL_EXERCISE_RULE || kind == (double)MCG_POL_TERMINAL))
            return fail(MCG_ERR_INVALID, "policy row %d: kind must be 0, 1 or 2 (got %g)", j, kind);
        const bool terminal = kind == (double)MCG_POL_TERMINAL;
        if (j == hdr->n_steps && !terminal) return fail(MCG_ERR_INVALID, "policy row %d (the last one) must be TERMINAL", j);
        if (j < hdr->n_steps && terminal) return fail(MCG_ERR_INVALID, "policy row %d: only row n_steps = %d may be TERMINAL", j, hdr->n_steps);
        if (kind == (double)MCG_POL_EXERCISE_RULE) {
            for (int t = 0; t < 16; ++t)
                if (!std::isfinite(row[t])) return fail(MCG_ERR_INVALID, "policy row %d: coefficient %d is not finite", j, t);
            if (!std::isfinite(row[17])) return fail(MCG_ERR_INVALID, "policy row %d: the centre is not finite", j);
        }
    }
    return MCG_OK;
}

// The coefficient blocks a fit's sweep exported (lsm_device.hpp's layout: [16] rows, [17] centre, [18] and [19] the solve's
// refinement request, spent by then; a date the sweep did not regress is all zeros) become policy rows in place.
void lsm_policy_from_blocks(const mcg_lsm_policy_hdr* hdr, double* coef) {
    for (int j = 0; j <= hdr->n_steps; ++j) {
        double* row = coef + (size_t)j * MCG_LSM_POLICY_STRIDE;
        int kind = MCG_POL_EXERCISE_RULE;
        if (j == hdr->n_steps) kind = MCG_POL_TERMINAL;
        else if ((double)j * hdr->dt > hdr->maturity) kind = MCG_POL_CONTINUE;  // the sweep only discounts there
        else if (!(row[16] > 0.0)) kind = MCG_POL_CONTINUE;                      // no in-the-money path at the fit
        // coefficients above the order, and everything but the count of a row that holds no rule, are 0
        for (int t = kind == MCG_POL_EXERCISE_RULE ? hdr->poly_order + 1 : 0; t < 16; ++t) row[t] = 0.0;
        if (kind != MCG_POL_EXERCISE_RULE) row[17] = 0.0;
        row[18] = (double)kind;
        row[19] = 0.0;
    }
}

// disc[j] = exp(-r dt j), j = 0 .. n_steps: what a cash flow at date j is worth at date 0.
void lsm_policy_discounts(const mcg_lsm_policy_hdr* hdr, double* disc) {
    for (int j = 0; j <= hdr->n_steps; ++j) disc[j] = std::exp(-hdr->r * hdr->dt * (double)j);
}

// Horner in y = (S/K - 1) - centre with fused multiply-adds, as lsm_continuation (lsm_device.hpp) evaluates a fit.
double lsm_policy_row_value(const double* row, int poly_order, double invK, double S) {
    const double y = std::fma(S, invK, -1.0) - row[17];
    double cont = row[poly_order];
    for (int t = poly_order - 1; t >= 0; --t) cont = std::fma(cont, y, row[t]);
    return cont;
}

}  // namespace mcg

extern "C" int mcg_lsm_policy_continuation(const mcg_lsm_policy_hdr* hdr, const double* coef, int date, const double* S, int64_t n,
                                           double* cont_out) {
    int rc = mcg::lsm_policy_check(hdr, coef);
    if (rc) return rc;
    if (date < 0 || date > hdr->n_steps) return mcg::fail(MCG_ERR_INVALID, "date must be in [0, n_steps = %d] (got %d)", hdr->n_steps, date);
    if (n < 0) return mcg::fail(MCG_ERR_INVALID, "n must be >= 0 (got %lld)", (long long)n);
    if (n > 0 && (!S || !cont_out)) return mcg::fail(MCG_ERR_INVALID, "S/cont_out is NULL");
    const double* row = coef + (size_t)date * MCG_LSM_POLICY_STRIDE;
    const double invK = 1.0 / hdr->K;
    for (int64_t i = 0; i < n; ++i) {
        if (row[18] == (double)MCG_POL_EXERCISE_RULE) cont_out[i] = mcg::lsm_policy_row_value(row, hdr->poly_order, invK, S[i]);
        else if (row[18] == (double)MCG_POL_CONTINUE) cont_out[i] = std::numeric_limits<double>::infinity();  // never exercised
        else cont_out[i] = 0.0;  // nothing lies beyond the last date
    }
    return MCG_OK;
}
