// mcg_cholesky_corr (include/mcgpu.h): the lower Cholesky factor of a correlation matrix, in the Cholesky-Banachiewicz order
// the header states.  A host translation unit: no FMA contraction here, so the loop below, written in any language's
// binary64, gives the same bits.
#include <cmath>

#include "../csrc/mcg_internal.hpp"

using mcg::fail;

extern "C" int mcg_cholesky_corr(const double* corr, int n, double* L) {
    if (!corr || !L) return fail(MCG_ERR_INVALID, "cholesky: corr/L is NULL");
    if (n < 1 || n > 8) return fail(MCG_ERR_INVALID, "cholesky: n must be in [1, 8] (got %d)", n);
    for (int i = 0; i < n * n; ++i)
        if (!std::isfinite(corr[i])) return fail(MCG_ERR_INVALID, "cholesky: corr[%d][%d] is not finite", i / n, i % n);
    for (int i = 0; i < n; ++i) {
        if (corr[i * n + i] != 1.0) return fail(MCG_ERR_INVALID, "cholesky: the diagonal of a correlation matrix is 1 (corr[%d][%d] = %.17g)", i, i, corr[i * n + i]);
        for (int j = 0; j < i; ++j) {
            if (corr[i * n + j] != corr[j * n + i])
                return fail(MCG_ERR_INVALID, "cholesky: corr is not symmetric (corr[%d][%d] = %.17g, corr[%d][%d] = %.17g)", i, j, corr[i * n + j], j, i, corr[j * n + i]);
            if (!(std::fabs(corr[i * n + j]) <= 1.0))
                return fail(MCG_ERR_INVALID, "cholesky: |corr[%d][%d]| exceeds 1 (%.17g)", i, j, corr[i * n + j]);
        }
    }
    double F[64];  // (L may alias corr: the factor is built here)
    for (int i = 0; i < n * n; ++i) F[i] = 0.0;
    for (int j = 0; j < n; ++j) {
        double sum = 0.0;
        for (int k = 0; k < j; ++k) sum = sum + F[j * n + k] * F[j * n + k];
        const double d = corr[j * n + j] - sum;
        if (!(d > 1e-10))
            return fail(MCG_ERR_INVALID, "cholesky: corr is not positive definite (pivot %d is %.3g; perfectly correlated assets are out of scope)", j, d);
        const double ljj = std::sqrt(d);
        F[j * n + j] = ljj;
        for (int i = j + 1; i < n; ++i) {
            double s = 0.0;
            for (int k = 0; k < j; ++k) s = s + F[i * n + k] * F[j * n + k];
            F[i * n + j] = (corr[i * n + j] - s) / ljj;
        }
    }
    for (int i = 0; i < n * n; ++i) L[i] = F[i];
    return MCG_OK;
}
