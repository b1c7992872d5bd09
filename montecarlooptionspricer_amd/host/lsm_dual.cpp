// Host side of the dual upper bound (include/mcgpu.h: mcg_lsm_dual_upper): what the call rejects of its policy and inner
// model before it looks at the ctx, and how the inner paths of one (outer path, date) are cut into slices.  Plain C++, no HIP
// header: it builds and runs without the runtime (tests/cpp/lsm_dual_host_main.cpp, under the sanitizers); the error channel
// is the library's mcg::fail, which that program supplies itself.
#include <cmath>

#include "../../include/mcgpu.h"

namespace mcg {
int fail(int status, const char* fmt, ...);
int lsm_policy_check(const mcg_lsm_policy_hdr* hdr, const double* coef);

// Everything of (hdr, coef, model) that is MCG_ERR_INVALID whatever the ctx and the matrix are.
int lsm_dual_check(const mcg_lsm_policy_hdr* hdr, const double* coef, const mcg_lsm_dual_model* model) {
    if (!hdr || !coef || !model) return fail(MCG_ERR_INVALID, "hdr/coef/model is NULL");
    if (model->n_inner < 1 || model->n_inner > MCG_LSM_DUAL_MAX_INNER)
        return fail(MCG_ERR_INVALID, "n_inner must be in [1, %d] (got %d)", MCG_LSM_DUAL_MAX_INNER, model->n_inner);
    if (!std::isfinite(model->sigma) || model->sigma < 0.0)
        return fail(MCG_ERR_INVALID, "the inner model's sigma must be finite and >= 0 (got %g)", model->sigma);
    if (!std::isfinite(model->q)) return fail(MCG_ERR_INVALID, "the inner model's q must be finite");
    if (hdr->n_steps > MCG_LSM_DUAL_MAX_STEPS)
        return fail(MCG_ERR_INVALID, "the inner draws number at most %d dates (the policy has %d)", MCG_LSM_DUAL_MAX_STEPS, hdr->n_steps);
    return lsm_policy_check(hdr, coef);
}

// The inner paths k = 0 .. n_inner - 1 of a date are summed in slices of *per_slice consecutive k, slice s = k / per_slice,
// *n_slices of them (the last one may be short); a slice's sum adds its v in ascending k, a date's sum its slices in
// ascending s.  The cut depends on n_inner and the date count only -- never on the outer paths -- so every split of an outer
// set into shards forms the same sums.  About 2048 / n_steps slices, 64 at most: with the 512 outer paths of a workgroup and
// n_steps dates that is a few thousand workgroups for the smallest outer set.
void lsm_dual_slices(int n_inner, int n_steps, int* per_slice, int* n_slices) {
    const int dates = n_steps < 1 ? 1 : n_steps;
    int want = (2048 + dates - 1) / dates;
    if (want > 64) want = 64;
    if (want > n_inner) want = n_inner;
    if (want < 1) want = 1;
    *per_slice = (n_inner + want - 1) / want;
    *n_slices = (n_inner + *per_slice - 1) / *per_slice;
}

}  // namespace mcg
