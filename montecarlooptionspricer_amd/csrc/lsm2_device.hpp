// Device-side pieces of the two-regressor Longstaff-Schwartz sweep (kernels_lsm2.hip; the contract is stated at
// mcg_price_lsm2 in include/mcgpu.h): the monomial basis in the two standardised regressors and the LDL^T solve that
// drops dependent columns.
#pragma once
#include "lsm_device.hpp"

namespace mcg {

constexpr int LSM2_MAX_ORDER = 3;
// monomials zx^a zw^b with a + b <= deg, ordered by total degree t = a + b and, within a degree, by descending a
// (= ascending b): (a, b) sits at t (t + 1)/2 + b
__host__ __device__ constexpr int lsm2_count(int deg) { return (deg + 1) * (deg + 2) / 2; }
__host__ __device__ constexpr int lsm2_index(int a, int b) { return (a + b) * (a + b + 1) / 2 + b; }
__host__ __device__ constexpr int lsm2_degree(int k) {  // total degree of monomial k
    int t = 0;
    while (lsm2_count(t) <= k) ++t;
    return t;
}
__host__ __device__ constexpr int lsm2_b(int k) { return k - lsm2_degree(k) * (lsm2_degree(k) + 1) / 2; }
__host__ __device__ constexpr int lsm2_a(int k) { return lsm2_degree(k) - lsm2_b(k); }

// Layout of the block a date's solve leaves for the update pass of that date (doubles): the fit at (S, F) is
//   sum_k coef[k] zx^a_k zw^b_k,  zx = (S - MU_X) ISD_X,  zw = (F - MU_W) ISD_W    (ISD = 0: constant on this date)
constexpr int LSM2_C_COUNT = 10;  // in-the-money paths of the date
constexpr int LSM2_C_MU_X = 11, LSM2_C_ISD_X = 12, LSM2_C_MU_W = 13, LSM2_C_ISD_W = 14;
constexpr int LSM2_COEF_DOUBLES = 16;
// ... and of the block the centre reduce leaves for the moment pass and the solve: {count, mu_x, isd_x, mu_w, isd_w}
constexpr int LSM2_CENTRE_DOUBLES = 5;
constexpr int LSM2_CENTRE_SUMS = 5;  // what the centre pass sums over the in-the-money paths: {1, S, S^2, F, F^2}

// phi[k] = zx^a_k zw^b_k for every monomial of degree <= DEG: each from the one a degree below it
template <int DEG>
__device__ __forceinline__ void lsm2_monomials(double zx, double zw, double (&phi)[lsm2_count(DEG)]) {
    phi[0] = 1.0;
#pragma unroll
    for (int t = 1; t <= DEG; ++t) {
        phi[lsm2_index(t, 0)] = phi[lsm2_index(t - 1, 0)] * zx;
#pragma unroll
        for (int b = 1; b <= t; ++b) phi[lsm2_index(t - b, b)] = phi[lsm2_index(t - b, b - 1)] * zw;
    }
}

// mean and inverse standard deviation of a regressor over n in-the-money paths from its sums; isd = 0 where it is constant
__device__ __forceinline__ void lsm2_standardise(double n, double sum, double sum2, double& mu, double& isd) {
    mu = sum / n;
    const double m2 = sum2 / n;
    const double var = fmax(m2 - mu * mu, 0.0);
    isd = var > 1e-12 * m2 ? 1.0 / sqrt(var) : 0.0;
}

// One thread.  mom: the lsm2_count(2 P) power sums, then the NB = lsm2_count(P) cross sums, of a date with mom[0] >= 1
// in-the-money paths.  Writes coef[0..NB) and returns the number of dropped columns.  A dropped column keeps a zero
// column of L, a zero pivot and a zero inverse pivot, so it adds exact zeros to everything behind it: no branch, the
// loops unroll and (as in lsm_solve_nb) the matrices stay in registers.
template <int P>
__device__ __forceinline__ int lsm2_solve(const double* mom, double* coef) {
    constexpr int NB = lsm2_count(P), NP = lsm2_count(2 * P);
    double L[NB][NB], piv[NB], inv_piv[NB], d[NB], sol[NB];
    int dropped = 0;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const double g = mom[lsm2_index(2 * lsm2_a(k), 2 * lsm2_b(k))];
        d[k] = g > 0.0 ? 1.0 / sqrt(g) : 0.0;
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        double dj = d[j] > 0.0 ? 1.0 : 0.0;  // the equilibrated diagonal
#pragma unroll
        for (int k = 0; k < j; ++k) dj -= L[j][k] * L[j][k] * piv[k];
        const bool keep = d[j] > 0.0 && dj > 1e-8;
        dropped += keep ? 0 : 1;
        piv[j] = keep ? dj : 0.0;
        inv_piv[j] = keep ? 1.0 / dj : 0.0;
#pragma unroll
        for (int i = j + 1; i < NB; ++i) {
            double v = mom[lsm2_index(lsm2_a(i) + lsm2_a(j), lsm2_b(i) + lsm2_b(j))] * d[i] * d[j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k] * piv[k];
            L[i][j] = v * inv_piv[j];
        }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {  // L y = rhs, then D^-1
        double v = mom[NP + i] * d[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[i][k] * sol[k] * piv[k];
        sol[i] = v * inv_piv[i];
    }
#pragma unroll
    for (int i = NB - 1; i >= 0; --i) {  // L^T x = y
        double v = sol[i];
#pragma unroll
        for (int k = i + 1; k < NB; ++k) v -= L[k][i] * sol[k];
        sol[i] = inv_piv[i] != 0.0 ? v : 0.0;
    }
#pragma unroll
    for (int k = 0; k < NB; ++k) coef[k] = sol[k] * d[k];
    return dropped;
}

}  // namespace mcg
