// The local-volatility step of include/mcgpu.h (mcg_paths_localvol), shared by its two generators: kernels_localvol.hip draws
// z from Philox, kernels_sobol.hip from a Sobol' point.
#pragma once
#include "devmath.hpp"
#include "fastmath.hpp"
#include "mcg_internal.hpp"

namespace mcg {

struct LocalVolArgs {
    double* out;            // [n_steps+1][ld] prices
    int64_t ld;
    int64_t n_paths;
    int n_steps;
    int nx1;                // n_x - 1: entries of a slice
    uint64_t path_begin;
    uint32_t k0, k1;        // Philox key = seed
    double S0;
    double inv_dx, u0, m;   // LocalVolScalars
    double u_max;           // (double)(n_x - 1)
    const double2* surf;    // [n_slices][nx1] {a_j, d_j}
    double K;
    int is_call;
    double* partials;       // [gridDim.x][2]
    const double2* tabs;    // fm::Tables on the device
};

// One step of the contract from the slice `sl` (LDS) and the draw z.
__device__ __forceinline__ void localvol_step(const LocalVolArgs& a, const double2* sl, double z, double& S, double& X) {
    const double u = __builtin_fmin(__builtin_fmax(__builtin_fma(X, a.inv_dx, a.u0), 0.0), a.u_max);
    const int j = min((int)u, a.nx1 - 1);
    const double f = u - (double)j;
    const double2 ad = sl[j];
    const double s = __builtin_fma(f, ad.y, ad.x);
    const double e = __builtin_fma(s, z, __builtin_fma(-0.5 * s, s, a.m));
    X = X + e;
    S = fm::scaled_exp(S, e);
}

// The step of mcg_mlmc_localvol_level_ex: localvol_step's lookup and, with MILSTEIN, the correction (s / 2) (ds / dX) (z z - 1)
// from the slope of the bilinear table, zero where the lookup clamps.  Returns the step volatility s.
template <bool MILSTEIN>
__device__ __forceinline__ double localvol_step_vol(const LocalVolArgs& a, const double2* sl, double z, double& S, double& X) {
    const double uu = __builtin_fma(X, a.inv_dx, a.u0);
    const double u = __builtin_fmin(__builtin_fmax(uu, 0.0), a.u_max);
    const int j = min((int)u, a.nx1 - 1);
    const double f = u - (double)j;
    const double2 ad = sl[j];
    const double s = __builtin_fma(f, ad.y, ad.x);
    double e = __builtin_fma(s, z, __builtin_fma(-0.5 * s, s, a.m));
    if constexpr (MILSTEIN) {
        const double g = (uu > 0.0 && uu < a.u_max) ? ad.y * a.inv_dx : 0.0;
        e = __builtin_fma((0.5 * s) * g, __builtin_fma(z, z, -1.0), e);
    }
    X = X + e;
    S = fm::scaled_exp(S, e);
    return s;
}

}  // namespace mcg
